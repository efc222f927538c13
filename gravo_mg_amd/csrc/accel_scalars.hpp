// accel_scalars.hpp -- the scalar decisions of the accelerated solve loop (gmg_config::accelerate: truncated GCR around the V-cycle), per
// right-hand-side column.  Compiles for the host and for the device: the reducing kernels of accel_kernels.hip.hpp call it, and a small
// stand-alone program runs it under a sanitizer (tests/test_accelerate_host.py).  No HIP, no engine state.
#pragma once

#if defined(__HIPCC__)
#define GMG_ACCEL_HD __host__ __device__
#else
#define GMG_ACCEL_HD
#endif

namespace gmg {

constexpr int kAccelMaxDepth = 4;                        // largest gmg_config::accelerate
constexpr int kAccelMaxStored = kAccelMaxDepth - 1;      // directions kept beside the current one

// A weighted square sum <q, q> a column may be divided by: not zero, not infinite, not a NaN.
GMG_ACCEL_HD inline bool accel_usable(double s) { return s != 0.0 && __builtin_isfinite(s); }

// Coefficient of the stored direction j in the new one: <q, q_j> / s_j, or 0 where that direction was never stored for this column (s_j = 0).
GMG_ACCEL_HD inline double accel_beta(double q_dot_qj, double s_j) { return accel_usable(s_j) ? q_dot_qj / s_j : 0.0; }

struct AccelStep {
    double alpha;      // step length along the orthogonalised direction; 1 when guarded
    double s_store;    // what the ring keeps as s_j for this direction; 0 when guarded (the direction is not stored)
    int guarded;       // 1: s = <q, q> is zero or not finite -- the column takes the cycle's own iterate (alpha = 1, every beta = 0)
};

// s = <q, q>, rho = <r, q> of the orthogonalised direction
GMG_ACCEL_HD inline AccelStep accel_step(double s, double rho) {
    AccelStep st;
    st.guarded = accel_usable(s) ? 0 : 1;
    st.alpha = st.guarded ? 1.0 : rho / s;
    st.s_store = st.guarded ? 0.0 : s;
    return st;
}

}  // namespace gmg
