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
// The floor guard: a direction with <q, q> <= kAccelFloorRel2 <b, b> (same weights: |q| below 3.2e-13 |b|) is rounding noise.  b - A x cannot be
// evaluated to better than eps |A| |x| >= eps |b|, so a q = r - r~ that small no longer is A z; dividing by its <q, q> (alpha, and every later
// beta of the stored copy) moved the iterate off the accuracy floor again -- to 1e+81 on a 2 x 2 system, 1e-5 on a diagonal one.
// Such a column takes the guard: the cycle's own iterate, nothing stored.  A residue of 1e-10 |b| is three digits above it: the iterations to any
// tolerance a caller can reach are unchanged (the counts are pinned in tests/test_accelerate_model_host.py).
constexpr double kAccelFloorRel2 = 1e-25;

// A weighted square sum <q, q> a column may be divided by: not zero, not infinite, not a NaN.
GMG_ACCEL_HD inline bool accel_usable(double s) { return s != 0.0 && __builtin_isfinite(s); }

// Coefficient of the stored direction j in the new one: <q, q_j> / s_j, or 0 where that direction was never stored for this column (s_j = 0).
GMG_ACCEL_HD inline double accel_beta(double q_dot_qj, double s_j) { return accel_usable(s_j) ? q_dot_qj / s_j : 0.0; }

struct AccelStep {
    double alpha;      // step length along the orthogonalised direction; 1 when guarded
    double s_store;    // what the ring keeps as s_j for this direction; 0 when guarded (the direction is not stored)
    int guarded;       // 1: s = <q, q> is zero, not finite or on the floor -- the column takes the cycle's own iterate (alpha = 1, every beta = 0)
};

// <q, q> at or below which a direction is noise, from bb = <b, b> of the column (0, negative or NaN: not known, no floor)
GMG_ACCEL_HD inline double accel_floor(double bb) { return bb > 0.0 ? kAccelFloorRel2 * bb : 0.0; }

// s = <q, q>, rho = <r, q> of the orthogonalised direction; floor2 = accel_floor(<b, b>) (0: no floor guard -- the first iteration of a solve)
GMG_ACCEL_HD inline AccelStep accel_step(double s, double rho, double floor2 = 0.0) {
    AccelStep st;
    st.guarded = accel_usable(s) && !(floor2 > 0.0 && s <= floor2) ? 0 : 1;
    st.alpha = st.guarded ? 1.0 : rho / s;
    st.s_store = st.guarded ? 0.0 : s;
    return st;
}

}  // namespace gmg
