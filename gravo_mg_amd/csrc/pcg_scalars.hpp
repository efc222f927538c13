// pcg_scalars.hpp -- the scalar decisions of the preconditioned CG solve loop (gmg_config::pcg: conjugate gradients with the handle's V-cycle as
// the preconditioner), per right-hand-side column.  Compiles for the host and for the device: the reducing kernels of pcg_kernels.hip.hpp call it,
// and a small stand-alone program runs it under a sanitizer (tests/test_pcg_host.py).  No HIP, no engine state.
#pragma once

#include "accel_scalars.hpp"

namespace gmg {

// beta of p = z + beta p from rho = <r, z> of this iteration and of the previous one.  fresh: the column starts a new recurrence -- the first
// iteration of a solve, the iteration after a guarded one, the iteration after a confirmation recomputed r -- and p = z is written without
// reading the old p.  A previous rho that cannot be divided by (zero, not finite) or a rho that is not finite gives 0 as well: the direction
// is then z alone, and pcg_step decides whether it is taken.
GMG_ACCEL_HD inline double pcg_beta(double rho, double rho_prev, bool fresh) {
    return !fresh && accel_usable(rho_prev) && __builtin_isfinite(rho) ? rho / rho_prev : 0.0;
}

struct PcgStep {
    double alpha;      // step length along p; 0 when guarded: x and r of the column stay as they are (the update does not read p or q then)
    int guarded;       // 1: the column took a guard in this iteration -- its next iteration is fresh (beta = 0)
};

// pq = <p, A p>, rho = <r, z> of the iteration; rr = the column's sum of w r^2 as the last check or update reported it and floor2 =
// accel_floor(sum of w b^2) (floor2 = 0: neither is known yet, the first iteration of a solve -- no floor guard).
// Guards: <p, q> not positive or not finite (p is no descent direction of the energy: rounding noise, a preconditioner that is not SPD, a NaN),
// rho not finite, or the residual on the floor of accel_scalars.hpp (rr <= 1e-25 <b, b>: b - A x cannot be evaluated more accurately, a step
// from such an r is noise divided by noise).
GMG_ACCEL_HD inline PcgStep pcg_step(double pq, double rho, double rr, double floor2) {
    PcgStep st;
    const bool frozen = floor2 > 0.0 && rr <= floor2;
    st.guarded = pq > 0.0 && __builtin_isfinite(pq) && __builtin_isfinite(rho) && !frozen ? 0 : 1;
    st.alpha = st.guarded ? 0.0 : rho / pq;
    return st;
}

}  // namespace gmg
