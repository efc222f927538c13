// cheby_coeffs.hpp -- the scalars of the Chebyshev smoother (GMG_SMOOTHER_CHEBYSHEV): the interval of a level from its Gershgorin bound and the
// two coefficients of step k.  Host only: the launch code (engine_cycle.hip.hpp::launch_cheby_steps) calls it and hands the coefficients to the
// kernel as arguments, and a small stand-alone program runs it under a sanitizer (tests/test_chebyshev_host.py).  No HIP, no engine state.
//
// Chebyshev iteration on D^-1 A over [lambda_max / ratio, lambda_max], lambda_max = Lambda (the level's bound, gmgs::gershgorin_rows):
//   theta = (lambda_max + lambda_min) / 2, delta = (lambda_max - lambda_min) / 2, sigma = theta / delta
//   step 0:      p = (1 / theta) D^-1 (b - A x),                                  x += p,  rho_0 = 1 / sigma
//   step k >= 1: rho_k = 1 / (2 sigma - rho_{k-1}),  p = rho_k rho_{k-1} p + (2 rho_k / delta) D^-1 (b - A x),  x += p
// After k + 1 steps the error is T_{k+1}((theta - D^-1 A) / delta) / T_{k+1}(sigma) times the initial one: of modulus below 1 on all of
// (0, lambda_max], so the iteration converges for every symmetric positive definite A whatever `ratio` is.
#pragma once

namespace gmg {

// lambda_max / lambda_min of the interval the polynomial is built for (GMG_CHEBY_RATIO overrides it: host_sparse.hpp::EnvSwitches).  Centre of the
// plateau of profiles/cheby/ratio_scan.json (cycles to 1e-4 at degrees 2 + 2 and 3 + 3 on the workloads of the gs_omega scan).
constexpr double kChebyRatio = 8.0;

// a ratio the recurrence can run with: delta > 0 needs ratio > 1 (and a finite one)
inline bool cheby_ratio_usable(double ratio) { return ratio > 1.0 && ratio <= 1e6; }

struct ChebyInterval {
    double theta, delta, sigma;
};

inline ChebyInterval cheby_interval(double lambda, double ratio) {
    const double lmax = lambda, lmin = lambda / ratio;
    ChebyInterval iv;
    iv.theta = 0.5 * (lmax + lmin);
    iv.delta = 0.5 * (lmax - lmin);
    iv.sigma = iv.theta / iv.delta;
    return iv;
}

struct ChebyStep {
    double c1;      // coefficient of the previous p (0 at step 0: the kernel's FIRST instantiation does not read p)
    double c2;      // coefficient of D^-1 (b - A x)
};

// the coefficients of step k (k = 0, 1, ...) of a polynomial that starts at step 0; k is a polynomial degree (a few steps): the rho recurrence
// is simply run from its start
inline ChebyStep cheby_step_coeffs(double lambda, double ratio, int k) {
    const ChebyInterval iv = cheby_interval(lambda, ratio);
    ChebyStep st;
    if (k <= 0) { st.c1 = 0.0; st.c2 = 1.0 / iv.theta; return st; }
    double rho_prev = 1.0 / iv.sigma, rho = rho_prev;
    for (int j = 1; j <= k; ++j) {
        rho = 1.0 / (2.0 * iv.sigma - rho_prev);
        if (j < k) rho_prev = rho;
    }
    st.c1 = rho * rho_prev;
    st.c2 = 2.0 * rho / iv.delta;
    return st;
}

}  // namespace gmg
