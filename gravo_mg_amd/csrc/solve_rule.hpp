// solve_rule.hpp -- the stopping rule of the solve loop (include/gravomg_hip.h, gmg_solve): the residue from the check's sums, when the loop goes
// on, when it has blown up, and when the caller is told GMG_DIVERGED.  Compiles for the host and for the device: gmgk::reduce_partials decides
// with it where the sums are, the host loop (engine_cycle.hip.hpp::solve_loop) once per cycle, and a small stand-alone program runs it under a
// sanitizer (tests/test_solve_rule_host.py).  sqrt and division are correctly rounded on both sides: the same bits, the same decision.
// No HIP, no engine state.
#pragma once

#if defined(__HIPCC__)
#define GMG_RULE_HD __host__ __device__
#else
#define GMG_RULE_HD
#endif

namespace gmg {

// residualCheck from its 2 d sums (s[2c]: sum of w r^2 of column c, s[2c + 1]: of w b^2), multigrid_solver.cpp:1228-1277
GMG_RULE_HD inline double norm_from_sums(const double* s, int d, int type) {
    if (type == 3) {
        double t = 0.0;
        for (int c = 0; c < d; ++c) t += s[2 * c];
        return __builtin_sqrt(t);
    }
    double out = 0.0;
    for (int c = 0; c < d; ++c) {
        const double v = type == 0 ? __builtin_sqrt(s[2 * c]) / __builtin_sqrt(s[2 * c + 1]) : __builtin_sqrt(s[2 * c] / s[2 * c + 1]);
        if (c == 0 || v > out) out = v;
    }
    return out;
}

// The smallest residue of this solve after cycle `cycle` (1, 2, ...) gave `residue`; the first cycle resets it.
GMG_RULE_HD inline double rule_least(double least_before, double residue, int cycle) {
    const double least = cycle <= 1 ? residue : least_before;
    return residue < least ? residue : least;
}
// No way back (the reference would spin to max_iter on NaNs): not finite, or from the third cycle on more than 1e4 x the smallest seen.
GMG_RULE_HD inline bool rule_blown(double residue, double least, int cycle) {
    return !__builtin_isfinite(residue) || (cycle >= 3 && residue > 1e4 * least);
}
// Another cycle is wanted (the host adds: and allowed, rule_goes_on).
GMG_RULE_HD inline bool rule_wants_more(double residue, double tol, bool blown) { return residue > tol && !blown; }

// What the host loop carries from cycle to cycle.
struct SolveRule {
    double tol; int max_iter;         // the caller's (max_iter >= 1)
    double first, least, residue;     // residue after the first cycle, the smallest so far, after the last cycle
    int cycles; bool blown;           // cycles done; the last residue allows no way back
};
// do { } while: at least one cycle (multigrid_solver.cpp:1411-1417)
GMG_RULE_HD inline SolveRule rule_begin(double tol, int max_iter) { return SolveRule{tol, max_iter < 1 ? 1 : max_iter, 0.0, 0.0, 0.0, 0, false}; }
// The state after one more cycle that gave `residue`.  By value: asking what a residue WOULD do commits nothing.
GMG_RULE_HD inline SolveRule rule_after(SolveRule r, double residue) {
    if (++r.cycles == 1) r.first = residue;
    r.least = rule_least(r.least, residue, r.cycles);
    r.residue = residue;
    r.blown = rule_blown(residue, r.least, r.cycles);
    return r;
}
// The accelerated loop (gmg_config::accelerate) reports the residue of a recurrence and confirms it on the iterate where it would end the loop.
// A confirmed residue of more than twice the recurrence's says the recurrence has lost touch with b - A x (it runs on below the accuracy floor):
// what it reported below the confirmed value was never seen on an iterate, and is no evidence of a blow-up -- `least` rises to the confirmed
// value.  A confirmed residue on the floor itself (at most `floor`: 1e-12 |b| in the stop type's measure, rule_floor) is measured against nothing
// smaller: a cycle that solves the system at once leaves a first recurrence of eps^2, `first` and `least` rise to the confirmed value -- a
// solve that ends on the floor has not diverged.  The state BEFORE rule_after(confirmed).
GMG_RULE_HD inline SolveRule rule_confirmed(SolveRule r, double recurrence, double confirmed, double floor) {
    if (r.cycles < 1) return r;
    const bool lost_touch = confirmed > 2.0 * recurrence, on_floor = confirmed <= floor;
    if ((lost_touch || on_floor) && r.least < confirmed) r.least = confirmed;
    if (on_floor && r.first < confirmed) r.first = confirmed;
    return r;
}
// 1e-12 |b| as a residue of this stop type, from the check's sums (s[2c + 1]: sum of w b^2): relative for types 0 .. 2
GMG_RULE_HD inline double rule_floor(const double* s, int d, int type) {
    if (type != 3) return 1e-12;
    double t = 0.0;
    for (int c = 0; c < d; ++c) t += s[2 * c + 1];
    return 1e-12 * __builtin_sqrt(t);
}
GMG_RULE_HD inline bool rule_goes_on(const SolveRule& r) { return rule_wants_more(r.residue, r.tol, r.blown) && r.cycles < r.max_iter; }
// Not contracting: the loop ended above the tolerance with a residue that is not finite, 1e4 x the smallest seen, or larger than after the first cycle.
GMG_RULE_HD inline bool rule_diverged(const SolveRule& r) { return !(r.residue <= r.tol) && (r.blown || (r.cycles > 1 && r.residue > r.first)); }

}  // namespace gmg
