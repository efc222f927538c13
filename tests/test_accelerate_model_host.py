"""The model of the accelerated solve loop (tests/accelerate_model.py) on the CPU: what the device comparisons of
tests/test_gpu_accelerate_shapes.py rely on.  The cycles are tests/vcycle_model.VcycleModel(smoother="jacobi") and
tests/chebyshev_model.ChebyshevModel(ratio 8) built from the oracle's operators: no device.  The catalogue is accelerate_model.shape_catalogue().

Floor table (test_floor_table): of 8 iterations with d = 8, stop type 2, the leading ones whose residue stays at or above FLOOR_REL = 1e-9 times
the first, for m = 1, 2, 3, 4:

  chain63 / 64 / 65 / 129 / 193-L1, isolated40x40, hub48x40        Jacobi [8, 8, 8, 8]   Chebyshev [8, 8, 8, 8]
  chain63 / 65 / 193-L2, chain193-L3                               Jacobi [8, 6, 6, 6]   Chebyshev [8, 7, 7, 7]
  chain64 / 129 / 513 / 1025-L2                                    Jacobi [8, 7, 7, 7]   Chebyshev [8, 7, 7, 7]
  chain129-coarsest1, clique65 (blocked or not)                    Jacobi [8, 8, 8, 8]   Chebyshev [8, 7, 7, 7]
  diagonal100                                                      Jacobi [5, 3, 2, 2]   Chebyshev [8, 6, 2, 2]
  chain2-L1 / L2                                                   Jacobi [5, 1, 2, 2] / [3, 1, 2, 2]   Chebyshev [8, 1, 2, 2] / [6, 1, 2, 2]
  grid2x2-coarsest1                                                Jacobi [6, 6, 5, 3]   Chebyshev [8, 8, 6, 3]

Every case the device comparison uses keeps at least 6 of 8; diagonal100 keeps 2 at m >= 3 and is compared in its first iteration only
(accelerate_model.EARLY_FLOOR), as are the shapes with fewer than 5 unknowns.

Sensitivity (test_sensitivity_sets_the_device_tolerance): the model run twice, the second time with every cycle output multiplied by
1 + 2^-52 standard_normal, over the covering selection of the device test.  Largest |delta residue| / residue[0] over the compared iterations
3.17e-13 (hub48x40, Jacobi cycle; 1.9e-13 with Chebyshev; the chain L1 cases 1.1e-14 .. 2.3e-14; everything else <= 1.3e-14), largest
max |delta x| / max |x| 3.63e-13 (hub48x40, Chebyshev; 1.85e-13 with Jacobi; everything else <= 2.8e-14).  SHAPE_TOL = max(100 x 3.63e-13, 1e-12) = 3.7e-11,
below the 1e-9 allowed.

Past the floor (tol below the accuracy floor, max_iter = 25): without the floor guard (accel_scalars.hpp::accel_floor, FLOOR_GUARD_REL2 here) the
loop stores directions made of rounding noise and divides by their <q, q>.  Worst returned residue over m, d in {1, 3, 8}, stop types 0, 2, 3,
seeds 300 and 301, relative to the plain loop's after the same count (Jacobi / exact-diagonal / Chebyshev cycle): one unknown 8e+15 / 1 / not
finite; chain2-L1 4e+95 / 1e+31 / 1e+73; chain2-L2 5e+37 / 2e+34 / 1e+61; the 2 x 2 grid 1e+20 / 4e+15 / 2e+14; diagonal100 with a cycle that
solves it exactly 1e+14 (a residue of 1e-5); chain5 up to 3e+2; everything larger <= 7.  With the guard: <= 4.5 on every shape and cycle, no
status worse than the plain loop's, and the residues above the floor keep their bits (test_floor_guard_*)."""
import functools

import numpy as np
import pytest

from tests import problems
from tests.accelerate_model import (EARLY_FLOOR, FLOOR_REL, NONINCREASING, SHAPE_TOL, above_floor, accelerated_loop, norm, plain_loop,
                                    shape_catalogue, weights)
from tests.chebyshev_model import ChebyshevModel
from tests.vcycle_model import VcycleModel

CASES, EARLY, TINY = shape_catalogue()
SPEC = {c[0]: c[1] for c in CASES + EARLY + TINY}
COMPARED = [c[0] for c in CASES]
CYCLES = ("jacobi", "chebyshev")
FLOOR_CYCLES = CYCLES + ("exact",)          # Jacobi with omega = 1: solves a diagonal system in one sweep, the floor from the first iteration on
# the covering selection of the device comparison: (d, m, stop type)
SELECTION = [(d, 4, 2) for d in range(1, 9)] + [(5, m, 2) for m in (1, 2, 3)] + [(3, 2, t) for t in (0, 1, 3)]


@functools.lru_cache(maxsize=None)
def _problem(name):
    return problems.synthetic_problem(**SPEC[name])


@functools.lru_cache(maxsize=None)
def _cycle(oracle, name, which):
    P = _problem(name)
    if which == "jacobi":
        return VcycleModel(None, P.U, P.mass, P.lhs, oracle, 1.0, smoother="jacobi").vcycle
    if which == "exact":
        return VcycleModel(None, P.U, P.mass, P.lhs, oracle, 1.0, smoother="jacobi", jacobi_omega=1.0).vcycle
    return ChebyshevModel(None, P.U, P.mass, P.lhs, oracle, 8.0).vcycle


def _rhs(name, d, seed=300):
    P = _problem(name)
    return P.mass[:, None] * np.random.default_rng(seed + d).standard_normal((P.n, d))


def _run(oracle, name, which, d, m, stop_type, tol=0.0, max_iter=8, **kw):
    P, b = _problem(name), _rhs(name, d)
    return accelerated_loop(P.lhs, P.mass, _cycle(oracle, name, which), b, b, m, stop_type, tol, max_iter, **kw)


def _colnorm(w, r):
    return np.sqrt((w * r * r).sum(axis=0))


@pytest.mark.parametrize("which", CYCLES)
@pytest.mark.parametrize("name", COMPARED + list(EARLY_FLOOR) + ["grid2x2-coarsest1"])
def test_step_is_the_minimal_residual_one(oracle, name, which):
    """Above the floor the weighted residue of every column is no larger than with alpha = 1, beta = 0 from the same state (the plain cycle's
    step), and no larger than with alpha (1 +- 1e-3) along the same direction; the stored directions are orthogonal to the new one."""
    P = _problem(name)
    for d, m, t in ((3, 1, 2), (3, 3, 2), (5, 4, 0), (2, 2, 3)):
        w = weights(P.mass, t)
        _, _, res, _, steps = _run(oracle, name, which, d, m, t, keep_vectors=True)
        for st in steps[:above_floor(res)]:
            assert not st["guarded"].any()
            r, q, al = st["r"], st["q"], st["alpha"]
            got = _colnorm(w, r - al * q)
            assert np.all(got <= NONINCREASING * _colnorm(w, r - st["q0"])), (name, d, m, t)
            for f in (1.0 - 1e-3, 1.0 + 1e-3):
                assert np.all(got <= NONINCREASING * _colnorm(w, r - f * al * q)), (name, d, m, t, f)
            for qj, sj in zip(st["stored_q"], st["stored_s"]):
                assert np.all(np.abs((w * q * qj).sum(axis=0)) <= 1e-10 * np.sqrt(st["s"] * sj)), (name, d, m, t)


@pytest.mark.parametrize("which", CYCLES)
@pytest.mark.parametrize("name", ["chain2-L1", "chain2-L2"])
def test_two_unknowns_are_solved_in_two_iterations(oracle, name, which):
    """Finite termination: with two directions kept (m >= 2) the Krylov space of a 2 x 2 system is exhausted after two iterations."""
    its = [_run(oracle, name, which, 1, m, 2, tol=1e-10, max_iter=25)[1] for m in (1, 2, 3, 4)]
    print(name, which, "iterations to 1e-10 for m = 1..4:", its)
    assert all(i <= 2 for i in its[1:]) and its[0] >= 2


def test_iteration_counts_to_1e_10(oracle):
    """The counts any change of the loop has to leave alone (Jacobi cycle, d = 3, stop type 2, m = 1..4)."""
    for name, want in (("chain63-L2", [8, 7, 7, 7]), ("hub48x40", [30, 28, 23, 22])):
        its = [_run(oracle, name, "jacobi", 3, m, 2, tol=1e-10, max_iter=60)[1] for m in (1, 2, 3, 4)]
        print(name, its)
        assert its == want


@pytest.mark.parametrize("name", COMPARED + list(EARLY_FLOOR) + [c[0] for c in TINY])
def test_floor_table(oracle, name):
    """Module docstring: every case the device comparison uses keeps at least 3 of 8 iterations above the floor, for both cycles and every depth;
    the early-floor list holds exactly the larger cases that do not."""
    for which in CYCLES:
        row = [above_floor(_run(oracle, name, which, 8, m, 2)[2]) for m in (1, 2, 3, 4)]
        print("FLOOR_TABLE", name, _problem(name).n, which, row)
        if name in COMPARED:
            assert min(row) >= 3, (name, which, row)
    if name in EARLY_FLOOR:
        assert min(min(above_floor(_run(oracle, name, which, 8, m, 2)[2]) for m in (1, 2, 3, 4)) for which in CYCLES) < 3


@functools.lru_cache(maxsize=None)
def _sensitivity(oracle, name, which):
    P, cyc = _problem(name), _cycle(oracle, name, which)
    rng = np.random.default_rng(7)

    def noisy(b, x):
        out = cyc(b, x)
        return out * (1.0 + 2.0 ** -52 * rng.standard_normal(out.shape))

    def x_after(x, steps, k):
        return x if k == len(steps) else steps[k]["xk"]          # (the iterate does not depend on where the loop is cut)

    dr = dx = 0.0
    for d, m, t in SELECTION:
        b = _rhs(name, d)
        x1, _, res, _, st1 = accelerated_loop(P.lhs, P.mass, cyc, b, b, m, t, 0.0, 8, keep_vectors=True)
        x2, _, res2, _, st2 = accelerated_loop(P.lhs, P.mass, noisy, b, b, m, t, 0.0, 8, keep_vectors=True)
        k = above_floor(res)
        dr = max(dr, float(np.max(np.abs(res[:k] - res2[:k])) / res[0]))
        x1, x2 = x_after(x1, st1, k), x_after(x2, st2, k)
        dx = max(dx, float(np.max(np.abs(x1 - x2)) / np.max(np.abs(x1))))
    return dr, dx


@pytest.mark.parametrize("name", COMPARED)
def test_sensitivity(oracle, name):
    """One case of the survey below (kept for it): the change stays below SHAPE_TOL / 100 on every case."""
    for which in CYCLES:
        dr, dx = _sensitivity(oracle, name, which)
        print("SENSITIVITY %-20s %-9s residue %.2e  x %.2e" % (name, which, dr, dx))
        assert max(dr, dx) <= SHAPE_TOL / 100.0


def test_sensitivity_sets_the_device_tolerance(oracle):
    """SHAPE_TOL is max(100 x the largest change one rounding per cycle output makes, 1e-12), and it is at most 1e-9 (module docstring)."""
    worst = max(max(_sensitivity(oracle, name, which)) for name in COMPARED for which in CYCLES)
    want = max(100.0 * worst, 1e-12)
    print("largest %.3e -> SHAPE_TOL %.3e (constant %.3e)" % (worst, want, SHAPE_TOL))
    assert want <= SHAPE_TOL <= 1.05 * want and SHAPE_TOL <= 1e-9


TINY_FLOOR = 1e-13          # residues relative to ||b|| (absolute with ||b|| = O(1) for stop type 3): eps x condition number of these systems


def _above_tiny_floor(res):
    k = 0
    while k < len(res) and res[k] >= max(FLOOR_REL * res[0], TINY_FLOOR):
        k += 1
    return k


@pytest.mark.parametrize("which", CYCLES)
@pytest.mark.parametrize("name", [c[0] for c in TINY] + list(EARLY_FLOOR))
def test_tiny_shapes_until_the_floor(oracle, name, which):
    """Levels of 1, 2 and 4 unknowns and the diagonal operator: eight iterations, every reported residue finite and non-increasing while above the
    floor; the first iteration is no worse than the plain cycle's."""
    P = _problem(name)
    for d, m, t in SELECTION:
        b = _rhs(name, d)
        _, _, res, _, _ = _run(oracle, name, which, d, m, t)
        pres = plain_loop(P.lhs, P.mass, _cycle(oracle, name, which), b, b, t, 0.0, 1)[2]
        k = _above_tiny_floor(res)          # (a system of one unknown is solved by the first cycle: the first residue is on the floor already)
        assert np.all(np.isfinite(res[:max(k, 1)])), (name, d, m, t, res)
        assert np.all(res[1:k] <= res[:max(k, 1) - 1] * NONINCREASING), (name, d, m, t, res)
        first = _run(oracle, name, which, d, m, t, max_iter=1)[2][0]                  # (the confirmed one)
        assert first <= pres[0] * NONINCREASING or first <= 1e-14, (name, d, m, t, first, pres)          # (1e-14: both solved the system)


def _past_the_floor(oracle, name, which, tols, floor_guard=True, seeds=(300,)):
    """The worst of returned residue / (10 max(plain, best)) and of returned / plain over m, d, stop types and the tolerances, and the number of
    runs that are not finite or end with a status worse than the plain loop's (above the first residue where the plain loop is not)."""
    P, cyc = _problem(name), _cycle(oracle, name, which)
    worst = vs_plain = 0.0
    bad = 0
    for seed in seeds:
        for d in (1, 3, 8):
            b = _rhs(name, d, seed)
            for t in (0, 2, 3):
                for tol in tols:
                    pres = plain_loop(P.lhs, P.mass, cyc, b, b, t, tol, 25)[2]
                    for m in (1, 2, 3, 4):
                        with np.errstate(all="ignore"):
                            x, it, res, _, steps = accelerated_loop(P.lhs, P.mass, cyc, b, b, m, t, tol, 25, floor_guard=floor_guard)
                        best = min(s["residue"] for s in steps if s["confirmed"])
                        if not (np.all(np.isfinite(x)) and np.isfinite(res[-1])):
                            bad += 1
                            continue
                        # (the verdict of solve_rule.hpp: above the tolerance and above the first residue -- unless on the floor, rule_confirmed)
                        floor = 1e-12 * (np.sqrt((b * b).sum()) if t == 3 else 1.0)
                        bad += (res[-1] > tol and it > 1 and res[-1] > res[0] and res[-1] > floor) and not (pres[-1] > tol and len(pres) > 1 and pres[-1] > pres[0])
                        worst = max(worst, res[-1] / (10.0 * max(pres[-1], best)) if res[-1] > 0 else 0.0)
                        vs_plain = max(vs_plain, res[-1] / pres[-1] if pres[-1] > 0 else 0.0)
    return worst, vs_plain, bad


# (the CPU cycles know no blocking: clique65-blocked is clique65 here)
@pytest.mark.parametrize("which", CYCLES)
@pytest.mark.parametrize("name", [n for n in COMPARED if n != "clique65-blocked"])
def test_past_the_floor_stays_on_the_floor(oracle, name, which):
    """tol = 1e-17 (and 0), max_iter = 25, m = 1..4, d in {1, 3, 8}, stop types 0, 2, 3: the returned residue and x are finite, the residue is at
    most 10 x max(the plain loop's after the same count, the smallest confirmed one of the history), and the loop does not end above its first
    residue where the plain loop does not."""
    # (tol = 0 differs from 1e-17 only where a residue of at most 1e-17 is reported: run on the small cases, which reach one)
    worst, vs_plain, bad = _past_the_floor(oracle, name, which, (1e-17, 0.0) if _problem(name).n <= 130 else (1e-17,))
    print("PAST_FLOOR", name, which, "returned / bound at most %.3e, returned / plain at most %.3e" % (worst, vs_plain))
    assert bad == 0 and worst <= 1.0 and vs_plain <= 10.0


@pytest.mark.parametrize("which", FLOOR_CYCLES)
@pytest.mark.parametrize("name", [c[0] for c in TINY] + list(EARLY_FLOOR))
def test_floor_guard_keeps_tiny_and_exactly_solved_systems_on_the_floor(oracle, name, which):
    """The same property on 1, 2 and 4 unknowns and the diagonal operator, seeds 300 and 301, also with a cycle that solves a diagonal system
    exactly -- where the loop without the guard returns 1e-5 .. 1e+95 or nothing finite (module docstring)."""
    worst, vs_plain, bad = _past_the_floor(oracle, name, which, (1e-17, 0.0), seeds=(300, 301))
    print("PAST_FLOOR", name, which, "returned / bound at most %.3e, returned / plain at most %.3e" % (worst, vs_plain))
    assert bad == 0 and worst <= 1.0 and vs_plain <= 10.0


def test_floor_guard_is_what_keeps_them_there(oracle):
    """Without the guard the loop leaves the floor on every tiny shape family and on the exactly solved diagonal system (this is what a device
    without the guard computes: the tests above would fail on it)."""
    for name, which in (("chain2-L1", "jacobi"), ("chain2-L2", "chebyshev"), ("grid2x2-coarsest1", "jacobi"), ("diagonal100", "exact"), ("chain1-L1", "chebyshev")):
        worst, vs_plain, bad = _past_the_floor(oracle, name, which, (1e-17,), floor_guard=False, seeds=(300, 301))
        print(name, which, "without the guard: returned / plain up to %.3e, %d runs not finite or with a worse status" % (vs_plain, bad))
        assert bad > 0 or vs_plain > 1e6


def test_floor_guard_leaves_the_iterations_above_the_floor_alone(oracle):
    """Every residue above the floor has the bits it has without the guard, over the covering selection on every compared case."""
    for name in COMPARED:
        if name == "clique65-blocked":
            continue
        P = _problem(name)
        for which in CYCLES:
            cyc = _cycle(oracle, name, which)
            for d, m, t in SELECTION[3::4] + [(8, 4, 2)]:
                b = _rhs(name, d)
                with_guard = accelerated_loop(P.lhs, P.mass, cyc, b, b, m, t, 0.0, 8)[2]
                without = accelerated_loop(P.lhs, P.mass, cyc, b, b, m, t, 0.0, 8, floor_guard=False)[2]
                k = above_floor(without)
                assert np.array_equal(with_guard[:k], without[:k]), (name, which, d, m, t)
