"""gmg_config::fold_head: the residual check also computes the next cycle's first colour update (residual_norm_slices_head -> level 0's side
vector) and the launch enqueued ahead of the loop's decision is the second colour launch, which reads the first colour's values from the side
vector and commits them to x (gs_color_commit).  It changes how the cycle is launched, never what it computes.

Every case builds two handles that differ in fold_head alone and asks for: the iterate after every cycle (run_cycles(k), k = 1 .. 5, from a fresh
load), the residue histories, iteration counts and returned iterates of solves that stop on the tolerance, on max_iter and after their first
cycle -- all bitwise (array_equal on the bit patterns); heads_folded > 0 on the folded handle where the configuration is eligible and == 0 where
it is not (a missing key counts as 0: a loop that enqueues no heads never makes it); head_decision_differs == 0.

Eligible (engine_cycle.hip.hpp::fold_eligible) is where the parent's head is enqueued, with pre_iters >= 1 and a second non-empty colour class
on level 0 whose launch in the first pre-sweep is a plain one: not the sweep's last launch, i.e. not the last colour unless pre_iters >= 2.
`_eligible` restates that from the handle's colour classes.

Not reachable from a colouring: a second colour class with FEWER slices than the first -- level 0's classes are laid out in ascending size
(every layout printed by the cases below).  The commit's workgroups are sized by the first class alone and do not depend on the second's."""
import numpy as np
import pytest

from tests import colcode_cases as cc
from tests import problems

pytestmark = pytest.mark.gpu

STOP_TYPES = (0, 1, 2, 3)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _key(eng, key):
    try:
        return eng.timing(key)
    except Exception:
        return 0.0


def _pair(cabi, P, lhs=None, **kw):
    out = []
    for fold in (1, 0):
        e = cabi.Engine(fold_head=fold, **kw)
        e.set_prolongations(P.U); e.set_mass(P.mass); e.set_system(P.lhs if lhs is None else lhs)
        out.append(e)
    return out


def _classes(eng):
    _, cb = eng.level_ordering(0)
    return np.diff(np.asarray(cb, np.int64) // 64)          # slices per colour class


def _eligible(eng, pre_iters):
    slices = _classes(eng)
    full = np.flatnonzero(slices > 0)
    if pre_iters < 1 or len(full) < 2 or full[0] >= len(slices) - 1:
        return False
    return bool(full[1] < len(slices) - 1 or pre_iters >= 2)


def _workload(eng, rhs, stop_types=STOP_TYPES, cycles=5):
    """Everything the two handles are compared on, as {name: tuple of arrays and numbers}."""
    out = {}
    for t in stop_types:
        for k in range(1, cycles + 1):                       # the iterate after every cycle (heads behind cycles 1 .. k - 1)
            eng.load_problem(rhs, rhs)
            hist = eng.run_cycles(k, t)
            out["cycles", t, k] = (hist.copy(), eng.fetch_solution())
        for name, tol, max_iter in (("tolerance", float(hist[2]) * (1.0 + 1e-12), 50), ("max_iter", 1e-300, 3), ("first cycle", 1e300, 50)):
            x, it, r, conv = eng.solve(rhs, tol=tol, stop_type=t, max_iter=max_iter)
            assert 1 <= it <= 3 and (name != "max_iter" or it == 3) and (name != "first cycle" or it == 1), (name, t, it)
            # (fetch_solution: what the stopped iteration left in x on the device)
            out[name, t] = (x.copy(), np.array([it]), np.array([r]), conv[:it, 1].copy(), eng.fetch_solution())
    return out


def _compare(a, b):
    assert a.keys() == b.keys()
    for name in a:
        assert len(a[name]) == len(b[name])
        for u, v in zip(a[name], b[name]):
            assert same(u, v), name


def _check(cabi, P, rhs, eligible=None, pre_iters=2, stop_types=STOP_TYPES, solve_is_cycles=True, **kw):
    """eligible: True / False, or None = what _eligible says about the handle's colour classes.  solve_is_cycles: the solve loop's iterates are
    those of run_cycles (not with accelerate > 0)."""
    on, off = _pair(cabi, P, pre_iters=pre_iters, **kw)
    try:
        rhs = np.asfortranarray(rhs if rhs.ndim == 2 else rhs[:, None])
        a, b = _workload(on, rhs, stop_types), _workload(off, rhs, stop_types)
        _compare(a, b)
        # a stopped solve left x untouched: the device's x after the folded handle's solve is the unfolded handle's iterate after that many cycles
        for t in stop_types if solve_is_cycles else ():
            it = int(a["tolerance", t][1][0])
            assert same(a["tolerance", t][4], b["cycles", t, it][1]) and same(a["tolerance", t][0], b["cycles", t, it][1]), t
            assert same(a["first cycle", t][4], b["cycles", t, 1][1]), t
        want = _eligible(on, pre_iters) if eligible is None else eligible
        folded, heads = _key(on, "heads_folded"), _key(on, "heads_enqueued")
        print(f"\n[fold_head] classes (slices) {list(_classes(on))} eligible {want}: heads_enqueued {heads:.0f} heads_folded {folded:.0f}")
        if want:
            assert folded > 0 and folded <= heads
        else:
            assert folded == 0.0
        assert _key(off, "heads_folded") == 0.0 and _key(off, "heads_enqueued") == heads
        assert _key(on, "head_decision_differs") == 0.0 and _key(off, "head_decision_differs") == 0.0
        return on.debug_col16(0), _classes(on)
    finally:
        on.close(); off.close()


def _torus(d=1):
    return problems.torus_problem(64, 48, "poisson", 100, d=d)       # 3 072 vertices, the size of smoke()


@pytest.mark.parametrize("omega", [1.0, 1.35])
@pytest.mark.parametrize("d", [1, 3, 4])
def test_small_torus_every_width_relaxation_and_stop_type(cabi, d, omega):
    P = _torus(d)
    _, classes = _check(cabi, P, P.rhs, eligible=True, gs_omega=omega)
    assert (classes > 0).sum() >= 3


@pytest.mark.parametrize("kw", [dict(fine_col16=1), dict(fine_col16=0), dict(uniform_slices=0)], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_both_index_paths_on_the_torus(cabi, kw):
    P = _torus(3)
    codes, _ = _check(cabi, P, P.rhs, eligible=True, stop_types=(2,), **kw)
    assert (codes["windows"] > 0) == (kw.get("fine_col16", 1) == 1)
    if "uniform_slices" in kw:
        assert codes["uniform_width"] == 0


@pytest.mark.parametrize("name,mode", [("flagged-8", 2), ("prefix", 1)])
def test_flagged_and_uncoded_slices(cabi, name, mode):
    """Level 0 with slices flagged one by one (row_dot_sel mode 2) and with a 32-bit prefix (mode 1, from > 0: the first colour class is the
    uncoded one, so the check's head rows and the commit lie in it while the second colour launch decodes)."""
    P = cc.problem(name)
    for fine_col16 in (1, 0):
        codes, classes = _check(cabi, P, P.rhs[:, :3], stop_types=(2,), fine_col16=fine_col16, **cc.engine_settings(name))
        if fine_col16:
            assert codes["windows"] > 0 and codes["mode"] == mode and (mode == 2 or codes["from"] > 0)
        else:
            assert codes["windows"] == 0
    assert (classes > 0).sum() >= 3


def test_irregular_colouring_with_a_partly_padded_first_class(cabi):
    """Hull-triangulated sphere: five or more classes of unequal size, the first of fewer than 64 rows -- the check's head and the commit cover
    one partly padded slice (padding rows included)."""
    P = problems.sphere_problem(3000, 80)
    on = cabi.Engine()
    on.set_prolongations(P.U); on.set_mass(P.mass); on.set_system(P.lhs)
    try:
        new2old, cb = on.level_ordering(0)
        slices = _classes(on)
        first = np.flatnonzero(slices > 0)[0]
        real = int((new2old[cb[first]:cb[first + 1]] >= 0).sum())
        assert (slices > 0).sum() >= 5 and len(set(slices[slices > 0])) >= 3 and slices[first] == 1 and 0 < real < 64, (list(slices), real)
    finally:
        on.close()
    for d in (1, 3):
        rhs = P.rhs if d == 1 else np.random.default_rng(3).standard_normal((P.n, d)) * P.mass[:, None]
        _check(cabi, P, rhs, eligible=True, stop_types=(2, 0))


@pytest.mark.parametrize("pre,post", [(1, 2), (2, 2), (0, 2), (2, 0), (1, 0)])
def test_sweep_counts(cabi, pre, post):
    """pre_iters = 0 falls back (no head at all); post_iters = 0: the check has no folded last colour and visits every slice."""
    P = _torus(3)
    _check(cabi, P, P.rhs, eligible=pre >= 1, pre_iters=pre, post_iters=post, stop_types=(2, 3))


def test_two_colour_classes_fold_only_with_a_second_pre_sweep(cabi):
    """A chain has two classes: with pre_iters = 1 the second colour launch is the pre-smoothing's last (it carries the residual) and the head
    stays the first colour launch; with pre_iters = 2 it is a plain launch and the head is folded."""
    P = problems.synthetic_problem(("chain", 4000), [4000, 1000, 100], kind="smoothing", d=3)
    for pre in (1, 2):
        _, classes = _check(cabi, P, P.rhs, eligible=pre >= 2, pre_iters=pre, stop_types=(2,), reorder_fine=0, block_fine=0)
        assert (classes > 0).sum() == 2


INELIGIBLE = {
    "graph": lambda cabi: dict(use_graph=True),
    "fp32-inner": lambda cabi: dict(inner_precision=1),
    "jacobi": lambda cabi: dict(smoother=cabi.SMOOTHER_JACOBI),
    "chebyshev": lambda cabi: dict(smoother=cabi.SMOOTHER_CHEBYSHEV),
    "blocked-level-0": lambda cabi: dict(block_from_level=0, gs_omega=1.0),
    "accelerate-2": lambda cabi: dict(accelerate=2),
    "no-speculation": lambda cabi: dict(speculate_head=0),
}


@pytest.mark.parametrize("variant", list(INELIGIBLE))
def test_ineligible_configurations_run_the_parents_launches(cabi, variant):
    P = _torus(3)
    _check(cabi, P, P.rhs, eligible=False, stop_types=(2,), solve_is_cycles=variant != "accelerate-2", **INELIGIBLE[variant](cabi))
