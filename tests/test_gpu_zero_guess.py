"""gmg_config::zero_guess_step on a real device: the first step of a pointwise smoother on a zero guess as x = c (b / diag) -- a streaming launch
(kernels.hip.hpp::pointwise_zero_step) or part of the restriction's launch (transfer<.., STEP0>) -- instead of a memset and a generic step.

Every comparison is against a handle of the same configuration with the field at 0 and is `np.array_equal` on the values: the zero step evaluates
what the generic step evaluates on a zero iterate (0 + v, b - 0: exact), so the only difference the algebra allows is the sign of a zero, which
array_equal does not see.  The counters "zero_guess_steps" / "restrict_steps_fused" are held to what the launch rule
(engine_cycle.hip.hpp::restrict_step0_ok, level0_zero_guess) predicts, per cycle with pre_iters >= 1 on a hierarchy of L prolongations:

    restrictions that compute the step   L - 1 with d <= 4 (levels 1 .. L - 1 are smoothed; the coarsest is not), 0 with more columns
    separate zero steps                  the levels 1 .. L - 1 that got none from the restriction, + 1 for level 0 where the engine supplies
                                         the zero guess (the fp32 inner cycle, the preconditioner application of pcg = 1)

Level sizes are those of tests/test_gpu_boundary_shapes.py's kind: n = 65 (n_pad 128: a last slice with one real row), n_pad = 64 (one slice),
a level 0 that is no multiple of 64, d = 5 (two column chunks)."""
import functools

import numpy as np
import pytest

from tests import problems
from tests.pcg_model import pcg_loop
from tests.test_gpu_accelerate import MODEL_TOL

pytestmark = pytest.mark.gpu

JACOBI, CHEBYSHEV = 1, 2
SMOOTHERS = {"jacobi": JACOBI, "chebyshev": CHEBYSHEV}
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _problem(name):
    if name == "deep":            # L = 4: smoothed levels of 1 023 (n_pad 1 024), 257 (320), 65 (128: last slice one real row), 40 (64: one slice)
        return problems.synthetic_problem(("grid", 33, 31), [1023, 257, 65, 40, 9], kind="poisson", prolong=("smooth",), d=8)
    if name == "flat":            # L = 1: the only coarse level is the coarsest -- no step there
        return problems.synthetic_problem(("grid", 13, 11), [143, 30], kind="poisson", prolong=("smooth",), d=8)
    if name == "torus":           # tests/test_gpu_pcg.py's system (1 073 rows)
        return problems.torus_problem(n1=37, n2=29, lower_bound=60)
    raise ValueError(name)


def _engine(cabi, P, **kw):
    eng = cabi.Engine(**kw)
    eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
    return eng


@functools.lru_cache(maxsize=None)
def _cached(name, zgs, cfg=()):
    from gravo_mg_amd import cabi
    return _engine(cabi, _problem(name), zero_guess_step=zgs, **dict(cfg))


def _vals(rng, n, d):
    return np.asfortranarray(rng.standard_normal((n, d)))


def _counters(eng):
    return eng.timing("zero_guess_steps"), eng.timing("restrict_steps_fused")


def _same(a, b):
    return all(np.array_equal(np.asarray(u), np.asarray(v)) for u, v in zip(a, b))


# ---- the operator-level hook: gmg_smooth_residual(from_zero = 1) ----------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 3, 4, 5])
@pytest.mark.parametrize("iters", [1, 2, 3, 5])
@pytest.mark.parametrize("smoother", sorted(SMOOTHERS))
def test_smooth_residual_from_zero_on_every_level(cabi, smoother, iters, d):
    cfg = (("smoother", SMOOTHERS[smoother]),)
    on, off = _cached("deep", 1, cfg), _cached("deep", 0, cfg)
    assert [on.level_info(k)["n_pad"] for k in range(4)] == [1024, 320, 128, 64] and on.level_info(2)["n"] == 65
    rng = np.random.default_rng(1000 * iters + d)
    for k in range(4):
        b = _vals(rng, on.level_info(k)["n"], d)
        z0, f0 = _counters(on)
        got, want = on.smooth_residual(k, b, None, iters, from_zero=True), off.smooth_residual(k, b, None, iters, from_zero=True)
        assert _same(got, want), (smoother, iters, d, k)
        assert _counters(on) == (z0 + 1, f0)                         # one zero step, whatever the column chunks; no restriction here
        # ... and from a caller's iterate nothing changes: no zero step
        x = _vals(rng, b.shape[0], d)
        assert _same(on.smooth_residual(k, b, x, iters), off.smooth_residual(k, b, x, iters)) and _counters(on) == (z0 + 1, f0)
    assert _counters(off) == (0, 0)


@pytest.mark.parametrize("d", [1, 3, 5])
@pytest.mark.parametrize("smoother", sorted(SMOOTHERS))
def test_fp32_twins_from_zero_on_every_level(cabi, smoother, d):
    """The fp32 instantiations: the smoothing from zero of each level, and the way down between two levels (the restriction computes the step
    where d <= 4, the separate launch runs with d = 5) -- gmg_debug_f32_op."""
    cfg = (("smoother", SMOOTHERS[smoother]), ("inner_precision", 1))
    on, off = _cached("deep", 1, cfg), _cached("deep", 0, cfg)
    rng = np.random.default_rng(77 + d)
    for iters in (1, 2, 3):
        for k in range(4):
            b = _vals(rng, on.level_info(k)["n"], d).astype(np.float32).astype(np.float64)
            assert _same(on.smooth_residual_f32(k, b, None, iters, from_zero=True), off.smooth_residual_f32(k, b, None, iters, from_zero=True)), (iters, k)
        for k in range(3):
            r = _vals(rng, on.level_info(k)["n"], d).astype(np.float32).astype(np.float64)
            z0, f0 = _counters(on)
            assert _same(on.restrict_sweeps_f32(k, r, iters), off.restrict_sweeps_f32(k, r, iters)), (iters, k)
            assert _counters(on) == ((z0, f0 + 1) if d <= 4 else (z0 + 1, f0))
    assert _counters(off) == (0, 0)


# ---- gmg_vcycle from a random x ---------------------------------------------------------------------------------------------------

SWEEPS = [(1, 1), (2, 2), (3, 3), (2, 1), (0, 2)]


@pytest.mark.parametrize("name", ["flat", "deep"])
@pytest.mark.parametrize("sweeps", SWEEPS, ids=[f"{a}+{b}" for a, b in SWEEPS])
@pytest.mark.parametrize("smoother", sorted(SMOOTHERS))
def test_vcycle_bits_and_counters(cabi, smoother, sweeps, name):
    """Both restriction layouts (block_lanes 1 / 4), with and without the output-row map (restrict_sigma 64 / 0), column-major and interleaved
    level-0 residual (d = 1 / 3), two column chunks (d = 5), fp64 and the fp32 inner cycle."""
    P = _problem(name)
    L = len(P.U)
    rng = np.random.default_rng(5)
    for sigma in (0, 64):
        for lanes in (1, 4):
            for inner in (0, 1):
                kw = dict(smoother=SMOOTHERS[smoother], pre_iters=sweeps[0], post_iters=sweeps[1], restrict_sigma=sigma, block_lanes=lanes, inner_precision=inner)
                on, off = _engine(cabi, P, zero_guess_step=1, **kw), _engine(cabi, P, zero_guess_step=0, **kw)
                try:
                    for d in (1, 3, 5):
                        b, x = np.asfortranarray(P.rhs[:, :d]), _vals(rng, P.n, d)
                        z0, f0 = _counters(on)
                        assert np.array_equal(on.vcycle(b, x), off.vcycle(b, x)), (kw, d)
                        fused = (L - 1) if (sweeps[0] >= 1 and d <= 4) else 0
                        separate = ((L - 1) - fused + (1 if inner else 0)) if sweeps[0] >= 1 else 0
                        assert _counters(on) == (z0 + separate, f0 + fused), (kw, d)
                    assert _counters(off) == (0, 0)
                finally:
                    on.close(); off.close()


def test_multicolour_handle_accepts_the_field_without_effect(cabi):
    P = _problem("deep")
    on, off = _engine(cabi, P, zero_guess_step=1), _engine(cabi, P)
    b = np.asfortranarray(P.rhs[:, :3])
    assert np.array_equal(on.vcycle(b, b), off.vcycle(b, b)) and _counters(on) == (0, 0)
    on.close(); off.close()


# ---- the preconditioned CG loop: level 0 starts from zero too, pcg_direction writes no zeros --------------------------------------------

def _solve_tuple(eng, rhs, **kw):
    x, it, res, conv = eng.solve(rhs, **kw)
    return x, it, res, conv[:, 1].copy(), eng.timing("pcg_guard_steps"), eng.timing("pcg_restarts"), eng.timing("pcg_confirmations")


def _same_solve(a, b):
    return a[1] == b[1] and a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3]) and a[4:] == b[4:]


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("smoother", sorted(SMOOTHERS))
def test_pcg_solve_is_that_of_the_field_at_zero_and_follows_the_model(cabi, smoother, d):
    """Eight iterations (tol = 0) and a solve to 1e-9 on the torus system of tests/test_gpu_pcg.py: iterate, residue history, iteration count,
    guard and restart counts of the zero_guess_step = 0 handle; and the numpy model of the loop (tests/pcg_model.py, the cycle of a pcg = 0
    handle) at that file's MODEL_TOL."""
    cfg = (("smoother", SMOOTHERS[smoother]), ("pcg", 1))
    P = _problem("torus")
    rhs = np.asfortranarray(P.mass[:, None] * np.random.default_rng(300 + d).standard_normal((P.n, d)))
    on, off = _cached("torus", 1, cfg), _cached("torus", 0, cfg)
    z0, f0 = _counters(on)
    a, b = _solve_tuple(on, rhs, tol=0.0, stop_type=2, max_iter=8), _solve_tuple(off, rhs, tol=0.0, stop_type=2, max_iter=8)
    assert _same_solve(a, b) and a[1] == 8
    L = len(P.U)
    assert _counters(on) == (z0 + 8, f0 + 8 * (L - 1)) and _counters(off) == (0, 0)      # level 0's step per application; the coarse ones ride on the restrictions
    assert _same_solve(_solve_tuple(on, rhs, tol=1e-9, stop_type=2, max_iter=40), _solve_tuple(off, rhs, tol=1e-9, stop_type=2, max_iter=40))
    plain = _cached("torus", 0, (("smoother", SMOOTHERS[smoother]),))
    mx, mit, mres, mguards, mrestarts = pcg_loop(P.lhs, P.mass, plain.vcycle, rhs, rhs, 2, 0.0, 8)[:5]
    rel = lambda g, w: float(np.max(np.abs(np.asarray(g) - np.asarray(w))) / np.max(np.abs(np.asarray(w))))
    dev_res, dev_x = rel(a[3], mres), rel(a[0].reshape(rhs.shape), mx)
    print(f"ZGS_PCG {smoother} d={d}: residues {dev_res:.3e} x {dev_x:.3e} against the model")
    assert mit == 8 and a[4] == mguards == 0 and a[5] == mrestarts == 0
    assert dev_res <= MODEL_TOL and dev_x <= MODEL_TOL


@pytest.mark.parametrize("d", [1, 5])
@pytest.mark.parametrize("n", [1, 2, 65])
def test_pcg_guarded_columns_leave_nothing_stale(cabi, n, d):
    """A 1-row system: the first iteration solves it exactly and every later one takes the guard in every column (a negative
    tolerance makes all 25 iterations run).  pcg_direction writes no zeros any more, the guard keeps x and r: the iterate is that of the field at
    0, finite, and the residue is that of the iterate returned."""
    P = problems.synthetic_problem(graph=("chain", n), sizes=[n, max(1, n // 4)], kind="poisson", prolong=("pc",), d=d)
    rhs = np.asfortranarray(P.rhs)
    kw = dict(smoother=CHEBYSHEV, pcg=1)
    on, off = _engine(cabi, P, zero_guess_step=1, **kw), _engine(cabi, P, zero_guess_step=0, **kw)
    try:
        for tol, max_iter in ((1e-12, 25), (-1.0, 25)):
            a, b = _solve_tuple(on, rhs, tol=tol, stop_type=2, max_iter=max_iter), _solve_tuple(off, rhs, tol=tol, stop_type=2, max_iter=max_iter)
            print(f"ZGS_GUARD chain{n} d={d} tol={tol}: {a[1]} iterations, residue {a[2]:.3e}, guards {a[4]:.0f}, restarts {a[5]:.0f}")
            assert _same_solve(a, b) and np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[3]))
            assert a[2] == on.residual_norm(rhs, a[0], 2)
        assert a[1] == 25
        if n == 1:
            assert a[4] >= 24 * d and a[2] <= 1e-15
    finally:
        on.close(); off.close()


def test_pcg_other_paths(cabi):
    """use_graph = 1 against stream launches; gmg_solve_device against gmg_solve; two runs; a values-only refresh against a fresh handle; d = 5
    then d = 1 on one handle."""
    torch = pytest.importorskip("torch")
    P = _problem("torus")
    rhs = np.asfortranarray(P.mass[:, None] * np.random.default_rng(9).standard_normal((P.n, 3)))
    kw = dict(tol=1e-9, stop_type=2, max_iter=7)
    ref = _solve_tuple(_cached("torus", 0, (("smoother", CHEBYSHEV), ("pcg", 1))), rhs, **kw)
    on = _cached("torus", 1, (("smoother", CHEBYSHEV), ("pcg", 1)))
    first, second = _solve_tuple(on, rhs, **kw), _solve_tuple(on, rhs, **kw)
    assert _same_solve(first, ref) and _same_solve(second, ref)
    graph = _cached("torus", 1, (("smoother", CHEBYSHEV), ("pcg", 1), ("use_graph", True)))
    assert _same_solve(_solve_tuple(graph, rhs, **kw), ref) and _same_solve(_solve_tuple(graph, rhs, **kw), ref)
    n, d = rhs.shape
    b = torch.tensor(np.ascontiguousarray(rhs), device=DEV)
    x = torch.full((n, d), float("nan"), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    it, res, conv = on.solve_device(b.data_ptr(), b.stride(), x.data_ptr(), x.stride(), d, **kw)
    assert it == ref[1] and res == ref[2] and np.array_equal(conv[:, 1], ref[3]) and np.array_equal(x.cpu().numpy(), ref[0].reshape(rhs.shape))
    # other column counts on the same handle (the loop's vectors are re-sized; d = 5: the separate zero steps on every level)
    for dd in (5, 1):
        r = np.asfortranarray(P.mass[:, None] * np.random.default_rng(20 + dd).standard_normal((P.n, dd)))
        assert _same_solve(_solve_tuple(on, r, **kw), _solve_tuple(_cached("torus", 0, (("smoother", CHEBYSHEV), ("pcg", 1))), r, **kw))
    # a values-only refresh, then a solve: a fresh handle's bits
    lhs2 = (P.lhs * 3.0).tocsc()
    lhs2.sort_indices()
    live = _engine(cabi, P, zero_guess_step=1, smoother=CHEBYSHEV, pcg=1)
    live.solve(rhs, **kw)
    live.set_system(lhs2)
    assert live.timing("setup_values_only") == 1
    fresh_on = cabi.Engine(zero_guess_step=1, smoother=CHEBYSHEV, pcg=1)
    fresh_off = cabi.Engine(zero_guess_step=0, smoother=CHEBYSHEV, pcg=1)
    for e in (fresh_on, fresh_off):
        e.set_prolongations(P.U); e.set_mass(P.mass); e.set_system(lhs2)
    got = _solve_tuple(live, rhs, **kw)
    assert _same_solve(got, _solve_tuple(fresh_on, rhs, **kw)) and _same_solve(got, _solve_tuple(fresh_off, rhs, **kw))
    for e in (live, fresh_on, fresh_off):
        e.close()


@pytest.mark.parametrize("cfg", [(), (("use_graph", True),)], ids=["stream", "graph"])
def test_cycles_outside_the_solve_on_a_pcg_handle(cabi, cfg):
    """gmg_vcycle / gmg_run_cycles start level 0 from the caller's iterate: after a PCG solve (whose cycles started from zero, under their own
    graphs) they give the bits of a pcg = 0, zero_guess_step = 0 handle."""
    P = _problem("torus")
    rhs = np.asfortranarray(P.mass[:, None] * np.random.default_rng(4).standard_normal((P.n, 3)))
    out = []
    for pcg, zgs in ((0, 0), (1, 1)):
        eng = _cached("torus", zgs, (("smoother", CHEBYSHEV), ("pcg", pcg)) + cfg)
        eng.solve(rhs, tol=0.0, stop_type=2, max_iter=3)
        v = eng.vcycle(rhs, rhs)
        eng.load_problem(rhs, rhs)
        res = eng.run_cycles(4, 2)
        out.append((v, res, eng.fetch_solution()))
        eng.solve(rhs, tol=0.0, stop_type=2, max_iter=3)
    assert _same(out[0], out[1])


# ---- the other solve loops and paths on a pcg = 0 handle ------------------------------------------------------------------------------

@pytest.mark.parametrize("more", [(), (("accelerate", 3),), (("inner_precision", 1),), (("use_graph", True),), (("use_graph", True), ("inner_precision", 1)),
                                  (("coarse_mode", 0),)], ids=["plain", "accelerate3", "mixed", "graph", "graph-mixed", "host-coarse"])
def test_solve_loops_give_the_bits_of_the_field_at_zero(cabi, more):
    P = _problem("deep")
    cfg = (("smoother", CHEBYSHEV),) + more
    on, off = _cached("deep", 1, cfg), _cached("deep", 0, cfg)
    for d in (3, 5):
        rhs = np.asfortranarray(P.rhs[:, :d])
        for _ in range(2):                                           # (two runs: a replayed graph, re-used vectors)
            a, b = on.solve(rhs, tol=1e-8, stop_type=2, max_iter=6), off.solve(rhs, tol=1e-8, stop_type=2, max_iter=6)
            assert a[1] == b[1] and a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[3][:, 1], b[3][:, 1]), (more, d)
    assert _counters(on)[0] + _counters(on)[1] > 0 and _counters(off) == (0, 0)
