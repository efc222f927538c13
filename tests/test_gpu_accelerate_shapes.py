"""gmg_config::accelerate on a real device at the shapes where its kernels and launches switch branches (accel_kernels.hip.hpp,
engine_cycle.hip.hpp::launch_accel_step / ensure_accel): a level 0 smaller than one 256-thread block and smaller than one 64-row slice, one
partial block, two and three blocks, every width of a column group (d = 1 .. 8: the DC = 1 .. 4 instantiations with stored directions, a full
second group and its offsets into alpha, guarded, beta and the stored s_j), a guarded column in the second group, a second trip of the
grid-stride loop, re-sizing on a live handle, graph replay and device-resident vectors.

Reference: tests/accelerate_model.accelerated_loop with `vcycle` of a second handle created with accelerate = 0 as its cycle -- the recombination is
the only difference.  Over the leading iterations whose model residue stays at or above FLOOR_REL = 1e-9 of the first one, residues are compared
relative to the first residue and x (the result of a solve cut at that count) relative to max |x|, both to SHAPE_TOL = 3.7e-11 = 100 x the
largest change one rounding per cycle output makes in the model over this catalogue (3.63e-13: tests/test_accelerate_model_host.py has the
figures per family and the floor table).  diagonal100 reaches its floor in two iterations and is compared in its first one (relative to the
initial residue, which is what the first step's rounding scales with).

Shapes of fewer than 5 unknowns (chain1, chain2, diagonal1, the 2 x 2 grid) exhaust their Krylov space within the window: like diagonal100 they
are compared in their first iteration, and every later reported residue is finite and does not grow until the floor.  Past the floor
(test_past_the_floor, every shape): the floor guard of accel_scalars.hpp keeps the iterate there -- `best` of the required property is the
residue the solve returns wherever the history holds one confirmed residue (tol below the floor: the last one), so what holds the device is:
finite, a status no worse than the plain loop's, the bound, and at most 10 x the plain loop's residue after the same count.

Measured on an MI355X (largest deviation per family over the covering selection, residues / x; the tests print them as ACCEL_SHAPE lines):
  chain63 .. 193-L1 (Poisson), three smoothers        2.6e-14 / 1.1e-14
  chain63 .. 1025-L2, chain193-L3, chain129-coarsest1   4.3e-15 / 4.1e-16
  isolated40x40 1.0e-15 / 2.1e-16     hub48x40 2.0e-13 / 7.8e-14     clique65 (blocked or not) 2.3e-15 / 5.4e-16
  diagonal100, first iteration                         1.5e-17 / 8.8e-16
  chain of 1 100 000 rows (second grid-stride trip)    7.4e-15 / 4.7e-16, 1.3 s with its set-up: it stays in this file
all under SHAPE_TOL = 3.7e-11; hub48x40 is the case that sets it in the model as well (3.6e-13 x 100)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests import problems
from tests.accelerate_model import (FLOOR_REL, NONINCREASING, SHAPE_TOL, above_floor, accelerated_loop, chain_n_pad, norm,
                                    shape_catalogue, weights)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES, EARLY, TINY = shape_catalogue()
SPEC = {c[0]: (c[1], c[2]) for c in CASES + EARLY + TINY}
SMOOTHERS = ("default", "jacobi", "chebyshev")
# the covering selection: (d, m, stop type) -- every d with m = 4, every m with d = 5, every stop type with d = 3, m = 2
SELECTION = [(d, 4, 2) for d in range(1, 9)] + [(5, m, 2) for m in (1, 2, 3)] + [(3, 2, t) for t in (0, 1, 3)]
BLOCKS = {"chain513-L2": 2, "chain1025-L2": 3}          # 256-thread blocks of row pairs on level 0
TINY_FLOOR = 1e-13


@functools.lru_cache(maxsize=None)
def _problem(name):
    return problems.synthetic_problem(**SPEC[name][0])


def _rhs(P, d, seed=300):
    return np.asfortranarray(P.mass[:, None] * np.random.default_rng(seed + d).standard_normal((P.n, d)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _smoother_kw(cabi, smoother):
    return {"default": {}, "jacobi": dict(smoother=cabi.SMOOTHER_JACOBI), "chebyshev": dict(smoother=cabi.SMOOTHER_CHEBYSHEV)}[smoother]


def _engine(cabi, P, **kw):
    eng = cabi.Engine(**kw)
    eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
    return eng


class Shape:
    """One problem with one smoother: engines by depth (0: the plain handle whose vcycle is the model's cycle), made on demand, closed together."""

    def __init__(self, cabi, name, smoother):
        self.cabi, self.name, self.smoother, self.P = cabi, name, smoother, _problem(name)
        self.kw = dict(SPEC[name][1], **_smoother_kw(cabi, smoother))
        self.engines = {}

    def eng(self, m, **kw):
        key = (m,) + tuple(sorted(kw.items()))
        if key not in self.engines:
            self.engines[key] = _engine(self.cabi, self.P, accelerate=m, **dict(self.kw, **kw))
        return self.engines[key]

    def model(self, rhs, x0, m, stop_type, tol, max_iter):
        return accelerated_loop(self.P.lhs, self.P.mass, self.eng(0).vcycle, rhs, x0, m, stop_type, tol, max_iter, keep_vectors=True)

    def close(self):
        for e in self.engines.values():
            e.close()
        self.engines = {}


def _shapes(names):
    """default smoother everywhere, Jacobi and Chebyshev on the chains"""
    return [(n, s) for n in names for s in SMOOTHERS if s == "default" or n.startswith("chain")]


def _fixture(params):
    @pytest.fixture(scope="module", params=params, ids=["%s-%s" % p for p in params])
    def fx(request, cabi):
        assert cabi.device_count() > 0, "gpu tests need a HIP device"
        s = Shape(cabi, *request.param)
        yield s
        s.close()
    return fx


shape = _fixture(_shapes([c[0] for c in CASES]))
early = _fixture(_shapes([c[0] for c in EARLY + TINY]))
floor_shape = _fixture([(c[0], s) for c in CASES + EARLY + TINY for s in SMOOTHERS])


def _rel(a, b, scale=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) if scale is None else scale))


def _check_n_pad(s):
    info = s.eng(0).level_info(0)
    n = s.P.n
    assert info["n"] == n and info["n_pad"] % 64 == 0 and info["n_pad"] >= n
    if s.name.startswith("chain") and s.smoother == "default":
        assert info["n_pad"] == chain_n_pad(n), info                       # two colour classes, each padded to 64 rows
    if s.name.startswith("chain") and n <= 193:
        assert info["n_pad"] <= 256                                        # one partial block of row pairs
    if s.name in BLOCKS:
        assert -(-(info["n_pad"] // 2) // 256) == BLOCKS[s.name] and (info["n_pad"] // 2) % 256 != 0, info
    return info["n_pad"]


def test_iterations_follow_the_model(shape):
    """tol = 0, max_iter = 8 over the covering selection: the residue history over the iterations above the floor and the x of a solve cut there
    agree with the model to SHAPE_TOL; those residues do not grow; at least 3 of the 8 iterations are compared."""
    s = shape
    n_pad = _check_n_pad(s)
    worst_r = worst_x = 0.0
    for d, m, t in SELECTION:
        rhs = _rhs(s.P, d)
        x, it, res, conv = s.eng(m).solve(rhs, tol=0.0, stop_type=t, max_iter=8)
        mx, mit, mres, mguards, steps = s.model(rhs, rhs, m, t, 0.0, 8)
        k = above_floor(mres)
        assert it == mit == 8 and k >= 3, (s.name, d, m, t, it, mres)
        assert not any(st["guarded"].any() for st in steps[:k])          # (no guard above the floor; on it the floor guard may act)
        if k < 8:
            x = s.eng(m).solve(rhs, tol=0.0, stop_type=t, max_iter=k)[0]
            mx = steps[k]["xk"]                                              # (the iterate does not depend on where the loop is cut)
        dev_r, dev_x = _rel(conv[:k, 1], mres[:k], scale=mres[0]), _rel(x.reshape(rhs.shape), mx)
        worst_r, worst_x = max(worst_r, dev_r), max(worst_x, dev_x)
        print("   d=%d m=%d type=%d: %d compared, residues %.2e x %.2e (first %.3e, last compared %.3e)" % (d, m, t, k, dev_r, dev_x, mres[0], mres[k - 1]))
        assert np.all(np.isfinite(conv[:, 1])) and np.all(conv[1:k, 1] <= conv[:k - 1, 1] * NONINCREASING), (s.name, d, m, t, conv[:, 1])
        assert dev_r <= SHAPE_TOL and dev_x <= SHAPE_TOL, (s.name, d, m, t, dev_r, dev_x)
    print("ACCEL_SHAPE %s %s n_pad=%d: residues %.2e x %.2e" % (s.name, s.smoother, n_pad, worst_r, worst_x))


def test_first_iteration_where_the_floor_comes_early(early):
    """diagonal100 and the shapes of 1, 2 and 4 unknowns (fewer than 3 of 8 iterations above the floor: not compared beyond the first): the first iteration agrees with the model to
    SHAPE_TOL relative to the initial residue, every reported residue is finite, and they do not grow until the floor."""
    s = early
    _check_n_pad(s)
    for d, m, t in SELECTION:
        rhs = _rhs(s.P, d)
        w = weights(s.P.mass, t)
        r0 = rhs - s.P.lhs @ rhs
        scale = norm((w * r0 * r0).sum(axis=0), (w * rhs * rhs).sum(axis=0), t)
        x1, it1, res1, conv1 = s.eng(m).solve(rhs, tol=0.0, stop_type=t, max_iter=1)
        mx1, _, mres1, _, _ = s.model(rhs, rhs, m, t, 0.0, 1)
        dev_r, dev_x = abs(res1 - mres1[0]) / scale, _rel(x1.reshape(rhs.shape), mx1)
        print("ACCEL_SHAPE %s %s d=%d m=%d type=%d first iteration: residue %.2e x %.2e" % (s.name, s.smoother, d, m, t, dev_r, dev_x))
        assert it1 == 1 and dev_r <= SHAPE_TOL and dev_x <= SHAPE_TOL
        _, it, res, conv = s.eng(m).solve(rhs, tol=0.0, stop_type=t, max_iter=8)
        h = conv[:it, 1]          # (a system of one unknown can reach a residue of exactly 0, which ends the loop)
        assert 1 <= it <= 8 and np.all(np.isfinite(h)) and np.isfinite(res), h
        k = 0
        while k < it and h[k] >= max(FLOOR_REL * h[0], TINY_FLOOR):
            k += 1
        assert np.all(h[1:k] <= h[:max(k, 1) - 1] * NONINCREASING), h


def test_five_unknowns(cabi):
    """chain5 of tests/test_gpu_boundary_shapes.py, one unknown more than the window holds directions: solved to 1e-12 in no more iterations than
    the plain loop needs."""
    from tests.test_gpu_boundary_shapes import CASES as BOUNDARY
    for name in ("A-chain5-L1", "A-chain5-L2"):
        (spec,) = [c[1] for c in BOUNDARY if c[0] == name]
        P = problems.synthetic_problem(**spec)
        assert P.n == 5
        rhs = _rhs(P, 3)
        plain, acc = _engine(cabi, P), _engine(cabi, P, accelerate=4)
        try:
            _, pit, pres, _ = plain.solve(rhs, tol=1e-12, stop_type=2, max_iter=100)
            _, it, res, _ = acc.solve(rhs, tol=1e-12, stop_type=2, max_iter=100)
            print(name, "plain", pit, pres, "accelerated", it, res)
            assert res <= 1e-12 and pres <= 1e-12 and it <= pit and not acc.diverged
        finally:
            plain.close(); acc.close()


GUARD_CASES = ("chain65-L2", "chain513-L2")


@pytest.mark.parametrize("name", GUARD_CASES)
def test_guarded_columns_in_both_groups(cabi, name):
    """d = 8, stop type 3, m = 3, six iterations with columns 1 and 6 of rhs and x0 zero (one guarded column per group of 4): those columns stay
    exactly zero, everything is finite, accel_guard_steps is the model's count, the other six columns agree with the model to SHAPE_TOL -- and
    have the bits of the same six columns solved with the zero columns at positions 0 and 7.  Every per-column quantity (alpha, guarded, the
    betas, the stored s_j) then sits in another slot of its group, or in the other group: a scalar read from a neighbour's slot changes bits.
    (The column sums of stop type 3 are added in column order; zeros in other places do not change that sum.)"""
    s = Shape(cabi, name, "default")
    try:
        P = s.P
        live = _rhs(P, 6)
        def spread(zero):
            out = np.zeros((P.n, 8), order="F")
            out[:, [c for c in range(8) if c not in zero]] = live
            return out
        rhs = spread((1, 6))
        x, it, res, conv = s.eng(3).solve(rhs, x0=rhs.copy(), tol=0.0, stop_type=3, max_iter=6)
        x = x.reshape(rhs.shape)
        guards = s.eng(3).timing("accel_guard_steps")
        mx, mit, mres, mguards, _ = s.model(rhs, rhs, 3, 3, 0.0, 6)
        k = above_floor(mres)
        assert np.all(x[:, (1, 6)] == 0.0)
        assert np.all(np.isfinite(x)) and np.all(np.isfinite(conv)) and np.isfinite(res)
        assert it == mit == 6 and guards == mguards == 12
        keep = [0, 2, 3, 4, 5, 7]
        if k == 6:
            dev_r, dev_x = _rel(conv[:, 1], mres, scale=mres[0]), _rel(x[:, keep], mx[:, keep])
            print("ACCEL_SHAPE guard %s: residues %.2e x %.2e" % (name, dev_r, dev_x))
            assert dev_r <= SHAPE_TOL and dev_x <= SHAPE_TOL
        else:
            assert k >= 3 and _rel(conv[:k, 1], mres[:k], scale=mres[0]) <= SHAPE_TOL
        rhs2 = spread((0, 7))
        x2, it2, res2, conv2 = s.eng(3).solve(rhs2, x0=rhs2.copy(), tol=0.0, stop_type=3, max_iter=6)
        x2 = x2.reshape(rhs.shape)
        assert np.all(x2[:, (0, 7)] == 0.0) and s.eng(3).timing("accel_guard_steps") == 12
        print("   moved zero columns: x differs by %.2e, residues by %.2e" % (_rel(x2[:, 1:7], x[:, keep]), _rel(conv2[:, 1], conv[:, 1])))
        assert np.array_equal(_bits(x2[:, 1:7]), _bits(x[:, keep])) and np.array_equal(_bits(conv2[:, 1]), _bits(conv[:, 1]))
    finally:
        s.close()


def _same(a, b):
    return a[1] == b[1] and _bits(a[2]) == _bits(b[2]) and np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[3][:, 1]), _bits(b[3][:, 1]))


def test_a_live_handle_is_resized_and_left_from_nothing(cabi):
    """One accelerated handle (m = 3): d = 3, d = 8, d = 2; a values-only refresh and d = 3; the prolongations, mass and system of a problem with
    another n_pad and d = 3.  Every solve has the bits (x, iteration count, residue history) of a fresh handle doing only that solve: ensure_accel
    re-sizes for the new width and the new n_pad, and nothing of an earlier solve's ring or stored s_j is read."""
    P, Q = _problem("chain193-L2"), _problem("chain513-L2")
    lhs2 = (P.lhs + sp.diags(P.lhs.diagonal())).tocsc()
    lhs2.sort_indices()
    kw = dict(tol=1e-13, stop_type=2, max_iter=7)

    def fresh(problem, lhs, d):
        e = cabi.Engine(accelerate=3)
        try:
            e.set_prolongations(problem.U); e.set_mass(problem.mass); e.set_system(lhs)
            return e.solve(_rhs(problem, d), **kw), e.level_info(0)["n_pad"]
        finally:
            e.close()

    eng = _engine(cabi, P, accelerate=3)
    try:
        for d in (3, 8, 2):
            assert _same(eng.solve(_rhs(P, d), **kw), fresh(P, P.lhs, d)[0]), d
        eng.set_system(lhs2)
        want, pad_p = fresh(P, lhs2, 3)
        assert _same(eng.solve(_rhs(P, 3), **kw), want)
        eng.set_prolongations(Q.U); eng.set_mass(Q.mass); eng.set_system(Q.lhs)
        want, pad_q = fresh(Q, Q.lhs, 3)
        assert pad_q != pad_p and eng.level_info(0)["n_pad"] == pad_q
        assert _same(eng.solve(_rhs(Q, 3), **kw), want)
        # ... and back to the wide one on the new system (the scalars are laid out by the handle's width: alpha, guarded, 3 betas, 3 s_j per column)
        assert _same(eng.solve(_rhs(Q, 8), **kw), fresh(Q, Q.lhs, 8)[0])
    finally:
        eng.close()


def test_graph_replay_and_device_vectors_give_the_same_bits(cabi):
    """chain193-L2, d = 8, m = 3: use_graph = 1 and gmg_solve_device (torch tensors) against the stream launches from host arrays."""
    torch = pytest.importorskip("torch")
    P = _problem("chain193-L2")
    rhs = _rhs(P, 8)
    kw = dict(tol=1e-13, stop_type=2, max_iter=8)
    s, g = _engine(cabi, P, accelerate=3), _engine(cabi, P, accelerate=3, use_graph=True)
    try:
        a = s.solve(rhs, **kw)
        assert _same(g.solve(rhs, **kw), a)
        n, d = rhs.shape
        b = torch.tensor(np.ascontiguousarray(rhs), device=DEV)
        x = torch.full((n, d), float("nan"), dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        it, res, conv = s.solve_device(b.data_ptr(), b.stride(), x.data_ptr(), x.stride(), d, **kw)
        assert it == a[1] and _bits(res) == _bits(a[2]) and np.array_equal(_bits(conv[:, 1]), _bits(a[3][:, 1]))
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(np.ascontiguousarray(a[0].reshape(rhs.shape))))
    finally:
        s.close(); g.close()


def test_second_trip_of_the_grid_stride_loop(cabi):
    """A chain of 1 100 000 rows (n_pad / 2 = 550 016 row pairs, more than the 2 048 x 256 one trip covers), aggregation, d = 5, m = 2, stop type 2,
    four iterations against the model."""
    import time
    n = 1100000
    t0 = time.time()
    P = problems.synthetic_problem(graph=("chain", n), sizes=[n, n // 64, n // 4096], kind="smoothing", prolong=("pc",))
    rhs = _rhs(P, 5)
    plain, acc = _engine(cabi, P), _engine(cabi, P, accelerate=2)
    try:
        n_pad = acc.level_info(0)["n_pad"]
        assert n_pad == chain_n_pad(n) and n_pad // 2 > 2048 * 256
        t1 = time.time()
        x, it, res, conv = acc.solve(rhs, tol=0.0, stop_type=2, max_iter=4)
        mx, mit, mres, mguards, _ = accelerated_loop(P.lhs, P.mass, plain.vcycle, rhs, rhs, 2, 2, 0.0, 4)
        dev_r, dev_x = _rel(conv[:, 1], mres, scale=mres[0]), _rel(x.reshape(rhs.shape), mx)
        print("ACCEL_SHAPE chain1100000 n_pad=%d: residues %.2e x %.2e, history %s; set-up %.1f s, solve + model %.1f s"
              % (n_pad, dev_r, dev_x, conv[:, 1], t1 - t0, time.time() - t1))
        assert it == mit == 4 and above_floor(mres) == 4 and mguards == 0
        assert dev_r <= SHAPE_TOL and dev_x <= SHAPE_TOL
    finally:
        plain.close(); acc.close()


def test_past_the_floor(floor_shape):
    """tol = 1e-17 and tol = 0 with max_iter = 25, m = 1..4, d in {1, 3, 8}, stop types 0, 2, 3, all three smoothers: the returned residue and x
    are finite, the residue is at most 10 x max(the plain loop's after the same count, the smallest confirmed residue of the history), and the
    status is no worse than the plain loop's (module docstring on `best`)."""
    s = floor_shape
    worst = 0.0
    for d in (1, 3, 8):
        rhs = _rhs(s.P, d)
        for t in (0, 2, 3):
            for tol in (1e-17, 0.0):
                _, pit, plain, _ = s.eng(0).solve(rhs, tol=tol, stop_type=t, max_iter=25)
                plain_diverged = s.eng(0).diverged
                for m in (1, 2, 3, 4):
                    x, it, res, conv = s.eng(m).solve(rhs, tol=tol, stop_type=t, max_iter=25)
                    best = res if s.eng(m).timing("accel_confirmations") == 1 else min(res, conv[it - 1, 1])
                    worst = max(worst, res / plain if plain > 0 else 0.0)
                    assert np.all(np.isfinite(x)) and np.isfinite(res), (s.name, s.smoother, d, t, tol, m, res)
                    assert res <= 10.0 * max(plain, best), (s.name, s.smoother, d, t, tol, m, res, plain)
                    # (1e-14 |b|: both solved the system as far as it can be)
                    assert res <= 10.0 * plain or res <= 1e-14 * (np.linalg.norm(rhs) if t == 3 else 1.0), (s.name, s.smoother, d, t, tol, m, res, plain)
                    assert plain_diverged or not s.eng(m).diverged, (s.name, s.smoother, d, t, tol, m, res, plain, conv[:it, 1])
    print("ACCEL_SHAPE floor %s %s: returned / plain at most %.2e" % (s.name, s.smoother, worst))
