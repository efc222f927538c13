"""GMG_SMOOTHER_CHEBYSHEV on a real device, against tests/chebyshev_model.ChebyshevModel (the oracle's operators, the recurrence in numpy).

Shapes are those of tests/test_gpu_boundary_shapes.py (same specs through tests/problems.synthetic_problem): levels smaller than one 64-row
slice and at slice boundaries with 1 .. 8 right-hand sides (column chunks of 4 and the offset of p behind them), rows without off-diagonals,
one very long row, and the torus at its default size (16-bit column codes and uniform slices on level 0).  No test depends on the interval
ratio: it is read from the engine ("cheby_ratio") and handed to the model.

Tolerances: the bound 1e-12 relative (rows have fewer than 1e3 entries, each bound a sum of positive terms: <= 1e3 * 2^-53).  The steps
(_step_close): STEP_TOL = 1e-13 relative to the result, what tests/test_gpu_parity.py holds the device's weighted Jacobi sweep to against the
oracle's residual, plus an absolute floor of 4 roundings per step of the quantities a step works on, 4 k Lambda eps (||x_0|| + ||D^-1 b||) after k
steps.  The floor is there because the steps CONTRACT: the result can be far smaller than the inputs (0.0088 from inputs of size 1 after 3 steps
on the 1 x 1 level 0 of chain1-L2), and a few ulps of the O(1) intermediates -- the device contracts a * b + c into one rounding, numpy does not
-- are then more than 1e-13 of the result (measured there: 1.13e-13, an absolute 1.0e-15 under a floor of 4.8e-15; every other case of the
catalogue measured <= 1.6e-15 relative).  Cycles as
tests/test_gpu_sweep_counts.py holds them (backward 1e-12 ||A|| ||x||, forward 1e-11 for M + S systems and 1e-6 for S + tau M ones, the fp32
inner cycle 2e-5); the energy norm (1 + 1e-12): the model satisfies it on every case and level of this catalogue (none dropped)."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import problems
from tests.chebyshev_model import ChebyshevModel
from tests.parity_checks import rel, timing_or_none

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "gravo_mg_amd", "dropin")
DEV = "cuda:0"

STEP_TOL = 1e-13
BOUND_TOL = 1e-12
D_SLICES, D_FEW = (1, 3, 4, 5, 8), (1, 3)
PAIRS = ((2, 2), (1, 3), (0, 2), (3, 0))


def _catalogue():
    cases = []
    for n in (1, 2, 63, 64, 65, 129, 193):
        cases.append(("chain%d-L1" % n, dict(graph=("chain", n), sizes=[n, max(1, n // 4)], kind="poisson", prolong=("pc",)), D_SLICES, {}))
        cases.append(("chain%d-L2" % n, dict(graph=("chain", n), sizes=[n, max(1, n // 2), max(1, n // 8)], kind="smoothing", prolong=("smooth", "pc")), D_SLICES, {}))
    cases.append(("chain193-L3", dict(graph=("chain", 193), sizes=[193, 96, 24, 6], kind="smoothing", prolong=("smooth", "pc", "pc")), D_SLICES, {}))
    cases.append(("chain129-coarsest1", dict(graph=("chain", 129), sizes=[129, 1], kind="smoothing", prolong=("pc",)), D_SLICES, {}))
    cases.append(("diagonal100", dict(graph=("diagonal", 100), sizes=[100, 25, 6], kind="poisson", prolong=("pc",)), D_FEW, {}))
    cases.append(("isolated40x40", dict(graph=("isolated", 40, 40), sizes=[1600, 400, 100], kind="smoothing", prolong=("smooth", "pc")), D_FEW, {}))
    cases.append(("hub48x40", dict(graph=("hub", 48, 40), sizes=[1921, 480, 120], kind="poisson", prolong=("pc",)), D_FEW, {}))
    n = 65 + 48 * 48
    cases.append(("clique65", dict(graph=("clique", 48, 48, 65), sizes=[n, n // 4, n // 16], kind="smoothing", prolong=("pc",)), D_FEW, dict(block_fine=False)))
    cases.append(("torus", None, D_FEW, {}))
    return cases


CASES = _catalogue()


def _problem(name):
    (spec,) = [c[1] for c in CASES if c[0] == name]
    return problems.torus_problem() if spec is None else problems.synthetic_problem(**spec)


def _engine(cabi, P, **kw):
    eng = cabi.Engine(**kw)
    eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
    return eng


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Case:
    def __init__(self, cabi, oracle, name, P, ds, kw):
        self.cabi, self.oracle, self.name, self.P, self.ds = cabi, oracle, name, P, ds
        self.kw = dict(kw, smoother=cabi.SMOOTHER_CHEBYSHEV)
        self.eng = _engine(cabi, P, **self.kw)
        self.ratio = self.eng.timing("cheby_ratio")
        self.M = ChebyshevModel(None, P.U, P.mass, P.lhs, oracle, self.ratio)          # the reference: computed once, shared, left unchanged
        self.L = len(P.U)
        self.smoothing = "smoothing" in P.name
        self.nA = spla.norm(P.lhs)

    def engine(self, **kw):
        return _engine(self.cabi, self.P, **dict(self.kw, **kw))

    def rhs(self, d):
        return self.P.mass[:, None] * np.random.default_rng(40 + d).standard_normal((self.P.n, d))

    def compatible_rhs(self, d):
        """rhs(d) with the mean of every column taken off: the right-hand sides of the solves to a tolerance.  torus_problem() is the Poisson system
        S + 1e-6 M of a closed surface; a right-hand side with a mean has a solution 1e6 times its size along the constant vector, and b - A x
        evaluated in fp64 then carries eps |A| |x| = a few 1e-8 of ||b|| (the floor tests/test_gpu_accelerate.py describes for these systems;
        measured here with rhs(3): 3.5e-8 after 100 cycles, plain and accelerated alike), above the 1e-8 these tests solve to.  A compatible
        (mean-free) right-hand side is the one such a problem is posed with, and its solution is of the size of the data.  The same on both problems."""
        b = self.rhs(d)
        return b - b.mean(axis=0)


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request, cabi, oracle):
    name, spec, ds, kw = request.param
    assert cabi.device_count() > 0, "gpu tests need a HIP device"
    c = Case(cabi, oracle, name, _problem(name), ds, kw)
    yield c
    c.eng.close()


def _step_close(M, k, b, x, iters, got, want):
    """||got - want|| <= STEP_TOL ||want|| + 4 iters Lambda_k eps (||x|| + ||D^-1 b||) (module docstring); returns the deviation relative to the result."""
    dg = M.diag[k][:, None] if np.ndim(b) == 2 else M.diag[k]
    floor = 4 * iters * M.lam[k] * np.finfo(np.float64).eps * (np.linalg.norm(x) + np.linalg.norm(b / dg))
    dev = np.linalg.norm(got - want)
    assert dev <= STEP_TOL * np.linalg.norm(want) + floor, (k, iters, dev, np.linalg.norm(want), floor)
    return dev / max(np.linalg.norm(want), 1e-300)


def _bounds(eng, L):
    return np.array([eng.timing("cheby_lambda_l%d" % k) for k in range(L)])


def test_bound_is_gershgorin_of_the_level_operator(case):
    """"cheby_lambda_l<k>" is max_i sum_j |a_ij| / |a_ii| of the oracle's level-k operator for every k < L, absent on a default handle, unchanged
    by set_system(2 lhs) and the model's new value after set_system(lhs + diag(lhs)) -- a values-only refresh."""
    P, L = case.P, case.L
    assert case.ratio > 1.0
    want = np.array(case.M.lam)
    got = _bounds(case.eng, L)
    print(case.name, "bounds", got, "relative deviation", np.abs(got - want) / want)
    assert np.all(np.abs(got - want) <= BOUND_TOL * want) and np.all(got >= 1.0)
    assert timing_or_none(case.eng, "cheby_lambda_l%d" % L) is None               # the coarsest level is not smoothed
    plain = _engine(case.cabi, P)
    try:
        assert timing_or_none(plain, "cheby_lambda_l0") is None and timing_or_none(plain, "cheby_ratio") is None
    finally:
        plain.close()
    eng = case.engine()
    jac = case.engine(smoother=case.cabi.SMOOTHER_JACOBI)
    try:
        eng.set_system((2.0 * P.lhs).tocsc())
        twice = _bounds(eng, L)
        assert np.all(np.abs(twice - got) <= BOUND_TOL * got), (twice, got)
        lhs2 = (P.lhs + sp.diags(P.lhs.diagonal())).tocsc()
        lhs2.sort_indices()
        eng.set_system(lhs2)
        # the values-only refresh wherever the handle reports one.  Two shapes of this catalogue are set up from scratch whatever the smoother is
        # (the handle reports 0): each has a row longer than the device layout builder takes (gmgs::kMaxRow = 96 entries: the 480-entry row of
        # hub48x40's level 1, the restriction's one row of 129 entries into chain129-coarsest1's single coarse unknown), their layouts come from
        # the host planner and there is nothing on the device to refill in place.  The route is the one a Jacobi handle takes through the same calls
        only = timing_or_none(eng, "setup_values_only")
        jac.set_system((2.0 * P.lhs).tocsc()); jac.set_system(lhs2)
        assert only == timing_or_none(jac, "setup_values_only")
        if only is not None and case.name not in ("chain129-coarsest1", "hub48x40"):
            assert only == 1.0
        M2 = ChebyshevModel(None, P.U, P.mass, lhs2, case.oracle, case.ratio)
        new, want2 = _bounds(eng, L), np.array(M2.lam)
        assert np.all(np.abs(new - want2) <= BOUND_TOL * want2), (new, want2)
        assert new[0] < got[0] or got[0] == 1.0                                     # (level 0 with a doubled diagonal: a smaller bound unless no row has off-diagonals)
        # ... and the steps run with the new bound
        b = case.rhs(1); x = np.random.default_rng(3).standard_normal((P.n, 1))
        _step_close(M2, 0, b, x, 3, eng.smooth(0, b, x, 3), M2.smooth(0, b, x, 3))
    finally:
        eng.close(); jac.close()


def test_steps_match_the_model(case):
    """gmg_smooth with 1, 2, 3, 5 steps on every level from a random x: FIRST alone, the first recurrence step, both parities of the ping-pong
    between x and tmp; 0 steps leave x bitwise untouched.  (On the parent of this feature smoother = 2 ran multicolour Gauss-Seidel.)"""
    rng = np.random.default_rng(21)
    worst = 0.0
    for k in range(case.L):
        n = case.M.A[k].shape[0]
        for d in case.ds:
            b = rng.standard_normal((n, d)); x = rng.standard_normal((n, d))
            assert np.array_equal(_bits(case.eng.smooth(k, b, x, 0)), _bits(x)), (k, d)
            for iters in (1, 2, 3, 5):
                got, want = case.eng.smooth(k, b, x, iters), case.M.smooth(k, b, x, iters)
                worst = max(worst, _step_close(case.M, k, b, x, iters, got, want))
    print(case.name, "largest relative deviation of the steps %.3e" % worst)


def test_energy_norm_of_the_error_does_not_grow(case):
    """b = A x*: ||x_k - x*||_A <= (1 + 1e-12) ||x_0 - x*||_A for k = 1, 2, 3, 5 on every level -- the guarantee (|T_k((theta - lambda) / delta) /
    T_k(sigma)| < 1 on (0, lambda_max]), with no measured number in it.  The model satisfies it on every case of this catalogue with that
    margin (asserted here as well): none was dropped."""
    rng = np.random.default_rng(22)
    for k in range(case.L):
        A = case.M.A[k]
        n = A.shape[0]
        for d in case.ds:
            xs = rng.standard_normal((n, d)); x0 = rng.standard_normal((n, d))
            b = A @ xs
            e0 = x0 - xs
            en0 = np.sqrt(np.sum(e0 * (A @ e0), axis=0))
            for iters in (1, 2, 3, 5):
                for who, xk in (("model", case.M.smooth(k, b, x0, iters)), ("device", case.eng.smooth(k, b, x0, iters))):
                    e = xk - xs
                    en = np.sqrt(np.sum(e * (A @ e), axis=0))
                    assert np.all(en <= (1.0 + 1e-12) * en0), (who, k, d, iters, en / en0)


@pytest.mark.parametrize("pair", PAIRS, ids=["%d+%d" % p for p in PAIRS])
def test_cycles_match_the_model(case, pair):
    """Three consecutive V-cycles cycle by cycle against the model, each restarted from the model's iterate; the fp32 inner cycle at 2 + 2."""
    pre, post = pair
    P, M = case.P, case.M
    e64 = case.eng if pair == (2, 2) else case.engine(pre_iters=pre, post_iters=post)
    e32 = case.engine(inner_precision=1) if pair == (2, 2) else None
    M.pre, M.post = pre, post
    try:
        for d in case.ds:
            b = case.rhs(d)
            x = b.copy()
            for cyc in range(3):
                xm = M.vcycle(b, x)
                xg = e64.vcycle(b, x)
                back, fwd = np.linalg.norm(P.lhs @ (xg - xm)), rel(xg, xm)
                assert back <= 1e-12 * case.nA * np.linalg.norm(xm), (d, cyc, back / (case.nA * np.linalg.norm(xm)))
                assert fwd <= (1e-11 if case.smoothing else 1e-6), (d, cyc, fwd)
                if e32 is not None:
                    xg = e32.vcycle(b, x)
                    assert np.linalg.norm(xg - xm) <= 2e-5 * np.linalg.norm(xm), ("fp32 inner", d, cyc, rel(xg, xm))
                x = xm
    finally:
        M.pre, M.post = 2, 2
        for e in (e64, e32):
            if e is not None and e is not case.eng:
                e.close()


# ---------------------------------------------------------------------------------------------- same bits on the other paths
@pytest.fixture(scope="module", params=["chain193-L3", "torus"])
def big(request, cabi, oracle):
    c = Case(cabi, oracle, request.param, _problem(request.param), (3,), dict([c for c in CASES if c[0] == request.param][0][3]))
    yield c
    c.eng.close()


def _same(a, b):
    return a[1] == b[1] and _bits(a[2]) == _bits(b[2]) and np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[3][:, 1]), _bits(b[3][:, 1]))


def test_graph_replay_gives_the_bits_of_stream_launches(big):
    """use_graph = 1: the same iterates, also after a values-only refresh has moved the bounds (the coefficients are kernel arguments of the
    captured launches: the graphs must not survive it)."""
    P = big.P
    b = big.compatible_rhs(3)
    g = big.engine(use_graph=True)
    s = big.engine()
    try:
        for refreshed in (False, True):
            if refreshed:
                lhs = (P.lhs + sp.diags(P.lhs.diagonal())).tocsc()
                lhs.sort_indices()
                g.set_system(lhs); s.set_system(lhs)
            x = b.copy()
            for cyc in range(3):
                xg, xs = g.vcycle(b, x), s.vcycle(b, x)
                assert np.array_equal(_bits(xg), _bits(xs)), cyc
                x = xs
            assert _same(g.solve(b, tol=1e-8, max_iter=60), s.solve(b, tol=1e-8, max_iter=60))
    finally:
        g.close(); s.close()


def test_two_runs_give_the_same_bits(big):
    b = big.compatible_rhs(3)
    assert _same(big.eng.solve(b, tol=1e-8, max_iter=60), big.eng.solve(b, tol=1e-8, max_iter=60))


def test_solve_device_gives_the_bits_of_solve(big):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    rhs = np.asfortranarray(big.compatible_rhs(3))
    n, d = rhs.shape
    kw = dict(tol=1e-8, stop_type=2, max_iter=60)
    x_a, it_a, res_a, conv_a = big.eng.solve(rhs, **kw)
    b = torch.tensor(np.ascontiguousarray(rhs), device=DEV)
    x = torch.full((n, d), float("nan"), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    it, res, conv = big.eng.solve_device(b.data_ptr(), b.stride(), x.data_ptr(), x.stride(), d, **kw)
    assert it == it_a and _bits(res) == _bits(res_a) and np.array_equal(_bits(conv[:, 1]), _bits(conv_a[:, 1]))
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(np.ascontiguousarray(x_a.reshape(rhs.shape))))


def test_accelerated_loop_on_a_chebyshev_handle(big):
    """accelerate = 2 reaches tol = 1e-8 in no more iterations than the plain loop of the same handle configuration, and the residue it reports
    has the bits of residual_norm on the returned x (the check of tests/test_gpu_accelerate.py).

    The right-hand side is a compatible one (Case.compatible_rhs)."""
    b = big.compatible_rhs(3)
    acc = big.engine(accelerate=2)
    try:
        x0, it0, res0, _ = big.eng.solve(b, tol=1e-8, stop_type=2, max_iter=100)
        x2, it2, res2, conv2 = acc.solve(b, tol=1e-8, stop_type=2, max_iter=100)
        print(big.name, "plain %d iterations (%.3e), accelerate = 2: %d (%.3e)" % (it0, res0, it2, res2))
        assert res0 <= 1e-8 and res2 <= 1e-8 and it2 <= it0
        assert _bits(res2) == _bits(acc.residual_norm(b, x2, 2)) and _bits(conv2[-1, 1]) == _bits(res2)
    finally:
        acc.close()


# ---------------------------------------------------------------------------------------------- refusals, drop-in
def test_multi_rank_entry_points_refuse_it_like_jacobi(cabi):
    """gmg_dist_setup(rank, 2), gmg_dist_partition + gmg_set_system and gmg_p2p_prepare(world = 2): the status codes a Jacobi handle gets from the
    same calls, with the smoother named; one rank is accepted."""
    P = _problem("chain193-L3")

    def code(f):
        with pytest.raises(cabi.GmgError) as ei:
            f()
        return ei.value.code, str(ei.value)

    got = {}
    for sm in (cabi.SMOOTHER_JACOBI, cabi.SMOOTHER_CHEBYSHEV):
        eng = _engine(cabi, P, smoother=sm, row_align=128)
        part = cabi.Engine(smoother=sm, row_align=128)
        try:
            part.set_prolongations(P.U); part.set_mass(P.mass)
            part.dist_partition(0, 2)
            got[sm] = (code(lambda: eng.dist_setup(0, 2)), code(lambda: part.set_system(P.lhs)), code(lambda: cabi.P2PCycle(eng, 0, 2, d=1)))
            part.dist_partition(0, 1)
            part.set_system(P.lhs)
            x, it, res, _ = part.solve(P.rhs[:, :1], tol=1e-6)
            assert res <= 1e-6
        finally:
            eng.close(); part.close()
    jac, che = got[cabi.SMOOTHER_JACOBI], got[cabi.SMOOTHER_CHEBYSHEV]
    assert [c for c, _ in che] == [c for c, _ in jac] and all(c < 0 for c, _ in che)
    assert all("GMG_SMOOTHER_CHEBYSHEV" in m for _, m in che), che
    assert all("GMG_SMOOTHER_JACOBI" in m for _, m in jac), jac


def test_dropin_option_reaches_the_engine(cabi):
    """set_engine_option("smoother", 2) on the problem of tests/test_dropin_api.py: M + 1e-3 S solved to 1e-4, and another iterate than the
    default solver's (by far more than rounding)."""
    import glob
    if not glob.glob(os.path.join(DROPIN, "gravomg_bindings*.so")):
        import __graft_entry__
        __graft_entry__.build()
    if DROPIN not in sys.path:
        sys.path.insert(0, DROPIN)
    import gravomg
    from gravo_mg_amd import meshgen
    V, F = meshgen.torus_mesh(48, 40)
    S, mass = meshgen.cotan_laplacian(V, F)
    M = sp.diags(mass).tocsr()
    neigh = gravomg.neighbors_from_stiffness(S)
    lhs, rhs = (M + 0.001 * S).tocsr(), M @ V
    out = []
    for smoother in (None, 2):
        solver = gravomg.MultigridSolver(V, neigh, M, lower_bound=40, tolerance=1e-4, max_iter=100)
        if smoother is not None:
            solver.set_engine_option("smoother", smoother)
        x = solver.solve(lhs, rhs)
        assert solver.residual(lhs, rhs, x) <= 1e-4
        out.append(np.array(x))
    diff = np.linalg.norm(out[1] - out[0]) / np.linalg.norm(out[0])
    print("Chebyshev against default solution: relative difference %.3e" % diff)
    assert 1e-12 < diff <= 1e-2          # (both within the tolerance of the same solution; rounding is 1e-16)
