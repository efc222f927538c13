"""GPU parity at the shapes where the launch code and the kernels switch branches: levels smaller than one 64-row slice and at slice
boundaries, operators without off-diagonals, one colour and hundreds of colours, coarsest levels from 1 to 8 193 unknowns (the 16-column tiles
of the dense inverse, the rows-per-wave switch of its product at 3 000, the device / host switch of GMG_COARSE_AUTO above 8 192), one transfer
level, 1 to 8 right-hand sides.  The hierarchy builder never makes these shapes, so every problem here brings its own operator and
prolongations (tests/problems.synthetic_problem).  The checks and tolerances are those of tests/test_gpu_parity.py.

Catalogue (test ids): A tiny and slice-boundary levels (chain, L = 1 and 2), B diagonal-only and partly isolated operators, C many colours and
a dense row on level 1, D coarsest sizes for the dense inverse (grid, n_0 ~ 4 n_L).  Right-hand sides: d in {1, 2, 3, 4, 5, 8} on A, {1, 3}
elsewhere."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import problems
from tests.parity_checks import SWITCHES, check_block_sweeps, check_multicolor_gs, engaged, rel, timing_or_none
from tests.vcycle_model import VcycleModel

pytestmark = pytest.mark.gpu

D_ALL, D_FEW = (1, 2, 3, 4, 5, 8), (1, 3)


def _grid_for(n_L):
    """A grid of about 4 n_L vertices (never fewer than n_L)."""
    n1 = max(1, int(np.ceil(np.sqrt(4 * n_L))))
    return n1, max(1, int(np.ceil(4 * n_L / n1)))


def _catalogue():
    cases = []
    for n in (1, 2, 5, 63, 64, 65, 127, 128, 129, 193):
        cases.append(("A-chain%d-L1" % n, dict(graph=("chain", n), sizes=[n, max(1, n // 4)], kind="poisson", prolong=("pc",)), D_ALL))
        cases.append(("A-chain%d-L2" % n, dict(graph=("chain", n), sizes=[n, max(1, n // 2), max(1, n // 8)], kind="smoothing",
                                                prolong=("smooth", "pc")), D_ALL))
    cases.append(("A-chain129-coarsest1", dict(graph=("chain", 129), sizes=[129, 1], kind="smoothing", prolong=("pc",)), D_ALL))
    cases.append(("A-chain193-L2-coarsest1", dict(graph=("chain", 193), sizes=[193, 48, 1], kind="smoothing", prolong=("smooth", "pc")), D_ALL))
    # (three transfer levels: a restriction into a level that is not the coarsest, where fuse_restrict_sweep can engage)
    cases.append(("A-chain193-L3", dict(graph=("chain", 193), sizes=[193, 96, 24, 6], kind="smoothing", prolong=("smooth", "pc", "pc")), D_ALL))
    for n, sizes in ((1, [1, 1]), (100, [100, 25, 6]), (4097, [4097, 1024, 256])):
        cases.append(("B-diagonal%d" % n, dict(graph=("diagonal", n), sizes=sizes, kind="poisson", prolong=("pc",)), D_FEW))
    cases.append(("B-isolated40x40", dict(graph=("isolated", 40, 40), sizes=[1600, 400, 100], kind="smoothing", prolong=("smooth", "pc")), D_FEW))
    # (rows this long make the engine block level 0 (gmg_config::block_fine, 64 colours at most per block); block_fine = 0 keeps the m colours
    # of the clique on a colour-major level 0 -- the clique-255 case is the most colours a level may have)
    for m in (65, 254, 255):
        n = m + 48 * 48
        cases.append(("C-clique%d" % m, dict(graph=("clique", 48, 48, m), sizes=[n, n // 4, n // 16], kind="smoothing", prolong=("pc",)), D_FEW,
                      dict(block_fine=False)))
    cases.append(("C-clique255-blocked-fine", dict(graph=("clique", 48, 48, 255), sizes=[2559, 639, 159], kind="smoothing", prolong=("pc",)), D_FEW))
    cases.append(("C-hub48x40", dict(graph=("hub", 48, 40), sizes=[1921, 480, 120], kind="poisson", prolong=("pc",)), D_FEW))
    for n_L in (1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 2999, 3000, 3001, 8192, 8193):
        n1, n2 = _grid_for(n_L)
        cases.append(("D-coarsest%d" % n_L, dict(graph=("grid", n1, n2), sizes=[n1 * n2, n_L], kind="poisson", prolong=("pc",)), D_FEW))
    return [c if len(c) == 4 else c + (dict(),) for c in cases]


CASES = _catalogue()


def _engine(cabi, P, **kw):
    eng = cabi.Engine(**kw)
    eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
    return eng


class Case:
    def __init__(self, name, P, ds, kw, eng):
        self.name, self.P, self.ds, self.kw, self.eng = name, P, ds, kw, eng

    def engine(self, cabi, **kw):
        """Another engine on this case's problem (the case's own settings, then kw)."""
        return _engine(cabi, self.P, **dict(self.kw, **kw))


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request, cabi):
    name, spec, ds, kw = request.param
    assert cabi.device_count() > 0, "gpu tests need a HIP device"
    P = problems.synthetic_problem(**spec)
    eng = _engine(cabi, P, **kw)
    if name.startswith("C-clique") and kw:
        assert eng.level_blocks(0) is None and eng.level_info(0)["n_colors"] == spec["graph"][3]
    yield Case(name, P, ds, kw, eng)
    eng.close()           # (one case at a time: the dense inverse of n_L = 8 192 is 512 MB)


def _is_smoothing(P):
    return "smoothing" in P.name


def test_shape_is_the_one_asked_for(case):
    """The engine kept the exact level sizes, and each family has the layout it is in the catalogue for: two colour classes of ceil(n / 2) and
    floor(n / 2) rows, each padded to 64, on a chain's level 0; one colour and no off-diagonal on every level of a diagonal operator; the
    clique's m colours (asserted by the fixture); a level-1 row coupled to every other on the hub; the device inverse up to 8 192 unknowns."""
    P, eng = case.P, case.eng
    assert eng.num_levels == len(P.U)
    for k in range(len(P.U) + 1):
        info = eng.level_info(k)
        assert info["n"] == (P.U[k].shape[0] if k < len(P.U) else P.U[-1].shape[1])
        if k < len(P.U):
            assert info["n_pad"] % 64 == 0 and info["n_pad"] >= info["n"] and 1 <= info["n_colors"]
    n = P.n
    if case.name.startswith("A-"):
        info = eng.level_info(0)
        assert eng.level_blocks(0) is None and info["n_colors"] == min(n, 2)
        assert info["n_pad"] == 64 * (-(-((n + 1) // 2) // 64) + -(-(n // 2) // 64)), info
    if case.name.startswith("B-diagonal"):
        for k in range(len(P.U) + 1):
            info = eng.level_info(k)
            assert info["nnz"] == info["n"], k
            if k < len(P.U):
                assert info["n_colors"] == 1, k
    if case.name.startswith("C-hub"):
        A1 = eng.level_operator(1)
        assert np.diff(A1.indptr).max() == A1.shape[0]
    assert eng.timing("coarse_on_device") == (1.0 if P.U[-1].shape[1] <= 8192 else 0.0)


def test_levels_and_galerkin(case, oracle):
    P, eng = case.P, case.eng
    O = oracle.Hierarchy(P.U, P.mass)
    O.set_system(P.lhs)
    for k in range(len(P.U) + 1):
        A, Ao = eng.level_operator(k), O.level_operator(k)
        assert A.shape == Ao.shape
        assert (A != 0).nnz <= Ao.nnz
        assert abs(A - Ao).max() <= 1e-13 * abs(Ao).max()


def test_spmv_residual(case, oracle):
    P, eng = case.P, case.eng
    rng = np.random.default_rng(0)
    for k in range(len(P.U)):
        A = eng.level_operator(k)
        for d in case.ds:
            x = rng.standard_normal((A.shape[0], d)); b = rng.standard_normal((A.shape[0], d))
            assert rel(eng.spmv(k, x), A @ x) <= 1e-13, (k, d)
            assert rel(eng.residual(k, b, x), oracle.residual(A, b, x)) <= 1e-13, (k, d)


def test_transfers(case, oracle):
    P, eng = case.P, case.eng
    rng = np.random.default_rng(1)
    for k, U in enumerate(P.U):
        for d in case.ds:
            r = rng.standard_normal((U.shape[0], d)); e = rng.standard_normal((U.shape[1], d)); x = rng.standard_normal((U.shape[0], d))
            assert rel(eng.restrict(k, r), oracle.restrict(U, r)) <= 1e-13, (k, d)
            assert rel(eng.prolong_add(k, e, x), oracle.prolong_add(U, e, x)) <= 1e-13, (k, d)


def test_exact_multicolour_gs_is_reference_gs_on_permuted_system(case, cabi, oracle):
    eng = case.engine(cabi, block_rows=0, gs_omega=1.0)
    try:
        check_multicolor_gs(case.P, eng, oracle, ds=case.ds)
    finally:
        eng.close()


def test_level0_sor_sweep_matches_model(case, oracle):
    P, eng = case.P, case.eng
    assert eng.gs_omega != 1.0                   # (a blocked level 0 is not over-relaxed: the model then takes its block form)
    M = VcycleModel(eng, P.U, P.mass, P.lhs, oracle, eng.gs_omega)
    rng = np.random.default_rng(12)
    for d in case.ds:
        b = rng.standard_normal((P.n, d)); x = rng.standard_normal((P.n, d))
        for iters in (1, 2):
            assert rel(eng.smooth(0, b, x, iters), M.smooth(0, b, x, iters)) <= 1e-12, (d, iters)


@pytest.mark.parametrize("kw", [dict(), dict(block_lanes=1)], ids=["default-layout", "block-lanes-1"])
def test_block_sweeps_match_matrix_form(case, cabi, oracle, kw):
    if kw:
        eng = case.engine(cabi, **kw)
    else:
        eng = case.eng
    try:
        check_block_sweeps(case.P, eng, oracle, ds=case.ds)
    finally:
        if kw:
            eng.close()


def test_smooth_residual_is_b_minus_Ax(case, cabi, oracle):
    """The residual the way down takes from the last sweep (or from its SpMV) on every blocked level, against b - A x of the same iterate:
    <= 1e-13 (|A||x| + |b|)."""
    P = case.P
    for kw in (dict(), dict(block_lanes=1)):
        eng = case.engine(cabi, **kw)
        try:
            rng = np.random.default_rng(11)
            for k in range(1, len(P.U)):
                A = eng.level_operator(k)
                absA = abs(A)
                for d in case.ds:
                    b = rng.standard_normal((A.shape[0], d)); x0 = rng.standard_normal((A.shape[0], d))
                    for iters in (1, 2, 3, 4, 5):
                        for from_zero in (False, True):
                            x, r = eng.smooth_residual(k, b, None if from_zero else x0, iters, from_zero=from_zero)
                            assert np.array_equal(x, eng.smooth(k, b, np.zeros_like(b) if from_zero else x0, iters))
                            scale = absA @ abs(x) + abs(b)
                            assert np.abs(r - oracle.residual(A, b, x)).max() <= 1e-13 * scale.max(), (kw, k, d, iters, from_zero)
        finally:
            eng.close()


def test_norms(case, oracle):
    P, eng = case.P, case.eng
    rng = np.random.default_rng(3)
    for d in case.ds:
        x = rng.standard_normal((P.n, d)); b = P.rhs[:, :d]
        for t in (0, 1, 2, 3):
            got = eng.residual_norm(b, x, t)
            want = oracle.residual_check(P.lhs, P.mass, b, x, t)
            assert abs(got - want) <= 1e-12 * abs(want), (d, t)


def _cond(A):
    """2-norm condition of the SPD coarsest operator (dense below 2 500 unknowns, else from its extreme eigenvalues)."""
    n = A.shape[0]
    if n <= 2500:
        return np.linalg.cond(A.toarray())
    hi = spla.eigsh(A, k=1, which="LA", return_eigenvectors=False)[0]
    lo = spla.eigsh(sp.csc_matrix(A), k=1, sigma=0, which="LM", return_eigenvectors=False)[0]
    return hi / lo


def test_coarse_solve_host_and_device(case, cabi, oracle):
    """GMG_COARSE_HOST_LDLT and GMG_COARSE_DEVICE_INVERSE against the oracle, with the condition-scaled bounds of
    test_device_built_coarse_inverse_against_the_host_factor; one column alone == that column of the block (bitwise); X = X^T; AUTO picks
    the device up to 8 192 unknowns."""
    P = case.P
    nl = P.U[-1].shape[1]
    assert case.eng.timing("coarse_on_device") == (1.0 if nl <= 8192 else 0.0)
    engines = []
    try:
        dev = case.engine(cabi, coarse_mode=cabi.COARSE_DEVICE_INVERSE); engines.append(dev)
        host = case.engine(cabi, coarse_mode=cabi.COARSE_HOST_LDLT); engines.append(host)
        assert dev.timing("coarse_on_device") == 1.0 and host.timing("coarse_on_device") == 0.0
        AL = dev.level_operator(len(P.U))
        O = oracle.Hierarchy(P.U, P.mass)
        O.set_system(P.lhs)
        nA = spla.norm(AL)
        cond = _cond(AL)
        rng = np.random.default_rng(11)
        for d in case.ds:
            rc = rng.standard_normal((nl, d))
            e_dev, e_host, e_o = dev.coarse_solve(rc), host.coarse_solve(rc), O.coarse_solve(rc)
            assert np.linalg.norm(AL @ e_host - rc) <= 1e-12 * (nA * np.linalg.norm(e_host) + np.linalg.norm(rc)), d
            assert np.linalg.norm(AL @ (e_host - e_o)) <= 1e-11 * nA * np.linalg.norm(e_o), d
            assert np.linalg.norm(AL @ (e_dev - e_host)) <= 1e-14 * cond * nA * np.linalg.norm(e_host) + 1e-10 * nA * np.linalg.norm(e_host), d
            assert rel(e_dev, e_host) <= 1e-13 * cond + 1e-9, d
            assert rel(e_dev, e_o) <= 1e-13 * cond + 1e-9, d
            for eng, e in ((dev, e_dev), (host, e_host)):
                j = d - 1
                assert np.array_equal(eng.coarse_solve(rc[:, j]).ravel(), e[:, j]), d
                if d >= 2:
                    assert abs(rc[:, 0] @ e[:, 1] - rc[:, 1] @ e[:, 0]) <= 1e-12 * np.abs(rc[:, 0] @ e[:, 1]) + 1e-12 * np.linalg.norm(e), d
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("inner_precision", [0, 1], ids=["fp64", "fp32-inner"])
def test_vcycles_match_model(case, cabi, oracle, inner_precision):
    """Two V-cycles of the default engine (and of the fp32 inner cycle) against tests/vcycle_model.VcycleModel, from identical inputs."""
    P, ref = case.P, case.eng
    eng = ref if inner_precision == 0 else case.engine(cabi, inner_precision=1)
    try:
        M = VcycleModel(ref, P.U, P.mass, P.lhs, oracle, ref.gs_omega)
        nA = spla.norm(P.lhs)
        for d in case.ds:
            b = P.rhs[:, :d]
            x = b.copy()
            for cyc in range(2):
                xg, xm = eng.vcycle(b, x), M.vcycle(b, x)
                if inner_precision:
                    assert np.linalg.norm(xg - xm) <= 2e-5 * np.linalg.norm(xm), (d, cyc)
                else:
                    assert np.linalg.norm(P.lhs @ (xg - xm)) <= 1e-12 * nA * np.linalg.norm(xm), (d, cyc)
                    assert rel(xg, xm) <= (1e-11 if _is_smoothing(P) else 1e-6), (d, cyc)
                x = xm
    finally:
        if eng is not ref:
            eng.close()


def test_solve_matches_the_oracle(case, oracle):
    P, eng = case.P, case.eng
    tol = 1e-4
    O = oracle.Hierarchy(P.U, P.mass)
    O.set_system(P.lhs)
    for d in case.ds:
        b = P.rhs[:, :d]
        x, it, res, conv = eng.solve(b, tol=tol, stop_type=2, max_iter=100)
        assert res <= tol and it < 100 and conv.shape == (it, 2), (d, it, res)
        assert abs(oracle.residual_check(P.lhs, P.mass, b, x, 2) - res) <= 1e-3 * res + 1e-7, d
        xo, ito, reso, _ = O.solve(b, tol=tol)
        assert reso <= tol
        assert it <= ito + 2, (d, it, ito)
        m = P.mass[:, None]
        dx = np.sqrt((m * (x - xo) ** 2).sum()) / np.sqrt((m * xo ** 2).sum())
        assert dx <= 20 * tol, d


# a catalogue shape on which each switch must engage (so that the bitwise comparison below compares two different launch sequences there)
ENGAGES_ON = {"speculate_head": "A-chain64-L1", "fuse_restrict_sweep": "A-chain193-L3", "uniform_slices": "A-chain193-L1", "fine_col16": "D-coarsest3000"}


@pytest.mark.parametrize("switch", SWITCHES)
def test_switches_change_nothing(case, cabi, switch):
    """Each of these switches changes how the cycle is launched, never what it computes: iterates, residue histories and solutions bit for
    bit with the switch on and off -- solves to a tolerance, a solve whose first cycle is enough, fixed cycle counts.  The timing keys say
    which path ran: switched off it never engages; the head needs a colour-major level 0 of at least two colours; a fused restriction needs a
    level below the one restricted into (none with one transfer level); and each switch engages on its ENGAGES_ON shape."""
    P = case.P
    out = []
    for on in (1, 0):
        eng = case.engine(cabi, **{switch: on})
        try:
            res = {}
            for d in (1, 3):
                b = P.rhs[:, :d]
                for name, tol, max_iter in (("to the tolerance", 1e-6, 100), ("max_iter", 1e-30, 3), ("first cycle is enough", 1e3, 100)):
                    x, it, r, conv = eng.solve(b, tol=tol, max_iter=max_iter)
                    res[(name, d)] = (x.copy(), it, r, conv[:, 1].copy())
                eng.load_problem(b, b)
                hist = eng.run_cycles(3, 2).copy()
                res[("run_cycles", d)] = (eng.fetch_solution().copy(), 3, hist, None)
            ran = engaged(eng, switch)
            if not on:
                assert ran == 0, (switch, ran)
            elif switch == "speculate_head":
                eligible = eng.level_blocks(0) is None and eng.level_info(0)["n_colors"] >= 2
                assert (ran > 0) == eligible, (eligible, ran)
            elif switch == "fuse_restrict_sweep" and len(P.U) == 1:
                assert ran == 0, ran
            if on and case.name == ENGAGES_ON[switch]:
                assert ran > 0, (switch, case.name)
            out.append(res)
        finally:
            eng.close()
    a, b = out
    for key in a:
        assert a[key][1] == b[key][1], key
        assert np.array_equal(a[key][2], b[key][2]), key
        if a[key][3] is not None:
            assert np.array_equal(a[key][3], b[key][3]), key
        assert np.array_equal(a[key][0], b[key][0]), key


# ---------------------------------------------------------------------------------------------- loud failures
def test_too_many_colours_on_level_0_is_refused_and_the_next_solve_is_a_state_error(cabi):
    """K_256 needs 256 colours; a level may have at most 255 (host_plan.hpp kMaxColors).  gmg_set_system refuses it with
    GMG_ERR_UNSUPPORTED, and the handle then has no system: a solve is GMG_ERR_STATE (include/gravomg_hip.h)."""
    m = 256
    W = sp.csc_matrix(np.ones((m, m)) - np.eye(m))
    S = problems._laplacian_of(W)
    mass = np.ones(m)
    lhs = (S + sp.identity(m)).tocsc()
    U = [problems.aggregation(m, 4)]
    eng = cabi.Engine(block_fine=False)          # (a blocked level 0 colours each 64-row block on its own)
    try:
        eng.set_prolongations(U); eng.set_mass(mass)
        with pytest.raises(cabi.GmgError) as ei:
            eng.set_system(lhs)
        assert ei.value.code == cabi.GMG_ERR_UNSUPPORTED and "colours" in str(ei.value)
        with pytest.raises(cabi.GmgError) as ei:
            eng.solve(np.ones(m))
        assert ei.value.code == cabi.GMG_ERR_STATE
        # one colour fewer is accepted by the same handle
        W = sp.csc_matrix(np.ones((m - 1, m - 1)) - np.eye(m - 1))
        eng.set_prolongations([problems.aggregation(m - 1, 4)]); eng.set_mass(mass[:-1])
        eng.set_system((problems._laplacian_of(W) + sp.identity(m - 1)).tocsc())
        assert eng.level_info(0)["n_colors"] == m - 1
        x, it, res, _ = eng.solve(np.ones(m - 1), tol=1e-8)
        assert res <= 1e-8
    finally:
        eng.close()


def test_fp32_twin_of_an_empty_block_csr_leaves_no_launch_error_behind(cabi):
    """A level that is one block has no off-block entry: with block_lanes = 1, block_ep = 0 its block-CSR is empty, and the mixed-precision set-up
    must not launch a conversion over 0 values -- a grid of 0 workgroups is refused, and the error it leaves on the thread was reported by the
    NEXT gmg_set_system (GMG_ERR_HIP "invalid configuration argument"), whatever handle that was."""
    (spec,) = [c[1] for c in CASES if c[0] == "A-chain193-L3"]
    P = problems.synthetic_problem(**spec)
    mix = _engine(cabi, P, block_lanes=1, block_ep=False, inner_precision=1)
    try:
        assert mix.level_info(2)["n"] == 24 and len(mix.level_blocks(2)[0]) == 2          # one block
        x, it, res, _ = mix.solve(P.rhs[:, :3], tol=1e-8)
        assert res <= 1e-8
        for kw in (dict(), dict(block_lanes=1, block_ep=False, inner_precision=1)):
            _engine(cabi, P, **kw).close()
    finally:
        mix.close()


def test_empty_hierarchy_is_a_state_error(cabi):
    P = problems.synthetic_problem(("chain", 64), [64, 16])
    eng = cabi.Engine()
    try:
        eng.set_prolongations([])
        eng.set_mass(P.mass)
        with pytest.raises(cabi.GmgError) as ei:
            eng.set_system(P.lhs)
        assert ei.value.code == cabi.GMG_ERR_STATE
    finally:
        eng.close()


def test_dropin_solver_on_a_mesh_at_or_below_lower_bound_raises(cabi):
    """The hierarchy builder returns no levels for a mesh at or below lower_bound; the drop-in solver must say so, not crash."""
    import glob
    import os
    import sys
    from gravo_mg_amd import meshgen
    dropin = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gravo_mg_amd", "dropin")
    if not glob.glob(os.path.join(dropin, "gravomg_bindings*.so")):
        import __graft_entry__
        __graft_entry__.build()
    if dropin not in sys.path:
        sys.path.insert(0, dropin)
    import gravomg
    V, F = meshgen.torus_mesh(12, 10)
    S, mass = meshgen.cotan_laplacian(V, F)
    neigh = gravomg.neighbors_from_stiffness(S)
    M = sp.diags(mass).tocsr()
    lhs = (M + 1e-3 * S).tocsr()
    for lb in (20, 120, 1000):                    # (120 vertices: even lower_bound = 20 leaves no level above it)
        solver = gravomg.MultigridSolver(V, neigh, M, lower_bound=lb)
        assert len(solver.prolongation_matrices) == 0
        with pytest.raises(RuntimeError, match="no levels"):
            solver.solve(lhs, M @ V)
