"""GPU parity: every hot-path operator, the V-cycle and the solve loop of libgravomg_hip.so (through the
C-ABI) against the CPU restatement in oracle/ on the same seeded inputs.

Tolerances (fp64, stated per test):
  * operators (SpMV, residual, restriction, prolongation, norms): <= 1e-13 relative (only the order of a
    handful of additions differs from the oracle);
  * multicolour Gauss-Seidel == the reference's lexicographic Gauss-Seidel applied to the colour-permuted
    system P A P^T: <= 1e-12 relative against the oracle run on P A P^T;
  * V-cycle / solve with the GPU smoother are a DIFFERENT (equally valid) iteration from natural-order GS:
    parity is on the converged solution -- both reach the reference's stopping test (M-norm <= tol) and the
    two solutions agree to ||dx||_M/||x||_M <= 20*tol; iteration counts are reported, equal +-2.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import problems
from tests.parity_checks import check_block_sweeps as _check_block_sweeps, check_multicolor_gs, colour_permuted_hierarchy, rel, timing_or_none

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["poisson-d1", "smoothing-d3", "pointcloud", "random-order", "irregular-sphere"])
def setup(request, cabi):
    if request.param == "poisson-d1":
        P = problems.torus_problem(96, 80, "poisson", 30)          # 7680 -> ~1250 -> ~200 -> ~33: L = 3
    elif request.param == "smoothing-d3":
        P = problems.torus_problem(64, 60, "smoothing", 60)        # L = 2, d = 3
    elif request.param == "pointcloud":
        P = problems.pointcloud_problem(3000)
    elif request.param == "irregular-sphere":
        P = problems.sphere_problem(6000)                           # valence 3..12, 7 colours
    else:
        P = problems.torus_problem(48, 40, "poisson", 60, order="random")
    assert cabi.device_count() > 0, "gpu tests need a HIP device"
    eng = cabi.Engine()
    eng.set_prolongations(P.U)
    eng.set_mass(P.mass)
    eng.set_system(P.lhs)
    return P, eng


@pytest.fixture(scope="module")
def setup_exact(setup, cabi):
    """Same problem, exact (global) multicolour Gauss-Seidel on EVERY level (block_rows=0), no over-relaxation:
    the reference's update in colour order."""
    P, _ = setup
    eng = cabi.Engine(block_rows=0, gs_omega=1.0)
    eng.set_prolongations(P.U)
    eng.set_mass(P.mass)
    eng.set_system(P.lhs)
    return P, eng


def test_levels_and_galerkin(setup, oracle):
    P, eng = setup
    O = oracle.Hierarchy(P.U, P.mass)
    O.set_system(P.lhs)
    assert eng.num_levels == len(P.U) >= 1
    for k in range(len(P.U) + 1):
        A, Ao = eng.level_operator(k), O.level_operator(k)
        assert A.shape == Ao.shape
        assert (A != 0).nnz <= Ao.nnz
        assert abs(A - Ao).max() <= 1e-13 * abs(Ao).max()


def test_spmv_residual(setup, oracle):
    P, eng = setup
    rng = np.random.default_rng(0)
    for k in range(len(P.U)):
        A = eng.level_operator(k)
        for d in (1, 3):
            x = rng.standard_normal((A.shape[0], d)); b = rng.standard_normal((A.shape[0], d))
            assert rel(eng.spmv(k, x), A @ x) <= 1e-13
            assert rel(eng.residual(k, b, x), oracle.residual(A, b, x)) <= 1e-13


def test_transfers(setup, oracle):
    P, eng = setup
    rng = np.random.default_rng(1)
    for k, U in enumerate(P.U):
        for d in (1, 3):
            r = rng.standard_normal((U.shape[0], d)); e = rng.standard_normal((U.shape[1], d)); x = rng.standard_normal((U.shape[0], d))
            assert rel(eng.restrict(k, r), oracle.restrict(U, r)) <= 1e-13
            assert rel(eng.prolong_add(k, e, x), oracle.prolong_add(U, e, x)) <= 1e-13


def test_block_hybrid_sweep_matches_matrix_form(setup, oracle):
    """Blocked levels (default: every level >= 1): one sweep == x + T^-1 (b - A x) with
    T = D + strict-lower(A restricted to the block diagonal) in device order: Jacobi between blocks, exact
    Gauss-Seidel inside a block.  The residual comes from the oracle, T^-1 from scipy."""
    P, eng = setup
    _check_block_sweeps(P, eng, oracle)


def test_block_hybrid_sweep_of_the_big_level_kernels(setup, cabi, oracle):
    """The same identity for the kernels big blocked levels use (one lane per row, 64-row blocks; forced here by
    block_lanes=1): the entry-parallel sweep (default), and the sweeps it replaced -- SELL for one right-hand side, off-block
    operator in block-CSR for several."""
    P, _ = setup
    for kw in (dict(block_lanes=1), dict(block_lanes=1, block_ep=False), dict(block_lanes=1, block_csr=False)):      # entry-parallel, block-CSR / SELL, SELL only
        eng = cabi.Engine(**kw)
        eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
        _check_block_sweeps(P, eng, oracle)


def test_residual_from_the_sweeps_explicit_part_equals_b_minus_Ax(setup, cabi, oracle):
    """On the way down, a level with the unpadded block storage takes its residual from the last sweep's explicit part,
    r_i = sum_E a_ij (x_old_j - x_new_j) (kernels.hip.hpp::residual_delta_ep), instead of a pass over the whole operator.  Against
    the oracle's b - A x of the same iterate, to the rounding of evaluating b - A x: |difference| <= 1e-13 (|A||x| + |b|)."""
    P, _ = setup
    eng = cabi.Engine(block_lanes=1)          # the big-level kernels on every blocked level
    eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
    rng = np.random.default_rng(11)
    used = 0
    for k in range(1, len(P.U)):
        A = eng.level_operator(k)
        absA = abs(A)
        for d in (1, 3):
            b = rng.standard_normal((A.shape[0], d)); x0 = rng.standard_normal((A.shape[0], d))
            for iters in (1, 2, 3):
                for from_zero in (False, True):
                    x, r = eng.smooth_residual(k, b, None if from_zero else x0, iters, from_zero=from_zero)
                    shortcut = eng.timing("residual_from_sweep") == 1.0
                    # (a sweep count whose result lands in the other buffer is copied over x -- which was x_old -- and falls back to the SpMV)
                    assert shortcut == (iters % 2 == 0 or (from_zero and iters == 1))
                    used += shortcut
                    assert np.array_equal(x, eng.smooth(k, b, np.zeros_like(b) if from_zero else x0, iters))
                    scale = absA @ abs(x) + abs(b)
                    assert np.abs(r - oracle.residual(A, b, x)).max() <= 1e-13 * scale.max(), (k, d, iters, from_zero)
    assert used > 0 or len(P.U) == 1


def test_multicolor_gs_is_reference_gs_on_permuted_system(setup_exact, oracle):
    P, eng = setup_exact
    check_multicolor_gs(P, eng, oracle)


def test_level0_sor_sweep_matches_model(setup, oracle):
    """The default engine over-relaxes the level-0 colour sweep (gmg_config::gs_omega): per colour
    x[rows] += omega (b - A x)[rows] / diag[rows], with the residual taken from the oracle."""
    from tests.vcycle_model import VcycleModel
    P, eng = setup
    assert eng.gs_omega != 1.0
    M = VcycleModel(eng, P.U, P.mass, P.lhs, oracle, eng.gs_omega)
    rng = np.random.default_rng(12)
    for d in (1, 3):
        b = rng.standard_normal((P.n, d)); x = rng.standard_normal((P.n, d))
        for iters in (1, 2):
            assert rel(eng.smooth(0, b, x, iters), M.smooth(0, b, x, iters)) <= 1e-12


def test_default_engine_vcycles_match_model_per_cycle(setup, oracle):
    """Three consecutive V-cycles of the DEFAULT engine (level-0 multicolour SOR, block-hybrid sweeps below, host LDL^T)
    against the model assembled from the oracle's operators with the device's orderings (tests/vcycle_model.py): the
    same iteration, so the iterates agree to rounding cycle by cycle."""
    import scipy.sparse.linalg as spla
    from tests.vcycle_model import VcycleModel
    P, eng = setup
    M = VcycleModel(eng, P.U, P.mass, P.lhs, oracle, eng.gs_omega)
    xg = P.rhs.copy(); xm = P.rhs.copy()
    nA = spla.norm(P.lhs)
    for cyc in range(3):
        xg = eng.vcycle(P.rhs, xg)
        xm = M.vcycle(P.rhs, xm)
        # backward-error bound (insensitive to the 1/tau conditioning of the Poisson systems) and a forward bound
        assert np.linalg.norm(P.lhs @ (xg - xm)) <= 1e-12 * nA * np.linalg.norm(xm), cyc
        assert rel(xg, xm) <= (1e-11 if "smoothing" in P.name else 1e-6), cyc
        xg = xm.copy()          # next cycle from identical input: no accumulation of conditioning-amplified rounding


def test_norms(setup, oracle):
    P, eng = setup
    rng = np.random.default_rng(3)
    d = P.rhs.shape[1]
    x = rng.standard_normal((P.n, d))
    for t in (0, 1, 2, 3):
        got = eng.residual_norm(P.rhs, x, t)
        want = oracle.residual_check(P.lhs, P.mass, P.rhs, x, t)
        assert abs(got - want) <= 1e-12 * abs(want)


def test_coarse_solve(setup, oracle):
    P, eng = setup
    AL = eng.level_operator(len(P.U))
    rng = np.random.default_rng(4)
    rc = rng.standard_normal((AL.shape[0], 3))
    e = eng.coarse_solve(rc)
    # backward error (the Poisson operators are nearly singular: cond ~ 1/tau)
    import scipy.sparse.linalg as spla
    assert np.linalg.norm(AL @ e - rc) <= 1e-12 * (spla.norm(AL) * np.linalg.norm(e) + np.linalg.norm(rc))
    O = oracle.Hierarchy(P.U, P.mass)
    O.set_system(P.lhs)
    eo = O.coarse_solve(rc)
    assert np.linalg.norm(AL @ (e - eo)) <= 1e-11 * (spla.norm(AL) * np.linalg.norm(eo))


def test_vcycle_matches_oracle_with_same_ordering(setup_exact, oracle):
    """One V-cycle (exact multicolour GS on every level) where the oracle is given the device's colour
    ordering on every level: same algebra, only floating-point summation order differs."""
    P, eng = setup_exact
    O, order0 = colour_permuted_hierarchy(P, eng, oracle)
    x0 = P.rhs.copy()
    got = eng.vcycle(P.rhs, x0)
    want_p = O.vcycle(P.rhs[order0], x0[order0])
    want = np.empty_like(want_p); want[order0] = want_p
    # backward-error style bound (insensitive to the 1/tau conditioning of the Poisson systems) ...
    import scipy.sparse.linalg as spla
    assert np.linalg.norm(P.lhs @ (got - want)) <= 1e-12 * spla.norm(P.lhs) * np.linalg.norm(want)
    # ... and a forward bound: 1e-12 for the well-conditioned smoothing system, 1e-6 where ||x||/||b|| ~ 1e8
    assert rel(got, want) <= (1e-12 if "smoothing" in P.name else 1e-6)


def test_solve_reaches_tolerance_and_matches_reference_solution(setup, oracle):
    P, eng = setup
    tol = 1e-4
    x, it, res, conv = eng.solve(P.rhs, tol=tol, stop_type=2, max_iter=100)
    assert res <= tol and it < 100 and conv.shape == (it, 2)
    # the oracle re-evaluates the GPU iterate's residue; fp64 cancellation in A x - b limits agreement to ~1e-8 absolute
    assert abs(oracle.residual_check(P.lhs, P.mass, P.rhs, x, 2) - res) <= 1e-3 * res + 1e-7
    O = oracle.Hierarchy(P.U, P.mass)
    O.set_system(P.lhs)
    xo, ito, reso, _ = O.solve(P.rhs, tol=tol)
    assert reso <= tol
    assert it <= ito + 2, (it, ito)
    m = P.mass[:, None] if x.ndim == 2 else P.mass
    dx = np.sqrt((m * (x - xo) ** 2).sum()) / np.sqrt((m * xo ** 2).sum())
    assert dx <= 20 * tol
    # tight solve: both converge to the same fixed point.  The Poisson systems (tau = 1e-6) have
    # ||x||/||b|| ~ 1e8, so fp64 residual evaluation floors at ~4e-8 on the CPU oracle and the GPU alike.
    tight = 1e-10 if "smoothing" in P.name else 1e-6
    x2, it2, res2, _ = eng.solve(P.rhs, tol=tight, max_iter=100)
    xo2, ito2, reso2, _ = O.solve(P.rhs, tol=tight)
    assert res2 <= tight and reso2 <= tight and it2 <= ito2 + 2       # (the over-relaxed level-0 sweep usually needs fewer cycles)
    dx2 = np.sqrt((m * (x2 - xo2) ** 2).sum()) / np.sqrt((m * xo2 ** 2).sum())
    assert dx2 <= 100 * tight
    # gmg_solve_x0_rhs (no x0 given: x is output only, rhs copied to x on the device) and gmg_solve from an explicit copy of rhs: the same bits
    x3, it3, res3, _ = eng.solve(P.rhs, x0=np.array(P.rhs, copy=True), tol=tol, stop_type=2, max_iter=100)
    assert it3 == it and res3 == res and np.array_equal(x3, x)


@pytest.mark.parametrize("variant", ["jacobi", "device_coarse", "graph", "exact_gs", "blocked_all", "small_blocks", "lane_per_row_blocks"])
def test_engine_variants(cabi, oracle, variant):
    P = problems.torus_problem(48, 40, "poisson", 60)
    kw = {"jacobi": dict(smoother=cabi.SMOOTHER_JACOBI), "device_coarse": dict(coarse_mode=cabi.COARSE_DEVICE_INVERSE),
          "graph": dict(use_graph=True), "exact_gs": dict(block_rows=0), "blocked_all": dict(block_from_level=0),
          "small_blocks": dict(block_rows=128), "lane_per_row_blocks": dict(block_lanes=1, block_rows=1024)}[variant]
    eng = cabi.Engine(gs_omega=1.0, **kw)            # (no over-relaxation on either side: blocked_all has no colour-major level 0 to relax)
    eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
    x, it, res, _ = eng.solve(P.rhs, tol=1e-6, max_iter=200)
    assert res <= 1e-6
    ref = cabi.Engine(gs_omega=1.0)
    ref.set_prolongations(P.U); ref.set_mass(P.mass); ref.set_system(P.lhs)
    xr, itr, resr, _ = ref.solve(P.rhs, tol=1e-6, max_iter=200)
    assert rel(x, xr) <= 1e-5
    if variant == "blocked_all":
        # level 0 in 30 blocks (runs of 64 points of the hierarchy's cluster order) instead of 4 global colours: 12 cycles against 8 to 1e-6 on this
        # 1 920-vertex mesh (9 with blocks grown breadth-first over the operator, GMG_FINE_BLOCKS_GROWN: profiles/r04/l_fine_blocks_probe.jsonl)
        assert abs(it - itr) <= 5
    elif variant in ("exact_gs", "small_blocks", "lane_per_row_blocks"):
        assert abs(it - itr) <= 2
    elif variant != "jacobi":
        assert it == itr
        assert rel(x, xr) <= 1e-6      # ||x||/||b|| ~ 1e8 on this Poisson system
    if variant == "jacobi":
        # weighted Jacobi sweep == x + w D^-1 (b - A x), checked against the oracle's residual
        A = eng.level_operator(0)
        rng = np.random.default_rng(5)
        b = rng.standard_normal(A.shape[0]); x0 = rng.standard_normal(A.shape[0])
        want = x0 + 0.67 * oracle.residual(A, b, x0) / A.diagonal()
        assert rel(eng.smooth(0, b, x0, 1), want) <= 1e-13


def test_errors_are_loud(cabi):
    eng = cabi.Engine()
    with pytest.raises(cabi.GmgError):
        eng.set_system(sp.identity(10, format="csc"))           # no hierarchy
    P = problems.torus_problem(48, 40, "poisson", 60)
    eng.set_prolongations(P.U)
    bad = P.lhs.tolil(); bad[5, 5] = 0.0
    with pytest.raises(cabi.GmgError) as ei:
        bad = sp.csc_matrix(bad); bad.eliminate_zeros(); eng.set_system(bad)
    assert ei.value.code == cabi.GMG_ERR_NUMERIC
    eng.set_system(P.lhs)
    with pytest.raises(cabi.GmgError):
        eng.residual_norm(P.rhs, P.rhs, 2)                       # mass not set


@pytest.mark.parametrize("kw", [dict(), dict(block_lanes=1)], ids=["default", "big-level-kernels"])
def test_more_than_four_right_hand_sides(cabi, oracle, kw):
    """d > 4 is processed in column chunks of <= 4 (the reference is only safe for d in {1, 3})."""
    P = problems.torus_problem(64, 60, "smoothing", 60)
    rng = np.random.default_rng(11)
    B = P.mass[:, None] * rng.standard_normal((P.n, 6))
    eng = cabi.Engine(**kw)
    eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
    A = eng.level_operator(0)
    X = rng.standard_normal((P.n, 6))
    assert rel(eng.spmv(0, X), A @ X) <= 1e-13
    assert rel(eng.residual(0, B, X), B - A @ X) <= 1e-13
    assert rel(eng.restrict(0, X), P.U[0].T @ X) <= 1e-13
    x, it, res, _ = eng.solve(B, tol=1e-8)
    assert res <= 1e-8
    for t in (0, 2, 3):
        assert abs(eng.residual_norm(B, x, t) - oracle.residual_check(P.lhs, P.mass, B, x, t)) <= 1e-6 * oracle.residual_check(P.lhs, P.mass, B, x, t) + 1e-14
    # each column is solved as if alone: same answer as a d = 1 solve of that column
    x1, _, _, _ = eng.solve(B[:, 4], tol=1e-10)
    xa, _, _, _ = eng.solve(B, tol=1e-10)
    assert rel(xa[:, 4], x1) <= 1e-7


def test_device_coarse_apply_against_the_oracle(setup, cabi, oracle):
    """GMG_COARSE_DEVICE_INVERSE (dense A_L^-1 applied on the device, no host round trip in the cycle) against the ORACLE,
    not against the default engine: the coarsest solve itself (multigrid_solver.cpp:1075, 1401) and whole V-cycles through
    the model assembled from the oracle's operators (tests/vcycle_model.py)."""
    import scipy.sparse.linalg as spla
    from tests.vcycle_model import VcycleModel
    P, _ = setup
    eng = cabi.Engine(coarse_mode=cabi.COARSE_DEVICE_INVERSE)
    eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
    AL = eng.level_operator(len(P.U))
    O = oracle.Hierarchy(P.U, P.mass)
    O.set_system(P.lhs)
    rc = np.random.default_rng(4).standard_normal((AL.shape[0], 3))
    e, eo = eng.coarse_solve(rc), O.coarse_solve(rc)
    nA = spla.norm(AL)
    assert np.linalg.norm(AL @ e - rc) <= 1e-11 * (nA * np.linalg.norm(e) + np.linalg.norm(rc))
    assert np.linalg.norm(AL @ (e - eo)) <= 1e-10 * nA * np.linalg.norm(eo)
    M = VcycleModel(eng, P.U, P.mass, P.lhs, oracle, eng.gs_omega)
    x = P.rhs.copy()
    nL = spla.norm(P.lhs)
    for cyc in range(2):
        xg, xm = eng.vcycle(P.rhs, x), M.vcycle(P.rhs, x)
        assert np.linalg.norm(P.lhs @ (xg - xm)) <= 1e-11 * nL * np.linalg.norm(xm), cyc
        assert rel(xg, xm) <= (1e-10 if "smoothing" in P.name else 1e-5), cyc
        x = xm
    xs, it, res, _ = eng.solve(P.rhs, tol=1e-4)
    xo, ito, reso, _ = O.solve(P.rhs, tol=1e-4)
    assert res <= 1e-4 and it <= ito + 2
    assert abs(oracle.residual_check(P.lhs, P.mass, P.rhs, xs, 2) - res) <= 1e-3 * res + 1e-7


def test_diverged_solve_returns_the_last_iterate_and_says_so(cabi):
    """gmg_solve: like the reference, x always receives the last iterate; an iteration that ends above the tolerance with a residue
    larger than after its first cycle (or not finite) returns GMG_DIVERGED (not an error) and timing key "diverged" = 1, and stops
    as soon as the residue is not finite or 1e4 x the smallest one seen (include/gravomg_hip.h)."""
    P = problems.torus_problem(64, 60, "poisson", 60)
    good = cabi.Engine(); good.set_prolongations(P.U); good.set_mass(P.mass); good.set_system(P.lhs)
    x, it, res, conv = good.solve(P.rhs, tol=1e-4, max_iter=30)
    assert res <= 1e-4 and good.timing("diverged") == 0.0 and not good.diverged
    # a solve that merely runs out of cycles while contracting is NOT "diverged"
    x2, it2, res2, conv2 = good.solve(P.rhs, tol=1e-30, max_iter=2)
    assert it2 == 2 and res2 > 1e-30 and not good.diverged and good.timing("diverged") == 0.0
    assert np.array_equal(conv2[:, 1], conv[:2, 1])
    bad = cabi.Engine(smoother=cabi.SMOOTHER_JACOBI, jacobi_omega=1.95)
    bad.set_prolongations(P.U); bad.set_mass(P.mass); bad.set_system(P.lhs)
    xb, itb, resb, convb = bad.solve(P.rhs, tol=1e-4, max_iter=40)
    assert not (resb <= 1e-4) and bad.diverged and bad.timing("diverged") == 1.0 and len(convb) == itb
    assert 3 <= itb < 40 and convb[-1, 1] > 1e4 * convb[:, 1].min()           # stopped early: blown up
    # the last iterate, not the initial guess: running the same number of cycles on the resident problem gives the same vector
    bad.load_problem(P.rhs, P.rhs); bad.run_cycles(itb, 2)
    assert np.array_equal(np.asarray(xb).reshape(-1), bad.fetch_solution().reshape(-1))
    assert not np.array_equal(np.asarray(xb).reshape(-1), np.asarray(P.rhs).reshape(-1))


def test_profile_cycle_splits_a_cycle_into_its_legs(cabi):
    """gmg_profile_cycle (what bench.py reports as roofline.levels): one entry per smoothed level, the coarsest solve and the residual check; the cycles it
    runs are ordinary cycles (the iterate moves exactly as with gmg_run_cycles) and the legs add up to about one cycle."""
    import time
    P = problems.torus_problem(96, 80, "poisson", 30)
    def engine():
        e = cabi.Engine(); e.set_prolongations(P.U); e.set_mass(P.mass); e.set_system(P.lhs); e.load_problem(P.rhs, P.rhs); return e
    a, b = engine(), engine()
    legs = a.profile_cycle(2, 3)
    b.run_cycles(3, 2)
    assert legs.shape == (a.num_levels + 2,) and np.all(legs > 0) and np.all(legs < 5.0)
    assert np.array_equal(a.fetch_solution(), b.fetch_solution())
    t = time.perf_counter(); b.run_cycles(20, 2); per_cycle = 50 * (time.perf_counter() - t)
    assert 0.3 * per_cycle <= legs.sum() <= 3.0 * per_cycle + 0.1
    a.close(); b.close()



def test_block_sweeps_with_blocks_beyond_the_register_windows(cabi, oracle):
    """gs_block_ep / residual_delta_ep keep 768 explicit and 512 lower entries of a block and 16 lower entries of a row in registers; what a
    block has beyond that goes through their slow paths (and through an LDS region sized by the largest block).  The hierarchy's own Galerkin
    operators stay near 22 entries per row whatever the fine graph is (explicit part of a block <= ~850, lower <= ~470), so this test
    brings its own prolongations: piecewise-constant aggregation of a kNN(120) graph on a structured point set -- coarse rows of 60-120
    entries, every window overflows.  Same checks as on the mesh levels: the sweep against its matrix form, the residual from the sweep's
    explicit part against b - A x."""
    from gravo_mg_amd import meshgen
    n1, n2 = 128, 64
    V, _ = meshgen.torus_mesh(n1, n2)
    S, mass = meshgen.knn_graph_laplacian(V, 120)
    lhs, rhs = meshgen.poisson_system(S, mass, tau=1e-3)
    idx = np.arange(n1 * n2).reshape(n1, n2)
    def aggregate(grid, a, b):
        g1, g2 = grid.shape
        agg = (np.arange(g1)[:, None] // a) * (g2 // b) + (np.arange(g2)[None, :] // b)
        return sp.csc_matrix((np.ones(g1 * g2), (grid.ravel(), agg.ravel())), shape=(g1 * g2, (g1 // a) * (g2 // b))), np.arange((g1 // a) * (g2 // b)).reshape(g1 // a, g2 // b)
    U0, grid1 = aggregate(idx, 2, 2)
    U1, _ = aggregate(grid1, 4, 2)
    P = problems.Problem(V, S, mass, [U0, U1], lhs, rhs, "dense-coarse")
    eng = cabi.Engine(block_lanes=1)
    eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
    e_ptr = np.asarray(eng.debug_sell(1, 7)["slice_ptr"]); l_ptr = np.asarray(eng.debug_sell(1, 6)["slice_ptr"])
    assert len(e_ptr) > 65, "level 1 does not run the entry-parallel sweep"
    over = ((e_ptr[64::64] - e_ptr[:-64:64]).max(), (l_ptr[64::64] - l_ptr[:-64:64]).max(), np.diff(l_ptr).max())
    assert over[0] > 768 and over[1] > 512 and over[2] > 16, over
    _check_block_sweeps(P, eng, oracle)
    rng = np.random.default_rng(5)
    A = eng.level_operator(1)
    absA = abs(A)
    for d in (1, 3):
        b = rng.standard_normal((A.shape[0], d)); x0 = rng.standard_normal((A.shape[0], d))
        x, r = eng.smooth_residual(1, b, x0, 2)
        assert eng.timing("residual_from_sweep") == 1.0
        scale = absA @ abs(x) + abs(b)
        assert np.abs(r - oracle.residual(A, b, x)).max() <= 1e-13 * scale.max()
    eng.close()


@pytest.mark.parametrize("n1,n2,kind,lower_bound", [(190, 190, "smoothing", 1000), (300, 280, "poisson", 1000), (130, 120, "poisson", 300), (64, 60, "poisson", 20)])
def test_device_built_coarse_inverse_against_the_host_factor(cabi, oracle, n1, n2, kind, lower_bound):
    """The dense inverse of the coarsest operator is built ON THE DEVICE from the host's sparse LDL^T factor (setup_kernels.hip.hpp::coarse_inverse_tiles:
    every 16-column tile of the identity through the factor at these sizes, lower triangle mirrored) and applied with the vectors permuted into the factor's
    numbering (gmgk::dense_symv).  Against the host back-substitution with the same factor (GMG_COARSE_HOST_LDLT) and the oracle's coarse solve
    (multigrid_solver.cpp:1075, 1401), at coarsest sizes from one tile to ~6 000 unknowns (94 tiles, the demos' size), three right-hand sides; two
    handles build the same bits (ranks of a multi-GPU job replicate this level)."""
    import scipy.sparse.linalg as spla
    from tests import problems
    P = problems.torus_problem(n1, n2, kind, lower_bound)
    dev = cabi.Engine()                                   # default: GMG_COARSE_AUTO -> device (n_L <= 8192)
    dev.set_prolongations(P.U); dev.set_mass(P.mass); dev.set_system(P.lhs)
    assert dev.timing("coarse_on_device") == 1.0 and dev.timing("coarse_inverse_ms") > 0
    host = cabi.Engine(coarse_mode=cabi.COARSE_HOST_LDLT)
    host.set_prolongations(P.U); host.set_mass(P.mass); host.set_system(P.lhs)
    assert host.timing("coarse_on_device") == 0.0
    AL = dev.level_operator(len(P.U))
    nl = AL.shape[0]
    rc = np.random.default_rng(11).standard_normal((nl, 3))
    e_dev, e_host = dev.coarse_solve(rc), host.coarse_solve(rc)
    nA = spla.norm(AL)
    # the explicit inverse is as accurate as cond(A_L) eps allows (a backward-stable solve is better than that in the residual): both bounds
    # carry the condition of this coarsest operator
    cond = np.linalg.cond(AL.toarray()) if nl <= 2500 else 1e9
    assert np.linalg.norm(AL @ (e_dev - e_host)) <= 1e-14 * cond * nA * np.linalg.norm(e_host) + 1e-10 * nA * np.linalg.norm(e_host)
    assert rel(e_dev, e_host) <= 1e-13 * cond + 1e-9
    O = oracle.Hierarchy(P.U, P.mass)
    O.set_system(P.lhs)
    assert rel(e_dev, O.coarse_solve(rc)) <= 1e-13 * cond + 1e-9
    # one column alone = that column of the block (the product kernel's instantiations for d = 1 and d = 3)
    assert np.array_equal(dev.coarse_solve(rc[:, 1]).ravel(), e_dev[:, 1])
    # symmetric: e = X rc with X = X^T  =>  rc_a . (X rc_b) = rc_b . (X rc_a)
    assert abs(rc[:, 0] @ e_dev[:, 1] - rc[:, 1] @ e_dev[:, 0]) <= 1e-12 * np.abs(rc[:, 0] @ e_dev[:, 1]) + 1e-12 * np.linalg.norm(e_dev)
    other = cabi.Engine()
    other.set_prolongations(P.U); other.set_mass(P.mass); other.set_system(P.lhs)
    assert np.array_equal(other.coarse_solve(rc), e_dev)
    # the solves agree in cycle count and residue
    xd, itd, resd, _ = dev.solve(P.rhs, tol=1e-4)
    xh, ith, resh, _ = host.solve(P.rhs, tol=1e-4)
    assert itd == ith and abs(resd - resh) <= 1e-3 * resh      # (tau = 1e-6: cond(A_L) ~ 1e8 -- the two coarse solves differ by cond x eps)


@pytest.mark.parametrize("kind,d", [("poisson", 1), ("smoothing", 3), ("cloud", 1), ("poisson-mixed", 1), ("poisson-quad", 1), ("smoothing-quad", 3), ("poisson-quad-mixed", 1)])
def test_restriction_fused_with_the_first_pre_sweep_gives_the_same_bits(cabi, kind, d):
    """gmg_config::fuse_restrict_sweep: the restriction into a level on the entry-parallel block sweep also runs that level's first pre-sweep
    (gmgk::restrict_sweep0: the coarse correction starts from zero, multigrid_solver.cpp:1069 + 1072-1073 + the first trip of :1063).  Same operations
    as transfer + gs_block_ep in two launches: cycles and solution bit for bit, for d = 1 and 3 (level-0 residual interleaved), a point cloud
    (blocked level 0) and the fp32 inner cycle; -quad: the small levels keep their quad layout, where the fused form is gs_block4<.., FR = true>."""
    from tests import problems
    if kind == "cloud":
        P = problems.pointcloud_problem(9000, 8, 120)
    else:
        P = problems.torus_problem(300, 280, "smoothing" if kind.startswith("smoothing") else "poisson", 100)
    kw = {} if "quad" in kind else dict(block_lanes=1)            # (one lane per row: the small levels of these problems take the big levels' layout -- the entry-parallel sweep)
    if "mixed" in kind:
        kw["inner_precision"] = 1
    out = []
    for fuse in (1, 0):
        eng = cabi.Engine(fuse_restrict_sweep=fuse, **kw)
        eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
        assert eng.level_blocks(1) is not None
        eng.load_problem(P.rhs, P.rhs)
        hist = eng.run_cycles(3, 2)
        out.append((hist, eng.fetch_solution()))
        eng.close()
    assert P.rhs.shape[1] == d
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("kind,d", [("poisson", 1), ("smoothing", 3), ("poisson-host-coarse", 1), ("poisson-omega1", 1), ("poisson-d2", 2), ("poisson-d4", 4)])
def test_head_of_the_next_cycle_is_enqueued_ahead_of_the_decision_and_changes_nothing(cabi, kind, d):
    """gmg_config::speculate_head: the solve loop (multigrid_solver.cpp:1408-1419) puts the first colour launch of the next cycle into the stream behind
    the residual check before the host has seen the norm; the check's reduction decides on the device whether the iteration goes on, and a stopped
    iteration's launch returns without touching x.  Iterates, iteration counts and residue histories are those of the loop that waits -- when the
    tolerance stops it, when max_iter stops it (no head behind the last allowed cycle), when the first cycle already meets the tolerance (the head
    is in the stream and must do nothing), and for a fixed number of cycles (gmg_run_cycles)."""
    from tests import problems
    P = problems.torus_problem(300, 280, "smoothing" if kind.startswith("smoothing") else "poisson", 100, d=(d if kind.endswith(("-d2", "-d4")) else 1))      # (more right-hand sides: the worst column decides)
    kw = {}
    if "host-coarse" in kind:
        kw["coarse_mode"] = cabi.COARSE_HOST_LDLT
    if "omega1" in kind:
        kw["gs_omega"] = 1.0
    out = []
    for spec in (1, 0):
        eng = cabi.Engine(speculate_head=spec, **kw)
        eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
        res = {}
        for name, tol, max_iter in (("to the tolerance", 1e-6, 100), ("max_iter", 1e-30, 3), ("one cycle allowed", 1e-30, 1), ("first cycle is enough", 1e3, 100),
                                     ("second solve", 1e-5, 100)):
            x, it, r, conv = eng.solve(P.rhs, tol=tol, max_iter=max_iter)
            res[name] = (x.copy(), it, r, conv[:, 1].copy())
        # every norm type the loop can stop on (0: ||r|| / ||b||, 1 / 2: M^-1- / M-weighted, 3: absolute): the device decides with the host's arithmetic
        for t in (0, 1, 2, 3):
            eng.load_problem(P.rhs, P.rhs)
            hist = eng.run_cycles(3, t)
            x, it, r, conv = eng.solve(P.rhs, tol=float(hist[2]) * (1.0 + 1e-12), stop_type=t, max_iter=50)
            res["norm type %d" % t] = (x.copy(), it, r, conv[:, 1].copy())
            assert it <= 3 and r == hist[it - 1]
        if spec:
            assert eng.timing("heads_enqueued") >= res["to the tolerance"][1] + 2 and eng.timing("head_decision_differs") == 0.0
        else:
            assert timing_or_none(eng, "heads_enqueued") is None
        eng.load_problem(P.rhs, P.rhs)
        res["run_cycles"] = (eng.run_cycles(4, 2).copy(), eng.fetch_solution().copy())
        if spec:
            assert eng.timing("heads_enqueued") >= res["to the tolerance"][1] + 2 + 3
        # a cycle through the plain entry points afterwards starts with its own first launch
        eng.load_problem(P.rhs, P.rhs)
        res["then one cycle"] = (eng.run_cycles(1, -1), eng.fetch_solution().copy())
        out.append(res)
        eng.close()
    assert (P.rhs.shape[1] if P.rhs.ndim == 2 else 1) == d
    a, b = out
    assert a["to the tolerance"][1] > 2 and a["max_iter"][1] == 3 and a["one cycle allowed"][1] == 1 and a["first cycle is enough"][1] == 1
    for name in ("to the tolerance", "max_iter", "one cycle allowed", "first cycle is enough", "second solve", "norm type 0", "norm type 1", "norm type 2", "norm type 3"):
        assert a[name][1] == b[name][1], name
        assert a[name][2] == b[name][2], name
        assert np.array_equal(a[name][3], b[name][3]), name
        assert np.array_equal(a[name][0], b[name][0]), name
    assert np.array_equal(a["run_cycles"][0], b["run_cycles"][0]) and np.array_equal(a["run_cycles"][1], b["run_cycles"][1])
    assert np.array_equal(a["then one cycle"][1], b["then one cycle"][1])
    # the stopped iteration's x is the one after its last cycle: one cycle from x0 = rhs, whatever was in the stream behind the check
    assert np.array_equal(a["first cycle is enough"][0], a["one cycle allowed"][0])

