"""gmg_config::device_coloring: level 0 coloured on the device in a cold gmg_set_system (setup_kernels.hip.hpp::jp_round / jp_compact, driven by
engine_setup.hip.hpp::device_jp_coloring).  The specification is the host's jp_coloring_host (tests/test_jp_coloring_host.py pins it): the device
must return its bytes, colour count and round count exactly -- on every pattern of tests/jp_coloring_cases.py, at the wave boundary (63, 64, 65
rows), with a worklist that ends inside a workgroup (4 097 rows), and in cases whose rounds outlast the rounds over all rows
(jp_coloring_cases.FULL_ROUNDS = 4: the path graph takes 5 rounds, the complete graph 70), so that the compacted worklist runs.  Then the option
in the engine: it reaches the ordering, the cycle is still the modelled cycle on the reported ordering, off and every fallback are bitwise the
default, a renumbered level 0 takes the colours too, and the values-only refresh behind a cold set-up gives a fresh handle's bits."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from tests import jp_coloring_cases as cases
from tests import problems
from tests.parity_checks import check_multicolor_gs, rel

pytestmark = pytest.mark.gpu

ALL_CASES = {**cases.cases(), **cases.boundary_cases()}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _engine(cabi, P, lhs=None, **kw):
    e = cabi.Engine(**kw)
    e.set_prolongations(P.U); e.set_mass(P.mass); e.set_system(P.lhs if lhs is None else lhs)
    return e


def _class_sizes(eng, A):
    """Real rows per colour class of level 0 in device order, after checking that the ordering is a permutation and the classes are proper for A."""
    new2old, cb = eng.level_ordering(0)
    n = A.shape[0]
    assert np.array_equal(np.sort(new2old[new2old >= 0]), np.arange(n))
    colour_of = np.full(n, -1)
    sizes = []
    for c in range(len(cb) - 1):
        rows = new2old[cb[c]:cb[c + 1]]
        rows = rows[rows >= 0]
        colour_of[rows] = c
        sizes.append(len(rows))
    coo = sp.coo_matrix(A)
    off = coo.row != coo.col
    assert np.all(colour_of[coo.row[off]] != colour_of[coo.col[off]])
    return sizes


def _three_cycles(eng, rhs):
    rhs = np.asfortranarray(rhs if rhs.ndim == 2 else rhs[:, None])
    eng.load_problem(rhs, rhs)
    hist = eng.run_cycles(3, 2).copy()
    return hist, eng.fetch_solution()


def _same_handle_results(a, b, rhs):
    for k in range(a.num_levels):
        for u, v in zip(a.level_ordering(k), b.level_ordering(k)):
            assert np.array_equal(u, v), k
    (ha, xa), (hb, xb) = _three_cycles(a, rhs), _three_cycles(b, rhs)
    assert same(ha, hb) and same(xa, xb)


# ---------------------------------------------------------------------------------------------- device against specification
@pytest.fixture(scope="module")
def lender(cabi):
    assert cabi.device_count() > 0, "gpu tests need a HIP device"
    return cabi.Engine()              # lends its stream and pool to gmg_jp_coloring_device


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_device_colours_are_the_specifications(cabi, lender, name):
    indptr, indices = ALL_CASES[name]
    want, want_ncol, want_rounds = cabi.jp_coloring(indptr, indices)
    got, ncol, rounds = cabi.jp_coloring(indptr, indices, eng=lender)
    print(f"\n[device_coloring] {name}: n {len(indptr) - 1} colours {want_ncol} rounds {want_rounds} (device: {ncol}, {rounds})")
    assert (ncol, rounds) == (want_ncol, want_rounds)
    assert np.array_equal(got, want)
    if name in ("path300", "complete70"):
        assert want_rounds > cases.FULL_ROUNDS         # the rounds over the compacted worklist ran


def test_device_reports_minus_one_like_the_host(cabi, lender):
    indptr, indices = cases.complete(300)
    assert cabi.jp_coloring(indptr, indices, eng=lender) == (None, -1, 0)
    got, ncol, rounds = cabi.jp_coloring(*cases.complete(254), eng=lender)
    assert ncol == 254 and rounds == 254 and sorted(got) == list(range(254))
    # ... and refuses arrays that would take the kernels out of bounds
    with pytest.raises(cabi.GmgError) as e:
        cabi.jp_coloring(np.array([0, 1, 2], np.int32), np.array([1, 2], np.int32), eng=lender)
    assert e.value.code == cabi.GMG_ERR_INVALID


# ---------------------------------------------------------------------------------------------- the option in the engine
def test_the_option_reaches_the_engine(cabi):
    """Fails without the feature: the ordering of level 0 is the counting sort of the specification's colours."""
    P = problems.torus_problem(48, 48, "poisson", 60)
    eng = _engine(cabi, P, device_coloring=1, row_align=64, block_from_level=1)
    assert eng.timing("colored_on_device") == 1.0
    assert eng.timing("device_coloring_rounds") >= 1 and eng.timing("device_coloring_ms") > 0
    a = cabi._csc(P.lhs)
    colours, ncol, rounds = cabi.jp_coloring(a.indptr, a.indices)
    assert eng.timing("device_coloring_rounds") == rounds
    sizes = _class_sizes(eng, a)
    assert len(sizes) == ncol and sizes == sorted(np.bincount(colours, minlength=ncol).tolist())
    # the rows of a class keep the input order (no renumbering here): class by class, ascending vertex numbers of one colour
    new2old, cb = eng.level_ordering(0)
    for c in range(ncol):
        rows = new2old[cb[c]:cb[c + 1]]; rows = rows[rows >= 0]
        assert len(set(colours[rows])) == 1


def test_sweep_is_gauss_seidel_on_the_reported_ordering(cabi, oracle):
    """gs_omega = 1, block_rows = 0: a sweep is the oracle's Gauss-Seidel on the system permuted by the reported ordering (1e-12, as in
    tests/test_gpu_parity.py), level 0 included -- with colours from the device."""
    P = problems.torus_problem(48, 48, "poisson", 60)
    eng = _engine(cabi, P, device_coloring=1, gs_omega=1.0, block_rows=0)
    assert eng.timing("colored_on_device") == 1.0
    check_multicolor_gs(P, eng, oracle)


@pytest.mark.parametrize("kind", ["poisson", "smoothing"])
def test_default_cycle_matches_the_model_on_the_reported_orderings(cabi, oracle, kind):
    """tests/vcycle_model.py with its tolerances of tests/test_gpu_parity.py::test_default_engine_vcycles_match_model_per_cycle."""
    import scipy.sparse.linalg as spla
    from tests.vcycle_model import VcycleModel
    P = problems.torus_problem(48, 48, kind, 60)
    eng = _engine(cabi, P, device_coloring=1)
    assert eng.timing("colored_on_device") == 1.0
    M = VcycleModel(eng, P.U, P.mass, P.lhs, oracle, eng.gs_omega)
    nA = spla.norm(P.lhs)
    xg = eng.vcycle(P.rhs, P.rhs.copy())
    xm = M.vcycle(P.rhs, P.rhs.copy())
    assert np.linalg.norm(P.lhs @ (xg - xm)) <= 1e-12 * nA * np.linalg.norm(xm)
    assert rel(xg, xm) <= (1e-11 if "smoothing" in P.name else 1e-6)


def test_solve_converges_to_the_solution_of_the_greedy_ordering(cabi, oracle):
    """Two converged solves of one system, stopped by the same rule at 1e-4 (mass-weighted relative residual): the smoothing system M + tau S is
    well conditioned in the M-norm, so solutions whose residuals are both below 1e-4 agree to 1e-3 relative in that norm."""
    P = problems.torus_problem(48, 48, "smoothing", 60)
    on, off = _engine(cabi, P, device_coloring=1), _engine(cabi, P, device_coloring=0)
    assert on.timing("colored_on_device") == 1.0 and off.timing("colored_on_device") == 0.0
    x1, it1, res1, _ = on.solve(P.rhs, tol=1e-4, stop_type=2, max_iter=100)
    x0, it0, res0, _ = off.solve(P.rhs, tol=1e-4, stop_type=2, max_iter=100)
    m = P.mass[:, None]
    dx = np.sqrt((m * (x1 - x0) ** 2).sum() / (m * x0 ** 2).sum())
    print(f"\n[device_coloring] solve: cycles on {it1} off {it0}, residues {res1:.3e} {res0:.3e}, M-norm difference {dx:.3e}")
    assert not on.diverged and res1 <= 1e-4 and res0 <= 1e-4
    for x, res in ((x1, res1), (x0, res0)):
        chk = oracle.residual_check(P.lhs, P.mass, P.rhs, x, 2)
        assert chk <= 1e-4 * (1 + 1e-3) and abs(chk - res) <= 1e-3 * res
    assert dx <= 1e-3


# ---------------------------------------------------------------------------------------------- off means off
def test_off_is_the_default_handle_bit_for_bit(cabi):
    P = problems.torus_problem(48, 48, "poisson", 60)
    off, plain = _engine(cabi, P, device_coloring=0), _engine(cabi, P)
    assert off.timing("colored_on_device") == 0.0 and plain.timing("colored_on_device") == 0.0
    assert off.timing("device_coloring_ms") == 0.0 and off.timing("device_coloring_rounds") == 0.0
    _same_handle_results(off, plain, P.rhs)


@pytest.mark.parametrize("why", ["blocked-fine-level", "chebyshev"])
def test_failed_preconditions_leave_the_host_colouring(cabi, why):
    if why == "blocked-fine-level":
        P, kw = problems.pointcloud_problem(3000), {}                      # kNN Laplacian: gmg_config::block_fine blocks level 0
    else:
        P, kw = problems.torus_problem(48, 48, "poisson", 60), {"smoother": cabi.SMOOTHER_CHEBYSHEV}
    on, off = _engine(cabi, P, device_coloring=1, **kw), _engine(cabi, P, device_coloring=0, **kw)
    if why == "blocked-fine-level":
        assert on.level_blocks(0) is not None
    assert on.timing("colored_on_device") == 0.0 and on.timing("device_coloring_rounds") == 0.0
    _same_handle_results(on, off, P.rhs)


# ---------------------------------------------------------------------------------------------- renumbered level 0
@pytest.mark.parametrize("source", ["prolongations", "hierarchy"])
def test_renumbered_level0_takes_the_device_colours(cabi, source):
    """A torus in random vertex order with reorder_fine = 1: the visit order decides the sequence of the rows inside a class, the colours are
    the specification's.  hierarchy: the handle knows the hierarchy's cluster order (the base order is chosen on the device); prolongations: it
    grows patches itself."""
    from gravo_mg_amd import meshgen
    P = problems.torus_problem(48, 40, "poisson", 60, order="random")
    eng = cabi.Engine(device_coloring=1, reorder_fine=1)
    if source == "hierarchy":
        H = cabi.Hierarchy(P.V, meshgen.neighbors_from_stiffness(P.S), lower_bound=60)
        eng.use_hierarchy(H)
    else:
        eng.set_prolongations(P.U)
    eng.set_mass(P.mass); eng.set_system(P.lhs)
    assert eng.timing("colored_on_device") == 1.0
    a = cabi._csc(P.lhs)
    colours, ncol, _ = cabi.jp_coloring(a.indptr, a.indices)
    assert _class_sizes(eng, a) == sorted(np.bincount(colours, minlength=ncol).tolist())
    x, it, res, _ = eng.solve(P.rhs, tol=1e-4, stop_type=2, max_iter=100)
    assert not eng.diverged and res <= 1e-4


# ---------------------------------------------------------------------------------------------- refresh and cache
def test_refresh_behind_a_device_coloured_set_up(cabi):
    P = problems.torus_problem(48, 48, "smoothing", 60)
    lhs2 = (sp.diags(P.mass) + 5e-3 * P.S).tocsc()
    eng = _engine(cabi, P, device_coloring=1)
    assert eng.timing("colored_on_device") == 1.0 and eng.timing("setup_values_only") == 0.0
    eng.set_system(lhs2)
    assert eng.timing("setup_values_only") == 1.0
    fresh = _engine(cabi, P, lhs=lhs2, device_coloring=1)
    assert fresh.timing("colored_on_device") == 1.0
    _same_handle_results(eng, fresh, P.rhs)
    lhs3 = lhs2.copy(); lhs3.data *= 1.5
    eng.set_system(lhs3)
    assert eng.timing("setup_ordering_cached") == 1.0
    x, it, res, _ = eng.solve(P.rhs, tol=1e-6)
    assert res <= 1e-6


# ---------------------------------------------------------------------------------------------- configuration
def test_configuration(cabi):
    with pytest.raises(cabi.GmgError) as e:
        cabi.Engine(device_coloring=2)
    assert e.value.code == cabi.GMG_ERR_INVALID
    assert cabi.lib().gmg_config_size() == C.sizeof(cabi.GmgConfig)
