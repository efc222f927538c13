"""gmg_config::reorder_pointwise on a real device: the locality renumbering of level 0 (reorder_fine) for the pointwise smoothers.

The system: a 64 x 64 torus mesh (4 096 vertices) in a RANDOM vertex permutation, lhs = M + S, with reorder_fine = 1.  The automatic mode
(reorder_fine = 2) asks for n > 65 536 and a mean |row - column| over the stored entries above max(32 768, n / 32)
(host_plan.hpp::wants_locality_reorder, the function both smoothers call).  A random numbering of a mesh with seven entries per row, the
diagonal among them, has a mean of 6 / 7 x n / 3, so the rule first engages at n > 114 689: one case runs it on a 346 x 346 torus (119 716
vertices, mean about 34 200).

The locality figure: mean |new(i) - new(j)| over the stored entries of the system.  A random numbering gives about n / 3 (1 365 here); the
cluster order and the breadth-first order of a surface mesh of this size give tens of rows, so the asked-for quarter is a loose cap.
gmg_host_plan_level (the host planner's entry point) cannot express the case on the CPU: it colours what it orders (multicolor = true in all of
its modes), and the one-class ordering of a pointwise smoother is what this option is about; the figure is therefore held on the device's
ordering only.

Bounds.  A renumbering changes the order in which a row's products are added and nothing else, so two evaluations of the same row are each within
gamma_m = m u / (1 - m u) (u = 2^-53, m the row's entry count + the added vector) of the exact value relative to the sum of the absolute
products (Higham, Accuracy and Stability, 3.1): |a - b|_i <= 2 gamma_(m_i + 2) (|A| |x| + |b|)_i componentwise, for gmg_spmv, gmg_residual,
gmg_restrict and gmg_prolong_add with their own matrices.  The smoothing steps compound: they are held to what tests/test_gpu_chebyshev.py
holds a device step to against the model (_step_close: 1e-13 relative + its floor), the cycles to that file's cycle tolerances against
tests/chebyshev_model.py (backward 1e-12 ||A|| ||x||, forward 1e-11 on an M + S system)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
from scipy.sparse.csgraph import breadth_first_order

from gravo_mg_amd import meshgen
from tests.chebyshev_model import ChebyshevModel
from tests.parity_checks import rel
from tests.test_gpu_chebyshev import _step_close

pytestmark = pytest.mark.gpu

JACOBI, CHEBYSHEV = 1, 2
U64 = 2.0 ** -53


class Mesh:
    def __init__(self, n1, n2):
        from gravo_mg_amd import cabi
        self.V, F = meshgen.torus_mesh(n1, n2, order="random")
        self.S, self.mass = meshgen.cotan_laplacian(self.V, F)
        self.H = cabi.Hierarchy(self.V, meshgen.neighbors_from_stiffness(self.S), lower_bound=40)          # (4 096 -> 512 -> 64: two smoothed levels)
        self.U = self.H.U
        self.lhs, _ = meshgen.smoothing_system(self.S, self.mass, self.V)
        self.lhs = sp.csc_matrix(self.lhs)
        self.lhs.sort_indices()
        self.n = self.lhs.shape[0]
        # a breadth-first order of the points over the system's graph: what a caller hands over with gmg_set_fine_order (the hierarchy builder
        # makes one itself only above 65 536 points)
        self.bfs = np.asarray(breadth_first_order(sp.csr_matrix(self.lhs), 0, directed=False, return_predecessors=False), dtype=np.int32)
        assert np.array_equal(np.sort(self.bfs), np.arange(self.n))


@functools.lru_cache(maxsize=None)
def _mesh(n1=64, n2=64):
    return Mesh(n1, n2)


SOURCES = ("bfs", "levels")


def _engine(cabi, P, source, lhs=None, **kw):
    """source "bfs": the hierarchy set level by level with a breadth-first order handed over (both base orders at hand: the set-up scores them);
    "levels": level by level without one (the cluster order alone); "built": the builder's hierarchy object (gmg_use_hierarchy: the point graph for
    prepare_structure, and above 65 536 points in a numbering without locality its own breadth-first order)."""
    eng = cabi.Engine(**dict(dict(smoother=CHEBYSHEV, reorder_fine=1), **kw))
    if source == "built":
        eng.use_hierarchy(P.H)
    elif source == "bfs":
        eng.set_prolongations(P.U, fine_order=P.bfs)
    else:
        assert source == "levels"
        eng.set_prolongations(P.U)
    eng.set_mass(P.mass)
    eng.set_system(P.lhs if lhs is None else lhs)
    return eng


@functools.lru_cache(maxsize=None)
def _cached(source, cfg=()):
    from gravo_mg_amd import cabi
    return _engine(cabi, _mesh(), source, **dict(cfg))


def _mean_distance(lhs, old2new):
    coo = sp.coo_matrix(lhs)
    return float(np.mean(np.abs(old2new[coo.row].astype(np.int64) - old2new[coo.col].astype(np.int64))))


def _old2new(eng, n):
    new2old, color_begin = eng.level_ordering(0)
    real = new2old >= 0
    assert real.sum() == n and np.array_equal(np.sort(new2old[real]), np.arange(n))          # a permutation of the rows
    assert len(color_begin) == 2 and color_begin[0] == 0 and color_begin[1] == len(new2old)  # one class: nothing is coloured
    assert np.all(real[:n]) and not np.any(real[n:])                                         # the real rows first, padding behind them
    old2new = np.empty(n, np.int64)
    old2new[new2old[:n]] = np.arange(n)
    return old2new, new2old


@pytest.mark.parametrize("device_setup", [1, 0])
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("smoother", [CHEBYSHEV, JACOBI], ids=["chebyshev", "jacobi"])
def test_ordering_is_one_class_in_a_locality_order(cabi, smoother, source, device_setup):
    P = _mesh()
    eng = _cached(source, (("smoother", smoother), ("reorder_pointwise", 1), ("device_setup", device_setup)))
    assert eng.timing("fine_level_reordered") == 1
    old2new, _ = _old2new(eng, P.n)
    before, after = _mean_distance(P.lhs, np.arange(P.n)), _mean_distance(P.lhs, old2new)
    choice, sc, sb = eng.timing("base_order_choice"), eng.timing("base_order_score_cluster"), eng.timing("base_order_score_bfs")
    print(f"\nREORDER smoother {smoother} base order from {source} device_setup {device_setup}: mean |new(i) - new(j)| {before:.1f} -> {after:.1f} "
          f"(n / 3 = {P.n / 3:.0f}); base order {choice:.0f}, scores cluster {sc:.3f} bfs {sb:.3f}")
    assert before > P.n / 4                                      # the caller's numbering is a random one
    assert after < 0.25 * before
    assert choice in (0.0, 1.0)
    if source == "bfs":                                          # both base orders at hand: both were scored, the better one taken
        assert sc > 0 and sb > 0 and choice == (1.0 if sb < sc else 0.0)
    else:                                                        # the cluster order alone
        assert choice == 0.0


@pytest.mark.parametrize("smoother", [CHEBYSHEV, JACOBI], ids=["chebyshev", "jacobi"])
def test_field_at_zero_keeps_the_callers_numbering(cabi, smoother):
    P = _mesh()
    for kw in (dict(reorder_pointwise=0), dict()):
        eng = _engine(cabi, P, "built", smoother=smoother, **kw)
        old2new, _ = _old2new(eng, P.n)
        assert np.array_equal(old2new, np.arange(P.n)) and eng.timing("fine_level_reordered") == 0
        eng.close()
    # reorder_fine = 0 with the field set: the decision is reorder_fine's
    eng = _engine(cabi, P, "built", smoother=smoother, reorder_pointwise=1, reorder_fine=0)
    assert np.array_equal(_old2new(eng, P.n)[0], np.arange(P.n)) and eng.timing("fine_level_reordered") == 0
    eng.close()
    # the multicolour smoother: the key is what its path implies, with and without the field, and the field changes nothing
    a, b = _engine(cabi, P, "built", smoother=cabi.SMOOTHER_MULTICOLOR_GS, reorder_pointwise=1), _engine(cabi, P, "built", smoother=cabi.SMOOTHER_MULTICOLOR_GS)
    assert a.timing("fine_level_reordered") == b.timing("fine_level_reordered") == 1
    assert np.array_equal(a.level_ordering(0)[0], b.level_ordering(0)[0])
    rhs = P.mass[:, None] * np.random.default_rng(1).standard_normal((P.n, 2))
    assert np.array_equal(a.vcycle(rhs, rhs), b.vcycle(rhs, rhs))
    a.close(); b.close()


def _gamma(m):
    return m * U64 / (1.0 - m * U64)


@pytest.mark.parametrize("source", SOURCES)
def test_level0_operators_agree_with_the_unreordered_handle(cabi, oracle, source):
    """gmg_spmv, gmg_residual, gmg_restrict, gmg_prolong_add componentwise (module docstring); gmg_smooth as a device step is held to the model."""
    P = _mesh()
    on, off = _cached(source, (("reorder_pointwise", 1),)), _cached(source, ())
    A, U0 = sp.csr_matrix(P.lhs), sp.csr_matrix(P.U[0])
    absA, absU, absUt = abs(A), abs(U0), abs(U0).T.tocsr()
    mA, mU, mUt = int(np.diff(A.indptr).max()), int(np.diff(U0.indptr).max()), int(np.diff(absUt.indptr).max())
    rng = np.random.default_rng(8)
    worst = {}

    def held(what, got, want, bound):
        assert np.all(np.abs(got - want) <= bound), (what, float(np.max(np.abs(got - want) / np.maximum(bound, 1e-300))))
        worst[what] = max(worst.get(what, 0.0), float(np.max(np.abs(got - want) / np.maximum(bound, 1e-300))))

    for d in (1, 3, 5):
        x, b = rng.standard_normal((P.n, d)), rng.standard_normal((P.n, d))
        e = rng.standard_normal((P.U[0].shape[1], d))
        held("spmv", on.spmv(0, x), off.spmv(0, x), 2 * _gamma(mA + 2) * (absA @ np.abs(x)))
        held("residual", on.residual(0, b, x), off.residual(0, b, x), 2 * _gamma(mA + 2) * (absA @ np.abs(x) + np.abs(b)))
        held("restrict", on.restrict(0, b), off.restrict(0, b), 2 * _gamma(mUt + 2) * (absUt @ np.abs(b)))
        held("prolong_add", on.prolong_add(0, e, x), off.prolong_add(0, e, x), 2 * _gamma(mU + 2) * (absU @ np.abs(e) + np.abs(x)))
    print(f"\nREORDER operators (base order from {source}): largest deviation as a fraction of the bound {worst}")
    M = ChebyshevModel(None, P.U, P.mass, P.lhs, oracle, on.timing("cheby_ratio"))
    for d in (1, 3):
        x, b = rng.standard_normal((P.n, d)), rng.standard_normal((P.n, d))
        for iters in (1, 2, 3, 5):
            want = M.smooth(0, b, x, iters)
            _step_close(M, 0, b, x, iters, on.smooth(0, b, x, iters), want)
            _step_close(M, 0, b, x, iters, on.smooth(0, b, x, iters), off.smooth(0, b, x, iters))


@pytest.mark.parametrize("pair", [(2, 2), (1, 3)], ids=["2+2", "1+3"])
def test_cycles_match_the_model(cabi, oracle, pair):
    """Three consecutive V-cycles cycle by cycle against tests/chebyshev_model.py, each restarted from the model's iterate (the tolerances of
    tests/test_gpu_chebyshev.py::test_cycles_match_the_model for an M + S system); the fp32 inner cycle at its 2e-5."""
    P = _mesh()
    cfg = (("reorder_pointwise", 1), ("pre_iters", pair[0]), ("post_iters", pair[1]))
    e64, e32 = _cached("bfs", cfg), _cached("bfs", cfg + (("inner_precision", 1),))
    M = ChebyshevModel(None, P.U, P.mass, P.lhs, oracle, e64.timing("cheby_ratio"), pre=pair[0], post=pair[1])
    nA = spla.norm(P.lhs)
    for d in (1, 3):
        b = P.mass[:, None] * np.random.default_rng(40 + d).standard_normal((P.n, d))
        x = b.copy()
        for cyc in range(3):
            xm, xg = M.vcycle(b, x), e64.vcycle(b, x)
            back, fwd = np.linalg.norm(P.lhs @ (xg - xm)), rel(xg, xm)
            assert back <= 1e-12 * nA * np.linalg.norm(xm), (d, cyc, back / (nA * np.linalg.norm(xm)))
            assert fwd <= 1e-11, (d, cyc, fwd)
            assert np.linalg.norm(e32.vcycle(b, x) - xm) <= 2e-5 * np.linalg.norm(xm), ("fp32 inner", d, cyc)
            x = xm


@pytest.mark.parametrize("smoother", [CHEBYSHEV, JACOBI], ids=["chebyshev", "jacobi"])
def test_pcg_takes_the_iteration_count_of_the_unreordered_handle(cabi, smoother):
    P = _mesh()
    rhs = np.asfortranarray(P.mass[:, None] * np.random.default_rng(12).standard_normal((P.n, 3)))
    on, off = _cached("bfs", (("smoother", smoother), ("pcg", 1), ("reorder_pointwise", 1))), _cached("bfs", (("smoother", smoother), ("pcg", 1)))
    a, b = on.solve(rhs, tol=1e-8, stop_type=2, max_iter=60), off.solve(rhs, tol=1e-8, stop_type=2, max_iter=60)
    print(f"\nREORDER pcg smoother {smoother}: iterations {a[1]} / {b[1]}, residues {a[2]:.3e} / {b[2]:.3e}, x {rel(a[0], b[0]):.3e}")
    assert a[1] == b[1] and a[2] <= 1e-8 and not on.diverged
    assert rel(a[0], b[0]) <= 1e-6


@pytest.mark.parametrize("device_setup", [1, 0])
def test_setup_paths_give_the_bits_of_a_fresh_handle(cabi, device_setup):
    """A second gmg_set_system with the same pattern -- the values-only refresh on the device path, the ordering-cache hit under the host planner --
    and a handle whose structure was prepared at gmg_finalize_hierarchy (prepare_structure = 1 with the builder's hierarchy): the ordering, the
    key and the bits of a fresh handle on the second system."""
    P = _mesh()
    lhs2 = (P.lhs + sp.diags(P.lhs.diagonal())).tocsc()
    lhs2.sort_indices()
    rhs = np.asfortranarray(P.mass[:, None] * np.random.default_rng(13).standard_normal((P.n, 3)))
    kw = dict(reorder_pointwise=1, device_setup=device_setup)
    fresh = _engine(cabi, P, "built", lhs=lhs2, prepare_structure=0, **kw)
    want_order = fresh.level_ordering(0)[0]
    want = fresh.vcycle(rhs, rhs), fresh.solve(rhs, tol=1e-8, max_iter=10)[0]
    live = _engine(cabi, P, "built", prepare_structure=0, **kw)
    live.vcycle(rhs, rhs)
    live.set_system(lhs2)
    if device_setup:
        assert live.timing("setup_values_only") == 1
    else:
        assert live.timing("setup_ordering_cached") == 1 and live.timing("setup_values_only") == 0
    prepared = cabi.Engine(smoother=CHEBYSHEV, reorder_fine=1, prepare_structure=1, **kw)
    prepared.use_hierarchy(P.H); prepared.set_mass(P.mass); prepared.set_system(lhs2)
    if device_setup:
        assert prepared.timing("setup_structure_prepared") == 1
    for eng in (live, prepared):
        assert eng.timing("fine_level_reordered") == 1 and np.array_equal(eng.level_ordering(0)[0], want_order)
        assert np.array_equal(eng.vcycle(rhs, rhs), want[0]) and np.array_equal(eng.solve(rhs, tol=1e-8, max_iter=10)[0], want[1])
    for eng in (fresh, live, prepared):
        eng.close()


@pytest.mark.parametrize("more", [(), (("pcg", 1),), (("inner_precision", 1),), (("accelerate", 3),), (("use_graph", True), ("pcg", 1))],
                         ids=["plain", "pcg", "mixed", "accelerate3", "graph-pcg"])
def test_both_fields_together(cabi, more):
    """On the permuted mesh, renumbered: zero_guess_step = 1 gives the bits of the same handle with zero_guess_step = 0."""
    P = _mesh()
    rhs = np.asfortranarray(P.mass[:, None] * np.random.default_rng(14).standard_normal((P.n, 3)))
    cfg = (("reorder_pointwise", 1),) + more
    on, off = _cached("bfs", cfg + (("zero_guess_step", 1),)), _cached("bfs", cfg)
    assert on.timing("fine_level_reordered") == 1
    a, b = on.solve(rhs, tol=1e-8, stop_type=2, max_iter=12), off.solve(rhs, tol=1e-8, stop_type=2, max_iter=12)
    assert a[1] == b[1] and a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[3][:, 1], b[3][:, 1])
    assert np.array_equal(on.vcycle(rhs, rhs), off.vcycle(rhs, rhs))
    assert on.timing("zero_guess_steps") + on.timing("restrict_steps_fused") > 0


def test_automatic_mode_above_its_threshold(cabi):
    """reorder_fine = 2 (the default) on 119 716 vertices in random order (module docstring): wants_locality_reorder's own rule decides for the
    pointwise handle as it does for the multicolour one; with the field at 0 nothing is renumbered."""
    P = _mesh(346, 346)
    assert P.n > 114689 and len(P.U) >= 2
    eng = _engine(cabi, P, "built", reorder_pointwise=1, reorder_fine=2)
    gs = _engine(cabi, P, "built", smoother=cabi.SMOOTHER_MULTICOLOR_GS, reorder_fine=2)
    old2new, _ = _old2new(eng, P.n)
    before, after = _mean_distance(P.lhs, np.arange(P.n)), _mean_distance(P.lhs, old2new)
    print(f"\nREORDER automatic: mean |new(i) - new(j)| {before:.1f} -> {after:.1f}")
    assert eng.timing("fine_level_reordered") == gs.timing("fine_level_reordered") == 1 and after < 0.25 * before
    # (at this size the builder's hierarchy brings its own breadth-first order: both base orders were scored, as on the multicolour handle)
    assert P.H.fine_order is not None and eng.timing("base_order_score_bfs") > 0 and eng.timing("base_order_score_cluster") > 0
    assert eng.timing("base_order_choice") == gs.timing("base_order_choice")
    off = _engine(cabi, P, "built", reorder_pointwise=0, reorder_fine=2)
    assert off.timing("fine_level_reordered") == 0
    for e in (eng, gs, off):
        e.close()
