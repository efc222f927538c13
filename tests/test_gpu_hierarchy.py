"""GPU-suite copy of the hierarchy parity check: the product's hierarchy builder (gmg_hierarchy_build, host_hierarchy.hpp)
against the independent pure-Python restatement of the reference's constructProlongation (oracle/hierarchy_restatement.py) --
same levels, same parents, same weights -- on the five BASELINE workload TYPES at sizes the Python version handles, and the
engine consuming that hierarchy: same Galerkin operators as the oracle given the restatement's U, same solve."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu


def _workload(kind):
    from gravo_mg_amd import meshgen
    if kind == "pointcloud":
        V = meshgen.torus_points(2500, noise=0.003)
        S, mass = meshgen.knn_graph_laplacian(V, 8)
        lhs, rhs = meshgen.poisson_system(S, mass)
    else:
        V, F = meshgen.torus_mesh(48, 40, order="random" if kind == "poisson-random" else "natural")
        S, mass = meshgen.cotan_laplacian(V, F)
        if kind == "smoothing-d3":
            lhs, rhs = meshgen.smoothing_system(S, mass, V)
        elif kind == "bilaplacian":
            lhs, rhs = meshgen.smoothing_system(meshgen.bilaplacian(S, mass), mass, V[:, :1], tau=1e-9)
        else:
            lhs, rhs = meshgen.poisson_system(S, mass)
    return V, meshgen.neighbors_from_stiffness(S), mass, lhs, rhs


@pytest.mark.parametrize("kind", ["smoothing-d3", "poisson", "pointcloud", "poisson-random", "bilaplacian"])
def test_builder_matches_restatement_and_engine_consumes_it(cabi, oracle, kind):
    V, neigh, mass, lhs, rhs = _workload(kind)
    H = cabi.Hierarchy(V, neigh, lower_bound=12)
    want = _restatement(kind)
    assert len(H.U) == len(want) >= 2
    for k, (a, b) in enumerate(zip(H.U, want)):
        a, b = sp.csc_matrix(a), sp.csc_matrix(b)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices), f"level {k}: different parents"
        np.testing.assert_allclose(a.data, b.data, rtol=1e-9, atol=1e-12)
    # the engine on the product's hierarchy vs the oracle on the restatement's: same Galerkin operators, same solve
    eng = cabi.Engine()
    eng.use_hierarchy(H); eng.set_mass(mass); eng.set_system(lhs)
    O = oracle.Hierarchy(want, mass)
    O.set_system(lhs)
    for k in range(1, len(want) + 1):
        A, Ao = eng.level_operator(k), O.level_operator(k)
        assert abs(A - Ao).max() <= 1e-9 * abs(Ao).max()
    tol = 1e-2 if kind == "bilaplacian" else 1e-4
    x, it, res, _ = eng.solve(rhs, tol=tol, max_iter=100)
    xo, ito, reso, _ = O.solve(rhs, tol=tol, max_iter=100)
    assert res <= tol and reso <= tol and it <= ito + 2
    m = mass[:, None]
    assert np.sqrt((m * (x - xo) ** 2).sum() / (m * xo ** 2).sum()) <= 20 * tol


@pytest.mark.parametrize("kind,weighting,nested", [("torus", 0, False), ("torus-random", 0, False), ("sphere", 0, False), ("pointcloud", 0, False),
                                                    ("torus", 2, False), ("torus", 1, True)])
def test_device_selection_stage_gives_the_host_bits(cabi, kind, weighting, nested):
    """The per-point parent selection (multigrid_solver.cpp:291-452) runs on the GPU for levels of >= 200 k points
    (csrc/hierarchy_kernels.hip.hpp); U must be bit-identical to the host loop's (gmg_hierarchy_options::use_device = 0), whatever the mesh."""
    import os
    from gravo_mg_amd import meshgen
    if kind.startswith("torus"):
        V, F = meshgen.torus_mesh(520, 500, order="random" if kind.endswith("random") else "natural")
        S, _ = meshgen.cotan_laplacian(V, F)
        neigh = meshgen.neighbors_from_stiffness(S)
    elif kind == "sphere":
        V, F = meshgen.sphere_mesh(230_000)
        S, _ = meshgen.cotan_laplacian(V, F)
        neigh = meshgen.neighbors_from_stiffness(S)
    else:
        V = meshgen.torus_points(240_000, noise=0.002)
        S, _ = meshgen.knn_graph_laplacian(V, 8)
        neigh = meshgen.neighbors_from_stiffness(S)
    Hh = cabi.Hierarchy(V, neigh, weighting=weighting, nested=nested, use_device=False)
    Hd = cabi.Hierarchy(V, neigh, weighting=weighting, nested=nested)
    assert Hh.timing("selection_on_device") == 0.0 and Hd.timing("selection_on_device") >= 1.0
    assert len(Hh.U) == len(Hd.U) >= 2
    for a, b in zip(Hh.U, Hd.U):
        assert a.shape == b.shape
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
        assert np.array_equal(a.data, b.data)            # bitwise


# ---- the device stage end to end at small size: gmg_hierarchy_options::use_device = 2 runs it on every level whatever its size
SMALL_INPUTS = ["smoothing-d3", "poisson", "pointcloud", "poisson-random", "bilaplacian", "open-cylinder", "sphere"]


@functools.lru_cache(maxsize=None)
def _small_input(kind):
    from gravo_mg_amd import meshgen
    if kind in ("open-cylinder", "sphere"):                     # an open mesh and one of irregular valence
        V, F = meshgen.open_cylinder_mesh(48, 40) if kind == "open-cylinder" else meshgen.sphere_mesh(2000)
        S, _ = meshgen.cotan_laplacian(V, F)
        return V, meshgen.neighbors_from_stiffness(S)
    return _workload(kind)[:2]


@functools.lru_cache(maxsize=None)
def _restatement(kind):
    """The Python restatement's U_k of a small input: computed once, shared, never modified."""
    from oracle import hierarchy_restatement as ref
    V, neigh = _small_input(kind)
    return ref.build(V, neigh, ratio=8.0, lower_bound=12)


def _same_bits(Hd, Hh):
    assert len(Hd.U) == len(Hh.U) >= 2
    assert Hh.timing("selection_on_device") == 0.0 and Hd.timing("selection_on_device") == len(Hd.U)      # every level ran on the device
    for k, (a, b) in enumerate(zip(Hd.U, Hh.U)):
        assert a.shape == b.shape
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices), f"level {k}: different parents"
        assert np.array_equal(a.data.view(np.uint64), b.data.view(np.uint64)), f"level {k}: different bits"      # (a signed zero counts)
        assert np.array_equal(Hd.row_kinds(k), Hh.row_kinds(k))


@pytest.mark.parametrize("kind", SMALL_INPUTS)
def test_every_level_on_the_device_gives_the_host_bits_and_the_restatement(cabi, kind):
    """~2 000 points, lower_bound 12: two levels, both through the device stage (use_device = 2).  U_k must have the host
    build's bits, and both must agree with the restatement to the bounds of test_builder_matches_restatement_and_engine_consumes_it."""
    V, neigh = _small_input(kind)
    Hd = cabi.Hierarchy(V, neigh, lower_bound=12, use_device=2)
    Hh = cabi.Hierarchy(V, neigh, lower_bound=12, use_device=0)
    _same_bits(Hd, Hh)
    want = _restatement(kind)
    assert len(Hd.U) == len(want)
    for k, (a, b) in enumerate(zip(Hd.U, want)):
        a, b = sp.csc_matrix(a), sp.csc_matrix(b)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices), f"level {k}: different parents"
        np.testing.assert_allclose(a.data, b.data, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("weighting,nested", [(1, False), (2, False), (0, True), (1, True), (2, True)])
def test_every_level_on_the_device_with_other_weightings_and_nested(cabi, weighting, nested):
    V, neigh = _small_input("sphere")
    _same_bits(cabi.Hierarchy(V, neigh, lower_bound=12, weighting=weighting, nested=nested, use_device=2),
               cabi.Hierarchy(V, neigh, lower_bound=12, weighting=weighting, nested=nested, use_device=0))


def test_small_inputs_reach_the_triangle_edge_and_closest_three_rows_on_the_device(cabi):
    """Which branches of the selection the small inputs above take on device-run levels (gmg_hierarchy_debug_row_kinds, summed over
    the levels; triangle / edge / closest three / single or one neighbour):
        smoothing-d3, poisson, bilaplacian (the same torus)   2 127 / 94 / 16 / 0
        poisson-random                                        2 055 / 108 / 20 / 0
        pointcloud                                            1 909 / 818 / 62 / 0
        open-cylinder                                         2 040 / 214 / 2 / 0
        sphere                                                2 216 / 80 / 11 / 0
    Every input has two levels and gives all three kinds.
    No small input has a cell with fewer than two neighbours, and none overflows the edge table: tests/test_gpu_select_parents.py
    covers those."""
    total = np.zeros(4, np.int64)
    for kind in SMALL_INPUTS:
        V, neigh = _small_input(kind)
        H = cabi.Hierarchy(V, neigh, lower_bound=12, use_device=2)
        assert H.timing("selection_on_device") == len(H.U)
        kinds = sum(H.row_kinds(k).astype(np.int64) for k in range(len(H.U)))
        assert kinds.sum() == sum(u.shape[0] for u in H.U)              # (not nested: every row has a kind)
        print(f"{kind}: rows by kind {kinds.tolist()}")
        total += kinds
    assert total[0] > 0 and total[1] > 0 and total[2] > 0
