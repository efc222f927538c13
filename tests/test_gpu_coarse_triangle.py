"""GMG_COARSE_DEVICE_TRIANGLE on the device: the coarsest solve applied from the packed lower triangle of A_L^-1 (64 x 64 blocks in the factor's
numbering, gravo_mg_amd/csrc/coarse_triangle.hpp) must be the matrix GMG_COARSE_DEVICE_INVERSE holds, bit for bit, and its product must have
one summation order per output value.

Coarsest sizes: 1, 2, 15, 16, 17 (the build's 16-column tiles); 63 .. 193 (block edges, up to three block rows, one item per row); and with the
run length R of an item: 64 R - 1, 64 R, 64 R + 1 and 128 R + 1 -- a block row of exactly one run, of two runs (the second one a single block),
and of two runs plus a third.  R is read from the header at collection and compared with the timing key "coarse_triangle_run_blocks" in every
case.  Problems: tests/problems.synthetic_problem on a grid of about 4 n_L vertices with one aggregation level."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import problems
from tests.parity_checks import rel
from tests.test_gpu_boundary_shapes import _cond, _grid_for
from tests.vcycle_model import VcycleModel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = int(re.search(r"constexpr int kTriRun = (\d+);", open(os.path.join(ROOT, "gravo_mg_amd", "csrc", "coarse_triangle.hpp")).read()).group(1))
SMALL = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 193)
BEYOND = tuple(n for n in (64 * R - 1, 64 * R, 64 * R + 1, 128 * R + 1) if n not in SMALL)
SIZES = SMALL + BEYOND
D_SMALL, D_BEYOND = (1, 2, 3, 4, 5, 8), (1, 3, 5)


def _problem(n_L):
    n1, n2 = _grid_for(n_L)
    return problems.synthetic_problem(graph=("grid", n1, n2), sizes=[n1 * n2, n_L], prolong=("pc",))


def _engine(cabi, P, **kw):
    eng = cabi.Engine(**kw)
    eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
    return eng


def _tri(cabi, P, **kw):
    eng = _engine(cabi, P, coarse_mode=cabi.COARSE_DEVICE_TRIANGLE, **kw)
    assert eng.timing("coarse_triangle") == 1.0 and eng.timing("coarse_on_device") == 1.0 and eng.timing("coarse_triangle_run_blocks") == R
    return eng


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _inverse(eng, nl):
    """A_L^-1 as the engine applies it: the coarsest solve of the identity, eight columns at a time (every sum has one nonzero term: exact)."""
    X = np.empty((nl, nl))
    eye = np.eye(nl)
    for c0 in range(0, nl, 8):
        X[:, c0:c0 + 8] = eng.coarse_solve(eye[:, c0:c0 + 8]).reshape(nl, -1)
    return X


class Case:
    def __init__(self, cabi, n_L):
        self.nl, self.P = n_L, _problem(n_L)
        self.ds = D_SMALL if n_L <= 193 else D_BEYOND
        self.tri = _tri(cabi, self.P)
        self.dev = _engine(cabi, self.P, coarse_mode=cabi.COARSE_DEVICE_INVERSE)
        self.X = None

    def inverse(self):
        if self.X is None:
            self.X = _inverse(self.tri, self.nl)
            self.X.setflags(write=False)
        return self.X

    def close(self):
        self.tri.close(); self.dev.close()


@pytest.fixture(scope="module", params=SIZES, ids=["nL%d" % n for n in SIZES])
def case(request, cabi):
    assert cabi.device_count() > 0, "gpu tests need a HIP device"
    c = Case(cabi, request.param)
    yield c
    c.close()


def test_the_same_matrix(case):
    """The packing, the diagonal-block rule and both permutations: the matrix the triangle engine applies is the one the full-inverse engine
    applies, bit for bit, and it is symmetric bit for bit."""
    nl = case.nl
    assert case.tri.level_info(len(case.P.U))["n"] == nl
    X_tri, X_dev = case.inverse(), _inverse(case.dev, nl)
    assert np.array_equal(_bits(X_tri), _bits(X_dev))
    assert np.array_equal(_bits(X_tri), _bits(X_tri.T))


def test_the_product(case, cabi, oracle):
    """The assertions of test_gpu_boundary_shapes.test_coarse_solve_host_and_device with the triangle engine in the device engine's place; the
    componentwise bound against the full-inverse product (both add the same n_L products, each sum with an error of at most gamma_n |X| |rc|);
    one column alone == that column of the block; the same bits from a second call and from a second engine."""
    P, nl, tri, dev = case.P, case.nl, case.tri, case.dev
    X = case.inverse()
    host = _engine(cabi, P, coarse_mode=cabi.COARSE_HOST_LDLT)
    twin = _tri(cabi, P)
    try:
        assert host.timing("coarse_on_device") == 0.0 and host.timing("coarse_triangle") == 0.0
        AL = tri.level_operator(len(P.U))
        O = oracle.Hierarchy(P.U, P.mass)
        O.set_system(P.lhs)
        nA = spla.norm(AL)
        cond = _cond(AL)
        rng = np.random.default_rng(11)
        for d in case.ds:
            rc = rng.standard_normal((nl, d))
            e_tri, e_dev, e_host, e_o = tri.coarse_solve(rc), dev.coarse_solve(rc), host.coarse_solve(rc), O.coarse_solve(rc)
            assert np.linalg.norm(AL @ e_host - rc) <= 1e-12 * (nA * np.linalg.norm(e_host) + np.linalg.norm(rc)), d
            assert np.linalg.norm(AL @ (e_host - e_o)) <= 1e-11 * nA * np.linalg.norm(e_o), d
            assert np.linalg.norm(AL @ (e_tri - e_host)) <= 1e-14 * cond * nA * np.linalg.norm(e_host) + 1e-10 * nA * np.linalg.norm(e_host), d
            assert rel(e_tri, e_host) <= 1e-13 * cond + 1e-9, d
            assert rel(e_tri, e_o) <= 1e-13 * cond + 1e-9, d
            bound = (nl + 1) * 2.0 ** -52 * (np.abs(X) @ np.abs(rc))
            assert np.all(np.abs(e_tri.reshape(nl, d) - e_dev.reshape(nl, d)) <= bound), (d, float(np.max(np.abs(e_tri.reshape(nl, d) - e_dev.reshape(nl, d)) - bound)))
            j = d - 1
            assert np.array_equal(_bits(tri.coarse_solve(rc[:, j]).ravel()), _bits(e_tri.reshape(nl, d)[:, j])), d
            if d >= 2:
                e = e_tri.reshape(nl, d)
                assert abs(rc[:, 0] @ e[:, 1] - rc[:, 1] @ e[:, 0]) <= 1e-12 * np.abs(rc[:, 0] @ e[:, 1]) + 1e-12 * np.linalg.norm(e), d
            assert np.array_equal(_bits(tri.coarse_solve(rc)), _bits(e_tri)), d
            assert np.array_equal(_bits(twin.coarse_solve(rc)), _bits(e_tri)), d
    finally:
        host.close(); twin.close()


CYCLE_SIZES = (65, 64 * R + 1)


@pytest.mark.parametrize("variant", ["fp64", "fp32-inner", "graph"])
@pytest.mark.parametrize("n_L", CYCLE_SIZES)
def test_vcycles_match_model(cabi, oracle, n_L, variant):
    """Two V-cycles against tests/vcycle_model.VcycleModel, from identical inputs, with the checks and tolerances of
    test_gpu_boundary_shapes.test_vcycles_match_model."""
    P = _problem(n_L)
    kw = {"fp64": dict(), "fp32-inner": dict(inner_precision=1), "graph": dict(use_graph=True)}[variant]
    ref = _tri(cabi, P)
    eng = _tri(cabi, P, **kw) if kw else ref
    try:
        M = VcycleModel(ref, P.U, P.mass, P.lhs, oracle, ref.gs_omega)
        nA = spla.norm(P.lhs)
        for d in (1, 3, 5):
            b = P.rhs[:, :d]
            x = b.copy()
            for cyc in range(2):
                xg, xm = eng.vcycle(b, x), M.vcycle(b, x)
                if variant == "fp32-inner":
                    assert np.linalg.norm(xg - xm) <= 2e-5 * np.linalg.norm(xm), (d, cyc)
                else:
                    assert np.linalg.norm(P.lhs @ (xg - xm)) <= 1e-12 * nA * np.linalg.norm(xm), (d, cyc)
                    assert rel(xg, xm) <= 1e-6, (d, cyc)
                x = xm
    finally:
        if eng is not ref:
            eng.close()
        ref.close()


def _cycles(eng, P, d=3, n=3):
    eng.load_problem(P.rhs[:, :d], P.rhs[:, :d])
    hist = eng.run_cycles(n, 2).copy()
    return hist, eng.fetch_solution().copy()


def _same(a, b):
    return np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_life_cycle_and_timing_keys(cabi):
    """A values-only refresh, then systems with other coarsest sizes (more blocks, then fewer): every time the bits of a fresh handle, and the
    keys of the mode.  The defaults did not move."""
    sizes = (65, 64 * R + 1, 17)
    P = _problem(sizes[0])
    eng = _tri(cabi, P)
    engines = [eng]
    try:
        lhs2 = (1.5 * P.lhs + sp.diags(P.mass)).tocsc()
        lhs2.sort_indices()
        assert np.array_equal(lhs2.indptr, P.lhs.indptr) and np.array_equal(lhs2.indices, P.lhs.indices)
        eng.set_system(lhs2)
        assert eng.timing("setup_values_only") == 1.0 and eng.timing("coarse_triangle") == 1.0
        P2 = problems.Problem(P.V, P.S, P.mass, P.U, lhs2, P.rhs, P.name)
        fresh = _tri(cabi, P2); engines.append(fresh)
        assert _same(_cycles(eng, P2), _cycles(fresh, P2))
        for n_L in sizes[1:]:
            Q = _problem(n_L)
            eng.set_prolongations(Q.U); eng.set_mass(Q.mass); eng.set_system(Q.lhs)
            fresh = _tri(cabi, Q); engines.append(fresh)
            nb = -(-n_L // 64)
            for e in (eng, fresh):
                assert e.timing("coarse_triangle") == 1.0 and e.timing("coarse_on_device") == 1.0 and e.timing("coarse_triangle_run_blocks") == R
                assert e.timing("coarse_inverse_bytes") == 8 * 4096 * nb * (nb + 1) // 2
            assert _same(_cycles(eng, Q), _cycles(fresh, Q)), n_L
            dev = _engine(cabi, Q, coarse_mode=cabi.COARSE_DEVICE_INVERSE); engines.append(dev)
            assert dev.timing("coarse_triangle") == 0.0 and dev.timing("coarse_triangle_run_blocks") == 0.0
            assert dev.timing("coarse_inverse_bytes") == 8 * n_L * (-(-n_L // 8) * 8)
            default = _engine(cabi, Q); engines.append(default)
            assert default.timing("coarse_triangle") == 0.0 and default.timing("coarse_on_device") == 1.0
            assert _same(_cycles(default, Q), _cycles(dev, Q)), n_L
            host = _engine(cabi, Q, coarse_mode=cabi.COARSE_HOST_LDLT); engines.append(host)
            assert host.timing("coarse_triangle") == 0.0 and host.timing("coarse_on_device") == 0.0
    finally:
        for e in engines:
            e.close()


def test_single_rank_engine_driven_cycle(cabi):
    """gmg_p2p_* on one rank (the multi-rank cycle's code path, tests/test_gpu_p2p.py) reaches the coarsest solve through the same dispatch: its
    iterates equal run_cycles bit for bit in the new mode."""
    from tests.test_gpu_p2p import _problem as p2p_problem
    P = p2p_problem("smoothing")
    d = P.rhs.shape[1]
    kw = dict(row_align=64, block_lanes=1)
    ref = _tri(cabi, P, **kw)
    eng = _tri(cabi, P, **kw)
    try:
        ref.load_problem(P.rhs, P.rhs)
        hist = ref.run_cycles(4, 2).copy()
        x = ref.fetch_solution().copy()
        rk = cabi.P2PCycle(eng, 0, 1, d)
        rk.connect([rk.export()])
        rk.load(P.rhs, P.rhs)
        hist_p = rk.cycles(4, 2)
        assert np.array_equal(_bits(rk.fetch()), _bits(x))
        assert np.allclose(hist_p, hist, rtol=1e-12, atol=0)
        del rk
    finally:
        ref.close(); eng.close()
