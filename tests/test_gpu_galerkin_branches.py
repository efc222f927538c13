"""The device Galerkin product (csrc/setup_kernels.hip.hpp::rap_rows<0/1/2> with the prefix sum under it) branch by branch, on the catalogue
of tests/rap_cases.py: through gmg_debug_device_galerkin -- the set-up's own upload / regrouping / count, scan and fill passes on arrays of
the test -- against the host product bit for bit and against the exact product with the derived bound; the numeric pass alone on a second
value array; and end to end through gmg_set_system on the problems whose chain stays on the device, leaves it at level 1 or leaves it in
the middle, told apart by the timing key "rap_device_levels".  tests/test_rap_model_host.py shows on the CPU that every case reaches the
branch it is listed for and that the host product is the model's."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import rap_cases, rap_model

pytestmark = pytest.mark.gpu


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def same_matrix(A, B):
    return A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and same(A.data, B.data)


def second_values(A, seed=31):
    """Seeded values on the pattern of A that have nothing to do with the first ones (not symmetric either: the product does not need it)"""
    rng = np.random.default_rng(seed)
    return A.data * (0.25 + rng.random(A.nnz)) + np.where(rng.random(A.nnz) < 0.1, 0.0, rng.standard_normal(A.nnz))


@pytest.fixture(scope="module")
def engines(cabi):
    a, b = cabi.Engine(), cabi.Engine()
    yield a, b
    a.close(); b.close()


@pytest.mark.parametrize("name", rap_cases.SMALL_NAMES)
def test_device_product_is_the_host_product(engines, cabi, name):
    """Status word as the model says; for a product the device makes: pointers, columns and values bit for bit the host's, every entry within
    gamma_(t+1) |U|^T |A| |U| of the exact one; the numeric pass alone (PASS 2) on second values gives the host product of the new matrix;
    a second call on the same handle and a call on another handle give the same bits."""
    c = rap_cases.case(name)
    eng, other = engines
    v2 = second_values(c.A)
    status, C1, V2 = cabi.device_galerkin(eng, c.A, c.U, val2=v2)
    assert status == rap_cases.expected_status(name)
    if status:
        assert C1 is None and cabi.device_galerkin(other, c.A, c.U)[0] == 1
        return
    H = cabi.host_galerkin(c.A, c.U, as_stored=True)
    assert np.array_equal(C1.indptr, H.indptr), "row pointers"
    assert np.array_equal(C1.indices, H.indices), "columns"
    assert same(C1.data, H.data), np.flatnonzero(C1.data.view(np.int64) != H.data.view(np.int64))[:8]
    assert rap_model.within_exact_bound(C1.data, rap_cases.model_exact(name)) == []
    A2 = sp.csc_matrix((v2, c.A.indices, c.A.indptr), shape=c.A.shape)
    H2 = cabi.host_galerkin(A2, c.U, as_stored=True)
    assert np.array_equal(H2.indptr, H.indptr) and np.array_equal(H2.indices, H.indices)
    assert same(V2, H2.data), np.flatnonzero(V2.view(np.int64) != H2.data.view(np.int64))[:8]
    assert H.nnz == 0 or not same(V2, C1.data)
    again = cabi.device_galerkin(eng, c.A, c.U)
    elsewhere = cabi.device_galerkin(other, c.A, c.U, val2=v2)
    assert again[0] == 0 and same_matrix(again[1], C1) and again[2] is None
    assert elsewhere[0] == 0 and same_matrix(elsewhere[1], C1) and same(elsewhere[2], V2)


def test_two_passes_of_the_tile_scan(engines, cabi):
    """n_c = 1024 * 2048 + 1 coarse rows: scan_tile_offsets goes round its loop twice and carries the first pass's total.  Against the host
    product (which tests/test_rap_model_host.py holds to the model on sampled rows); no exact reference at this size."""
    c = rap_cases.case("scan-carry")
    assert rap_cases.model_branches("scan-carry")["scan_passes"] == 2
    v2 = second_values(c.A)
    status, C1, V2 = cabi.device_galerkin(engines[0], c.A, c.U, val2=v2)
    assert status == 0
    H = cabi.host_galerkin(c.A, c.U, as_stored=True)
    assert np.array_equal(C1.indptr, H.indptr) and np.array_equal(C1.indices, H.indices) and same(C1.data, H.data)
    H2 = cabi.host_galerkin(sp.csc_matrix((v2, c.A.indices, c.A.indptr), shape=c.A.shape), c.U, as_stored=True)
    assert same(V2, H2.data) and not same(V2, C1.data)


def test_arguments_are_checked(engines, cabi):
    """indices the kernels would follow out of their arrays, and a capacity the product does not fit"""
    import ctypes as C
    c = rap_cases.case("tail-group3")
    eng = engines[0]
    bad = c.A.copy(); bad.indices[4] = c.A.shape[0]
    with pytest.raises(cabi.GmgError) as ei:
        cabi.device_galerkin(eng, bad, c.U)
    assert ei.value.code == cabi.GMG_ERR_INVALID
    badu = c.U.copy(); badu.indices[0] = -1
    with pytest.raises(cabi.GmgError) as ei:
        cabi.device_galerkin(eng, c.A, badu)
    assert ei.value.code == cabi.GMG_ERR_INVALID
    nc = c.U.shape[1]
    colptr, idx, val, status = np.zeros(nc + 1, np.int32), np.zeros(4, np.int32), np.zeros(4), C.c_int(-1)
    rc = cabi.lib().gmg_debug_device_galerkin(eng._h, c.A.shape[0], cabi._pi(c.A.indptr), cabi._pi(c.A.indices), cabi._pd(c.A.data), None, nc, cabi._pi(c.U.indptr),
                                              cabi._pi(c.U.indices), cabi._pd(c.U.data), 4, cabi._pi(colptr), cabi._pi(idx), cabi._pd(val), None, C.byref(status))
    assert rc == cabi.GMG_ERR_INVALID and colptr[nc] == 13 and not idx.any()      # the pointers say how much room it takes; nothing else was written


def _engine(cabi, P, lhs=None, **kw):
    e = cabi.Engine(**kw)
    e.set_prolongations(P.U)
    e.set_mass(P.mass)
    e.set_system(P.lhs if lhs is None else lhs)
    return e


def _cycles(e, P, n=2):
    e.load_problem(P.rhs, P.rhs)
    return e.run_cycles(n, 2), e.fetch_solution()


def test_hook_leaves_the_handle_as_it_was(cabi):
    """A handle with a live system runs the hook (a product the device makes, with PASS 2, and one it declines) and then does what a handle
    that never saw the hook does: same keys, same operators, same cycles, bit for bit."""
    P = rap_cases.cnt_problem(193, "smooth")
    a, b = _engine(cabi, P), _engine(cabi, P)
    try:
        before = {k: a.timing(k) for k in ("rap_device_levels", "setup_values_only", "device_bytes", "device_bytes_now")}      # (everything the hook takes goes back to the pool)
        for name in ("two-hub-level1", "two-hub-level2", "u-row-of-4"):
            c = rap_cases.case(name)
            assert cabi.device_galerkin(a, c.A, c.U, val2=second_values(c.A))[0] == rap_cases.expected_status(name)
        assert {k: a.timing(k) for k in before} == before
        for k in range(len(P.U) + 1):
            assert same_matrix(a.level_operator(k), b.level_operator(k))
        (ra, xa), (rb, xb) = _cycles(a, P), _cycles(b, P)
        assert same(ra, rb) and same(xa, xb)
    finally:
        a.close(); b.close()


# (problem, prolongation, levels 1 .. L the device chain makes; the two-hub graph is built for piecewise-constant prolongations)
END_TO_END = tuple((f"cnt{cnt}", pro, 0 if cnt > rap_model.K_RAP_SET else 2) for cnt in (65, 193, 256, 257) for pro in ("pc", "smooth")) + (("two-hub", "pc", 1),)


def _problem(which, prolong, levels=3):
    return rap_cases.two_hub_problem() if which == "two-hub" else rap_cases.cnt_problem(int(which[3:]), prolong, levels)


@pytest.mark.parametrize("which,prolong,device_levels", END_TO_END)
def test_set_system_end_to_end(cabi, oracle, which, prolong, device_levels):
    """gmg_set_system at its default settings: the key says how far the device chain came (as the model says: all levels, none -- level 1
    overflows --, or level 1 only), every operator is the one of an engine on the host product bit for bit, two cycles give the same
    histories and iterates, and the operators are the oracle's to 1e-13 of its largest entry (test_gpu_boundary_shapes.py)."""
    P = _problem(which, prolong)
    declined = [rap_cases.expected_status(n) for n in ((f"{which}-level1", f"{which}-level2") if which == "two-hub" else (f"{which}-{prolong}", f"second-{which}-{prolong}"))]
    assert device_levels == (0 if declined[0] else 1 if declined[1] else 2)
    dev, host = _engine(cabi, P), _engine(cabi, P, device_rap=False)
    try:
        assert dev.timing("rap_device_levels") == device_levels and host.timing("rap_device_levels") == 0
        O = oracle.Hierarchy(P.U, P.mass)
        O.set_system(P.lhs)
        for k in range(len(P.U) + 1):
            A, Ah, Ao = dev.level_operator(k), host.level_operator(k), O.level_operator(k)
            assert same_matrix(A, Ah), k
            assert A.shape == Ao.shape and (A != 0).nnz <= Ao.nnz and abs(A - Ao).max() <= 1e-13 * abs(Ao).max()
        (rd, xd), (rh, xh) = _cycles(dev, P), _cycles(host, P)
        assert same(rd, rh) and same(xd, xh)
    finally:
        dev.close(); host.close()


def _rescaled(lhs, seed=21):
    """New symmetric values on the pattern of lhs: every off-diagonal pair shrunk by its own seeded factor in [0.6, 1) (still diagonally
    dominant, signs kept)"""
    A = sp.csc_matrix(lhs).copy()
    coo = A.tocoo()
    lo, hi = np.minimum(coo.row, coo.col).astype(np.int64), np.maximum(coo.row, coo.col).astype(np.int64)
    h = (lo * 2654435761 + hi * 40503 + seed) % 1000 / 1000.0
    A.data = coo.data * np.where(lo == hi, 1.0, 0.6 + 0.4 * h)
    assert A.nnz == sp.csc_matrix(lhs).nnz and abs(A - A.T).max() == 0.0
    return A


@pytest.mark.parametrize("prolong", ("pc", "smooth"))
@pytest.mark.parametrize("cnt", (65, 193, 256))
def test_values_only_refresh_runs_the_numeric_pass(cabi, cnt, prolong):
    """Two levels, a second gmg_set_system with other values on the same pattern: the values-only refresh (PASS 2 on the resident pattern of
    a row with 2, 4 and 4 column groups) gives the operators of a fresh engine on the host product, bit for bit."""
    P = rap_cases.cnt_problem(cnt, prolong, levels=2)
    lhs2 = _rescaled(P.lhs)
    dev, fresh = _engine(cabi, P), _engine(cabi, P, lhs=lhs2, device_rap=False)
    try:
        assert dev.timing("setup_values_only") == 0.0 and dev.timing("rap_device_levels") == 1
        first = dev.level_operator(1)
        dev.set_system(lhs2)
        assert dev.timing("setup_values_only") == 1.0 and dev.timing("rap_device_levels") == 1
        assert fresh.timing("rap_device_levels") == 0
        for k in (0, 1):
            assert same_matrix(dev.level_operator(k), fresh.level_operator(k)), k
        assert not same(first.data, dev.level_operator(1).data)
        (rd, xd), (rf, xf) = _cycles(dev, P), _cycles(fresh, P)
        assert same(rd, rf) and same(xd, xf)
    finally:
        dev.close(); fresh.close()
