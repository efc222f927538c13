"""The device-built coarse inverse entry by entry, at every tile width: setup_kernels.hip.hpp::coarse_inverse_tiles<16 / 32 / 64>,
mirror_lower_to_upper, permute_symmetric, permute_symmetric_scatter and pack_lower_blocks through gmg_debug_coarse_inverse -- the set-up's own
upload and launch code on the matrices of tests/coarse_inverse_cases.py (which branches each one reaches is asserted on the host,
tests/test_coarse_inverse_model_host.py).  The criterion is the componentwise residual bound of tests/coarse_inverse_model.py, evaluated in
longdouble from the exported factor: no condition number, no other device result.  The follow-up kernels move values: bitwise."""
import numpy as np
import pytest

from tests import coarse_inverse_cases as cc
from tests import coarse_inverse_model as cm
from tests import problems
from tests.test_gpu_boundary_shapes import _grid_for

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def lender(cabi):
    assert cabi.device_count() > 0, "gpu tests need a HIP device"
    eng = cabi.Engine()          # no hierarchy, no system: the hook needs the stream and the pool only
    yield eng
    eng.close()


_runs = {}


def tiles(cabi, lender, name, width):
    """(X of mode 1, info, export) of a case at a width, once."""
    key = (name, width)
    if key not in _runs:
        X, info, E = cabi.coarse_inverse(lender, cc.BY_NAME[name].A, width=width, mode=1, export=True)
        X.setflags(write=False)
        _runs[key] = (X, info, E)
    return _runs[key]


RUNS = [(c.name, w) for c in cc.CASES for w in c.widths]
IDS = ["%s-W%d" % r for r in RUNS]


@pytest.mark.parametrize("name,width", RUNS, ids=IDS)
def test_tiles_and_mirror(cabi, lender, name, width):
    """Mode 1: every column of the lower triangle inside the residual bound; the upper triangle is its mirror bit for bit; the case reached its
    labels on this machine too (same export as the host's)."""
    X, info, E = tiles(cabi, lender, name, width)
    c = cc.BY_NAME[name]
    assert info["width"] == width and c.must[width] <= cc.labels(info, E, width, c.flags)
    _, info0, E0 = cabi.coarse_inverse(None, c.A, width=width, mode=0, export=True)
    assert info0 == info and all(np.array_equal(E[k], E0[k]) for k in E)
    assert np.all(np.isfinite(X))
    q = cm.Bound(E, info).column_ratios(X, width)
    print(f"{name} W={width}: residual / bound, largest over the columns {q.max():.4f} (terms {cm.gamma_terms(E, info, width)})")
    assert np.all(q <= 1.0), (name, width, int(np.argmax(q)), float(q.max()))
    assert np.array_equal(_bits(X), _bits(X.T))
    assert np.array_equal(_bits(X), _bits(cm.mirror(X)))


@pytest.mark.parametrize("name,width", RUNS, ids=IDS)
def test_permutations_and_packing(cabi, lender, name, width):
    """Modes 2 and 3 are the model's permutation of mode 1 and equal each other; mode 4 is the model's packing, padding rows and columns zero."""
    X, info, E = tiles(cabi, lender, name, width)
    A = cc.BY_NAME[name].A
    n = A.shape[0]
    want = cm.permute(X, E["perm"])
    X2 = cabi.coarse_inverse(lender, A, width=width, mode=2)[0]
    X3 = cabi.coarse_inverse(lender, A, width=width, mode=3)[0]
    assert np.array_equal(_bits(X2), _bits(want))
    assert np.array_equal(_bits(X3), _bits(want))
    T, info4, _ = cabi.coarse_inverse(lender, A, width=width, mode=4)
    nb = -(-n // 64)
    assert T.size == info4["out_doubles"] == nb * (nb + 1) // 2 * 4096
    assert np.array_equal(_bits(T), _bits(cm.pack(X)))
    last = T[cm.tri_block_offset(nb - 1, nb - 1) * 4096:].reshape(64, 64)
    pad = n - (nb - 1) * 64
    assert not np.any(last[pad:, :]) and not np.any(last[:, pad:])


@pytest.mark.parametrize("name", cc.TWINS)
def test_exact_twins(cabi, lender, name):
    """Every intermediate is exactly representable (proved on the host): the device returns exactly X* at every width, so the three
    instantiations agree bit for bit."""
    ref = None
    for w in cc.WIDTHS:
        X, info, E = tiles(cabi, lender, name, w)
        if ref is None:
            ref = np.asarray(cm.reference(E), np.float64)
            assert np.array_equal(_bits(ref), _bits(np.array([[float(v) for v in row] for row in cm.reference_exact(E)])))
        assert np.array_equal(_bits(X), _bits(ref)), w


@pytest.mark.parametrize("name", ["n33", "forest", "dense215", "clique-fringe", "galerkin-torus"])
def test_determinism(cabi, lender, name):
    """A second call and a second handle give the same bits, in every mode."""
    c = cc.BY_NAME[name]
    other = cabi.Engine()
    try:
        for w in c.widths:
            for mode in (1, 2, 3, 4):
                a = cabi.coarse_inverse(lender, c.A, width=w, mode=mode)[0]
                b = cabi.coarse_inverse(lender, c.A, width=w, mode=mode)[0]
                o = cabi.coarse_inverse(other, c.A, width=w, mode=mode)[0]
                assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(o)), (w, mode)
                if mode == 1:
                    assert np.array_equal(_bits(a), _bits(tiles(cabi, lender, name, w)[0]))
    finally:
        other.close()


def _inverse(eng, nl):
    """A_L^-1 as the engine applies it (tests/test_gpu_coarse_triangle._inverse): the coarsest solve of the identity, eight columns at a time"""
    X = np.empty((nl, nl))
    eye = np.eye(nl)
    for c0 in range(0, nl, 8):
        X[:, c0:c0 + 8] = eng.coarse_solve(eye[:, c0:c0 + 8]).reshape(nl, -1)
    return X


NEW_KEYS = {"coarse_inverse_width": "width", "coarse_inverse_big_chunks": "big_chunks", "coarse_inverse_max_level_chunks": "max_level_chunks",
            "coarse_inverse_chunks": "chunks", "coarse_inverse_levels": "levels"}


@pytest.mark.parametrize("n_L", [17, 65, 193])
def test_the_hook_is_the_production_path(cabi, n_L):
    """An engine with GMG_COARSE_DEVICE_INVERSE applies exactly the matrix the hook's mode 2 returns for that engine's coarsest operator (as the
    engine stores it), its timing keys say what the hook's info[] says, and the hook leaves the engine as it was."""
    n1, n2 = _grid_for(n_L)
    P = problems.synthetic_problem(graph=("grid", n1, n2), sizes=[n1 * n2, n_L], prolong=("pc",))
    eng = cabi.Engine(coarse_mode=cabi.COARSE_DEVICE_INVERSE)
    tri = cabi.Engine(coarse_mode=cabi.COARSE_DEVICE_TRIANGLE)
    try:
        for e in (eng, tri):
            e.set_prolongations(P.U); e.set_mass(P.mass); e.set_system(P.lhs)
        assert eng.timing("coarse_on_device") == 1.0 and eng.level_info(len(P.U))["n"] == n_L
        AL = eng.level_operator(len(P.U))
        X_engine = _inverse(eng, n_L)
        keys = {k: eng.timing(k) for k in list(NEW_KEYS) + ["coarse_inverse_bytes", "coarse_inverse_tiles_ms", "coarse_inverse_ms"]}
        X_hook, info, E = cabi.coarse_inverse(eng, AL, width=0, mode=2, export=True)
        assert np.array_equal(_bits(X_engine), _bits(X_hook))
        for key, name in NEW_KEYS.items():
            assert eng.timing(key) == info[name] and tri.timing(key) == info[name], key
        assert info["width"] == 16
        assert {k: eng.timing(k) for k in keys} == keys                          # the hook wrote no key ...
        assert np.array_equal(_bits(_inverse(eng, n_L)), _bits(X_engine))       # ... and not into the engine's matrix
        # the triangle engine applies the same matrix from the packing of the same tiles
        assert np.array_equal(_bits(_inverse(tri, n_L)), _bits(X_hook))
        X1 = cabi.coarse_inverse(tri, AL, width=0, mode=1)[0]
        assert np.array_equal(_bits(cm.permute(X1, E["perm"])), _bits(X_hook))
        assert cm.Bound(E, info).ratio(X1, 16) <= 1.0
    finally:
        eng.close(); tri.close()
