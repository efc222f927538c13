"""The catalogue of tests/coarse_inverse_cases.py and the model of tests/coarse_inverse_model.py, verified without a device: every case reaches its
labels (read from gmg_debug_coarse_inverse in mode 0), the host's restatement of the kernel and a float64 restatement in the device's order stay
inside the residual bound, the exact twins are exact, and the checks the GPU file makes catch seeded defects."""
from fractions import Fraction

import numpy as np
import pytest

from tests import coarse_inverse_cases as cc
from tests import coarse_inverse_model as cm

_cache = {}


def export_of(cabi, name, width):
    """(mode 0 matrix, info, export, Bound) of a case at a width, computed once."""
    key = (name, width)
    if key not in _cache:
        X, info, E = cabi.coarse_inverse(None, cc.BY_NAME[name].A, width=width, mode=0, export=True)
        X.setflags(write=False)
        first = _cache.get((name, "bound"))
        if first is None:
            first = _cache[(name, "bound")] = cm.Bound(E, info)
        _cache[key] = (X, info, E, first)
    return _cache[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", cc.NAMES)
def test_case_reaches_its_labels(cabi, name):
    c = cc.BY_NAME[name]
    for w in c.widths:
        _, info, E, _ = export_of(cabi, name, w)
        assert info["width"] == w and info["big_rows"] == cc.K_BIG_ROWS and info["waves"] == cc.K_WAVES
        got = cc.labels(info, E, w, c.flags)
        assert c.must[w] <= got, (name, w, sorted(c.must[w] - got))
    if c.A.shape[0] <= 8192:
        assert cabi.coarse_inverse(None, c.A, width=0, mode=0)[1]["width"] == 16          # the production rule


def test_every_label_has_a_case(cabi):
    reached, promised = set(), set()
    for c in cc.CASES:
        for w in c.widths:
            _, info, E, _ = export_of(cabi, c.name, w)
            reached |= cc.labels(info, E, w, c.flags)
            promised |= c.must[w]
    assert promised >= set(cc.ALL_LABELS), sorted(set(cc.ALL_LABELS) - promised)
    assert reached <= set(cc.ALL_LABELS), sorted(reached - set(cc.ALL_LABELS))


def test_the_export_is_consistent(cabi):
    """The arrays the kernel indexes without bounds: every index in range, levels after their ancestors, tile paths ascending."""
    for c in cc.CASES:
        w = c.widths[0]
        _, info, E, _ = export_of(cabi, c.name, w)
        n = c.A.shape[0]
        assert sorted(E["perm"]) == list(range(n))
        assert E["q_rptr"][0] == 0 and np.all(np.diff(E["q_rptr"]) >= 0) and E["q_rptr"][-1] == info["row_entries"]
        assert np.all((E["rows"] >= 0) & (E["rows"] < n)) if info["row_entries"] else True
        assert np.all((E["q_w"] >= 1) & (E["q_w"] <= cc.K_CHUNK)) and np.all(E["q_col0"] + E["q_w"] <= n)
        assert sorted(E["lev_q"]) == list(range(info["chunks"]))
        assert np.all((E["tile_q"] >= 0) & (E["tile_q"] < info["chunks"]))
        for t in range(info["tiles"]):
            assert np.all(np.diff(E["tile_q"][E["tile_ptr"][t]:E["tile_ptr"][t + 1]]) > 0)
        for q in range(info["chunks"]):      # rows of a chunk lie below its own columns, each once
            r = E["rows"][E["q_rptr"][q]:E["q_rptr"][q + 1]]
            assert len(set(r)) == len(r) and (len(r) == 0 or r.min() >= E["q_col0"][q] + E["q_w"][q])


RATIOS = {}


@pytest.mark.parametrize("name", cc.NAMES)
def test_host_order_and_device_order_stay_inside_the_bound(cabi, name):
    """Mode 0 (the host's order) and the float64 restatement of the device's order at every width of the case: residual ratio <= 1."""
    c = cc.BY_NAME[name]
    for w in c.widths:
        X0, info, E, bound = export_of(cabi, name, w)
        r0 = bound.ratio(X0, None)
        Xd = cm.device_order(E, info, w)
        rd = bound.ratio(Xd, w)
        RATIOS[(name, w)] = (r0, rd)
        print(f"{name} W={w}: terms host {cm.gamma_terms(E, info, None)} device {cm.gamma_terms(E, info, w)}; residual / bound host order {r0:.3f}, device order {rd:.3f}")
        assert r0 <= 1.0, (name, w, r0)
        assert rd <= 1.0, (name, w, rd)
        assert cm.gamma_terms(E, info, w) <= 700 and cm.gamma_terms(E, info, None) <= 700


@pytest.mark.parametrize("name", cc.TWINS)
def test_twins_are_exact(cabi, name):
    """The exported factor is the hand-made one up to perm; float64 in two summation orders (and the host's third) and the exact rational
    result have the same bits: every intermediate is exactly representable, so any correct kernel returns exactly X*."""
    c = cc.BY_NAME[name]
    X0, info, E, _ = export_of(cabi, name, 16)
    assert info["tiles"] >= 2
    L, dinv = cm.dense_factor(E)
    p = E["perm"]
    assert np.array_equal(L, c.L[np.ix_(p, p)]) and np.array_equal(1.0 / dinv, c.D[p])
    exact = cm.reference_exact(E)
    Xs = np.array([[float(v) for v in row] for row in exact])
    assert all(v == float(v) for v in exact.ravel())
    for w in c.widths:
        _, info_w, E_w, _ = export_of(cabi, name, w)
        assert np.array_equal(_bits(cm.device_order(E_w, info_w, w)), _bits(Xs)), w
        assert np.array_equal(_bits(cm.device_order(E_w, info_w, w, reverse=True)), _bits(Xs)), w
    assert np.array_equal(_bits(np.tril(X0)), _bits(np.tril(Xs)))
    assert np.array_equal(_bits(np.asarray(cm.reference(E), np.float64)), _bits(Xs))


@pytest.mark.parametrize("name", cc.SMALL)
def test_longdouble_reference_against_exact_fractions(cabi, name):
    """On the small cases the longdouble X* agrees with the exact one.  The computed inverse factor Y of L obeys |Y - L^-1| <= gamma_n M with
    M = |L^-1| |L| |L^-1| >= |L^-1| (forward substitution, Higham 8.1), so the product Y^T D^-1 Y is within (3 n + 4) 2^-64 M^T |D^-1| M of X*:
    eleven more bits than float64 carries, good enough to measure float64 against.  And the residual of the criterion, evaluated in longdouble on
    the host's float64 result, is within n 2^-63 of its absolute-value expression of the exact residual -- the term bound() adds."""
    X0, info, E, bound = export_of(cabi, name, 16)
    exact = cm.reference_exact(E)
    ref = cm.reference(E)
    L, dinv = cm.dense_factor(E, cm.LD)
    aLi = np.abs(cm.unit_lower_inverse(L))
    M = aLi @ np.abs(L) @ aLi
    scale = M.T @ (np.abs(dinv)[:, None] * M)
    n = L.shape[0]
    for j in range(n):
        for k in range(n):
            assert abs(_exact(ref[j, k]) - exact[j, k]) <= _exact(scale[j, k]) * (3 * n + 4) * Fraction(1, 2 ** 64), (name, j, k)
    if n in (9, 17, 33):
        Lf = np.array([[Fraction(float(v)) for v in row] for row in np.asarray(L, np.float64)], dtype=object).reshape(n, n)
        Df = np.array([1 / Fraction(float(v)) for v in dinv], dtype=object)
        Xf = np.array([[Fraction(float(v)) for v in row] for row in np.tril(X0)], dtype=object).reshape(n, n)
        Z = Df[:, None] * Lf.T.dot(Xf)
        Rf = Lf.dot(np.tril(Z)) - np.array([[Fraction(int(j == k)) for k in range(n)] for j in range(n)], dtype=object)
        R, B = bound.residual(X0)
        for j in range(n):
            for k in range(j + 1):
                assert abs(abs(Rf[j, k]) - _exact(R[j, k])) <= _exact(B[j, k]) * n * Fraction(1, 2 ** 63), (name, j, k)


def _exact(x):
    """a longdouble as a Fraction (two float64 pieces)"""
    hi = float(x)
    return Fraction(hi) + Fraction(float(x - cm.LD(hi)))


# ---- seeded defects: each must fail the check the GPU file makes -----------------------------------------------------------------------------------

def _first_nonzero_row_term(E):
    i, jj = np.argwhere(E["vals"] != 0)[len(np.argwhere(E["vals"] != 0)) // 2]
    return int(i), int(jj)


@pytest.mark.parametrize("name,width", [("n33", 16), ("dense60", 64), ("rows%d" % (cc.K_BIG_ROWS + 1), 32), ("galerkin-torus", 16)])
def test_a_dropped_row_term_is_caught(cabi, name, width):
    _, info, E, bound = export_of(cabi, name, width)
    bad = dict(E); bad["vals"] = E["vals"].copy()
    bad["vals"][_first_nonzero_row_term(E)] = 0.0
    assert bound.ratio(cm.device_order(bad, info, width), width) > 1.0


@pytest.mark.parametrize("name,width", [("rows%d" % cc.K_BIG_ROWS, 16), ("rows%d" % (cc.K_BIG_ROWS + 1), 64), ("dense215", 64)])
def test_an_omitted_wave_sum_is_caught(cabi, name, width):
    _, info, E, bound = export_of(cabi, name, width)
    assert info["big_chunks"] >= 1
    for wave in (0, cc.K_WAVES - 1):
        assert bound.ratio(cm.device_order(E, info, width, drop_wave=wave), width) > 1.0, wave


@pytest.mark.parametrize("name,width", [("n17", 16), ("galerkin-torus", 32), ("twin-comb", 16)])
def test_a_shifted_dinv_index_is_caught(cabi, name, width):
    _, info, E, bound = export_of(cabi, name, width)
    bad = dict(E); bad["dinv"] = np.roll(E["dinv"], 1)
    assert bound.ratio(cm.device_order(bad, info, width), width) > 1.0


@pytest.mark.parametrize("name,width", [("n9", 16), ("dense60", 32), ("twin-comb", 64)])
def test_a_stale_own_column_value_is_caught(cabi, name, width):
    _, info, E, bound = export_of(cabi, name, width)
    assert np.any(E["tri"] != 0)
    assert bound.ratio(cm.device_order(E, info, width, stale_own=True), width) > 1.0


@pytest.mark.parametrize("name,width", [("n33", 16), ("n65", 32), ("n129", 64)])
def test_a_mirror_from_the_wrong_triangle_is_caught(cabi, name, width):
    """What the tiles leave above the diagonal is zero outside a tile's own rows: mirrored downwards it breaks the residual bound, and the matrix
    is no longer the model's mirror."""
    _, info, E, bound = export_of(cabi, name, width)
    X = cm.before_mirror(cm.device_order(E, info, width), width)
    good, wrong = cm.mirror(X), cm.mirror(X.T)
    assert bound.ratio(good, width) <= 1.0
    assert not np.array_equal(_bits(wrong), _bits(good)) and bound.ratio(wrong, width) > 1.0


@pytest.mark.parametrize("name", ["n17", "galerkin-torus"])
def test_perm_in_the_place_of_its_inverse_is_caught(cabi, name):
    _, info, E, _ = export_of(cabi, name, 16)
    p = E["perm"]
    assert not np.array_equal(p[p], np.arange(len(p)))          # (an involution would hide it)
    X = cm.mirror(cm.device_order(E, info, 16))
    wrong = np.empty_like(X)
    wrong[p] = X[:, p]                                          # out[perm[j]][c] = X[j][perm[c]]
    good = cm.permute(X, p)
    assert not np.array_equal(_bits(wrong), _bits(good))
    assert np.array_equal(_bits(good[np.ix_(p, p)]), _bits(X))      # good[perm[j]][perm[c]] == X[j][c]


@pytest.mark.parametrize("name,width", [("n65", 16), ("n129", 64)])
def test_a_diagonal_block_taken_from_the_upper_side_is_caught(cabi, name, width):
    _, info, E, _ = export_of(cabi, name, width)
    X = cm.before_mirror(cm.device_order(E, info, width), width)
    good = cm.pack(X)
    wrong = cm.pack(X.T)          # every diagonal-block entry above the diagonal from the upper side (the lower blocks transposed with them)
    n = X.shape[0]
    d0 = slice(0, cm.TRI_BLOCK * cm.TRI_BLOCK)
    assert not np.array_equal(_bits(wrong[d0]), _bits(good[d0]))
    blk = good[d0].reshape(64, 64)
    assert np.array_equal(_bits(blk), _bits(blk.T)) and np.array_equal(_bits(blk[:min(n, 64), :min(n, 64)]), _bits(cm.mirror(X)[:64, :64]))
    assert good.size == cm.tri_block_offset(-(-n // 64), 0) * 4096


def test_device_modes_fail_loudly_without_a_gpu(cabi):
    if cabi.device_count() > 0:
        pytest.skip("a HIP device is present")
    A = cc.BY_NAME["n9"].A
    try:
        eng = cabi.Engine()
    except cabi.GmgError as e:
        assert e.code == cabi.GMG_ERR_NO_DEVICE
        return
    for mode in (1, 2, 3, 4):
        with pytest.raises(cabi.GmgError) as ei:
            cabi.coarse_inverse(eng, A, mode=mode)
        assert ei.value.code == cabi.GMG_ERR_NO_DEVICE
    assert cabi.coarse_inverse(eng, A, mode=0)[0].shape == (9, 9)
    eng.close()


def test_bad_arguments_are_refused(cabi):
    A = cc.BY_NAME["n9"].A.copy()
    with pytest.raises(cabi.GmgError) as ei:
        cabi.coarse_inverse(None, A, width=48)
    assert ei.value.code == cabi.GMG_ERR_INVALID
    bad = A.copy(); bad.indices = bad.indices.copy(); bad.indices[3] = 9
    with pytest.raises(cabi.GmgError) as ei:
        cabi.coarse_inverse(None, bad)
    assert ei.value.code == cabi.GMG_ERR_INVALID
    import scipy.sparse as sp
    with pytest.raises(cabi.GmgError) as ei:
        cabi.coarse_inverse(None, sp.csc_matrix(np.ones((2, 2))))          # singular: a zero pivot
    assert ei.value.code == cabi.GMG_ERR_NUMERIC
