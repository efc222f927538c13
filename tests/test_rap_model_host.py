"""The host Galerkin product (csrc/host_sparse.hpp::galerkin_rap, through gmg_host_galerkin) against the plain restatement of
tests/rap_model.py on the catalogue of tests/rap_cases.py -- pattern, order and values bit for bit -- and against the exact product with a
derived entrywise bound; and the catalogue against the model of the device kernel's choices: every case reaches the branch it is listed
for, every branch label has a case.  No device."""
import numpy as np
import pytest

from tests import rap_cases, rap_model


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


@pytest.mark.parametrize("name", rap_cases.SMALL_NAMES)
def test_host_product_is_the_model_bit_for_bit(cabi, name):
    c = rap_cases.case(name)
    H = cabi.host_galerkin(c.A, c.U, as_stored=True)
    ptr, idx, val = rap_model.product(c.A, c.U)
    assert np.array_equal(H.indptr, ptr), "row pointers"
    assert np.array_equal(H.indices, idx), "columns (sorted, pattern kept structurally)"
    assert same_bits(H.data, val), np.flatnonzero(H.data.view(np.int64) != val.view(np.int64))[:8]


def test_host_product_is_the_model_on_sampled_rows_of_the_largest_case(cabi):
    """n_c = 1024 * 2048 + 1 rows: the rows that carry a link, the rows at tile edges of the prefix sum, the first and the last"""
    c = rap_cases.case("scan-carry")
    assert c.U.shape == (rap_cases.N_CARRY, rap_cases.N_CARRY) and len(c.sample) >= 100
    H = cabi.host_galerkin(c.A, c.U, as_stored=True)
    ptr, idx, val = rap_model.product(c.A, c.U, rows=c.sample)
    lengths = set()
    for k, p in enumerate(c.sample):
        lo, hi = H.indptr[p], H.indptr[p + 1]
        assert np.array_equal(H.indices[lo:hi], idx[ptr[k]:ptr[k + 1]]), p
        assert same_bits(H.data[lo:hi], val[ptr[k]:ptr[k + 1]]), p
        lengths.add(hi - lo)
    assert len(lengths) >= 3          # ends of the chain, plain rows, rows with links


@pytest.mark.parametrize("name", rap_cases.SMALL_NAMES)
def test_host_product_is_within_the_derived_bound_of_the_exact_product(cabi, name):
    """|host - exact| <= gamma_(t+1) (|U|^T |A| |U|) for every entry, t its number of terms (rap_model.within_exact_bound)"""
    c = rap_cases.case(name)
    H = cabi.host_galerkin(c.A, c.U, as_stored=True)
    ex = rap_cases.model_exact(name)
    assert np.array_equal(H.indptr, ex[0]) and np.array_equal(H.indices, ex[1])
    assert rap_model.within_exact_bound(H.data, ex) == []


def test_the_bound_can_fail():
    """eight units in the last place (>= 8 u relative) on an entry of one term are outside gamma_2 ~ 2 u, whatever its own two roundings did"""
    c = rap_cases.case("tail-group1")
    ex = rap_cases.model_exact("tail-group1")
    _, _, val = rap_model.product(c.A, c.U)
    e = ex[3].index(1)
    assert rap_model.within_exact_bound(val, ex) == []
    val = val.copy()
    for _ in range(8):
        val[e] = np.nextafter(val[e], np.inf)
    assert rap_model.within_exact_bound(val, ex) == [e]


@pytest.mark.parametrize("name", rap_cases.NAMES)
def test_case_reaches_the_branch_it_is_listed_for(name):
    c = rap_cases.case(name)
    got = rap_model.labels(rap_cases.model_branches(name))
    assert c.wanted and c.wanted <= set(rap_model.ALL_LABELS)
    assert c.wanted <= got, (sorted(c.wanted - got), sorted(got))


def test_shapes_the_catalogue_promises():
    """the counts the cases are built around, from the pattern alone"""
    for cnt in rap_cases.CNTS:
        for pro in ("pc", "smooth"):
            first, second = rap_cases.case(f"cnt{cnt}-{pro}"), rap_cases.case(f"second-cnt{cnt}-{pro}")
            rows = rap_cases.model_branches(first.name)["rows"]
            assert rows[first.row]["cnt"] == cnt == max(r["cnt"] for r in rows.values())
            assert np.diff(first.A.indptr).max() <= 35                                 # no row of A_0 is walked straight from memory
            assert np.diff(second.A.indptr)[rap_cases.HUB_GROUP] == cnt == np.diff(second.A.indptr).max()
            assert 19 <= rap_cases.model_branches(second.name)["rows"][second.row]["cnt"] <= 70
            assert rap_cases.expected_status(first.name) == (1 if cnt > rap_model.K_RAP_SET else 0) and rap_cases.expected_status(second.name) == 0
    for ch in (64, 65, 128, 129):
        c = rap_cases.case(f"children{ch}-diagonal-pc")
        rows = rap_cases.model_branches(c.name)["rows"]
        assert all(r["children"] == ch and r["windows"] == -(-ch // 64) and r["chunks"][0]["pairs"] == 64 for r in rows.values())
        rows = rap_cases.model_branches(f"children{ch}-chain-pc")["rows"]
        assert all(k["children"] <= 22 for r in rows.values() for k in r["chunks"]) and any(k["children"] == 21 for r in rows.values() for k in r["chunks"])
    h1, h2 = rap_cases.model_branches("two-hub-level1")["rows"], rap_cases.model_branches("two-hub-level2")["rows"]
    assert [h1[g]["cnt"] for g in rap_cases.HUBS] == [153, 153] and h2[rap_cases.HUBS[0] // 3]["cnt"] == 303
    assert rap_cases.expected_status("two-hub-level1") == 0 and rap_cases.expected_status("two-hub-level2") == 1
    assert rap_cases.expected_status("u-row-of-4") == 1
    for nc in (2047, 2048, 2049, 4097):
        c = rap_cases.case(f"scan-nc{nc}")
        cnts = [r["cnt"] for _, r in sorted(rap_cases.model_branches(c.name)["rows"].items())]
        assert len(cnts) == nc
        for e in list(range(rap_model.K_SCAN_TILE, nc, rap_model.K_SCAN_TILE)) + [nc - 1]:      # the counts differ across every tile edge
            assert cnts[e - 1] != cnts[e], (nc, e)
    br = rap_cases.model_branches("scan-carry")
    assert br["scan_tiles"] == rap_model.SCAN_BLOCK + 1 and br["scan_passes"] == 2


def test_every_branch_label_has_a_case():
    reached = set()
    for name in rap_cases.NAMES:
        reached |= rap_model.labels(rap_cases.model_branches(name))
    assert reached >= set(rap_model.ALL_LABELS), sorted(set(rap_model.ALL_LABELS) - reached)
    assert reached <= set(rap_model.ALL_LABELS), sorted(reached - set(rap_model.ALL_LABELS))


def test_device_product_fails_loudly_without_a_gpu(cabi):
    """gmg_debug_device_galerkin has no host rows behind it: GMG_ERR_NO_DEVICE (from the handle's creation, or from the call)"""
    if cabi.device_count() > 0:
        pytest.skip("a HIP device is present")
    c = rap_cases.case("tail-group2")
    try:
        eng = cabi.Engine()
    except cabi.GmgError as e:
        assert e.code == cabi.GMG_ERR_NO_DEVICE
        return
    with pytest.raises(cabi.GmgError) as ei:
        cabi.device_galerkin(eng, c.A, c.U)
    assert ei.value.code == cabi.GMG_ERR_NO_DEVICE
    with pytest.raises(cabi.GmgError) as ei:
        eng.timing("rap_device_levels")          # no system was ever set: the key does not exist yet
    assert ei.value.code == cabi.GMG_ERR_INVALID
