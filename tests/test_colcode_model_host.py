"""The plain model of level 0's 16-bit column codes (tests/colcode_model.py) checked on hand-made column sets, and the catalogue of
tests/colcode_cases.py checked to reach the branch each case is there for -- from the host planner's ordering alone, so that a case that stops
reaching its branch is found without a GPU (tests/test_gpu_column_codes.py then compares the device with the same model)."""
import itertools

import numpy as np
import pytest

from tests import colcode_cases as cc
from tests import colcode_model as cm


def _layout(slices, lanes=7):
    """SELL layout of slices given as lists of columns: column i of a slice becomes an entry of row (lanes i) % 64 of that slice (rows of several
    entries once a slice has more than 64 columns or lanes folds), every entry real."""
    rows = [[] for _ in range(64 * len(slices))]
    for s, cols in enumerate(slices):
        for i, c in enumerate(cols):
            rows[64 * s + (lanes * i) % 64].append(int(c))
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    flat = np.array([c for r in rows for c in r], np.int64)
    sp_, col, _, real = cm.sell_from_rows(ptr, flat, np.ones(len(flat)))
    return sp_, col, real


def _spread(count, span, start=5):
    return [start + span * k for k in range(count)]


@pytest.mark.parametrize("nw", [8, 32])
def test_decoding_the_models_codes_gives_back_the_columns(nw):
    rng = np.random.default_rng(nw)
    span = cm.SPAN[nw]
    slices = [sorted(rng.choice(span * nw // 2, size=rng.integers(1, 150), replace=False) + 1000 * s) for s in range(6)] + [[], [17], _spread(nw, span)]
    for lanes in (7, 1, 64):                      # (lanes = 64: every column of a slice in ONE row -- both halves of every word used)
        sp_, col, real = _layout(slices, lanes)
        enc = cm.encode(sp_, col, real, nw)
        assert enc["failed"] == 0
        got = cm.decode(sp_, enc["words"], enc["win_base"], nw)
        assert np.array_equal(got[real], col[real])
        first = np.repeat(enc["win_base"][:, 0], np.diff(sp_))      # padding: code 0 = the slice's first base
        assert np.array_equal(got[~real], first[~real])
        assert np.all(enc["win_base"][6] == 0) and np.all(enc["win_base"][7] == 17)      # an empty slice: base 0; unused bases repeat the last one
        assert np.all(np.diff(enc["win_base"], axis=1) >= 0)


def _fewest_windows(cols, span):
    """Brute force: the fewest windows [b, b + span) covering the sorted distinct columns -- over every split into runs of neighbours."""
    m = len(cols)
    best = m
    for cuts in itertools.product((0, 1), repeat=m - 1):
        edges = [0] + [i + 1 for i, c in enumerate(cuts) if c] + [m]
        if all(cols[b - 1] - cols[a] < span for a, b in zip(edges[:-1], edges[1:])):
            best = min(best, len(edges) - 1)
    return best


def test_the_greedy_cover_is_minimal():
    rng = np.random.default_rng(3)
    for span in (2048, 8192):
        for _ in range(60):
            cols = np.unique(rng.integers(0, 6 * span, size=rng.integers(1, 11)))
            bases = cm.greedy_cover(cols, span)
            assert len(bases) == _fewest_windows(list(cols), span)
            assert all(any(b <= c < b + span for b in bases) for c in cols)


@pytest.mark.parametrize("nw", [8, 32])
def test_span_edges(nw):
    span = cm.SPAN[nw]
    sp_, col, real = _layout([[100, 100 + span - 1], [100, 100 + span], [100, 100 + span - 1, 100 + span, 100 + 2 * span - 1, 100 + 2 * span]])
    enc = cm.encode(sp_, col, real, nw)
    assert list(enc["needed"]) == [1, 2, 3]
    assert list(enc["win_base"][0][:2]) == [100, 100] and list(enc["win_base"][1][:3]) == [100, 100 + span, 100 + span]
    assert list(enc["win_base"][2][:4]) == [100, 100 + span, 100 + 2 * span, 100 + 2 * span]
    codes = {int(c): int(w) & 0xffff for c, w in zip(col[real], enc["words"][real]) if c in (100 + span - 1, 100 + span)}      # (one entry per row here: the low half)
    assert codes[100 + span - 1] == span - 1 and codes[100 + span] == 1 << cm.DBITS[nw]
    assert np.array_equal(cm.decode(sp_, enc["words"], enc["win_base"], nw)[real], col[real])


@pytest.mark.parametrize("nw", [8, 32])
def test_window_count_edges(nw):
    span = cm.SPAN[nw]
    sp_, col, real = _layout([_spread(nw, span), _spread(nw + 1, span), [3, 4]])
    enc = cm.encode(sp_, col, real, nw)
    assert list(enc["needed"]) == [nw, nw + 1, 1] and enc["failed"] == 1 and enc["last"] == 2
    assert enc["win_base"][0, 0] == 5 and enc["win_base"][0, -1] == 5 + span * (nw - 1)
    assert enc["win_base"][1, 0] == -1 and list(enc["win_base"][1, 1:]) == _spread(nw, span)[1:]      # uncovered: first base -1, the rest as covered
    assert not enc["words"][sp_[1]:sp_[2]].any() and enc["words"][sp_[0]:sp_[1]].any()                  # ... and every code word 0
    # 32 columns 2 048 apart are exactly 8 windows of 8 192 and exactly 32 of 2 048; one more is 9 and 33
    for count, want in ((32, (8, 32)), (33, (9, 33))):
        sp2, col2, real2 = _layout([_spread(count, 2048)])
        assert (cm.encode(sp2, col2, real2, 8)["needed"][0], cm.encode(sp2, col2, real2, 32)["needed"][0]) == want


def _with_uncovered(n_slices, which, count=9, span=8192):
    return _layout([_spread(count, span) if s in which else [s, s + 1] for s in range(n_slices)])


def test_verdict_thresholds():
    assert [cm.mode_of(f, l, n) for f, l, n in ((0, 0, 1), (2, 2, 32), (1, 3, 32), (4, 32, 32), (5, 32, 32), (1, 1, 15), (1, 1, 16), (1, 1, 7), (1, 1, 8), (0, 0, 7))] == \
        [1, 1, 2, 2, 0, 2, 1, 0, 2, 1]
    # last == n_slices // 16 against + 1
    m = cm.model(*_with_uncovered(32, {0, 1}))
    assert (m["windows"], m["mode"], m["from"], m["failed"]) == (8, 1, 2, 2) and not m["recoded"]
    m = cm.model(*_with_uncovered(32, {2}))
    assert (m["windows"], m["mode"], m["failed"], m["last"]) == (8, 2, 1, 3)
    # failed == n_slices // 8 against + 1 (the slices that 8 windows leave uncovered are covered by 32: the recode)
    m = cm.model(*_with_uncovered(32, {3, 10, 20, 31}))
    assert (m["windows"], m["mode"], m["failed"], m["last"]) == (8, 2, 4, 32)
    m = cm.model(*_with_uncovered(32, {3, 10, 20, 30, 31}))
    assert (m["windows"], m["mode"], m["failed"], m["recoded"]) == (32, 1, 0, True) and m["needed8"].max() == 9
    # n_slices < 16: n // 16 = 0, any uncovered slice is flagged; n_slices < 8: n // 8 = 0 too, one uncovered slice drops the format
    m = cm.model(*_with_uncovered(15, {0}))
    assert (m["windows"], m["mode"], m["failed"]) == (8, 2, 1)
    m = cm.model(*_with_uncovered(16, {0}))
    assert (m["windows"], m["mode"], m["from"]) == (8, 1, 1)
    m = cm.model(*_with_uncovered(7, {0}))
    assert (m["windows"], m["mode"], m["recoded"]) == (32, 1, True)
    m = cm.model(*_with_uncovered(7, {6}, count=33, span=2048))
    assert (m["windows"], m["mode"], m["recoded"], m["failed"], m["words"]) == (0, 0, True, 1, None) and m["uniform_width"] == 0 and m["from"] == 0


def test_recode_decision():
    """The verdict after a mode 0 with 8 windows is that of the pass with 32 windows, whatever it is: all covered, a prefix, flagged, or none."""
    wide = lambda which: _layout([_spread(33, 2048) if s in which else _spread(9, 8192) for s in range(32)])     # every slice uncovered by 8 windows
    for which, want in ((set(), (32, 1, 0)), ({0, 1}, (32, 1, 2)), ({5, 9}, (32, 2, 10)), ({1, 2, 3, 4, 5}, (0, 0, 0))):
        m = cm.model(*wide(which))
        assert m["recoded"] and (m["windows"], m["mode"], m["from"]) == want, (which, m["windows"], m["mode"], m["from"])
        if m["windows"]:
            assert m["win_base"].shape == (32, 32)
    m = cm.model(*_layout([_spread(9, 8192)] + [[1, 2]] * 31))          # one uncovered slice at the front: no recode, a prefix
    assert not m["recoded"] and (m["windows"], m["mode"], m["from"]) == (8, 1, 1) and m["win_base"].shape == (32, 8)


def test_what_is_real():
    """The operator: entry j of a row is real when j < the row's stored off-diagonal count, whatever its value; a transfer: value != 0."""
    sp_ = np.array([0, 128]); row_len = np.zeros(64, int); row_len[:3] = (2, 1, 0)
    real = cm.real_of_operator(sp_, row_len)
    assert real.sum() == 3 and real[0] and real[64] and real[1] and not real[65] and not real[2]
    assert list(cm.real_of_transfer(np.array([0.5, 0.0, -0.0, 1e-300]))) == [True, False, False, True]
    sp1, _, real1 = _layout([[3, 3, 3]])
    assert cm.uniform_width_of(sp1) == 1 and cm.uniform_width_of(np.array([0, 64, 192])) == 0 and cm.uniform_width_of(np.array([0, 0])) == 0
    assert cm.uniform_width_of(np.array([0, 64 * 63])) == 63 and cm.uniform_width_of(np.array([0, 64 * 64])) == 0


# ---- the catalogue reaches its branches ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def verdicts(cabi):
    """The model's verdict for A, P and R of every catalogue case on the host planner's layouts (cases that share a graph and the pinned layout
    share the computation)."""
    out, seen = {}, {}
    for name, (links, sizes, kw, _) in cc.CASES.items():
        key = (links, tuple(sizes or ()), kw.get("block_lanes", 0), kw.get("prolong"))
        if key not in seen:
            L = cc.host_layouts(cabi, cc.problem(name), block_lanes=kw.get("block_lanes", 0))
            seen[key] = ({which: cm.model(*L[which]) for which in (0, 3, 4)}, L)
        out[name] = seen[key]
    return out


@pytest.mark.parametrize("name", [n for n, c in cc.CASES.items() if c[3] is not None])
def test_case_reaches_its_branch_on_the_host_planners_ordering(verdicts, name):
    cc.check_branch(name, verdicts[name][0][0])


def test_the_transfers_reach_several_windows_and_the_second_format(verdicts):
    """R and P take what the level-1 numbering gives.  For the cases with piecewise-constant prolongations the planner entry reproduces that
    numbering, and they are the ones relied on: R in the format of 32 windows (flagged-32: every slice covered; dropped: slices flagged), P with
    several windows in a slice (prefix, flagged-32) and flagged (dropped).  (With smoothed prolongations the engine's level-1 blocks are not the
    planner entry's; what those cases give the transfers is read on the device: tests/test_gpu_column_codes.py, EXPECT_TRANSFER.)"""
    R = {n: v[0][4] for n, v in verdicts.items()}
    Pm = {n: v[0][3] for n, v in verdicts.items()}
    assert (R["flagged-32"]["windows"], R["flagged-32"]["mode"]) == (32, 1) and R["flagged-32"]["recoded"] and R["flagged-32"]["used"].max() > 8
    assert (R["dropped"]["windows"], R["dropped"]["mode"]) == (32, 2) and R["dropped"]["failed"] > 0
    assert Pm["prefix"]["used"].max() >= 2 and R["prefix"]["used"].max() >= 2 and Pm["flagged-32"]["used"].max() >= 2
    assert (Pm["dropped"]["windows"], Pm["dropped"]["mode"]) == (8, 2) and Pm["dropped"]["used"].max() >= 2


def test_span_edge_case_places_both_edges(verdicts):
    """The hand-placed links keep the chain's two colour classes where the case's docstring says, and give: a real column at exactly base + 8 191
    that stays in its window, a window opened at exactly base + 8 192, a slice of exactly eight windows and one of exactly nine."""
    m, L = verdicts["span-edge"][0][0], verdicts["span-edge"][1]
    n, H = cc.SPAN_EDGE_N, cc.span_edge_half()
    n2o = L["plan0"]["new2old"]
    assert L["plan0"]["n_colors"] == 2 and np.array_equal(n2o[: n // 2], np.arange(0, n, 2)) and np.array_equal(n2o[H: H + n // 2], np.arange(1, n, 2))
    sp_, col, real = L[0]
    wb = m["win_base"]
    assert list(m["needed"][:4]) == [9, 1, 2, 8] and wb[0, 0] == -1 and m["from"] == 1
    cols1 = col[sp_[1]:sp_[2]][real[sp_[1]:sp_[2]]]
    assert wb[1, 0] == H + 63 and cols1.max() == wb[1, 0] + 8191 and wb[1, 1] == wb[1, 0]
    assert wb[2, 0] == H + 127 and wb[2, 1] == wb[2, 0] + 8192 and wb[2, 2] == wb[2, 1]
    assert list(np.diff(wb[3])) == [8192] * 7
