"""The catalogue of synthetic level-0 operators that take the 16-bit column codes (tests/colcode_model.py) through every branch of their
set-up, shared by tests/test_colcode_model_host.py (the branch is reached from the host planner's ordering alone) and
tests/test_gpu_column_codes.py (the device against the model and against the 32-bit path).

Every case is a chain or ring of n vertices plus long links (problems.synthetic_problem, graph kind "links"), hand-made prolongations and a
"smoothing" system.  expect: the branch of the OPERATOR the case is in the catalogue for -- windows, mode and, where named, from > 0
("prefix"), failed > 0 ("failed"), a recode ("recoded"), slices with several windows ("multi"), a uniform width."""
import functools

import numpy as np
import scipy.sparse as sp

from tests import colcode_model as cm
from tests import problems

PINNED = dict(reorder_fine=0, block_fine=0)      # no renumbering of a level with long links, no blocking of the offset graphs (Stieltjes, > 9 entries per row)


def _offsets(n, step, count):
    a = [np.arange(n - step * j) for j in range(1, count + 1)]
    return np.concatenate(a), np.concatenate([x + step * j for j, x in enumerate(a, start=1)])


def _two_window():
    return 20000, False, np.arange(20000 - 9001), np.arange(20000 - 9001) + 9001


def _ring_uniform():
    n = 20480
    return n, True, np.arange(n), (np.arange(n) + 9001) % n


def _prefix():
    n, rng = 90000, np.random.default_rng(11)
    hubs = rng.choice(n, 5, replace=False)
    return n, False, np.repeat(hubs, 40), rng.integers(0, n, 200)


def _flagged_8():
    return (90000, False) + _offsets(90000, 8201, 9)


def _recode_32():
    return (120000, False) + _offsets(120000, 8201, 12)


def _flagged_32():
    n, rng = 120000, np.random.default_rng(12)
    a, b = _offsets(n, 8201, 12)
    rows = np.concatenate([np.arange(6400 * k, 6400 * k + 200) for k in range(1, 18)])
    return n, False, np.concatenate([a, rows]), np.concatenate([b, rng.integers(0, n, len(rows))])


def _dropped():
    n, rng = 120000, np.random.default_rng(13)
    return n, False, np.arange(n), rng.integers(0, n, n)


SPAN_EDGE_N = 132000


def span_edge_half(n=SPAN_EDGE_N):
    """First device row of the odd naturals of a chain: the even naturals' colour class padded to whole slices."""
    return 64 * (-(-((n + 1) // 2) // 64))


def _span_edge():
    """A chain keeps its two colour classes when every link joins an even natural to an odd one: even i sits in device row i / 2, odd i in
    H + (i - 1) / 2.  Slice s of the even class holds the even naturals 128 s .. 128 s + 126; its chain columns are H + 64 s - 1 .. H + 64 s + 63
    (from H for s = 0), so its first base is b_s = H + 64 s - 1 (H for s = 0).  Links, one per row, from the rows 128 s + 2 m of slice s to the odd
    natural in device column t: slice 0: t = b_0 + 8192 m, m = 1 .. 8 -- nine windows, uncovered; slice 1: t = b_1 + 8191 -- the last column of its
    first window; slice 2: t = b_2 + 8192 -- opens a window at exactly base + span; slice 3: t = b_3 + 8192 m, m = 1 .. 7 -- exactly eight."""
    n = SPAN_EDGE_N
    H = span_edge_half(n)
    b = [H] + [H + 64 * s - 1 for s in (1, 2, 3)]
    rows, targets = [], []
    for s, ts in ((0, [b[0] + 8192 * m for m in range(1, 9)]), (1, [b[1] + 8191]), (2, [b[2] + 8192]), (3, [b[3] + 8192 * m for m in range(1, 8)])):
        for m, t in enumerate(ts, start=1):
            rows.append(128 * s + 2 * m); targets.append(2 * (t - H) + 1)
    assert max(targets) < n
    return n, False, np.array(rows), np.array(targets)


def _sizes(n):
    return [n, n // 4, n // 40, n // 400]


# name -> (links, sizes or None for the usual ones, engine settings, expected branch of A)
FALLBACK = "host-fallback"      # not in CASES: the prefix graph with smoothed prolongations, level-1 rows of 127 entries

CASES = {
    "two-window": (_two_window, None, PINNED, dict(windows=8, mode=1, prefix=False, failed=False, multi=True)),
    "ring-uniform": (_ring_uniform, None, PINNED, dict(windows=8, mode=1, prefix=False, failed=False, multi=True, uniform_width=4)),
    # (piecewise-constant prolongations where long or random links make the coarse operators dense: a row of more than 96 entries on a level
    # below the coarsest sends the whole set-up to the host planner, which makes no codes -- the case "host-fallback")
    "prefix": (_prefix, None, dict(PINNED, prolong=("pc",)), dict(windows=8, mode=1, prefix=True, failed=True)),
    "flagged-8": (_flagged_8, None, PINNED, dict(windows=8, mode=2, failed=True, multi=True)),
    "recode-32": (_recode_32, None, PINNED, dict(windows=32, mode=1, recoded=True, multi=True)),
    "flagged-32": (_flagged_32, None, dict(PINNED, prolong=("pc",)), dict(windows=32, mode=2, recoded=True, failed=True, multi=True)),
    "dropped": (_dropped, [120000, 30000, 3000], dict(PINNED, prolong=("pc",)), dict(windows=0, mode=0, recoded=True, failed=True)),
    "span-edge": (_span_edge, None, PINNED, dict(windows=8, mode=1, prefix=True, failed=True, multi=True)),
    "defaults": (_flagged_8, None, dict(), None),
    "blocked-lane1": (_recode_32, None, dict(block_lanes=1), None),      # (reorder_fine = 0 would keep level 0 colour-major)
    # recode-32 with a level 1 of more than 65 536 rows: the default layout then gives level 1 one lane per row and the entry-parallel sweep, and the
    # restriction its quad layout -- what the fused restriction + first sweep (restrict_sweep0) needs.  (block_lanes = 1 gives the restriction one
    # lane per row, which that kernel does not take; with n_1 = n / 4 level 1 gets four lanes per row and no entry-parallel sweep.)
    "fused-restrict": (_recode_32, [120000, 66000, 3000, 300], PINNED, dict(windows=32, mode=1, recoded=True, multi=True)),
}


@functools.lru_cache(maxsize=2)
def problem(name, d=8, prolong=None):
    links, sizes, kw, _ = CASES[name] if name != FALLBACK else (_prefix, None, PINNED, None)
    n, ring, a, b = links()
    return problems.synthetic_problem(("links", n, ring, a, b), sizes or _sizes(n), kind="smoothing", prolong=prolong or kw.get("prolong", ("smooth", "pc")), d=d)


def engine_settings(name):
    return {k: v for k, v in CASES[name][2].items() if k != "prolong"}


def check_branch(name, m):
    """Does the model's verdict m (colcode_model.model) for the operator lie on the branch the case is in the catalogue for?"""
    want = CASES[name][3]
    if want is None:
        return
    assert m["windows"] == want["windows"] and m["mode"] == want["mode"], (name, m["windows"], m["mode"], m["failed"], m["last"])
    if "prefix" in want:
        assert (m["from"] > 0) == want["prefix"], (name, m["from"])
    if "failed" in want:
        assert (m["failed"] > 0) == want["failed"], (name, m["failed"])
    if "recoded" in want:
        assert m["recoded"] == want["recoded"], name
    if want.get("multi"):
        assert m["used"].max() >= 2, name
    if "uniform_width" in want:
        assert m["uniform_width"] == want["uniform_width"], (name, m["uniform_width"])


def describe(m):
    return dict(windows=m["windows"], mode=m["mode"], **{"from": m["from"]}, failed=m["failed"], last=m["last"], uniform_width=m["uniform_width"],
                max_used=int(m["used"].max()) if len(m["used"]) else 0, max_needed=int(m["needed"].max()) if len(m["needed"]) else 0,
                multi_slices=int((m["used"] >= 2).sum()), n_slices=len(m["used"]))


# ---- the three level-0 layouts from the host planner alone (no device) ----------------------------------------------------------------
def _device_csr(M, row_new, col_new, n_rows):
    """CSR over device rows of the entries of M (coo): row r = row_new[M.row], column col_new[M.col], in the source's column order."""
    M = sp.coo_matrix(M)
    r, c = row_new[M.row], col_new[M.col]
    order = np.lexsort((M.col, r))
    ptr = np.zeros(n_rows + 1, np.int64)
    np.add.at(ptr, r + 1, 1)
    return np.cumsum(ptr), c[order], M.data[order]


def host_layouts(cabi, P, block_lanes=0, restrict_sigma=64):
    """(slice_ptr, col, real) of A (off-diagonal), P and R of level 0 as the engine lays them out under the pinned settings, from
    cabi.host_plan_level alone: level 0 colour-major (mode 0, sigma 0), level 1 = the Galerkin product in block order (64 rows per block); the
    restriction with four lanes per row (one with block_lanes = 1) and its rows sorted by length inside windows of restrict_sigma rows."""
    lhs = sp.csc_matrix(P.lhs)
    n = lhs.shape[0]
    plan0 = cabi.host_plan_level(lhs, mode=0, sigma=0)
    n2o = plan0["new2old"]
    o2n = np.full(n, -1, np.int64); o2n[n2o[n2o >= 0]] = np.flatnonzero(n2o >= 0)
    coo = lhs.tocoo()
    off = coo.row != coo.col
    A = sp.coo_matrix((np.ones(off.sum()), (coo.row[off], coo.col[off])), shape=lhs.shape)
    sa = cm.sell_from_rows(*_device_csr(A, o2n, o2n, len(n2o)))
    U = sp.csc_matrix(P.U[0])
    A1 = cabi.host_galerkin(lhs, U)
    plan1 = cabi.host_plan_level(A1, mode=1, block_rows=64)
    n2o1 = plan1["new2old"]
    o2n1 = np.full(U.shape[1], -1, np.int64); o2n1[n2o1[n2o1 >= 0]] = np.flatnonzero(n2o1 >= 0)
    sp_ = cm.sell_from_rows(*_device_csr(U, o2n, o2n1, len(n2o)))
    ptr, cols, vals = _device_csr(U.T, o2n1, o2n, len(n2o1))
    if restrict_sigma:
        length = np.diff(ptr)
        order = np.concatenate([w + np.argsort(-length[w:w + restrict_sigma], kind="stable") for w in range(0, len(length), restrict_sigma)])
        gather = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in order]) if len(cols) else np.zeros(0, int)
        ptr, cols, vals = np.concatenate([[0], np.cumsum(length[order])]), cols[gather], vals[gather]
    sr = cm.sell_from_rows(ptr, cols, vals, lpr=1 if block_lanes == 1 else 4)
    return {"plan0": plan0, "plan1": plan1, 0: sa[:2] + (sa[3],), 3: sp_[:2] + (sp_[3] & (sp_[2] != 0),), 4: sr[:2] + (sr[3] & (sr[2] != 0),)}
