"""Catalogue of Galerkin products U^T A U, one (or a few) per branch of the device kernel (csrc/setup_kernels.hip.hpp::rap_rows) and of the
prefix sum under it.  Every case names the labels (tests/rap_model.py::ALL_LABELS) it is in the catalogue for; tests/test_rap_model_host.py
asserts from the model alone that it reaches them, tests/test_gpu_galerkin_branches.py runs every case on the device.

All graphs come from tests/problems.py::synthetic_problem ("links", "chain", "diagonal"); "pc" prolongations have rows of 1 entry, "smooth"
ones rows of 2 and 3 with different weights.  A case is built on first use and kept (the largest one takes a few seconds).
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

from tests import problems, rap_model

CNTS = (64, 65, 128, 129, 192, 193, 256, 257)      # distinct columns of one coarse row: either side of every group edge and of the set's capacity
assert rap_model.K_RAP_SET == 256 and rap_model.K_RAP_SLOTS == 192 and rap_model.K_SCAN_TILE == 2048, "the catalogue's shapes follow these constants: move them along"


class Case:
    def __init__(self, name, A, U, wanted, row=None, big=False, sample=None, problem=None):
        self.name, self.A, self.U, self.wanted, self.row, self.big, self.sample, self.problem = name, A, U, set(wanted), row, big, sample, problem


def raw(m):
    """CSC with int32 indices whose stored order and stored zeros are kept"""
    m = sp.csc_matrix(m)
    return sp.csc_matrix((m.data.astype(np.float64), m.indices.astype(np.int32), m.indptr.astype(np.int32)), shape=m.shape)


# ---- one coarse row of exactly cnt distinct columns ---------------------------------------------------------------------------------------
HUB_GROUP = 150        # level-1 group of the chain of 2 400 in groups of 8 whose 8 children share the links


def cnt_links(cnt, prolong):
    """Links of the 8 children of level-1 group 150 (vertices 1200 .. 1207) to first vertices of far groups, such that level-1 row 150 has
    exactly cnt distinct columns.  pc: the row has 3 columns from the chain and one per link.  smooth: 7 from the chain (groups 147 .. 153), 3
    per link to a group 3 m + 1 (columns 3 m .. 3 m + 2, disjoint from one another) and 2 per link to group 0 or 299 (the ends' rows of U)."""
    if prolong == "pc":
        far = [g for g in range(2, 298) if abs(g - HUB_GROUP) > 3][:cnt - 3]
    else:
        threes, twos = divmod(cnt - 7, 3)
        if twos == 1:                      # 3 a + 1 = 3 (a - 1) + 2 + 2
            threes, twos = threes - 1, 2
        else:
            twos = twos // 2
        far = [3 * m + 1 for m in range(1, 99) if not 47 <= m <= 52][:threes] + [0, 299][:twos]
        assert len(far) == threes + twos
    a = 8 * HUB_GROUP + np.arange(len(far)) % 8
    return a, 8 * np.asarray(far, np.int64)


@functools.lru_cache(maxsize=None)
def cnt_problem(cnt, prolong, levels=3):
    a, b = cnt_links(cnt, prolong)
    return problems.synthetic_problem(("links", 2400, False, a, b), [2400, 300, 75][:levels], prolong=(prolong,), d=2)


def _level1(P, cabi):
    """A_1 of a problem: the host product (tests/test_rap_model_host.py holds it to the model bit for bit)"""
    return raw(cabi.host_galerkin(raw(P.lhs), raw(P.U[0]), as_stored=True))


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------------------
def _groups_label(cnt):
    return "overflow" if cnt > rap_model.K_RAP_SET else f"groups={-(-cnt // 64)}"


def _cnt_case(cnt, prolong, cabi):
    P = cnt_problem(cnt, prolong)
    wanted = {_groups_label(cnt)} | ({"list g>=2"} if 64 < cnt <= rap_model.K_RAP_SET else set())
    return Case(f"cnt{cnt}-{prolong}", raw(P.lhs), raw(P.U[0]), wanted, row=HUB_GROUP, problem=P)


def _second_case(cnt, prolong, cabi):
    """The second product of the same problem: A_1 has one row (150) of exactly cnt entries -- 64 of them are one full list, from 65 on the
    row is walked straight from memory; the level-2 row it belongs to has 19 .. 70 distinct columns (two column groups from 256 entries on)."""
    P = cnt_problem(cnt, prolong)
    wanted = {"list full"} if cnt == 64 else {"straight g=1"} if cnt < 256 else {"straight g>=2"}
    return Case(f"second-cnt{cnt}-{prolong}", _level1(P, cabi), raw(P.U[1]), wanted, row=HUB_GROUP // 4, problem=P)


def _children_case(graph, children, prolong, cabi):
    P = problems.synthetic_problem((graph, 3 * children), [3 * children, 3], prolong=(prolong,), d=1)
    wanted = {"list of several children"} | ({"windows>=2"} if children > 64 else set()) | ({"list full"} if graph == "diagonal" else set())
    return Case(f"children{children}-{graph}-{prolong}", raw(P.lhs), raw(P.U[0]), wanted, problem=P)


def _tail_case(group, cabi):
    """chain of 5 groups of `group` vertices, pc: lists of 3 group entries (one less at the two ends) on one column group"""
    P = problems.synthetic_problem(("chain", 5 * group), [5 * group, 5], prolong=("pc",), d=1)
    tails = {(3 * 3 * group) % 4, (3 * (3 * group - 1)) % 4}
    return Case(f"tail-group{group}", raw(P.lhs), raw(P.U[0]), {f"list g=1 tail={t}" for t in tails} | {"groups=1", "scan tiles=1"}, problem=P)


def _empty_column(cabi):
    P = problems.synthetic_problem(("chain", 12), [12, 4], prolong=("smooth",), d=1)
    U = sp.csc_matrix(P.U[0])
    U = sp.hstack([U[:, :2], sp.csc_matrix((12, 1)), U[:, 2:]]).tocsc()       # coarse column 2 has no entry
    return Case("empty-coarse-column", raw(P.lhs), raw(U), {"groups=0", "no children"})


def _empty_fine_row(cabi):
    P = problems.synthetic_problem(("chain", 12), [12, 4], prolong=("smooth",), d=1)
    A = sp.lil_matrix(P.lhs)
    A[5, :] = 0; A[:, 5] = 0
    A = sp.csc_matrix(A); A.eliminate_zeros(); A.sort_indices()
    assert A.indptr[6] == A.indptr[5]
    return Case("fine-row-without-entries", raw(A), raw(P.U[0]), {"child without entries"})


def _tiny(n, cabi):
    P = problems.synthetic_problem(("chain", n), [n, 1], prolong=("pc",), d=1) if n > 1 else problems.synthetic_problem(("diagonal", 1), [1, 1], d=1)
    return Case(f"one-coarse-row-n{n}", raw(P.lhs), raw(P.U[0]), {"groups=1", "scan tiles=1"})


def _storage_problem():
    rng = np.random.default_rng(11)
    a, b = rng.integers(0, 240, 60), rng.integers(0, 240, 60)
    return problems.synthetic_problem(("links", 240, True, a, b), [240, 40], prolong=("smooth",), d=1)


def _unsorted(cabi):
    P = _storage_problem()
    A = raw(P.lhs)
    rng = np.random.default_rng(12)
    idx, val = A.indices.copy(), A.data.copy()
    for i in range(A.shape[0]):                 # every row in a seeded order of its own
        lo, hi = A.indptr[i], A.indptr[i + 1]
        perm = rng.permutation(hi - lo)
        idx[lo:hi], val[lo:hi] = idx[lo:hi][perm], val[lo:hi][perm]
    A = sp.csc_matrix((val, idx, A.indptr), shape=A.shape)
    assert not (np.diff(A.indices)[np.setdiff1d(np.arange(A.nnz - 1), A.indptr[1:-1] - 1)] > 0).all()
    return Case("unsorted-rows-of-A", A, raw(P.U[0]), {"list of several children"})


def _stored_zeros(cabi):
    P = _storage_problem()
    A, U = raw(P.lhs), raw(P.U[0])
    rng = np.random.default_rng(13)
    A.data[rng.choice(A.nnz, A.nnz // 5, replace=False)] = 0.0
    U.data[rng.choice(U.nnz, U.nnz // 5, replace=False)] = 0.0
    A.data[A.indptr[7]:A.indptr[8]] = 0.0        # a whole row of A and a whole column of U: entries of the product that are sums of zeros
    U.data[U.indptr[3]:U.indptr[4]] = 0.0
    return Case("stored-zeros", A, U, {"list of several children"})


def _four_entry_row(cabi):
    P = _storage_problem()
    U = sp.lil_matrix(P.U[0])
    assert U[100].nnz == 3 and U[100, 30] == 0
    U[100, 30] = 0.125
    return Case("u-row-of-4", raw(P.lhs), raw(sp.csc_matrix(U)), {"flagged"})


def _scan_case(nc, cabi):
    """chain of 2 nc vertices in groups of 2 with links that give the coarse rows next to every tile edge counts of their own"""
    n = 2 * nc
    edges = [e for e in range(rap_model.K_SCAN_TILE, nc, rap_model.K_SCAN_TILE)] + [nc - 1]
    a, b = [], []
    for e in edges:
        for off, extra in ((-2, 1), (-1, 3), (0, 2), (1, 4)):      # coarse rows e - 2 .. e + 1 get 1, 3, 2, 4 links
            if 0 <= e + off < nc:
                for s in range(extra):
                    a.append(2 * (e + off)); b.append(2 * ((e + off + 37 * (s + 1) + 11 * extra) % nc))
    rng = np.random.default_rng(nc)
    a, b = np.concatenate([a, rng.integers(0, n, 20)]), np.concatenate([b, rng.integers(0, n, 20)])
    P = problems.synthetic_problem(("links", n, False, a, b), [n, nc], prolong=("pc",), d=1)
    return Case(f"scan-nc{nc}", raw(P.lhs), raw(P.U[0]), {"scan tiles=1" if nc <= rap_model.K_SCAN_TILE else "scan tiles>=2"}, problem=P)


N_CARRY = rap_model.SCAN_BLOCK * rap_model.K_SCAN_TILE + 1      # the first size at which the scan of the tile sums takes a second pass


def _scan_carry(cabi):
    n = N_CARRY
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, n, 1000), rng.integers(0, n, 1000)
    a[:8] = [1, 2, n - 2, n - 3, n - 2049, n - 2050, 2047, 2048]      # (the two ends of the chain keep their rows of 2)
    P = problems.synthetic_problem(("links", n, False, a, b), [n, n], prolong=("pc",), d=1)      # aggregation(n, n): U = identity
    ends = np.unique(np.concatenate([a, b]))
    tiles = np.arange(rap_model.K_SCAN_TILE, n, rap_model.K_SCAN_TILE)[[0, 1, 511, 1022, 1023]]
    sample = np.unique(np.clip(np.concatenate([ends[:120], ends[-40:], tiles - 1, tiles, tiles + 1, [0, 1, n - 2, n - 1]]), 0, n - 1))
    return Case("scan-carry", raw(P.lhs), raw(P.U[0]), {"scan passes>=2", "scan tiles>=2"}, big=True, sample=sample)


HUBS = (600, 601)       # level-1 groups of the two-hub graph


@functools.lru_cache(maxsize=None)
def two_hub_problem():
    """chain of 9 600, level-1 groups of 8, level-2 groups of 3 level-1 groups.  Level-1 groups 600 and 601 get 150 links each, to the first
    vertices of level-1 groups 3 m with 300 distinct m: level-1 rows 600 / 601 have 153 columns (device), level-2 row 200 has 303 (declined)."""
    ms = [m for m in range(400) if abs(m - 200) > 1][:300]
    a = np.concatenate([8 * g + np.arange(150) % 8 for g in HUBS])
    return problems.synthetic_problem(("links", 9600, False, a, 24 * np.asarray(ms, np.int64)), [9600, 1200, 400], prolong=("pc",), d=2)


def _two_hub(level, cabi):
    P = two_hub_problem()
    if level == 1:
        return Case("two-hub-level1", raw(P.lhs), raw(P.U[0]), {"groups=3", "list g>=2"}, row=HUBS[0], problem=P)
    return Case("two-hub-level2", _level1(P, cabi), raw(P.U[1]), {"overflow"}, row=HUBS[0] // 3, problem=P)


BUILDERS = {}
for _cnt in CNTS:
    for _pro in ("pc", "smooth"):
        BUILDERS[f"cnt{_cnt}-{_pro}"] = functools.partial(_cnt_case, _cnt, _pro)
        BUILDERS[f"second-cnt{_cnt}-{_pro}"] = functools.partial(_second_case, _cnt, _pro)
for _ch in (64, 65, 128, 129):
    BUILDERS[f"children{_ch}-diagonal-pc"] = functools.partial(_children_case, "diagonal", _ch, "pc")
    BUILDERS[f"children{_ch}-diagonal-smooth"] = functools.partial(_children_case, "diagonal", _ch, "smooth")
    BUILDERS[f"children{_ch}-chain-pc"] = functools.partial(_children_case, "chain", _ch, "pc")
    BUILDERS[f"children{_ch}-chain-smooth"] = functools.partial(_children_case, "chain", _ch, "smooth")
for _g in (1, 2, 3, 4):
    BUILDERS[f"tail-group{_g}"] = functools.partial(_tail_case, _g)
BUILDERS["empty-coarse-column"] = _empty_column
BUILDERS["fine-row-without-entries"] = _empty_fine_row
BUILDERS["one-coarse-row-n7"] = functools.partial(_tiny, 7)
BUILDERS["one-coarse-row-n1"] = functools.partial(_tiny, 1)
BUILDERS["unsorted-rows-of-A"] = _unsorted
BUILDERS["stored-zeros"] = _stored_zeros
BUILDERS["u-row-of-4"] = _four_entry_row
for _nc in (2047, 2048, 2049, 4097):
    BUILDERS[f"scan-nc{_nc}"] = functools.partial(_scan_case, _nc)
BUILDERS["scan-carry"] = _scan_carry
BUILDERS["two-hub-level1"] = functools.partial(_two_hub, 1)
BUILDERS["two-hub-level2"] = functools.partial(_two_hub, 2)

NAMES = tuple(BUILDERS)
SMALL_NAMES = tuple(n for n in NAMES if n != "scan-carry")


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    from gravo_mg_amd import cabi
    c = BUILDERS[name](cabi)
    assert c.name == name, (c.name, name)
    return c


@functools.lru_cache(maxsize=None)
def model_branches(name):
    c = case(name)
    return rap_model.branches(c.A, c.U, rows=c.sample)


@functools.lru_cache(maxsize=None)
def model_exact(name):
    c = case(name)
    return rap_model.exact(c.A, c.U)


def expected_status(name) -> int:
    """1 when the device declines: a U row of more than 3 entries, or a coarse row of more distinct columns than the hash set holds"""
    br = model_branches(name)
    return int(br["flagged"] or any(r["overflow"] for r in br["rows"].values()))
