"""Plain restatement of the Galerkin product Ac = U^T A U as the engine computes it (csrc/host_sparse.hpp::galerkin_rap on the host,
csrc/setup_kernels.hip.hpp::rap_rows on the device), and of the choices the device kernel makes on the way.  numpy and Python scalars only:
no ctypes, no library call.

    product(A, U)   the host's walk -- for i in column p of U / for j in row i of A as stored / for c in row j of U ascending -- with the
                    multiply and the add rounded separately in float64; the pattern is kept structurally and every row sorted
    exact(A, U)     the same entries without rounding, the number of terms of every entry and |U|^T |A| |U|
    branches(A, U)  per coarse row what rap_rows does with it: distinct columns, column groups, overflow, the chunks of children, windows

A is n x n in compressed storage with a symmetric pattern, read "as stored" (column i of the arrays is row i of the walk); U is n x n_c by
coarse column.  Both are taken as (indptr, indices, data) of a scipy CSC matrix without touching their order.
"""
from __future__ import annotations

import os
import re
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "gravo_mg_amd", "csrc", "setup_kernels.hip.hpp")).read()


def _constant(name: str) -> int:
    return int(re.search(r"constexpr int %s = (\d+);" % name, _SRC).group(1))


K_RAP_SET = _constant("kRapSet")          # hash-set capacity of one coarse row
K_RAP_SLOTS = _constant("kRapSlots")      # LDS list of one chunk of children: 3 slots per entry of A
K_SCAN_TILE = _constant("kScanTile")      # items of one tile of the prefix sum
SCAN_BLOCK = 1024                         # tile sums one pass of scan_tile_offsets takes (its block size)
U_ROUND = Fraction(1, 2 ** 53)            # unit roundoff of float64


def gamma(k: int) -> Fraction:
    """gamma_k = k u / (1 - k u)"""
    return k * U_ROUND / (1 - k * U_ROUND)


def rows_of(U):
    """U regrouped by fine row, columns ascending (host: transpose(); device: ell3_from_csc + ell3_sort): (ptr, col, val)."""
    n = U.shape[0]
    col_of = np.repeat(np.arange(U.shape[1]), np.diff(U.indptr))
    order = np.argsort(U.indices, kind="stable")          # entries of a row in the order of their columns
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(U.indices, minlength=n), out=ptr[1:])
    return ptr, col_of[order], U.data[order]


def _walk(A, U, rows=None):
    """The triples of every coarse row p (or of `rows`) in the host's order: yields (p, [(q, u_ip, a_ij, u_jq), ...])."""
    rptr, rcol, rval = rows_of(U)
    ap, ai, av = A.indptr, A.indices, A.data
    up, ui, uv = U.indptr, U.indices, U.data
    for p in (range(U.shape[1]) if rows is None else rows):
        out = []
        for a in range(up[p], up[p + 1]):
            i, uip = int(ui[a]), float(uv[a])
            for b in range(ap[i], ap[i + 1]):
                j, aij = int(ai[b]), float(av[b])
                for c in range(rptr[j], rptr[j + 1]):
                    out.append((int(rcol[c]), uip, aij, float(rval[c])))
        yield int(p), out


def product(A, U, rows=None):
    """(indptr, indices, data) of Ac in float64, bit for bit what the host computes.  rows: only these coarse rows (indptr then counts them
    in the order given)."""
    ptr, idx, val = [0], [], []
    for p, triples in _walk(A, U, rows):
        acc = {}
        for q, uip, aij, ujq in triples:
            w = uip * aij                      # rounded
            pr = w * ujq                       # rounded
            acc[q] = acc.get(q, 0.0) + pr      # rounded; a first term is added to 0.0 like the host's
        for q in sorted(acc):
            idx.append(q); val.append(acc[q])
        ptr.append(len(idx))
    return np.asarray(ptr, np.int64), np.asarray(idx, np.int64), np.asarray(val, np.float64)


def _dyadic(x: float):
    """x = m / 2^e with integers m, e >= 0"""
    m, d = x.as_integer_ratio()
    return m, d.bit_length() - 1


def exact(A, U, rows=None):
    """(indptr, indices, value, terms, absvalue): the entries of U^T A U as Fractions, the number of terms t of each and the same sum over
    absolute values.  Sums are carried as integers over a power of two (every float64 is dyadic): no rounding anywhere."""
    ptr, idx, val, terms, absval = [0], [], [], [], []
    for p, triples in _walk(A, U, rows):
        acc = {}
        for q, uip, aij, ujq in triples:
            (m1, e1), (m2, e2), (m3, e3) = _dyadic(uip), _dyadic(aij), _dyadic(ujq)
            m, e = m1 * m2 * m3, e1 + e2 + e3
            s = acc.get(q)
            if s is None:
                acc[q] = [m, abs(m), e, 1]
                continue
            if e > s[2]:
                s[0] <<= e - s[2]; s[1] <<= e - s[2]; s[2] = e
            s[0] += m << (s[2] - e); s[1] += abs(m) << (s[2] - e); s[3] += 1
        for q in sorted(acc):
            m, ma, e, t = acc[q]
            idx.append(q); val.append(Fraction(m, 1 << e)); absval.append(Fraction(ma, 1 << e)); terms.append(t)
        ptr.append(len(idx))
    return np.asarray(ptr, np.int64), np.asarray(idx, np.int64), val, terms, absval


def within_exact_bound(values, ex):
    """Entry by entry |value - exact| <= gamma_(t+1) |U|^T |A| |U|: every term of an entry carries two roundings (u_ip a_ij, then times u_jq)
    and the entry t - 1 additions (the first one, to 0.0, is exact), so its computed value is sum_k term_k (1 + theta_k) with
    |theta_k| <= gamma_(t+1).  Returns the positions that miss the bound (empty = holds)."""
    _, _, val, terms, absval = ex
    assert len(values) == len(val)
    return [e for e in range(len(val)) if abs(Fraction(float(values[e])) - val[e]) > gamma(terms[e] + 1) * absval[e]]


# ---- what the device kernel does with a coarse row ------------------------------------------------------------------------------------
def branches(A, U, rows=None):
    """{"flagged": a row of U has more than 3 entries (the product kernel is not launched), "scan_tiles": tiles of the prefix sum over the row
    counts, "scan_passes": passes of the one-block scan over the tile sums, "rows": per coarse row a dict
        cnt, groups (= ceil(cnt / 64): column slots per lane), overflow (cnt > kRapSet: the row does not fit the hash set),
        children, windows (= ceil(children / 64)),
        chunks: the kernel's walk over the children -- of the next 64 the longest prefix whose rows of A hold at most kRapSlots / 3 entries
                goes through the LDS list ({"kind": "list", "children", "pairs", "tail": 3 pairs % 4, "full": pairs == kRapSlots / 3, "empty": children without an entry});
                when not even the first one fits, that child is walked straight from memory ({"kind": "straight", "pairs"}) }"""
    rptr, rcol, _ = rows_of(U)
    rcnt = np.diff(rptr)
    flagged = bool((rcnt > 3).any())
    alen = np.diff(A.indptr)
    per_row = {}
    nc = U.shape[1]
    for p in (range(nc) if rows is None else rows):
        kids = U.indices[U.indptr[p]:U.indptr[p + 1]]
        cols = set()
        for i in kids:
            for j in A.indices[A.indptr[i]:A.indptr[i + 1]]:
                cols.update(rcol[rptr[j]:rptr[j] + min(int(rcnt[j]), 3)].tolist())
        cnt = len(cols)
        chunks, t0 = [], 0
        while t0 < len(kids):
            incl = np.cumsum(alen[kids[t0:t0 + 64]])
            m = int((3 * incl <= K_RAP_SLOTS).sum())              # incl does not decrease: the fitting children are a prefix
            if m == 0:
                chunks.append({"kind": "straight", "pairs": int(incl[0])})
                t0 += 1
                continue
            pairs = int(incl[m - 1])
            chunks.append({"kind": "list", "children": m, "pairs": pairs, "tail": 3 * pairs % 4, "full": 3 * pairs == K_RAP_SLOTS,
                           "empty": int((alen[kids[t0:t0 + m]] == 0).sum())})
            t0 += m
        per_row[int(p)] = {"cnt": cnt, "groups": -(-cnt // 64), "overflow": cnt > K_RAP_SET, "children": len(kids),
                           "windows": -(-len(kids) // 64), "chunks": chunks}
    tiles = max(1, -(-nc // K_SCAN_TILE))
    return {"flagged": flagged, "scan_tiles": tiles, "scan_passes": -(-tiles // SCAN_BLOCK), "rows": per_row}


ALL_LABELS = (
    "groups=0", "groups=1", "groups=2", "groups=3", "groups=4", "overflow", "flagged",
    "list g=1 tail=0", "list g=1 tail=1", "list g=1 tail=2", "list g=1 tail=3", "list g>=2", "list full", "list of several children",
    "straight g=1", "straight g>=2", "windows>=2", "no children", "child without entries",
    "scan tiles=1", "scan tiles>=2", "scan passes>=2",
)


def labels(br):
    """The branch labels (ALL_LABELS) a product reaches, from branches() alone.  A flagged product reaches nothing else (no launch); rows
    past an overflow still run in the counting pass, but the product is declined, so an overflowing product counts for "overflow" only."""
    if br["flagged"]:
        return {"flagged"}
    if any(r["overflow"] for r in br["rows"].values()):
        return {"overflow"}
    out = {"scan tiles=1" if br["scan_tiles"] == 1 else "scan tiles>=2"}
    if br["scan_passes"] >= 2:
        out.add("scan passes>=2")
    for r in br["rows"].values():
        g = r["groups"]
        out.add(f"groups={g}")
        if r["children"] == 0:
            out.add("no children")
        if r["windows"] >= 2:
            out.add("windows>=2")
        for c in r["chunks"]:
            if c["kind"] == "straight":
                out.add("straight g=1" if g == 1 else "straight g>=2" if g >= 2 else "straight g=0")
                continue
            if c["empty"]:
                out.add("child without entries")
            if c["children"] >= 2:
                out.add("list of several children")
            if c["full"]:
                out.add("list full")
            if g == 1:
                out.add(f"list g=1 tail={c['tail']}")
            elif g >= 2:
                out.add("list g>=2")
    return out
