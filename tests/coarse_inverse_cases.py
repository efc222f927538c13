"""The smallest matrices that reach each branch of the device-built coarse inverse (setup_kernels.hip.hpp::coarse_inverse_tiles and its
follow-up kernels), for tests/test_coarse_inverse_model_host.py and tests/test_gpu_coarse_inverse_tiles.py.  Every matrix is generated here.

A case: a name, a symmetric positive definite matrix, the tile widths it runs at, and per width the labels it must reach.  Reaching is read
from gmg_debug_coarse_inverse's info[] and exported arrays in mode 0 (host only) by labels(): the catalogue is verified without a device."""
import os
import re

import numpy as np
import scipy.sparse as sp

from tests import problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "gravo_mg_amd", "csrc", "setup_kernels.hip.hpp")).read()
K_BIG_ROWS = int(re.search(r"constexpr int kInvBigRows = (\d+);", _SRC).group(1))
K_WAVES = int(re.search(r"constexpr int kInvWaves = (\d+);", _SRC).group(1))
K_CHUNK = int(re.search(r"constexpr int kInvChunk = (\d+);", _SRC).group(1))
WIDTHS = (16, 32, 64)

PER_WIDTH = ("one-tile", "tiles-ragged", "tile-two-trees", "big-gather-second-trip", "down-second-trip", "big-ragged-rows", "small-gather-second-trip")
PLAIN = ("narrow-chunk", "full-chunk", "no-rows", "round-robin-second-trip", "many-roots", "deep-chain", "forest", "big-chunk", "big-and-small-level",
         "rows-below-big-1", "rows-at-big", "rows-above-big+1", "galerkin", "twin")
ALL_LABELS = tuple(f"{p}-{w}" for p in PER_WIDTH for w in WIDTHS) + PLAIN


def labels(info, E, width, flags=()):
    """What the kernel at `width` does on this export, as a set of labels."""
    S = 64 // width
    n = len(E["perm"])
    out = set(flags)
    rows_of = np.diff(E["q_rptr"])
    lev_of = np.empty(info["chunks"], np.int64)
    for v in range(info["levels"]):
        lev_of[E["lev_q"][E["lev_ptr"][v]:E["lev_ptr"][v + 1]]] = v
    if info["tiles"] == 1:
        out.add(f"one-tile-{width}")
    if info["tiles"] >= 2 and n % width:
        out.add(f"tiles-ragged-{width}")
    if info["narrow_chunks"]:
        out.add("narrow-chunk")
    if np.any(E["q_w"] == K_CHUNK):
        out.add("full-chunk")
    if info["row_entries"] == 0:
        out.add("no-rows")
    if info["max_level_chunks"] > K_WAVES:
        out.add("round-robin-second-trip")
    if info["roots"] > K_WAVES:
        out.add("many-roots")
    if info["levels"] >= max(n // 8, 2) and np.all(np.diff(E["lev_ptr"]) == 1):
        out.add("deep-chain")
    if info["roots"] >= 2 and info["row_entries"] > 0:
        out.add("forest")
    for t in range(info["tiles"]):           # a tile whose columns lie in different trees: two chunks without rows (roots) on its way down
        tq = E["tile_q"][E["tile_ptr"][t]:E["tile_ptr"][t + 1]]
        if np.sum(rows_of[tq] == 0) >= 2 and np.any(rows_of[tq] > 0):
            out.add(f"tile-two-trees-{width}")
    if info["big_chunks"]:
        out.add("big-chunk")
        big = rows_of[rows_of >= K_BIG_ROWS]
        if big.max() > 8 * K_WAVES * S:
            out.add(f"big-gather-second-trip-{width}")
        if np.any(big % (K_WAVES * S)):
            out.add(f"big-ragged-rows-{width}")
    if info["max_rows"] > 4 * K_WAVES * S:
        out.add(f"down-second-trip-{width}")
    if info["max_small_rows"] > 8 * S:
        out.add(f"small-gather-second-trip-{width}")
    for v in range(info["levels"]):
        r = rows_of[E["lev_q"][E["lev_ptr"][v]:E["lev_ptr"][v + 1]]]
        if np.any(r >= K_BIG_ROWS) and np.any((r < K_BIG_ROWS) & (r > 0)):
            out.add("big-and-small-level")
    for d, name in ((-1, "rows-below-big-1"), (0, "rows-at-big"), (1, "rows-above-big+1")):
        if info["max_rows"] == K_BIG_ROWS + d:
            out.add(name)
    return out


# ---- matrices -------------------------------------------------------------------------------------------------------------------------------------

def _spd_from_edges(n, a, b, rng):
    w = 0.5 + rng.random(len(a))
    W = sp.coo_matrix((w, (a, b)), shape=(n, n)).tocsc()
    W = W + W.T
    A = (sp.diags(np.asarray(W.sum(axis=1)).ravel() + 0.1 + rng.random(n)) - W).tocsc()
    A.sort_indices()
    return A


def sparse_spd(n, seed=3):
    """A ring with n // 2 seeded chords: diagonally dominant, elimination trees with branches and supernodes of several widths."""
    rng = np.random.default_rng(seed + n)
    if n == 1:
        return sp.csc_matrix(np.array([[1.5]]))
    a, b = np.arange(n), (np.arange(n) + 1) % n
    ca, cb = rng.integers(0, n, n // 2), rng.integers(0, n, n // 2)
    key = np.unique(np.minimum(np.concatenate([a, ca]), np.concatenate([b, cb])) * n + np.maximum(np.concatenate([a, ca]), np.concatenate([b, cb])))
    a, b = key // n, key % n
    keep = a != b
    return _spd_from_edges(n, a[keep], b[keep], rng)


def dense_spd(n, seed=7):
    rng = np.random.default_rng(seed + n)
    B = rng.standard_normal((n, n)) / np.sqrt(n)
    A = sp.csc_matrix(B @ B.T + np.diag(1.0 + rng.random(n)))
    A.sort_indices()
    return A


def diagonal(n, seed=1):
    return sp.diags(0.5 + np.random.default_rng(seed).random(n)).tocsc()


def tridiagonal(n, seed=2):
    rng = np.random.default_rng(seed)
    return _spd_from_edges(n, np.arange(n - 1), np.arange(1, n), rng)


def forest(sizes=(23, 9, 41, 14, 30), seed=4):
    """Block diagonal of unequal random trees plus a few chords each."""
    rng = np.random.default_rng(seed)
    a, b, off = [], [], 0
    for m in sizes:
        for i in range(1, m):
            a.append(off + i); b.append(off + int(rng.integers(0, i)))
        for _ in range(m // 6):
            i, j = rng.integers(0, m, 2)
            if i != j:
                a.append(off + int(i)); b.append(off + int(j))
        off += m
    key = np.unique(np.minimum(a, b) * off + np.maximum(a, b))
    return _spd_from_edges(off, key // off, key % off, rng)


def clique_with_fringe(m=210, tail=1, seed=6):
    """A dense clique of m vertices; off every clique vertex hangs a path of `tail` vertices."""
    rng = np.random.default_rng(seed)
    n = m * (1 + tail)
    B = rng.standard_normal((m, m)) / np.sqrt(m)
    C = B @ B.T + np.diag(1.0 + rng.random(m))
    a, b = [], []
    for i in range(m):
        prev = i
        for t in range(tail):
            v = m + i * tail + t
            a.append(prev); b.append(v); prev = v
    F = _spd_from_edges(n, np.array(a), np.array(b), rng).tolil()
    F[:m, :m] = F[:m, :m] + C
    A = sp.csc_matrix(F)
    A.sort_indices()
    return A


def torus_galerkin(n1=36, n2=34, n_c=300, seed=8):
    """U^T (S + 1e-2 M) U of a weighted n1 x n2 torus graph with 3-entry prolongation rows: a coarsest operator as the set-up forms them."""
    rng = np.random.default_rng(seed)
    idx = np.arange(n1 * n2).reshape(n1, n2)
    a = np.concatenate([idx.ravel(), idx.ravel()])
    b = np.concatenate([np.roll(idx, -1, 0).ravel(), np.roll(idx, -1, 1).ravel()])
    n = n1 * n2
    w = 0.5 + rng.random(len(a))
    W = sp.coo_matrix((w, (a, b)), shape=(n, n)).tocsc()
    W = W + W.T
    S = sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W
    lhs = S + 1e-2 * sp.diags(0.5 + rng.random(n))
    U = problems.smoothed_aggregation(n, n_c)
    A = sp.csc_matrix(U.T @ lhs @ U)
    A = ((A + A.T) * 0.5).tocsc()
    A.sort_indices()
    return A


# ---- exact twins: A = L D L^T from a hand-made unit lower triangular L with entries in {-1, 0, 1} on a forest (column j holds one entry, at its
# parent; vertices numbered in postorder, so that there is no fill), D powers of two.  L^-1 has entries in {-1, 0, 1} (path products), so every
# intermediate of both passes is an integer multiple of 2^-3 far below 2^53: any order of operations, fused or not, gives the same bits.

def _twin(parent, seed):
    parent = np.asarray(parent)
    n = len(parent)
    rng = np.random.default_rng(seed)
    L = np.eye(n)
    for j in range(n):
        if parent[j] >= 0:
            assert parent[j] > j
            L[parent[j], j] = rng.choice([-1.0, 1.0])
    D = 2.0 ** rng.integers(-3, 4, n)
    A = sp.csc_matrix(L @ np.diag(D) @ L.T)
    A.sort_indices()
    return A, L, D


def _postorder_parents(children_of_root):
    """parents of a tree given as nested lists (a vertex = the list of its children), numbered in postorder; the root is last"""
    parent = []

    def walk(node):
        kids = [walk(k) for k in node]
        me = len(parent)
        parent.append(-1)
        for k in kids:
            parent[k] = me
        return me
    walk(children_of_root)
    return parent


def _binary(depth):
    return [] if depth == 0 else [_binary(depth - 1), _binary(depth - 1)]


def twin_star(n=40):
    return _twin(_postorder_parents([[] for _ in range(n - 1)]), 11)


def twin_binary(depth=5):
    return _twin(_postorder_parents(_binary(depth)), 12)


def twin_forest():
    parent, off = [], 0
    for tree in ([[[], []], [[]], []], _binary(3), [[[[]]], []], [[] for _ in range(9)]):
        p = _postorder_parents(tree)
        parent += [v + off if v >= 0 else -1 for v in p]
        off = len(parent)
    return _twin(parent, 13)


def twin_comb(k=20):
    node = [[]]
    for _ in range(k - 1):
        node = [node, []]
    return _twin(_postorder_parents(node), 14)


class Case:
    def __init__(self, name, make, widths, must, flags=(), twin=False):
        self.name, self._make, self.widths, self.must, self.flags, self.twin = name, make, widths, must, flags, twin
        self._A = None

    @property
    def A(self):
        if self._A is None:
            made = self._make()
            self._A, self.L, self.D = made if self.twin else (made, None, None)
        return self._A


def _w(label, *widths):
    return {w: {f"{label}-{w}"} for w in widths}


def _merge(*maps):
    out = {}
    for m in maps:
        for w, s in m.items():
            out.setdefault(w, set()).update(s)
    return out


SIZES = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
B = K_BIG_ROWS


def _size_must(n):
    m = {}
    for w in WIDTHS:
        m[w] = {f"one-tile-{w}"} if n <= w else ({f"tiles-ragged-{w}"} if n % w else set())
        if n < K_CHUNK:
            m[w].add("narrow-chunk")
    return m


CASES = [Case(f"n{n}", (lambda n=n: sparse_spd(n)), WIDTHS, _size_must(n)) for n in SIZES] + [
    Case("diagonal300", lambda: diagonal(300), WIDTHS, {w: {"no-rows", "round-robin-second-trip", "many-roots"} for w in WIDTHS}),
    Case("chain200", lambda: tridiagonal(200), WIDTHS, {w: {"deep-chain"} for w in WIDTHS}),
    Case("forest", forest, WIDTHS, _merge({w: {"forest"} for w in WIDTHS}, _w("tile-two-trees", 16, 32, 64))),
    Case("dense60", lambda: dense_spd(60), WIDTHS, _merge(_w("small-gather-second-trip", 16, 32, 64), {w: {"full-chunk", "narrow-chunk"} for w in WIDTHS})),
    Case("dense215", lambda: dense_spd(215), (64,), _merge(_w("big-gather-second-trip", 64), _w("down-second-trip", 64), _w("big-ragged-rows", 64), {64: {"big-chunk"}})),
    Case("dense283", lambda: dense_spd(283), (32,), _merge(_w("big-gather-second-trip", 32), _w("down-second-trip", 32), _w("big-ragged-rows", 32), {32: {"big-chunk"}})),
    Case("dense541", lambda: dense_spd(541), (16,), _merge(_w("big-gather-second-trip", 16), _w("down-second-trip", 16), _w("big-ragged-rows", 16), {16: {"big-chunk"}})),
    Case("clique-fringe", clique_with_fringe, WIDTHS, {w: {"big-and-small-level", "big-chunk"} for w in WIDTHS}),
    Case(f"rows{B - 1}", lambda: dense_spd(B - 1 + K_CHUNK), WIDTHS, {w: {"rows-below-big-1"} for w in WIDTHS}),
    Case(f"rows{B}", lambda: dense_spd(B + K_CHUNK), WIDTHS, {w: {"rows-at-big", "big-chunk"} for w in WIDTHS}),
    Case(f"rows{B + 1}", lambda: dense_spd(B + 1 + K_CHUNK), WIDTHS, {w: {"rows-above-big+1", "big-chunk"} for w in WIDTHS}),
    Case("galerkin-torus", torus_galerkin, WIDTHS, {w: {"galerkin"} for w in WIDTHS}, flags=("galerkin",)),
    Case("twin-star", twin_star, WIDTHS, {w: {"twin"} for w in WIDTHS}, flags=("twin",), twin=True),
    Case("twin-binary", twin_binary, WIDTHS, {w: {"twin"} for w in WIDTHS}, flags=("twin",), twin=True),
    Case("twin-forest", twin_forest, WIDTHS, _merge({w: {"twin", "forest"} for w in WIDTHS}), flags=("twin",), twin=True),
    Case("twin-comb", twin_comb, WIDTHS, {w: {"twin"} for w in WIDTHS}, flags=("twin",), twin=True),
]
NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
TWINS = [c.name for c in CASES if c.twin]
SMALL = [c.name for c in CASES if c.name.startswith("n") and int(c.name[1:]) <= 65]
