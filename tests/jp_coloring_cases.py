"""Patterns and the independent restatement for the Jones-Plassmann colouring of gmg_config::device_coloring (test infrastructure, shared by
tests/test_jp_coloring_host.py and tests/test_gpu_device_coloring.py).

The restatement below is the specification written a second time, in numpy, without looking at a row twice in any particular order:
synchronous rounds; priority of v = (mix32(v), v); an uncoloured vertex wins a round when no neighbour that is uncoloured at the start of the
round has a larger priority; a winner takes the smallest colour no neighbour held before the round.  mix32, copied from the comment in
csrc/host_plan.hpp:   x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16   (mod 2^32)."""
import functools

import numpy as np
import scipy.sparse as sp

from gravo_mg_amd import meshgen

MAX_COLOURS = 254          # colours 0 .. 253 fit the byte colouring; beyond: -1
FULL_ROUNDS = 4            # csrc/engine_setup.hip.hpp::kJpFullRounds: the device's rounds over all rows; later rounds run over the compacted worklist


def mix32(v):
    x = np.asarray(v, np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x


def restatement(indptr, indices):
    """(colours uint8, n_colors, rounds), or (None, -1, 0) when 254 colours do not suffice."""
    indptr = np.asarray(indptr, np.int64); indices = np.asarray(indices, np.int64)
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    keep = rows != indices                                     # self-loops are ignored
    r, c = rows[keep], indices[keep]
    prio = (mix32(np.arange(n)) << np.uint64(32)) | np.arange(n, dtype=np.uint64)      # lexicographic (hash, index) as one integer
    colour = np.full(n, -1, np.int64)
    rounds = 0
    while (colour < 0).any():
        unc = colour < 0
        beaten = unc[r] & unc[c] & (prio[c] > prio[r])
        lose = np.zeros(n, bool); lose[r[beaten]] = True
        win = unc & ~lose
        assert win.any()
        used = np.zeros((n, 256), bool)
        seen = win[r] & ~unc[c]                                # the winners' neighbours coloured before this round
        used[r[seen], colour[c[seen]]] = True
        first = np.argmin(used[win], axis=1)                   # first False of every winner's row
        assert not used[win].all(axis=1).any()
        if (first >= MAX_COLOURS).any():
            return None, -1, 0
        colour[win] = first
        rounds += 1
    return colour.astype(np.uint8), int(colour.max(initial=-1)) + 1, rounds


def _pattern(M):
    M = sp.csc_matrix(M)
    M.sort_indices()
    return M.indptr.astype(np.int32), M.indices.astype(np.int32)


def _from_edges(n, a, b, loops=()):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    rows = np.concatenate([a, b, np.asarray(loops, np.int64)]); cols = np.concatenate([b, a, np.asarray(loops, np.int64)])
    M = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n)).tocsc()
    M.sum_duplicates()
    return _pattern(M)


def path(n, chords=False):
    """0 - 1 - .. - n-1; chords: also i - (7 i + 3) mod n for every third i (rows of different lengths)."""
    a, b = np.arange(n - 1), np.arange(1, n)
    if chords:
        i = np.arange(0, n, 3); j = (7 * i + 3) % n
        ok = i != j
        a, b = np.concatenate([a, i[ok]]), np.concatenate([b, j[ok]])
    return _from_edges(n, a, b)


def complete(n):
    a, b = np.triu_indices(n, 1)
    return _from_edges(n, a, b)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (indptr, indices): symmetric patterns, int32, rows ascending."""
    V, F = meshgen.torus_mesh(24, 24)
    S, _ = meshgen.cotan_laplacian(V, F)
    Vs, Fs = meshgen.sphere_mesh(2000)
    Ss, _ = meshgen.cotan_laplacian(Vs, Fs)
    Sk, _ = meshgen.knn_graph_laplacian(meshgen.torus_points(2000, noise=0.002), 8)
    out = {
        "torus24x24": _pattern(S),
        "sphere2000": _pattern(Ss),
        "torus-two-ring": _pattern(sp.csc_matrix(S) @ sp.csc_matrix(S)),
        "knn8-2000": _pattern(Sk),
        "path300": path(300),
        "complete70": complete(70),                            # 70 colours: past the 64-bit mask
        # 0 - 1 - 2 - 3, a loop on 1, vertex 4 without any entry, vertex 5 with its loop only
        "isolated-and-loop": _from_edges(6, [0, 1, 2], [1, 2, 3], loops=[1, 5]),
        "single": (np.array([0, 1], np.int32), np.array([0], np.int32)),
    }
    return out


@functools.lru_cache(maxsize=None)
def boundary_cases():
    """The wave boundary (63, 64, 65 rows) and a worklist that spans more than one workgroup and ends inside one (4 097 rows)."""
    return {f"chords{n}": path(n, chords=True) for n in (63, 64, 65, 4097)}


def degrees(indptr, indices):
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    off = rows != indices
    return np.bincount(rows[off], minlength=n)


def assert_proper(indptr, indices, colours, n_colors):
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    off = rows != indices
    assert np.all(colours[rows[off]] != colours[indices[off]])
    assert np.array_equal(np.unique(colours), np.arange(n_colors))


def other_representations(indptr, indices, seed=0):
    """The same symmetric pattern as the CSC arrays of the transpose, and with every row's index list in a shuffled order."""
    n = len(indptr) - 1
    A = sp.csc_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n))
    T = sp.csc_matrix(A.T)                                    # (CSR of A reread as CSC: the rows' lists come out as the conversion leaves them)
    rng = np.random.default_rng(seed)
    shuffled = np.array(indices, copy=True)
    for i in range(n):
        rng.shuffle(shuffled[indptr[i]:indptr[i + 1]])
    return [(T.indptr.astype(np.int32), T.indices.astype(np.int32)), (np.asarray(indptr, np.int32), shuffled.astype(np.int32))]
