"""Plain numpy model of the 16-bit column codes of level 0 (csrc/setup_kernels.hip.hpp::compress_cols and the mode logic behind it in
csrc/engine_setup.hip.hpp, c16_launch / c16_mode_of), restated from their header comments.

A SELL-64 layout stores the entries of slice s at slice_ptr[s] + 64 j + lane (j = 0 .. width - 1).  The model takes such a layout (slice_ptr,
col) and a mask of its REAL entries and gives what the set-up must leave on the device:

  window cover   the sorted distinct real columns of a slice are covered greedily: base_0 = the smallest column, base_k = the smallest column
                 >= base_{k-1} + span; span = 8 192 with 8 windows, 2 048 with 32.  Unused bases repeat the last one, an empty slice gets base 0.
  uncovered      a slice that needs more than NW windows: first base -1 (the others stay what the cover gave), every code word 0.
  code           k << dbits | (c - base_k), entries 2 q and 2 q + 1 of a row share word q of the slice's region; padding gets code 0.
  verdict        failed = uncovered slices, last = 1 + the index of the last of them; mode 1 when last <= n_slices // 16, else mode 2 when
                 failed <= n_slices // 8, else mode 0.  Mode 0 with 8 windows: the verdict is that of the pass with 32; mode 0 again: no codes.
  uniform width  every slice is w entries wide, 1 <= w <= 63 (and the operator kept its codes).

What is real: for the operator, entry j of a row when j < the row's stored off-diagonal count (never a value: a stored zero is real); for a
transfer, an entry whose value is != 0."""
import numpy as np

SPAN = {8: 8192, 32: 2048}
DBITS = {8: 13, 32: 11}


def real_of_operator(slice_ptr, row_len):
    """Mask over the stored entries of an operator layout with one lane per row: entry j of device row r is real when j < row_len[r]."""
    slice_ptr = np.asarray(slice_ptr, np.int64)
    real = np.zeros(int(slice_ptr[-1]), bool)
    for s in range(len(slice_ptr) - 1):
        p0, w = int(slice_ptr[s]), int(slice_ptr[s + 1] - slice_ptr[s]) >> 6
        real[p0:p0 + 64 * w] = (np.arange(w)[:, None] < np.asarray(row_len[64 * s:64 * s + 64])[None, :]).ravel()
    return real


def real_of_transfer(val):
    return np.asarray(val) != 0.0


def greedy_cover(cols, span):
    """Bases of the greedy cover of a sorted array of distinct columns with windows [base, base + span)."""
    bases = []
    i = 0
    while i < len(cols):
        bases.append(int(cols[i]))
        i = int(np.searchsorted(cols, cols[i] + span, side="left"))
    return bases


def encode(slice_ptr, col, real, nw):
    """One pass of the coding with nw windows per slice: win_base (n_slices x nw), the code words (indexed like col) with the mask of the words
    the pass writes, failed / last, and the windows every slice NEEDS (which may exceed nw)."""
    slice_ptr = np.asarray(slice_ptr, np.int64); col = np.asarray(col); real = np.asarray(real, bool)
    span, dbits = SPAN[nw], DBITS[nw]
    ns = len(slice_ptr) - 1
    win_base = np.zeros((ns, nw), np.int32)
    words = np.zeros(int(slice_ptr[-1]), np.uint32); written = np.zeros(int(slice_ptr[-1]), bool)
    needed = np.zeros(ns, np.int64)
    failed = last = 0
    for s in range(ns):
        p0, w = int(slice_ptr[s]), int(slice_ptr[s + 1] - slice_ptr[s]) >> 6
        c = col[p0:p0 + 64 * w].reshape(w, 64).astype(np.int64); r = real[p0:p0 + 64 * w].reshape(w, 64)
        bases = greedy_cover(np.unique(c[r]), span)
        needed[s] = len(bases)
        bad = len(bases) > nw
        kept = bases[:nw]
        if kept:
            win_base[s, :len(kept)] = kept
            win_base[s, len(kept):] = kept[-1]
        code = np.zeros((w, 64), np.uint32)
        if bad:
            failed += 1; last = s + 1
            win_base[s, 0] = -1
        elif kept:
            k = np.searchsorted(np.asarray(kept), c, side="right") - 1
            k = np.where(r, k, 0)
            off = np.where(r, c - np.asarray(kept)[k], 0)
            assert np.all((off >= 0) & (off < span))
            code = np.where(r, (k << dbits) | off, 0).astype(np.uint32)
        nq = (w + 1) // 2
        if w & 1:
            code = np.vstack([code, np.zeros((1, 64), np.uint32)])
        words[p0:p0 + 64 * nq] = (code[0::2] | (code[1::2] << np.uint32(16))).ravel()
        written[p0:p0 + 64 * nq] = True
    return {"win_base": win_base, "words": words, "written": written, "failed": failed, "last": last, "needed": needed}


def mode_of(failed, last, n_slices):
    return 1 if last <= n_slices // 16 else (2 if failed <= n_slices // 8 else 0)


def uniform_width_of(slice_ptr):
    w = np.diff(np.asarray(slice_ptr, np.int64)) >> 6
    return int(w[0]) if len(w) and np.all(w == w[0]) and 1 <= w[0] <= 63 else 0


def model(slice_ptr, col, real, uniform_slices=True):
    """The whole set-up of one operator: the pass with 8 windows, the recode with 32 where that gives mode 0, the verdict.  Returns windows
    (0 / 8 / 32), mode, from (= last; the kernels use it in mode 1), failed, last, uniform_width, win_base / words / written (None without
    codes), used (windows every slice uses: 0 for an uncovered slice), needed (windows it needs in the final format), recoded."""
    ns = len(slice_ptr) - 1
    first = encode(slice_ptr, col, real, 8)
    out, nw, recoded = first, 8, False
    if mode_of(first["failed"], first["last"], ns) == 0:
        out, nw, recoded = encode(slice_ptr, col, real, 32), 32, True
    mode = mode_of(out["failed"], out["last"], ns)
    res = {"failed": out["failed"], "last": out["last"], "mode": mode, "recoded": recoded, "needed": out["needed"], "needed8": first["needed"]}
    if mode == 0:
        res.update(windows=0, uniform_width=0, win_base=None, words=None, written=None, used=np.zeros(ns, np.int64))
        res["from"] = 0
    else:
        res.update(windows=nw, uniform_width=uniform_width_of(slice_ptr) if uniform_slices else 0, win_base=out["win_base"], words=out["words"],
                   written=out["written"], used=np.where(out["needed"] > nw, 0, out["needed"]))
        res["from"] = out["last"]
    return res


def decode(slice_ptr, words, win_base, nw):
    """The columns the kernels read from the codes (kernels.hip.hpp::row_dot_group16), indexed like col: base[u >> dbits] + (u & mask) for every
    stored entry, padding included (code 0 = the slice's first base).  Slices with first base -1 give -1 everywhere."""
    slice_ptr = np.asarray(slice_ptr, np.int64)
    dbits = DBITS[nw]
    out = np.full(int(slice_ptr[-1]), -1, np.int64)
    for s in range(len(slice_ptr) - 1):
        p0, w = int(slice_ptr[s]), int(slice_ptr[s + 1] - slice_ptr[s]) >> 6
        if w == 0 or win_base[s, 0] < 0:
            continue
        nq = (w + 1) // 2
        wd = words[p0:p0 + 64 * nq].reshape(nq, 64)
        u = np.empty((2 * nq, 64), np.int64)
        u[0::2] = wd & 0xffff; u[1::2] = wd >> 16
        u = u[:w]
        out[p0:p0 + 64 * w] = (win_base[s].astype(np.int64)[u >> dbits] + (u & ((1 << dbits) - 1))).ravel()
    return out


def sell_from_rows(ptr, cols, vals, lpr=1):
    """SELL-64 layout of a CSR over device rows (len(ptr) - 1 a multiple of 64 // lpr) with lpr lanes per row: 64 // lpr rows per slice, entry e of
    a row in lane lpr (row % (64 // lpr)) + e % lpr at j = e // lpr, slice width = the longest row's ceil(len / lpr).  Padding: column 0, value 0.
    Returns slice_ptr, col, val and real (the entries that came from the CSR)."""
    ptr = np.asarray(ptr, np.int64)
    rps = 64 // lpr
    n_rows = len(ptr) - 1
    assert n_rows % rps == 0
    ns = n_rows // rps
    length = np.diff(ptr)
    width = (-(-length // lpr)).reshape(ns, rps).max(axis=1) if ns else np.zeros(0, np.int64)
    slice_ptr = np.concatenate([[0], np.cumsum(64 * width)]).astype(np.int64)
    col = np.zeros(int(slice_ptr[-1]), np.int32); val = np.zeros(int(slice_ptr[-1])); real = np.zeros(int(slice_ptr[-1]), bool)
    row = np.repeat(np.arange(n_rows), length)
    e = np.arange(len(row)) - ptr[row]
    pos = slice_ptr[row // rps] + 64 * (e // lpr) + lpr * (row % rps) + e % lpr
    col[pos] = np.asarray(cols)[: len(row)]; val[pos] = np.asarray(vals)[: len(row)]; real[pos] = True
    return slice_ptr, col, val, real
