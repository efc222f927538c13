"""Plain model of the fp32 inner cycle's operators, one operator at a time (numpy and scipy only; test infrastructure).

The device holds every level operator and every prolongation rounded to float32 (refresh_fp32_twins) and computes on float32 vectors.  The
model works in float64 on those same operands -- A32_k = float64(float32(A_k)), the same rounding of U_k -- in the order the device reports
(level_ordering, level_blocks), and returns next to each value a componentwise bound on what a float32 evaluation may differ by.  Nothing in
a bound is fitted: u = 2^-24, gamma_k = k u / (1 - k u).

Products (residual, spmv, restrict, prolong-add): |fl(y_i) - y_i| <= gamma_{m_i + 2} (sum_j |a_ij| |x_j| + |b_i|), m_i = stored entries of
row i (the diagonal among them) + 1 for the added vector.  Holds for every summation order, with or without fused multiply-adds; padding
lanes add exact zeros.

Sweeps: x_i <- x_i + omega ((b_i - sum_{j != i} a_ij x_j) / a_ii - x_i), colour by colour on a colour-major level (later colours read the
updated values), on a blocked level colour by colour inside every block (in-block columns of an earlier colour read the updated value,
everything else the sweep's input), all rows at once from the input for weighted Jacobi.  Beside the values runs the error bound
    E_i <- |1 - omega| E_i + omega (sum_{j != i} |a_ij| E_j / |a_ii| + delta_i),
    delta_i = gamma_{m_i + 6} (|b_i| + sum_{j != i} |a_ij| |x_j|) / |a_ii| + u X_i
through the same order (E_j of an updated column is the updated one).  The + 6 covers the subtraction, the division (or reciprocal and
product) and the roundings of the relaxation.  X_i is what the last roundings act on: |x_i^new| for omega = 1 (the kernel then reads no x_i);
with relaxation the old x_i enters twice (x^GS - x_i and its product with omega) and the new one once, X_i = 2 |x_i^old| + |x_i^new| / omega,
so that omega u X_i is the first-order sum of the three.

Exactness: where every operand is a multiple of 2^-q and (|b_i| + sum_j |a_ij| |x_j|) 2^q < 2^24 in every row -- and, for a sweep, every
diagonal entry is a power of two and omega = 1 -- each partial sum in any order is a float32 number, so a float32 evaluation gives the
float64 model's bits.  `exact` is True only where the model has verified that condition for the stage at hand."""
from __future__ import annotations

import collections

import numpy as np
import scipy.sparse as sp

U32, U64 = 2.0 ** -24, 2.0 ** -53

Result = collections.namedtuple("Result", "value bound exact")
Swept = collections.namedtuple("Swept", "value bound exact x_old e_old delta")


def gamma(k, u=U32):
    k = np.asarray(k, np.float64)
    return k * u / (1.0 - k * u)


def f32(a):
    """float64 of the float32 rounding of a."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def f32_matrix(M):
    M = sp.csr_matrix(M, dtype=np.float64, copy=True)
    M.sort_indices()
    M.data = f32(M.data)
    return M


def grid_exponent(*arrays):
    """Smallest q >= 0 such that every entry of every array is a multiple of 2^-q (from the lowest set bit of each float64)."""
    q = 0
    for a in arrays:
        if a is None:
            continue
        a = np.asarray(a, np.float64).ravel()
        a = a[a != 0]
        if a.size == 0:
            continue
        m, e = np.frexp(a)
        mi = (np.abs(m) * 2.0 ** 53).astype(np.int64)
        low = e.astype(np.int64) - 53 + np.log2((mi & -mi).astype(np.float64)).astype(np.int64)
        q = max(q, int(-low.min()))
    return q


def elem_exponent(a):
    """Per entry: the smallest q >= 0 with a 2^q an integer (0 for a zero)."""
    a = np.asarray(a, np.float64)
    m, e = np.frexp(a)
    mi = (np.abs(m) * 2.0 ** 53).astype(np.int64)
    low = e.astype(np.int64) - 53 + np.log2(np.maximum(mi & -mi, 1).astype(np.float64)).astype(np.int64)
    return np.where(a == 0, 0, np.maximum(-low, 0))


def _row_max(M, v):
    """max over the stored entries j of row i of v[j] (n x d), 0 for an empty row."""
    out = np.zeros((M.shape[0], v.shape[1]), v.dtype)
    cnt = np.diff(M.indptr)
    rows = np.flatnonzero(cnt > 0)
    if len(rows):
        out[rows] = np.maximum.reduceat(v[M.indices], M.indptr[:-1][rows], axis=0)
    return out


def _fits_f32(scale, q):
    """(scale * 2^q).max() < 2^24 for a grid of spacing 2^-q that float64 still resolves."""
    return q <= 100 and (scale.size == 0 or float(scale.max()) * 2.0 ** q < 2.0 ** 24)


def _2d(a):
    a = np.asarray(a, np.float64)
    assert a.ndim == 2, "the model takes n x d blocks"
    return a


def product(M, x, add=None, sign=1.0):
    """add + sign M x in float64, the bound gamma_{m_i + 2} (|M| |x| + |add|)_i and whether float32 computes it exactly."""
    M = sp.csr_matrix(M)
    x = _2d(x)
    value = sign * (M @ x)
    scale = abs(M) @ np.abs(x)
    if add is not None:
        add = _2d(add)
        value = add + value
        scale = scale + np.abs(add)
    m = np.diff(M.indptr).astype(np.float64) + 1.0
    q = max(grid_exponent(M.data) + grid_exponent(x), grid_exponent(add))
    return Result(value, gamma(m + 2.0)[:, None] * scale, _fits_f32(scale, q))


def layout_from_plan(new2old, color_begin=None, blocks=None):
    """The update order of a level from what the engine (level_ordering, level_blocks) or the host planner reports:
    ("colour", [rows of colour 0, rows of colour 1, ...]) or ("block", natural row per real device position, its block, its in-block colour)."""
    new2old = np.asarray(new2old)
    if blocks is None:
        rows = [new2old[color_begin[c]:color_begin[c + 1]] for c in range(len(color_begin) - 1)]
        return ("colour", [r[r >= 0] for r in rows])
    blk_begin, row_color = blocks
    real = new2old >= 0
    blk = np.repeat(np.arange(len(blk_begin) - 1), np.diff(blk_begin))[real]
    return ("block", new2old[real], blk, np.asarray(row_color)[real].astype(np.int64))


class _LevelSweep:
    """One level's smoother as a list of row groups updated one after the other: `new` holds the couplings that read values updated earlier
    in the same sweep, `old` those that read the sweep's input."""

    def __init__(self, A, layout, omega):
        A = sp.csr_matrix(A)
        n = A.shape[0]
        self.omega = float(omega)
        self.diag = A.diagonal()
        assert np.all(self.diag != 0)
        coo = A.tocoo()
        offd = coo.row != coo.col
        r, c, v = coo.row[offd], coo.col[offd], coo.data[offd]
        self.off = sp.csr_matrix((v, (r, c)), shape=A.shape)
        self.m = np.diff(A.indptr).astype(np.float64) + 1.0
        if layout[0] == "jacobi":
            reads_new = np.zeros(len(r), bool)
            groups = [np.arange(n)]
        elif layout[0] == "colour":
            groups = [g for g in layout[1] if len(g)]
            colour = np.full(n, -1, np.int64)
            for ci, g in enumerate(groups):
                colour[g] = ci
            assert np.all(colour >= 0) and np.all(colour[r] != colour[c]), "not a proper colouring"
            reads_new = colour[c] < colour[r]
        else:
            _, order, blk, colour_p = layout
            assert len(order) == n
            blk_of, colour = np.empty(n, np.int64), np.empty(n, np.int64)
            blk_of[order], colour[order] = blk, colour_p
            same = blk_of[r] == blk_of[c]
            assert np.all(colour[r[same]] != colour[c[same]]), "not a proper colouring inside a block"
            reads_new = same & (colour[c] < colour[r])
            groups = [np.flatnonzero(colour == ci) for ci in range(int(colour.max()) + 1 if n else 0)]
            groups = [g for g in groups if len(g)]
        self.reads_new = reads_new
        self.entries = (r, c, v)
        self.groups = groups
        self._split()

    def _split(self):
        r, c, v = self.entries
        n = len(self.diag)
        new = sp.csr_matrix((v[self.reads_new], (r[self.reads_new], c[self.reads_new])), shape=(n, n))
        old = sp.csr_matrix((v[~self.reads_new], (r[~self.reads_new], c[~self.reads_new])), shape=(n, n))
        self.parts = [(g, new[g], old[g], abs(new[g]), abs(old[g])) for g in self.groups]

    def sweep(self, b, x_old, e_old):
        """One sweep: (x, E, delta, exact).  exact: in every row the operands read are multiples of 2^-q_i and (|b_i| + sum |a_ij| |x_j|) 2^q_i
        < 2^24, the diagonal is a power of two and omega = 1 -- every partial sum and the quotient are float32 numbers."""
        om, d = self.omega, self.diag
        x, e = x_old.copy(), e_old.copy()
        delta = np.zeros_like(x)
        exact = om == 1.0 and bool(np.all(np.frexp(np.abs(d))[0] == 0.5))
        q_a, q_old, q_b = grid_exponent(self.off.data), elem_exponent(x_old), elem_exponent(b)
        for g, new, old, anew, aold in self.parts:
            dg = d[g][:, None]
            scale = np.abs(b[g]) + anew @ np.abs(x) + aold @ np.abs(x_old)
            if exact:
                q = np.maximum(q_b[g], q_a + np.maximum(_row_max(new, elem_exponent(x)), _row_max(old, q_old)))
                exact = bool(np.all(q <= 100)) and bool(np.all(scale * 2.0 ** np.minimum(q, 100) < 2.0 ** 24))
            gs = (b[g] - (new @ x + old @ x_old)) / dg
            xn = gs if om == 1.0 else x_old[g] + om * (gs - x_old[g])
            last = np.abs(xn) if om == 1.0 else 2.0 * np.abs(x_old[g]) + np.abs(xn) / om
            dl = gamma(self.m[g] + 6.0)[:, None] * scale / np.abs(dg) + U32 * last
            e[g] = abs(1.0 - om) * e_old[g] + om * ((anew @ e + aold @ e_old) / np.abs(dg) + dl)
            x[g] = xn
            delta[g] = dl
        return x, e, delta, exact


class MixedModel:
    """A: the fp64 level operators 0 .. L (rounded to float32 here); U: the prolongations; layouts: one layout_from_plan per smoothed level;
    omega: gmg_config::gs_omega (level 0's colour-major sweep only); smoother "gs" or "jacobi" (then jacobi_omega on every level)."""

    def __init__(self, A, U, layouts, omega=1.0, smoother="gs", jacobi_omega=0.67):
        assert smoother in ("gs", "jacobi")
        self.L = len(U)
        self.A64 = [sp.csr_matrix(a, dtype=np.float64) for a in A]
        self.A = [f32_matrix(a) for a in A]
        self.U = [f32_matrix(u) for u in U]
        self.UT = [sp.csr_matrix(u.T) for u in self.U]
        self.layouts = list(layouts)
        self.sweeps = []
        for k in range(self.L):
            if smoother == "jacobi":
                self.sweeps.append(_LevelSweep(self.A[k], ("jacobi",), jacobi_omega))
            else:
                self.sweeps.append(_LevelSweep(self.A[k], layouts[k], omega if (k == 0 and layouts[k][0] == "colour") else 1.0))

    @classmethod
    def from_engine(cls, eng, U, smoother="gs", jacobi_omega=0.67):
        L = len(U)
        A = [eng.level_operator(k) for k in range(L + 1)]
        layouts = []
        for k in range(L):
            n2o, cb = eng.level_ordering(k)
            layouts.append(layout_from_plan(n2o, cb, eng.level_blocks(k)))
        return cls(A, U, layouts, eng.gs_omega, smoother, jacobi_omega)

    # -- products
    def spmv(self, k, x):
        return product(self.A[k], x)

    def residual(self, k, b, x):
        return product(self.A[k], x, add=b, sign=-1.0)

    def restrict(self, k, r):
        return product(self.UT[k], r)

    def prolong_add(self, k, e, x):
        return product(self.U[k], e, add=x)

    # -- sweeps
    def smooth(self, k, b, x, iters, from_zero=False):
        b = _2d(b)
        x = np.zeros_like(b) if from_zero else _2d(x).copy()
        e = np.zeros_like(x)
        sw = self.sweeps[k]
        exact, x_old, e_old, delta = True, x, e, np.zeros_like(x)
        for _ in range(iters):
            x_old, e_old = x, e
            x, e, delta, ok = sw.sweep(b, x_old, e_old)
            exact = exact and ok
        return Swept(x, e, exact, x_old, e_old, delta)

    def residual_behind(self, k, b, x_dev, swept, from_sweep):
        """b - A x_dev for the iterate the device returned, as the way down forms it behind its sweeps.  from_sweep (the timing key
        residual_from_sweep): the residual is the sweep's explicit part applied to x_old - x_new, which equals b - A x_new up to a_ii times
        the rounding of the last update of row i (<= |a_ii| omega delta_i) and is itself summed in float32 over |a_ij| (|x_old_j| + |x_new_j|)."""
        res = self.residual(k, b, x_dev)
        if not from_sweep:
            return res
        sw = self.sweeps[k]
        extra = np.abs(sw.diag)[:, None] * sw.omega * swept.delta + gamma(sw.m + 2.0)[:, None] * (abs(sw.off) @ (np.abs(swept.x_old) + swept.e_old + np.abs(x_dev)))
        return Result(res.value, res.bound + extra, res.exact and swept.exact)

    # -- the fp64 steps around the inner cycle
    def defect(self, b, x):
        """b - A x of the fp64 level 0 (in extended precision) and the bound u |r_i| + gamma64_{m_i + 2} (|A| |x| + |b|)_i on float32 of the
        device's fp64 residual."""
        A = self.A64[0].tocoo()
        b, x = _2d(b), _2d(x)
        r = b.astype(np.longdouble)
        for c in range(b.shape[1]):
            np.subtract.at(r[:, c], A.row, A.data.astype(np.longdouble) * x[A.col, c].astype(np.longdouble))
        m = np.diff(self.A64[0].indptr).astype(np.float64) + 1.0
        scale = abs(self.A64[0]) @ np.abs(x) + np.abs(b)
        return Result(r, U32 * np.abs(r).astype(np.float64) + gamma(m + 2.0, U64)[:, None] * scale, False)

    @staticmethod
    def correct(e32, x):
        return _2d(x) + f32(_2d(e32))


# ---- a float32 evaluation of the same operators, entry by entry (host tests: does an honest float32 implementation stay inside the bounds,
# ---- does a defective one leave them) -------------------------------------------------------------------------------------------------

def _padded(M, reverse):
    """Rows of a CSR matrix as (cols, float32 vals) of equal width, in stored order or reversed; padding: column 0, value 0."""
    M = sp.csr_matrix(M)
    cnt = np.diff(M.indptr)
    w = int(cnt.max()) if len(cnt) else 0
    j = np.arange(w)[None, :]
    src = M.indptr[:-1, None] + (cnt[:, None] - 1 - j if reverse else j)
    ok = j < cnt[:, None]
    src = np.where(ok, src, 0)
    cols = np.where(ok, M.indices[src] if M.nnz else 0, 0)
    vals = np.where(ok, M.data[src] if M.nnz else 0.0, 0.0).astype(np.float32)
    return cols, vals


def _dot32(cols, vals, x32, n_rows):
    acc = np.zeros((n_rows, x32.shape[1]), np.float32)
    for j in range(cols.shape[1]):
        acc += vals[:, j, None] * x32[cols[:, j]]
    return acc


def product_f32(M, x, add=None, sign=1.0, reverse=False):
    M = sp.csr_matrix(M)
    cols, vals = _padded(M, reverse)
    acc = _dot32(cols, vals, _2d(x).astype(np.float32), M.shape[0])
    if add is None:
        return (np.float32(sign) * acc).astype(np.float64)
    add = _2d(add).astype(np.float32)
    return (add + acc if sign > 0 else add - acc).astype(np.float64)


def smooth_f32(sw, b, x, iters, reverse=False):
    """`iters` sweeps of a _LevelSweep in float32 arithmetic."""
    b32, x32 = _2d(b).astype(np.float32), _2d(x).astype(np.float32)
    om = np.float32(sw.omega)
    padded = [(_padded(new, reverse), _padded(old, reverse)) for _, new, old, _, _ in sw.parts]
    for _ in range(iters):
        x_old = x32.copy()
        for (g, _, _, _, _), ((cn, vn), (co, vo)) in zip(sw.parts, padded):
            acc = _dot32(cn, vn, x32, len(g)) + _dot32(co, vo, x_old, len(g))
            gs = (b32[g] - acc) / sw.diag[g].astype(np.float32)[:, None]
            x32[g] = gs if sw.omega == 1.0 else x_old[g] + om * (gs - x_old[g])
    return x32.astype(np.float64)


def with_defect(sw, kind, seed=0):
    """A copy of a _LevelSweep with one injected defect: "drop_last" -- the last stored off-diagonal entry of one row is lost; "stale" -- one
    coupling that reads an updated value reads the sweep's input instead; "shift_col" -- one entry's column is off by one.  Returns
    (defective sweep, the row touched), or None where the level has no entry of that kind."""
    import copy
    rng = np.random.default_rng(seed)
    r, c, v = (a.copy() for a in sw.entries)
    reads_new = sw.reads_new.copy()
    n = len(sw.diag)
    if kind == "stale":
        cand = np.flatnonzero(reads_new)
    else:
        cand = np.arange(len(r))
    if len(cand) == 0:
        return None
    i = int(rng.choice(cand))
    row = int(r[i])
    if kind == "drop_last":
        i = int(np.flatnonzero(r == row)[np.argmax(c[r == row])])
        v[i] = 0.0
    elif kind == "stale":
        reads_new[i] = False
    elif kind == "shift_col":
        for step in (1, -1, 2, -2):                 # (a neighbouring column that exists and is not the diagonal)
            if 0 <= c[i] + step < n and c[i] + step != row:
                c[i] += step
                break
    else:
        raise ValueError(kind)
    out = copy.copy(sw)
    out.entries, out.reads_new = (r, c, v), reads_new
    out._split()
    return out, row


def matrix_with_defect(M, kind, seed=0):
    """The same defects on a product's matrix ("stale" has no meaning there)."""
    M = sp.csr_matrix(M, copy=True)
    M.sort_indices()
    rng = np.random.default_rng(seed)
    rows = np.flatnonzero(np.diff(M.indptr) > 0)
    row = int(rng.choice(rows))
    last = M.indptr[row + 1] - 1
    if kind == "drop_last":
        M.data[last] = 0.0
    elif kind == "shift_col":
        M.indices[last] = (M.indices[last] + 1) % M.shape[1]
    else:
        raise ValueError(kind)
    return M, row
