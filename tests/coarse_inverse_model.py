"""Reference, error bound and exact restatements for the device-built coarse inverse (gravo_mg_amd/csrc/setup_kernels.hip.hpp::coarse_inverse_tiles,
mirror_lower_to_upper, permute_symmetric, permute_symmetric_scatter, pack_lower_blocks), for tests/test_coarse_inverse_model_host.py and
tests/test_gpu_coarse_inverse_tiles.py.

Everything starts from the EXPORTED factor (cabi.coarse_inverse(..., export=True)): L from tri / vals / rows, D^-1 = dinv as the kernel reads
them, in the factor's numbering.  The factorisation's own rounding and the condition number of the operator therefore stay out of the bound.

Reference.  X* = L^-T D^-1 L^-1 in numpy.longdouble (64-bit significand on x86-64), and in exact fractions.Fraction for small n.

Criterion.  Column c of the computed lower triangle, x = X[c:, c], is the result of two substitutions on I = {c .. n - 1}: L_I y = e_c (way
down), L_I^T x = D_I^-1 y (way up).  A substitution in ANY order of its additions, fused or not, solves a system with a perturbed matrix
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., chapter 8): (L_I + E1) y = e_c and (L_I + E2)^T x = D_I^-1 (1 + d) y with
|E1| <= gamma_k1 |L_I|, |E2| <= gamma_k2 |L_I|, |d| <= u, where k1 / k2 is the largest number of rounded operations that any one term goes
through.  Eliminating y,

    |L_I D_I L_I^T x - e_c|  <=  gamma_(k1 + k2 + 1) |L_I| |D_I| |L_I|^T |x|        componentwise,

with no condition number in it.  For all columns at once: R = tril(L tril(D L^T X_low)) - I against the same expression in absolute values.

The constant (derived from the schedule; not tuned).  u = 2^-53, gamma_k = k u / (1 - k u).
  way down, a value x[row]:   a chunk's update of a row is sum_{jj < 8} V[jj] y[jj] (8 padded terms added one after the other to 0: a product
      and at most 8 additions), then ONE subtraction x[row] - acc per chunk that lists the row; a row is listed by at most C chunks (C: the
      largest count in `rows`), so a term goes through at most C subtractions; the chunk's own columns then take at most 7 more subtractions
      (the 8 x 8 triangle).                                                                k1 = 1 + 8 + C + 7
  way up, a column of a chunk with r rows below it:   a lane adds its share of the r products one after the other (a product and an addition
      each: ceil(r / S) of them where one wave takes the chunk, ceil(r / (16 S)) where all waves do, r on the host), the S = 64 / W slots
      are added in log2 S steps, the 16 waves' sums one after the other (16 additions), D^-1 y is added (1), the triangle takes 7 more.
                                 k2 = 1 + max(ceil(r_small / S), ceil(r_max / (16 S)) + 16) + log2 S + 1 + 7      at width W
                                 k2 = 1 + r_max + 1 + 7                                                          in the host's order
  the product with D^-1:        1
gamma_terms() returns k1 + k2 + 1 for an export and an order; no case of the catalogue brings it beyond 700 (gamma < 8e-14).
The residual itself is evaluated in longdouble: two nested sums of at most n terms at unit roundoff 2^-64, i.e. n 2^-63 of the same
absolute-value expression, which bound() adds.

Exact restatements (bitwise): mirror(), permute(), pack().  Restatement of the kernel's order of operations in float64: device_order()."""
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
K_CHUNK = 8
K_WAVES = 16
TRI_BLOCK = 64


def dense_factor(E, dtype=np.float64):
    """(L unit lower triangular n x n, dinv) of an export, factor's numbering."""
    n = len(E["perm"])
    L = np.zeros((n, n), dtype)
    L[np.arange(n), np.arange(n)] = 1
    for q in range(len(E["q_col0"])):
        c0, w, r0, r1 = int(E["q_col0"][q]), int(E["q_w"][q]), int(E["q_rptr"][q]), int(E["q_rptr"][q + 1])
        for jj in range(w):
            for ii in range(jj + 1, w):
                L[c0 + ii, c0 + jj] = E["tri"][q, ii, jj]
            L[E["rows"][r0:r1], c0 + jj] = E["vals"][r0:r1, jj]
    return L, np.asarray(E["dinv"], dtype)


def unit_lower_inverse(L):
    """L^-1 by forward substitution in L's own dtype (object arrays of Fractions included)."""
    n = L.shape[0]
    Y = np.zeros_like(L)
    Y[np.arange(n), np.arange(n)] = 1
    for j in range(n):
        nz = np.nonzero(L[j + 1:, j])[0] + j + 1
        if len(nz):
            Y[nz, :j + 1] -= L[nz, j][:, None] * Y[j, :j + 1][None, :]
    return Y


def reference(E):
    """X* = L^-T D^-1 L^-1 in longdouble."""
    L, dinv = dense_factor(E, LD)
    Li = unit_lower_inverse(L)
    return Li.T @ (dinv[:, None] * Li)


def reference_exact(E):
    """X* in exact rational arithmetic (object array of Fractions): for n <= 65."""
    L, dinv = dense_factor(E)
    n = L.shape[0]
    Lf = np.array([[Fraction(float(v)) for v in row] for row in L], dtype=object).reshape(n, n)
    df = np.array([Fraction(float(v)) for v in dinv], dtype=object)
    Li = unit_lower_inverse(Lf)
    X = np.empty((n, n), dtype=object)
    for j in range(n):
        for c in range(j + 1):
            X[j, c] = X[c, j] = sum((Li[i, j] * df[i] * Li[i, c] for i in range(j, n)), Fraction(0))
    return X


def gamma_terms(E, info, width=None):
    """k1 + k2 + 1 of the module docstring; width None: the host's order (emulate_device_column)."""
    C = int(np.bincount(E["rows"]).max()) if len(E["rows"]) else 0
    k1 = 1 + 8 + C + 7
    r_max, r_small, big = info["max_rows"], info["max_small_rows"], info["big_rows"]
    if width is None:
        k2 = 1 + r_max + 1 + 7
    else:
        S = 64 // width
        log2s = {1: 0, 2: 1, 4: 2}[S]
        lane = -(-r_small // S)
        if r_max >= big:
            lane = max(lane, -(-r_max // (K_WAVES * S)) + K_WAVES)
        k2 = 1 + lane + log2s + 1 + 7
    return k1 + k2 + 1


def gamma(k):
    return k * U / (1.0 - k * U)


class Bound:
    """The residual criterion of one export; the longdouble pieces are computed once and shared."""

    def __init__(self, E, info):
        self.E, self.info = E, info
        self.L, self.dinv = dense_factor(E, LD)
        self.D = LD(1) / self.dinv
        self.n = self.L.shape[0]
        self.aL = np.abs(self.L)

    def residual(self, X):
        """(|R|, B): R = tril(L tril(D L^T X_low)) - I in longdouble and an upper bound B of tril(|L| tril(|D| |L|^T |X_low|)): that sum of
        non-negative terms evaluated in float64, divided by 1 - gamma_(2 n + 2) (every term is rounded at most 2 n + 2 times)."""
        Xl = np.tril(np.asarray(X, LD))
        Z = np.tril(self.D[:, None] * (self.L.T @ Xl))
        R = np.tril(self.L @ Z) - np.eye(self.n, dtype=LD)
        aL, aD = self.aL.astype(np.float64), np.abs(self.D).astype(np.float64) * (1.0 + 2.0 * U)
        B = np.tril(aL @ np.tril(aD[:, None] * (aL.T @ np.abs(np.tril(np.asarray(X, np.float64))))))
        return np.abs(R), (B / (1.0 - gamma(2 * self.n + 2))).astype(LD)

    def ratio(self, X, width=None):
        """max over the entries of |R| / ((gamma + n 2^-63) B): at most 1 for a correct result.  An entry with B = 0 must have R = 0."""
        R, B = self.residual(X)
        g = LD(gamma(gamma_terms(self.E, self.info, width))) + LD(self.n) * LD(2.0) ** -63
        lim = g * B
        if np.any(R[lim == 0] != 0):
            return np.inf
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(lim > 0, R / np.where(lim > 0, lim, 1), 0)
        return float(q.max())

    def column_ratios(self, X, width=None):
        R, B = self.residual(X)
        g = LD(gamma(gamma_terms(self.E, self.info, width))) + LD(self.n) * LD(2.0) ** -63
        lim = g * B
        bad = (lim == 0) & (R != 0)
        q = np.where(lim > 0, R / np.where(lim > 0, lim, 1), 0)
        q = np.where(bad, np.inf, q)
        return q.max(axis=0).astype(np.float64)


# ---- exact restatements -------------------------------------------------------------------------------------------------------------------------

def mirror(X):
    """mirror_lower_to_upper: X[j][c] = X[c][j] for j < c."""
    return np.tril(X) + np.tril(X, -1).T


def permute(X, perm):
    """permute_symmetric / permute_symmetric_scatter: out[perm[j]][perm[c]] = X[j][c]."""
    out = np.empty_like(X)
    out[np.ix_(perm, perm)] = X
    return out


def tri_block_offset(bi, bj):
    return bi * (bi + 1) // 2 + bj


def pack(X):
    """pack_lower_blocks on the lower triangle of X: 64 x 64 blocks (bi >= bj) in the order of coarse_triangle.hpp, zero padded; a diagonal
    block takes entry (j, c) from X[max(j, c)][min(j, c)].  Flat array."""
    n = X.shape[0]
    nb = -(-n // TRI_BLOCK)
    P = np.zeros((nb * TRI_BLOCK, nb * TRI_BLOCK))
    P[:n, :n] = mirror(X)
    out = np.zeros(nb * (nb + 1) // 2 * TRI_BLOCK * TRI_BLOCK)
    for bi in range(nb):
        for bj in range(bi + 1):
            o = tri_block_offset(bi, bj) * TRI_BLOCK * TRI_BLOCK
            out[o:o + TRI_BLOCK * TRI_BLOCK] = P[bi * 64:bi * 64 + 64, bj * 64:bj * 64 + 64].ravel()
    return out


def before_mirror(X, width):
    """What the tiles leave behind: of column c the rows from the first column of c's tile on; zeros above."""
    n = X.shape[0]
    j, c = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.where(j >= (c // width) * width, X, 0.0)


# ---- the kernel's order of operations, in float64 ------------------------------------------------------------------------------------------------

def device_order(E, info, width=None, dtype=np.float64, drop_wave=None, stale_own=False, reverse=False):
    """All columns of the inverse at once by the kernel's schedule on the exported layout, one numpy row operation per kernel step: way down in
    push form chunk by chunk, way up in pull form level by level with the rows of a chunk dealt to 16 S lanes (big chunks) or S lanes (the
    others), the lanes' sums added slots first, then waves.  width None: one lane adds all rows (the host's order).  Unfused float64: not the
    device's bits, but its summation order.  Returns the full matrix (the way up computes both triangles when no tile is skipped).
    Seeded defects: drop_wave = w leaves wave w's partial sum out of the big path; stale_own leaves the way down's own-column values
    y[jj], jj >= 1, unstored.  reverse: every lane adds its rows last to first (a second summation order for the exactness proof)."""
    n = len(E["perm"])
    X = np.zeros((n, n), dtype)
    X[np.arange(n), np.arange(n)] = 1
    vals, tri, rows = E["vals"].astype(dtype), E["tri"].astype(dtype), E["rows"]
    dinv = E["dinv"].astype(dtype)
    nq = len(E["q_col0"])
    zero = np.zeros(n, dtype)
    for q in range(nq):
        c0, w, r0, r1 = int(E["q_col0"][q]), int(E["q_w"][q]), int(E["q_rptr"][q]), int(E["q_rptr"][q + 1])
        y = [X[c0 + jj].copy() if jj < w else zero.copy() for jj in range(K_CHUNK)]
        for jj in range(K_CHUNK):
            for ii in range(jj + 1, K_CHUNK):
                y[ii] = y[ii] - tri[q, ii, jj] * y[jj]
        if not stale_own:
            for jj in range(1, w):
                X[c0 + jj] = y[jj]
        if r1 > r0:
            acc = np.zeros((r1 - r0, n), dtype)
            for jj in range(K_CHUNK):
                acc = acc + vals[r0:r1, jj][:, None] * y[jj][None, :]
            X[rows[r0:r1]] = X[rows[r0:r1]] - acc
    S = 1 if width is None else 64 // width
    big_rows = info["big_rows"]

    def lanes_sum(r0, r1, G):
        """per lane g < G: - sum of V[i] x[rows[i]] over i = r0 + g, r0 + g + G, ... one after the other; shape (G, 8, n)"""
        r = r1 - r0
        trips = -(-r // G) if r else 0
        acc = np.zeros((G, K_CHUNK, n), dtype)
        V = np.zeros((trips * G, K_CHUNK), dtype); V[:r] = vals[r0:r1]
        Xi = np.zeros((trips * G, n), dtype); Xi[:r] = X[rows[r0:r1]]
        order = range(trips - 1, -1, -1) if reverse else range(trips)
        for t in order:
            acc = acc - V[t * G:(t + 1) * G, :, None] * Xi[t * G:(t + 1) * G, None, :]
        return acc

    def slots_sum(a):            # a: (S, ...) -> the total every slot holds
        if S == 1:
            return a[0]
        if S == 2:
            return a[0] + a[1]
        return (a[0] + a[1]) + (a[2] + a[3])

    for v in range(len(E["lev_ptr"]) - 1):
        new = {}
        for k in range(int(E["lev_ptr"][v]), int(E["lev_ptr"][v + 1])):
            q = int(E["lev_q"][k])
            c0, w, r0, r1 = int(E["q_col0"][q]), int(E["q_w"][q]), int(E["q_rptr"][q]), int(E["q_rptr"][q + 1])
            yv = [X[c0 + jj] * dinv[c0 + jj] if jj < w else zero.copy() for jj in range(K_CHUNK)]
            if width is None:
                acc = lanes_sum(r0, r1, 1)[0]
            elif r1 - r0 >= big_rows:
                part = lanes_sum(r0, r1, K_WAVES * S).reshape(K_WAVES, S, K_CHUNK, n)
                acc = np.zeros((K_CHUNK, n), dtype)
                for wv in range(K_WAVES):
                    if wv != drop_wave:
                        acc = acc + slots_sum(part[wv])
            else:
                acc = slots_sum(lanes_sum(r0, r1, S))
            a = [acc[jj] + yv[jj] for jj in range(K_CHUNK)]
            for jj in range(K_CHUNK - 2, -1, -1):
                for ii in range(jj + 1, K_CHUNK):
                    a[jj] = a[jj] - tri[q, ii, jj] * a[ii]
            for jj in range(w):
                new[c0 + jj] = a[jj]
        for j, val in new.items():      # (the chunks of a level do not read each other)
            X[j] = val
    return X
