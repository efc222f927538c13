"""numpy restatement of what gmg_config::nullspace = 1 adds to a solve -- test infrastructure, shared by the host tests of the
model and the device comparisons.

The system is symmetric positive SEMI-definite with the null space span{1} (a stiffness matrix, a Bilaplacian without a mass term).  Nothing of
the cycle changes; three things around it do:

  * the coarsest solve applies the pseudo-inverse of the coarsest Galerkin operator (numpy.linalg.pinv here; the engine: the LDL^T with its
    last pivot pinned, G = [[A11^-1, 0], [0, 0]], and P G P with P = I - 1 1^T / n_L) -- `with_pinv_coarse` puts it into one of the existing
    model classes (tests/vcycle_model.py, tests/chebyshev_model.py);
  * after the load b <- b - (1^T b / n) 1, the orthogonal projection onto range(A): the loops and their residual checks see the projected b;
  * before the fetch x <- x - (m^T x / m^T 1) 1 with m the mass (unit weights without one).

The loops are the existing ones (tests/accelerate_model.py::plain_loop / accelerated_loop, tests/pcg_model.py::pcg_loop)."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from tests.accelerate_model import accelerated_loop, plain_loop
from tests.pcg_model import pcg_loop

ROWSUM_MAX = 1e-9          # host_ldlt.hpp::kNullspaceRowsumMax


def rowsum_figure(A):
    """max_i |sum_j a_ij| / sum_j |a_ij| (a row without a nonzero entry counts 0): what the set-up checks on level 0 and on the coarsest level."""
    A = sp.csr_matrix(A)
    s = np.abs(np.asarray(A.sum(axis=1)).ravel())
    m = np.asarray(abs(A).sum(axis=1)).ravel()
    return float(np.max(np.where(m > 0.0, s / np.where(m > 0.0, m, 1.0), 0.0))) if A.shape[0] else 0.0


def pinned_inverse(A, pinned=None):
    """G = [[A11^-1, 0], [0, 0]] with the unknown `pinned` (default: the last) in the role of the pinned one, dense."""
    A = np.asarray(A.todense() if sp.issparse(A) else A, dtype=np.float64)
    n = A.shape[0]
    pinned = n - 1 if pinned is None else pinned
    keep = np.array([i for i in range(n) if i != pinned], dtype=int)
    G = np.zeros((n, n))
    if n > 1:
        G[np.ix_(keep, keep)] = np.linalg.inv(A[np.ix_(keep, keep)])
    return G


def double_centre(G):
    """P G P, P = I - 1 1^T / n: entry (i, j) = G_ij - (s_i + s_j) / n + mu with s the column sums and mu = sum(s) / n^2."""
    n = G.shape[0]
    s = G.sum(axis=0)
    return G - (s[:, None] + s[None, :]) / n + s.sum() / (n * n)


class _PinvCoarse:
    def __init__(self, A):
        self.pinv = np.linalg.pinv(np.asarray(A.todense()), hermitian=True)

    def coarse_solve(self, rc):
        return self.pinv @ np.asarray(rc, dtype=np.float64)


def with_pinv_coarse(model):
    """The model with e = A_L^+ rc as its coarsest solve (its Galerkin operators were taken from the oracle at construction: they stay)."""
    model.O = _PinvCoarse(model.A[model.L])
    return model


def project_rhs(rhs):
    rhs = np.asarray(rhs, dtype=np.float64)
    rhs = rhs[:, None] if rhs.ndim == 1 else rhs
    return rhs - rhs.mean(axis=0)


def rhs_defect(rhs):
    """max over the columns of |1^T b| / (sqrt(n) |b|_2): the timing key nullspace_rhs_defect (a zero column counts 0)."""
    rhs = np.asarray(rhs, dtype=np.float64)
    rhs = rhs[:, None] if rhs.ndim == 1 else rhs
    nb = np.sqrt((rhs * rhs).sum(axis=0))
    return float(np.max(np.where(nb > 0.0, np.abs(rhs.sum(axis=0)) / (np.sqrt(rhs.shape[0]) * np.where(nb > 0.0, nb, 1.0)), 0.0)))


def centre(x, mass=None):
    """x - (m^T x / m^T 1) 1 per column."""
    x = np.asarray(x, dtype=np.float64)
    m = np.ones(x.shape[0]) if mass is None else np.asarray(mass, dtype=np.float64)
    return x - (m @ x) / m.sum()


def nullspace_solve(lhs, mass, cycle, rhs, x0, stop_type, tol, max_iter, loop="plain", depth=0):
    """A solve as the engine runs it on a nullspace = 1 handle: the right-hand side projected, the loop (plain, "accelerate" with `depth`, or "pcg")
    on the projected right-hand side from the caller's x0, the iterates centred.  Returns (x, iterations, residues, centred iterates or None)."""
    b = project_rhs(rhs)
    x0 = np.asarray(x0, dtype=np.float64).reshape(b.shape)
    iterates = None
    if loop == "pcg":
        x, it, res, guards, restarts, _, iterates = pcg_loop(lhs, mass, cycle, b, x0, stop_type, tol, max_iter)
        assert guards == 0, "the model's PCG loop took a guard"
        iterates = [centre(v, mass) for v in iterates]
    elif loop == "accelerate":
        x, it, res = accelerated_loop(lhs, mass, cycle, b, x0, depth, stop_type, tol, max_iter)[:3]
    else:
        x, it, res = plain_loop(lhs, mass, cycle, b, x0, stop_type, tol, max_iter)[:3]
    return centre(np.asarray(x).reshape(b.shape), mass), it, np.asarray(res), iterates


def least_squares_solution(lhs, rhs, mass=None):
    """The dense least-squares solution of lhs x = rhs (minimum norm), centred like the engine's answer."""
    A = np.asarray(sp.csr_matrix(lhs).todense())
    rhs = np.asarray(rhs, dtype=np.float64)
    rhs = rhs[:, None] if rhs.ndim == 1 else rhs
    return centre(np.linalg.lstsq(A, rhs, rcond=None)[0], mass)
