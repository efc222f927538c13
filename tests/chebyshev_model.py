"""CPU model of the V-cycle with the Chebyshev smoother (GMG_SMOOTHER_CHEBYSHEV), assembled from the oracle's operators (test infrastructure).

A sibling of tests/vcycle_model.VcycleModel: the cycle (level order, zero coarse guess, residual / restriction / prolongation / coarsest solve)
is inherited; the smoother is written out here in numpy with the oracle's residual.  Per level k, with A = the oracle's level operator:

  Lambda = max_i sum_j |a_ij| / |a_ii|            (Gershgorin bound of D^-1 A, diagonal term included)
  lambda_max = Lambda, lambda_min = Lambda / ratio, theta = (lambda_max + lambda_min) / 2, delta = (lambda_max - lambda_min) / 2, sigma = theta / delta
  step 0:      p = (1 / theta) D^-1 (b - A x),  x += p,  rho_0 = 1 / sigma
  step k >= 1: rho_k = 1 / (2 sigma - rho_{k-1}),  p = rho_k rho_{k-1} p + (2 rho_k / delta) D^-1 (b - A x),  x += p

Every call of smooth() starts a new polynomial at step 0.  No ordering of the device enters; `ratio` is an argument (tests read the engine's
"cheby_ratio").  eng may be None."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from tests.vcycle_model import VcycleModel


def gershgorin_bound(A):
    """max_i sum_j |a_ij| / |a_ii| of a sparse matrix with a non-zero diagonal."""
    A = sp.csr_matrix(A)
    return float((np.asarray(abs(A).sum(axis=1)).ravel() / np.abs(A.diagonal())).max())


def cheby_coefficients(lam, ratio, steps):
    """[(c1, c2)] of steps 0 .. steps - 1: p <- c1 p + c2 D^-1 r (c1 = 0 at step 0)."""
    lmax, lmin = lam, lam / ratio
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma = theta / delta
    out, rho = [], 1.0 / sigma
    for k in range(steps):
        if k == 0:
            out.append((0.0, 1.0 / theta))
        else:
            rho_new = 1.0 / (2.0 * sigma - rho)
            out.append((rho_new * rho, 2.0 * rho_new / delta))
            rho = rho_new
    return out


class ChebyshevModel(VcycleModel):
    def __init__(self, eng, U, mass, lhs, oracle, ratio, pre=2, post=2):
        # (the Jacobi form of the parent: no ordering of a device is asked for; its smoother table is replaced below)
        super().__init__(eng, U, mass, lhs, oracle, 1.0, pre=pre, post=post, smoother="jacobi")
        self.ratio = float(ratio)
        self.lam = [gershgorin_bound(self.A[k]) for k in range(self.L)]
        self.diag = [self.A[k].diagonal() for k in range(self.L)]
        self.sm = [("chebyshev", self.lam[k], self.diag[k]) for k in range(self.L)]

    def smooth(self, k, b, x, iters, omega=None):
        x = np.array(x, dtype=np.float64, copy=True)
        dg = self.diag[k][:, None] if x.ndim == 2 else self.diag[k]
        p = None
        for c1, c2 in cheby_coefficients(self.lam[k], self.ratio, iters):
            z = self.oracle.residual(self.A[k], b, x) / dg
            p = c2 * z if p is None else c1 * p + c2 * z
            x = x + p
        return x
