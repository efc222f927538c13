"""numpy restatement of the preconditioned CG solve loop (gmg_config::pcg: conjugate gradients with the V-cycle as the preconditioner;
engine.hip::solve_common, pcg_kernels.hip.hpp, pcg_scalars.hpp) -- test infrastructure, shared by the host tests of the model and the device
comparisons.

The cycle is an argument, as in tests/accelerate_model.py: `cycle(b, x)` returns the cycle's iterate from x for the right-hand side b (n x d in,
n x d out); the loop calls it as cycle(r, 0).  The device tests hand in `vcycle` of a second handle created with pcg = 0, the host tests
tests/chebyshev_model.ChebyshevModel built from the oracle's operators.  A x is scipy's, everything fp64: the model differs from the device only
in the order of its sums.

Per iteration, per column (<u, v> = sum_i u_i v_i; w: the stop type's weights):

  z = cycle(r, 0),  rho = <r, z>
  beta = rho / rho_prev -- 0 in a FRESH recurrence (the first iteration, the iteration after a guarded one, the iteration after a confirmation
  recomputed r) and where rho_prev is zero or not finite or rho is not finite
  p = z + beta p (beta = 0: p = z, the old p is not read),  q = A p
  guarded (<p, q> not positive or not finite, rho not finite, or -- from the second iteration on -- sum w r^2 <= 1e-25 sum w b^2 as the last
  update or confirmation reported it): alpha = 0, x and r stay.  Otherwise alpha = rho / <p, q>,  x += alpha p,  r -= alpha q.
  A residue that would end the loop is confirmed by b - A x; the loop goes on from that residual, fresh, where it does not hold."""
from __future__ import annotations

import numpy as np

from tests.accelerate_model import FLOOR_GUARD_REL2, norm, usable, weights


def pcg_loop(lhs, mass, cycle, rhs, x0, stop_type, tol, max_iter):
    """Returns (x, iterations, residues, guarded steps, restarts, steps, iterates).  steps[k] holds the scalars of iteration k + 1: "rho", "beta",
    "pq", "alpha" (d each), "guarded", "fresh" (d, bool), "confirmed" and "residue"; iterates[k] is x after iteration k + 1.  guarded steps and
    restarts count (iteration, column) pairs as the timing keys pcg_guard_steps and pcg_restarts do (restarts: fresh ones after the first iteration)."""
    A = lhs.tocsr()
    w = weights(mass, stop_type)
    rhs = np.asarray(rhs, dtype=np.float64)
    if rhs.ndim == 1:
        rhs = rhs[:, None]
    x = np.array(np.asarray(x0, dtype=np.float64).reshape(rhs.shape), order="F")
    d = rhs.shape[1]
    r = rhs - A @ x
    bb = (w * rhs * rhs).sum(axis=0)
    floor2 = np.where(bb > 0.0, FLOOR_GUARD_REL2 * bb, 0.0)
    p = np.zeros_like(x)
    rho_prev = np.zeros(d)
    restart = np.zeros(d, dtype=bool)
    rr = None                  # sum w r^2 as last reported: not known in the first iteration
    fresh_all = False
    residues, steps, iterates, guards, restarts, it = [], [], [], 0, 0, 0
    while True:
        first = it == 0
        z = np.asarray(cycle(r, np.zeros_like(r))).reshape(rhs.shape)
        rho = (r * z).sum(axis=0)
        fresh = restart | first | fresh_all
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            beta = np.where(~fresh & usable(rho_prev) & np.isfinite(rho), rho / rho_prev, 0.0)
            if not first:
                restarts += int(fresh.sum())
            on = beta != 0.0
            p = np.where(on, z + beta * np.where(on, p, 0.0), z)
            q = A @ p
            pq = (p * q).sum(axis=0)
            g = ~((pq > 0.0) & np.isfinite(pq) & np.isfinite(rho))
            if rr is not None:
                g = g | ((floor2 > 0.0) & (rr <= floor2))
            alpha = np.where(g, 0.0, rho / pq)
            go = alpha != 0.0
            x = np.where(go, x + alpha * np.where(go, p, 0.0), x)
            r = np.where(go, r - alpha * np.where(go, q, 0.0), r)
        guards += int(g.sum())
        restart, rho_prev, fresh_all = g, rho, False
        rr = (w * r * r).sum(axis=0)
        res = norm(rr, bb, stop_type)
        it += 1
        confirmed = not (res > tol and it < max_iter)
        if confirmed:
            r_true = rhs - A @ x
            rr = (w * r_true * r_true).sum(axis=0)
            res = norm(rr, bb, stop_type)
        residues.append(res)
        iterates.append(x)
        steps.append(dict(rho=rho, beta=beta, pq=pq, alpha=alpha, guarded=g, fresh=fresh, confirmed=confirmed, residue=res))
        if not (res > tol and it < max_iter):
            return x, it, np.array(residues), guards, restarts, steps, iterates
        if confirmed:
            r, fresh_all = r_true, True
