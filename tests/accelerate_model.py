"""numpy restatement of the accelerated solve loop (gmg_config::accelerate: truncated GCR around the V-cycle; engine.hip::solve_common,
accel_kernels.hip.hpp, accel_scalars.hpp) -- test infrastructure, shared by the host tests of the model and the device comparisons.

The cycle is an argument: `cycle(b, x)` returns the cycle's iterate from x for the right-hand side b (n x d in, n x d out).  The device tests
hand in `vcycle` of a second handle created with accelerate = 0, the host tests tests/vcycle_model.VcycleModel or
tests/chebyshev_model.ChebyshevModel built from the oracle's operators.  A x is scipy's, everything fp64: the model differs from the device
only in the order of its sums.

Per iteration, per column (w: the stop type's weights, <u, v> = sum_i w_i u_i v_i):

  x~ = cycle(b, x_k),  r~ = b - A x~,  z0 = x~ - x_k,  q0 = r - r~
  beta_j = <q0, q_j> / s_j for every stored direction with a usable s_j (all from q0: classical Gram-Schmidt), else 0
  z = z0 - sum beta_j z_j,  q = q0 - sum beta_j q_j,  s = <q, q>,  rho = <r, q>
  guarded (s zero or not finite, or -- from the second iteration on -- s <= 1e-25 <b, b>: a direction below 3.2e-13 |b| is rounding noise, the
  iterate is on its accuracy floor): alpha = 1 and z0, q0 take the place of z, q; the direction is stored with s_j = 0.  Otherwise alpha = rho / s.
  x_{k+1} = x_k + alpha z,  r -= alpha q;  the last m - 1 directions are kept.
  A residue that would end the loop is confirmed by b - A x_{k+1}; the loop goes on from that residual where it does not hold."""
from __future__ import annotations

import numpy as np


def weights(mass, stop_type):
    n = len(mass)
    return {0: np.ones(n), 1: 1.0 / mass, 2: mass, 3: np.ones(n)}[stop_type][:, None]


def norm(rr, bb, stop_type):
    """solve_rule.hpp::norm_from_sums on the per-column sums of w r^2 and w b^2."""
    if stop_type == 3:
        return float(np.sqrt(rr.sum()))
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.sqrt(rr) / np.sqrt(bb) if stop_type == 0 else np.sqrt(rr / bb)
    out = v[0]
    for t in v[1:]:
        if t > out:
            out = t
    return float(out)


FLOOR_GUARD_REL2 = 1e-25      # gmg::kAccelFloorRel2


def usable(s):
    return np.isfinite(s) & (s != 0.0)


def accelerated_loop(lhs, mass, cycle, rhs, x0, m, stop_type, tol, max_iter, keep_vectors=False, floor_guard=True):
    """Returns (x, iterations, residues, guarded steps, steps).  steps[k] holds the scalars of iteration k + 1: "alpha" (d), "betas" (one array of
    d per stored direction, oldest first), "s", "rho" (d), "stored_s" (the s_j the betas were divided by), "guarded" (d, bool), "confirmed" and
    "residue"; with keep_vectors also the state the step started from and what it formed: "xk", "r", "z0", "q0", "z", "q" (the ones the update used:
    z0, q0 in a guarded column), "stored_q" and "bb" -- enough to evaluate the residue of any other alpha / beta from the same state.
    floor_guard = False: the loop without its floor guard (what the device ran before it had one), for the tests that show what the guard is for."""
    A = lhs.tocsr()
    w = weights(mass, stop_type)
    rhs = np.asarray(rhs, dtype=np.float64)
    x = np.array(x0, dtype=np.float64, order="F")
    r = rhs - A @ x
    bb = (w * rhs * rhs).sum(axis=0)
    stored, residues, guards, steps = [], [], 0, []
    it = 0
    while True:
        xk = x
        xt = np.asarray(cycle(rhs, xk)).reshape(rhs.shape)
        rt = rhs - A @ xt
        z0, q0 = xt - xk, r - rt
        z, q = z0.copy(), q0.copy()
        with np.errstate(invalid="ignore", divide="ignore"):
            betas = [np.where(usable(sj), (w * q0 * qj).sum(axis=0) / sj, 0.0) for (_, qj, sj) in stored]      # all from q0: classical Gram-Schmidt
            for beta, (zj, qj, _) in zip(betas, stored):
                on = beta != 0.0
                z[:, on] -= beta[on] * zj[:, on]
                q[:, on] -= beta[on] * qj[:, on]
            s, rho = (w * q * q).sum(axis=0), (w * r * q).sum(axis=0)
            g = ~usable(s)
            if it > 0 and floor_guard:          # the floor guard (accel_scalars.hpp::accel_floor): <b, b> is known from the first update on
                g = g | ((bb > 0.0) & (s <= FLOOR_GUARD_REL2 * bb))
            alpha = np.where(g, 1.0, rho / s)
        guards += int(g.sum())
        zu, qu = np.where(g, z0, z), np.where(g, q0, q)
        step = dict(alpha=alpha, betas=betas, s=s, rho=rho, stored_s=[sj for (_, _, sj) in stored], guarded=g)
        if keep_vectors:
            step.update(xk=xk, r=r, z0=z0, q0=q0, z=zu, q=qu, stored_q=[qj for (_, qj, _) in stored], bb=bb)
        x = xk + alpha * zu
        r = r - alpha * qu
        if m > 1:
            stored.append((z, q, np.where(g, 0.0, s)))
            stored = stored[-(m - 1):]
        res = norm((w * r * r).sum(axis=0), bb, stop_type)
        it += 1
        confirmed = not (res > tol and it < max_iter)
        if confirmed:
            r_true = rhs - A @ x
            res = norm((w * r_true * r_true).sum(axis=0), bb, stop_type)
        residues.append(res)
        step.update(confirmed=confirmed, residue=res)
        steps.append(step)
        if not (res > tol and it < max_iter):
            return x, it, np.array(residues), guards, steps
        if confirmed:
            r = r_true


def shape_catalogue():
    """The boundary shapes the accelerated loop is tested at: three lists of (name, synthetic_problem spec, engine settings) -- the compared cases,
    those that reach the floor too early for that, and the tiny ones (fewer than 5 unknowns), compared in their first iteration only.

    The specs are those of tests/test_gpu_chebyshev.py and tests/test_gpu_boundary_shapes.py (imported, not copied), plus two chains whose level 0
    has more than one 256-thread block of row pairs: a chain's level 0 is two colour classes of ceil(n / 2) and floor(n / 2) rows, each padded to
    64 (test_shape_is_the_one_asked_for), so n = 513 gives n_pad = 576 (288 pairs: two blocks, 32 threads of the second at work) and n = 1 025
    gives n_pad = 1 088 (544 pairs: three blocks)."""
    from tests.test_gpu_boundary_shapes import CASES as BOUNDARY
    from tests.test_gpu_chebyshev import CASES as CHEBY
    cheby = {c[0]: c for c in CHEBY}
    boundary = {c[0]: c for c in BOUNDARY}
    out = []
    for n in (63, 64, 65, 129, 193):
        out += [cheby["chain%d-L1" % n], cheby["chain%d-L2" % n]]
    out += [cheby[k] for k in ("chain193-L3", "chain129-coarsest1", "diagonal100", "isolated40x40", "hub48x40", "clique65")]
    cases = [(name, spec, dict(kw)) for name, spec, _, kw in out]
    cases.append(("clique65-blocked", cheby["clique65"][1], {}))
    for n in (513, 1025):
        cases.append(("chain%d-L2" % n, dict(graph=("chain", n), sizes=[n, n // 2, n // 8], kind="smoothing", prolong=("smooth", "pc")), {}))
    tiny = [(name, cheby[name][1], {}) for name in ("chain1-L1", "chain1-L2", "chain2-L1", "chain2-L2")]
    tiny.append(("diagonal1", boundary["B-diagonal1"][1], {}))
    tiny.append(("grid2x2-coarsest1", boundary["D-coarsest1"][1], {}))
    assert tiny[-1][1]["graph"] == ("grid", 2, 2) and tiny[-1][1]["sizes"] == [4, 1]
    # diagonal100: every cycle solves a diagonal system (almost) exactly, fewer than 3 of 8 iterations stay above the floor (the floor table of
    # tests/test_accelerate_model_host.py): compared in its first iteration only, like the tiny shapes
    early = [c for c in cases if c[0] in EARLY_FLOOR]
    cases = [c for c in cases if c[0] not in EARLY_FLOOR]
    return cases, early, tiny


EARLY_FLOOR = ("diagonal100",)
FLOOR_REL = 1e-9              # an iteration is "above the floor" while its model residue is at least this times the first residue
NONINCREASING = 1.0 + 1e-10
# 100 x the largest sensitivity of the model to one rounding per cycle output (3.63e-13 in x, hub48x40 with the Chebyshev cycle:
# tests/test_accelerate_model_host.py::test_sensitivity_sets_the_device_tolerance measures it and holds this constant to it)
SHAPE_TOL = 3.7e-11


def above_floor(residues):
    """The number of leading iterations whose residue is at least FLOOR_REL times the first one: the iterations a comparison looks at."""
    k = 0
    while k < len(residues) and residues[k] >= FLOOR_REL * residues[0]:
        k += 1
    return k


def chain_n_pad(n):
    """n_pad of a chain's colour-major level 0: two colour classes, each padded to 64 rows."""
    return 64 * (-(-((n + 1) // 2) // 64) + -(-(n // 2) // 64))


def plain_loop(lhs, mass, cycle, rhs, x0, stop_type, tol, max_iter):
    """The unaccelerated loop (accelerate = 0): one cycle, the residue of its iterate, the same stopping rule.  Returns (x, iterations, residues)."""
    A = lhs.tocsr()
    w = weights(mass, stop_type)
    rhs = np.asarray(rhs, dtype=np.float64)
    bb = (w * rhs * rhs).sum(axis=0)
    x = np.array(x0, dtype=np.float64, order="F")
    residues = []
    while True:
        x = np.asarray(cycle(rhs, x)).reshape(rhs.shape)
        r = rhs - A @ x
        residues.append(norm((w * r * r).sum(axis=0), bb, stop_type))
        if not (residues[-1] > tol and len(residues) < max_iter):
            return x, len(residues), np.array(residues)
