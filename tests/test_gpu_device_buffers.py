"""Who owns the device arrays of a handle.  Every array the engine takes from its per-handle pool has one owner, and an owner that is
replaced or dropped gives its block back: the same sequence of calls, repeated on one handle, holds the same number of pool blocks after every
step ("device_blocks_now"; blocks, not bytes -- identical calls make identical allocation requests, whichever parked block the pool hands
back) and computes the same iterates bit for bit.  One round goes through everything that replaces or drops an owner: a hierarchy, a full
set-up, vectors regrown for more right-hand sides, a values-only refresh, a set-up that fails, the set-up after it, and a new hierarchy over a
live system.  The configurations are those that own different arrays.  Shape: the four-level chain of tests/test_gpu_call_order.py."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import problems

pytestmark = pytest.mark.gpu

SHAPE = dict(graph=("chain", 193), sizes=[193, 96, 24, 6], kind="smoothing", prolong=("smooth", "pc", "pc"))
ROUNDS = 4


def _configs():
    from gravo_mg_amd import cabi
    return {
        "default": dict(),
        "lane-per-row": dict(block_lanes=1),                               # entry-parallel arrays and source maps
        "block-csr": dict(block_lanes=1, block_ep=False),                  # block-CSR and the split SELL pair
        "fp32-inner": dict(inner_precision=1),
        "accelerate": dict(accelerate=2),
        "coarse-triangle": dict(coarse_mode=cabi.COARSE_DEVICE_TRIANGLE),
        "coarse-host": dict(coarse_mode=cabi.COARSE_HOST_LDLT),
        "chebyshev": dict(smoother=cabi.SMOOTHER_CHEBYSHEV),
        "host-planner": dict(device_setup=False),
        "graph": dict(use_graph=True),
    }


def _round(cabi, eng, P):
    """One round on `eng`: the block count after every step, and the iterate of every solve."""
    blocks, iterates = [], []

    def step(name, f):
        out = f()
        blocks.append((name, eng.timing("device_blocks_now")))
        return out

    def solve(name, rhs):
        x, it, res, _ = step(name, lambda: eng.solve(rhs, tol=1e-6))
        iterates.append((name, x, it, res))

    def malformed():
        with pytest.raises(cabi.GmgError):
            eng.set_system(sp.csc_matrix(P.lhs.shape) + sp.identity(P.n, format="csc") * 0.0)

    step("set_prolongations", lambda: eng.set_prolongations(P.U))
    step("set_mass", lambda: eng.set_mass(P.mass))
    step("set_system", lambda: eng.set_system(P.lhs))
    solve("solve d=1", P.rhs[:, :1])
    solve("solve d=3", P.rhs[:, :3])                                       # regrows the vectors
    step("set_system values", lambda: eng.set_system(P.lhs * 1.5))         # same pattern: values only
    solve("solve scaled", P.rhs[:, :3])
    step("malformed", malformed)
    step("set_system again", lambda: eng.set_system(P.lhs))
    solve("solve again", P.rhs[:, :3])
    step("set_prolongations over a system", lambda: eng.set_prolongations(P.U))      # drops system and transfers
    return blocks, iterates


@pytest.mark.parametrize("config", sorted(_configs()))
def test_repeated_rounds_hold_the_same_blocks(cabi, config):
    P = problems.synthetic_problem(d=3, **SHAPE)
    eng = cabi.Engine(**_configs()[config])
    try:
        rounds = [_round(cabi, eng, P) for _ in range(ROUNDS)]
    finally:
        eng.close()
    for blocks, _ in rounds:
        print(config, [int(c) for _, c in blocks])
    want_blocks, want_iterates = rounds[1]
    assert all(c > 0 for name, c in want_blocks if name.startswith(("set_system", "solve")))
    for r in (2, 3):
        blocks, iterates = rounds[r]
        assert blocks == want_blocks, (config, r)
        for (name, x, it, res), (_, wx, wit, wres) in zip(iterates, want_iterates):
            assert it == wit and res == wres and np.array_equal(x, wx), (config, r, name)


def test_bound_vectors_are_borrowed_not_owned(cabi):
    """gmg_dist_bind puts the caller's vectors in the place of level 0's and parks the engine's: whatever then releases the level -- a
    values-only refresh does not, a new hierarchy over the bound system does -- must release the engine's vectors and never the caller's."""
    import torch
    P = problems.synthetic_problem(d=3, **SHAPE)
    d, guard = 3, 256
    eng = cabi.Engine()
    eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
    n_pad = eng.level_info(0)["n_pad"]
    n_colors = len(eng.level_ordering(0)[1]) - 1
    x, b, r = (torch.full((n_pad * d + guard,), 7.0, dtype=torch.float64, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    counts, sums = [], []
    try:
        for rnd in range(ROUNDS):
            c = []
            eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)       # (rounds 2 ..: over a system bound to x, b, r)
            c.append(eng.timing("device_blocks_now"))
            eng.dist_setup(0, 1)
            eng.dist_bind(x.data_ptr(), b.data_ptr(), r.data_ptr(), d)
            c.append(eng.timing("device_blocks_now"))
            eng.load_problem(P.rhs[:, :d], P.rhs[:, :d])
            torch.cuda.synchronize()
            b_loaded = b.clone()
            for _ in range(2):
                for col in range(n_colors):
                    eng.dist_smooth_color(col)
            eng.dist_residual_own(); eng.dist_coarse_cycle(); eng.dist_prolong_own()
            sums.append(eng.dist_norm_partial(2, d))
            c.append(eng.timing("device_blocks_now"))
            eng.set_system(P.lhs * 1.5)                                                    # values only: stays bound
            c.append(eng.timing("device_blocks_now"))
            torch.cuda.synchronize()
            assert torch.equal(b, b_loaded)
            counts.append(c)
        print(counts)
        assert counts[1] == counts[2] == counts[3]
        assert np.array_equal(sums[1], sums[2]) and np.array_equal(sums[1], sums[3])
    finally:
        eng.close()
    # the handle is gone; the tensors are the caller's, whole and readable
    torch.cuda.synchronize()
    assert torch.equal(b, b_loaded)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(r).all())
    for t in (x, b, r):
        assert bool((t[n_pad * d:] == 7.0).all())
