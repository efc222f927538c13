"""The catalogue of tests/test_gpu_mixed_operators.py (the fp32 inner cycle's kernels, operator by operator, on the device) and
tests/test_mixed_model_host.py (the model behind it, on the host): the shapes of the boundary catalogue (tests/test_gpu_boundary_shapes.py)
at which the fp32 instantiations switch branches, and "exact twins" on which float32 arithmetic commits no rounding at all.

Level sizes, finest first, and what each case is here for:
  chain<n>-L1 / -L2, n in 1, 5, 63, 64, 65, 129, 193   levels below, at and above one 64-row slice; d in 1, 2, 3, 4, 5, 8 (d = 8: two column chunks)
  chain193-L3      [193, 96, 24, 6]     a restriction into a level that is smoothed: the fused restriction + first sweep
  diagonal100      [100, 25, 6]         no off-diagonal entry, one colour per level
  isolated40x40    [1600, 400, 100]     rows without off-diagonals among ordinary ones
  hub48x40         [1921, 480, 120]     one level-1 row denser than the entry-parallel sweep's window (kEpW)
  clique65         [2369, 592, 148]     65 colours on a colour-major level 0 (block_fine = 0)
  coarsest1 / 17 / 65                   the conversions around the fp64 coarsest solve
  exact-chain193, exact-grid17x13, exact-hub48x40       integer operators with a power-of-two diagonal: bitwise equality with the model"""
import functools

import numpy as np
import scipy.sparse as sp

from tests import problems

D_ALL, D_FEW = (1, 2, 3, 4, 5, 8), (1, 3)
ITERS = (1, 2)


@functools.lru_cache(maxsize=None)
def exact_problem(graph, sizes, seed=3, d=8):
    """The exact twin of a synthetic graph: integer edge weights in {1, 2, 3}, lhs = 2^p I - W with 2^p the smallest power of two above twice
    the largest weighted degree (power-of-two diagonal, strictly diagonally dominant), piecewise-constant prolongations (Galerkin operators
    and transfers stay integer), unit mass, integer right-hand sides in [-8, 8]."""
    P = problems.synthetic_problem(graph=graph, sizes=list(sizes), kind="poisson", prolong=("pc",), d=d)
    rng = np.random.default_rng(seed)
    pat = sp.triu(sp.coo_matrix(P.S), k=1).tocoo()
    w = rng.integers(1, 4, pat.nnz).astype(np.float64)
    n = P.n
    W = sp.coo_matrix((w, (pat.row, pat.col)), shape=(n, n)).tocsc()
    W = (W + W.T).tocsc()
    deg = np.asarray(W.sum(axis=1)).ravel()
    p = 1
    while 2.0 ** p <= 2.0 * max(deg.max(), 0.5):
        p += 1
    lhs = (2.0 ** p * sp.identity(n) - W).tocsc()
    lhs.sort_indices()
    rhs = rng.integers(-8, 9, (n, d)).astype(np.float64)
    S = (sp.diags(deg) - W).tocsc()
    return problems.Problem(None, S, np.ones(n), P.U, lhs, rhs, "exact-" + P.name)


def integer_block(rng, n, d):
    """An n x d block of integers in [-8, 8]."""
    return rng.integers(-8, 9, (n, d)).astype(np.float64)


def f32_block(rng, n, d):
    """An n x d block of float32-representable normal deviates."""
    return rng.standard_normal((n, d)).astype(np.float32).astype(np.float64)


def _grid_for(n_L):
    n1 = max(1, int(np.ceil(np.sqrt(4 * n_L))))
    return n1, max(1, int(np.ceil(4 * n_L / n1)))


class CaseSpec:
    def __init__(self, name, spec, ds, kw=None, exact=False, all_variants=False):
        self.name, self.spec, self.ds, self.kw, self.exact, self.all_variants = name, spec, ds, dict(kw or {}), exact, all_variants

    def problem(self):
        if self.exact:
            return exact_problem(self.spec["graph"], tuple(self.spec["sizes"]))
        return problems.synthetic_problem(**self.spec)

    def block(self, rng, n, d):
        return (integer_block if self.exact else f32_block)(rng, n, d)


def _catalogue():
    c = []
    for n in (1, 5, 63, 64, 65, 129, 193):
        c.append(CaseSpec("chain%d-L1" % n, dict(graph=("chain", n), sizes=[n, max(1, n // 4)], kind="poisson", prolong=("pc",)), D_ALL))
        c.append(CaseSpec("chain%d-L2" % n, dict(graph=("chain", n), sizes=[n, max(1, n // 2), max(1, n // 8)], kind="smoothing",
                                                 prolong=("smooth", "pc")), D_ALL))
    c.append(CaseSpec("chain193-L3", dict(graph=("chain", 193), sizes=[193, 96, 24, 6], kind="smoothing", prolong=("smooth", "pc", "pc")), D_ALL,
                      all_variants=True))
    c.append(CaseSpec("diagonal100", dict(graph=("diagonal", 100), sizes=[100, 25, 6], kind="poisson", prolong=("pc",)), D_FEW))
    c.append(CaseSpec("isolated40x40", dict(graph=("isolated", 40, 40), sizes=[1600, 400, 100], kind="smoothing", prolong=("smooth", "pc")), D_FEW))
    c.append(CaseSpec("hub48x40", dict(graph=("hub", 48, 40), sizes=[1921, 480, 120], kind="poisson", prolong=("pc",)), D_FEW, all_variants=True))
    c.append(CaseSpec("clique65", dict(graph=("clique", 48, 48, 65), sizes=[2369, 592, 148], kind="smoothing", prolong=("pc",)), D_FEW,
                      kw=dict(block_fine=False)))
    for n_L in (1, 17, 65):
        n1, n2 = _grid_for(n_L)
        c.append(CaseSpec("coarsest%d" % n_L, dict(graph=("grid", n1, n2), sizes=[n1 * n2, n_L], kind="poisson", prolong=("pc",)), D_FEW))
    c.append(CaseSpec("exact-chain193", dict(graph=("chain", 193), sizes=[193, 96, 24, 6]), D_ALL, exact=True, all_variants=True))
    c.append(CaseSpec("exact-grid17x13", dict(graph=("grid", 17, 13), sizes=[221, 55, 13]), D_FEW, exact=True, all_variants=True))
    c.append(CaseSpec("exact-hub48x40", dict(graph=("hub", 48, 40), sizes=[1921, 480, 120]), D_FEW, exact=True, all_variants=True))
    return c


CASES = _catalogue()
BY_NAME = {c.name: c for c in CASES}

# engine settings beside inner_precision = 1 (the smoother constants are cabi's: 1 = GMG_SMOOTHER_JACOBI; coarse modes 0 host LDL^T, 3 device triangle)
VARIANTS = {
    "default": dict(),
    "lanes1-ep": dict(block_lanes=1),                          # gs_block_ep with the 8-byte fp32 records
    "lanes1-bcsr": dict(block_lanes=1, block_ep=False),        # the block-CSR
    "lanes4-rows128": dict(block_lanes=4, block_rows=128),     # gs_block4
    "multicolour": dict(block_rows=0),                         # colour-major on every level
    "blocked-fine": dict(block_from_level=0),
    "jacobi": dict(smoother=1),
    "unfused": dict(fuse_restrict_sweep=False),
    "coarse-host": dict(coarse_mode=0),
    "coarse-triangle": dict(coarse_mode=3),
}

# level-0 sweep counts at which float32 is exact on the exact twins (verified by the model: tests/test_mixed_model_host.py).  The hub's diagonal
# is 2^12 and its graph has three colours: the third colour of the first sweep already reads multiples of 2^-24 beside integers, so only its
# products are exact.
EXACT_FINE_SWEEPS = {"exact-chain193": (1, 2), "exact-grid17x13": (1, 2), "exact-hub48x40": ()}


def runs():
    """(case, variant name) pairs of the GPU test: every variant on the all_variants cases, the default alone elsewhere."""
    out = []
    for c in CASES:
        for v in (VARIANTS if c.all_variants else ("default",)):
            out.append((c, v))
    return out
