"""No entry point depends on what ran before it on the handle.  The launches of a cycle hand things to one another -- the head of the next
cycle enqueued ahead of the solve loop's decision, the first pre-sweep a restriction ran for the level below, the iterate a residual is formed
from, the sums a colour launch formed for the residual check -- and none of that may outlive the call it belongs to: after a solve that ended
with a head in the stream, and after fixed numbers of cycles with and without a residual check, every call computes bit for bit what it
computes on an engine that has done nothing else.  Shapes of the boundary-shape catalogue on which these hand-overs engage: a two-colour level
0 with one transfer level (the head, both folds) and with three (the fused restriction, the residual from the sweep, the interleaved copy at
d = 3)."""
import numpy as np
import pytest

from tests import problems
from tests.parity_checks import engaged

pytestmark = pytest.mark.gpu

SHAPES = {
    "chain193": dict(graph=("chain", 193), sizes=[193, 96, 24, 6], kind="smoothing", prolong=("smooth", "pc", "pc")),
    "chain64": dict(graph=("chain", 64), sizes=[64, 16], kind="poisson", prolong=("pc",)),
}


def _engine(cabi, P, **kw):
    eng = cabi.Engine(**kw)
    eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
    return eng


def _probes(P, d):
    """The calls compared, each as (name, f(engine) -> tuple of arrays and numbers)."""
    rng = np.random.default_rng(3)
    rhs = P.rhs[:, :d]
    n1 = P.U[0].shape[1]
    b0, x0 = rng.standard_normal((P.n, d)), rng.standard_normal((P.n, d))
    b1 = rng.standard_normal((n1, d))

    def solve(eng):
        x, it, res, conv = eng.solve(rhs, tol=1e-6)
        return x, it, res, conv[:, 1]
    probes = []
    if len(P.U) > 1:           # (level 1 is a transfer level)
        probes.append(("smooth_residual(1, from_zero)", lambda eng: eng.smooth_residual(1, b1, None, 2, from_zero=True)))
    probes += [("smooth_residual(0)", lambda eng: eng.smooth_residual(0, b0, x0, 2)),
               ("smooth(0)", lambda eng: (eng.smooth(0, b0, x0, 2),)),
               ("vcycle", lambda eng: (eng.vcycle(rhs, rhs),)),
               ("solve", solve)]
    return rhs, probes


# (lane-per-row: the small levels take the layout of big ones -- the entry-parallel block sweep, with the residual from the sweep and the interleaved copy)
@pytest.mark.parametrize("kw", [dict(), dict(use_graph=True), dict(block_lanes=1)], ids=["default", "graph", "lane-per-row"])
@pytest.mark.parametrize("d", (1, 3))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_calls_do_not_depend_on_earlier_calls(cabi, shape, d, kw):
    P = problems.synthetic_problem(d=3, **SHAPES[shape])
    rhs, probes = _probes(P, d)
    used = _engine(cabi, P, **kw)
    try:
        for name, probe in probes:
            # what ran before: a solve that stops early (heads were enqueued, the last one behind the decision that ended the loop), one cycle
            # with a residual check and one without
            _, it, _, _ = used.solve(rhs, tol=1e-6)
            assert it < 100, it                   # (stopped by the tolerance)
            # (the hand-overs did engage: heads in the stream; the quad-layout levels of the default configuration fuse the restriction into
            # level 1 of the four-level chain with its first pre-sweep)
            if not kw.get("use_graph"):
                assert engaged(used, "speculate_head") > 0
            if not kw.get("block_lanes") and len(P.U) > 1:
                assert engaged(used, "fuse_restrict_sweep") > 0
            used.load_problem(rhs, rhs)
            used.run_cycles(1, 2)
            used.run_cycles(1, -1)
            got = probe(used)
            if kw.get("block_lanes") and name.startswith("smooth_residual(1"):          # (entry-parallel sweep: the residual came from the sweep)
                assert used.timing("residual_from_sweep") == 1.0
            fresh = _engine(cabi, P, **kw)
            try:
                want = probe(fresh)
            finally:
                fresh.close()
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert np.array_equal(np.asarray(g), np.asarray(w)), (name, shape, d)
    finally:
        used.close()
