"""The V-cycle at pre_iters / post_iters other than the default 2 + 2.

The launch code branches on the two counts in many places: the ping-pong of the block sweeps between x and tmp (which buffer the result lands
in, whether it is copied back, whether the residual may be formed from the last sweep's x_old - x_new), the first pre-sweep that rides on the
restriction, the cleared coarse iterates and the plain level-0 residual without pre-smoothing, the residual check that cannot ride on a last
colour launch and the prolongation that must read x without post-smoothing, the head of the next cycle that must not be enqueued without
pre-smoothing -- on one GPU (engine_cycle.hip.hpp), in the partitioned cycle (engine_dist.hip.hpp) and in gmg_profile_cycle.  Every check here
compares with the CPU model of the same iteration (tests/vcycle_model.VcycleModel, assembled from the oracle with the same counts; the oracle
itself is pinned at other counts by tests/test_oracle.py) or with the oracle directly, at the tolerances of tests/test_gpu_parity.py,
tests/test_gpu_boundary_shapes.py and tests/test_gpu_cycle_model.py; engine-against-engine comparisons are bitwise ones only.

Pairs: {0..3}^2, 4 + 1, 1 + 4, 5 + 5.  0 + 0 (the coarse-grid correction alone) is a legal configuration and takes part in every per-cycle check;
it does not contract, so only the checks that need convergence leave it out.
Problems: two hierarchy-builder tori (three transfer levels; smoothing with d = 3, Poisson), a point cloud whose level 0 runs the block sweep,
and three shapes of the boundary catalogue (a fused restriction engages on A-chain193-L3, the head on A-chain64-L1, D-coarsest65 has one
transfer level and the device inverse)."""
import os
import socket
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from tests import problems
from tests.parity_checks import SWITCHES, colour_permuted_hierarchy, engaged, rel
from tests.vcycle_model import VcycleModel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAIRS = [(pre, post) for pre in range(4) for post in range(4)] + [(4, 1), (1, 4), (5, 5)]
FEW_PAIRS = [(0, 0), (0, 2), (1, 1), (2, 0), (3, 3)]
BITWISE_PAIRS = [(0, 2), (1, 0), (1, 1), (2, 0), (3, 2)]
PROBLEMS = ["torus-smoothing", "torus-poisson", "cloud", "A-chain193-L3", "A-chain64-L1", "D-coarsest65"]


def _pid(pair):
    return "%d+%d" % pair


def _catalogue_spec(name):
    from tests.test_gpu_boundary_shapes import CASES
    (spec,) = [c[1] for c in CASES if c[0] == name]
    return spec


class Case:
    """One problem, its right-hand-side widths, and what is shared between the tests of a (pre, post) pair: the default engine, its model, the
    model's iterates from x0 = rhs."""

    def __init__(self, name, cabi, oracle):
        self.name, self.cabi, self.oracle = name, cabi, oracle
        if name == "torus-smoothing":
            self.P, self.ds = problems.torus_problem(96, 80, "smoothing", 30), (3, 1)
        elif name == "torus-poisson":
            self.P, self.ds = problems.torus_problem(96, 80, "poisson", 30), (1,)
        elif name == "cloud":
            self.P, self.ds = problems.pointcloud_problem(9000, 8, 120), (1,)
        else:
            self.P, self.ds = problems.synthetic_problem(**_catalogue_spec(name)), (1, 3, 5)
        self.smoothing = "smoothing" in self.P.name
        self.nA = spla.norm(self.P.lhs)
        self._engines, self._models, self._chains = {}, {}, {}

    def rhs(self, d):
        b = self.P.rhs if self.P.rhs.ndim == 2 else self.P.rhs[:, None]
        assert b.shape[1] >= d
        return np.ascontiguousarray(b[:, :d])

    def new_engine(self, pre, post, **kw):
        P = self.P
        eng = self.cabi.Engine(pre_iters=pre, post_iters=post, **kw)
        eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
        assert eng.num_levels == len(P.U)
        return eng

    def engine(self, pre, post):
        """The default engine of a pair (kept for the module: several tests use it)."""
        if (pre, post) not in self._engines:
            self._engines[(pre, post)] = self.new_engine(pre, post)
        return self._engines[(pre, post)]

    def model(self, pre, post):
        if (pre, post) not in self._models:
            eng = self.engine(pre, post)
            self._models[(pre, post)] = VcycleModel(eng, self.P.U, self.P.mass, self.P.lhs, self.oracle, eng.gs_omega, pre=pre, post=post)
        return self._models[(pre, post)]

    def chain(self, pre, post, d, upto):
        """Iterates x_1 .. of the model from x0 = rhs (d columns) and their type-2 residues, extended until the residue is <= upto or 100 cycles."""
        key = (pre, post, d)
        b = self.rhs(d)
        if key not in self._chains:
            self._chains[key] = ([], [])
        xs, res = self._chains[key]
        M = self.model(pre, post)
        while len(xs) < 100 and (len(xs) < 3 or not res[-1] <= upto):
            xs.append(M.vcycle(b, xs[-1] if xs else b.copy()))
            res.append(self.oracle.residual_check(self.P.lhs, self.P.mass, b, xs[-1], 2))
        return xs, res

    def close(self):
        for e in self._engines.values():
            e.close()
        self._engines.clear()


@pytest.fixture(scope="module", params=PROBLEMS)
def case(request, cabi, oracle):
    assert cabi.device_count() > 0, "gpu tests need a HIP device"
    c = Case(request.param, cabi, oracle)
    yield c
    c.close()


def test_problems_have_the_layouts_they_are_here_for(case):
    eng = case.engine(2, 2)
    P = case.P
    if case.name.startswith("torus"):
        assert len(P.U) == 3 and eng.level_blocks(0) is None and eng.level_blocks(1) is not None
        assert (P.rhs.shape[1] if P.rhs.ndim == 2 else 1) == (3 if case.smoothing else 1)
    if case.name == "cloud":
        assert eng.level_blocks(0) is not None
    if case.name == "A-chain193-L3":
        assert [u.shape[0] for u in P.U] + [P.U[-1].shape[1]] == [193, 96, 24, 6]
    if case.name in ("A-chain64-L1", "D-coarsest65"):
        assert len(P.U) == 1 and eng.timing("coarse_on_device") == 1.0
    assert P.n <= 12000


# ---------------------------------------------------------------------------------------------- (a), (b): cycle by cycle against the model
def _check_cycles(case, M, eng64, eng32, what):
    """Three V-cycles of eng64 (fp64 bounds) and eng32 (fp32 inner cycle, 2e-5) against the model M, each restarted from the model's iterate."""
    P = case.P
    for d in case.ds:
        b = case.rhs(d)
        x = b.copy()
        for cyc in range(3):
            xm = M.vcycle(b, x)
            if eng64 is not None:
                xg = eng64.vcycle(b, x)
                back, fwd = np.linalg.norm(P.lhs @ (xg - xm)), rel(xg, xm)
                assert back <= 1e-12 * case.nA * np.linalg.norm(xm), (what, d, cyc, back / (case.nA * np.linalg.norm(xm)))
                assert fwd <= (1e-11 if case.smoothing else 1e-6), (what, d, cyc, fwd)
            if eng32 is not None:
                xg = eng32.vcycle(b, x)
                assert np.linalg.norm(xg - xm) <= 2e-5 * np.linalg.norm(xm), (what, "fp32 inner", d, cyc, rel(xg, xm))
            x = xm


@pytest.mark.parametrize("pair", PAIRS, ids=_pid)
def test_default_engine_matches_model_cycle_by_cycle(case, pair):
    pre, post = pair
    mix = case.new_engine(pre, post, inner_precision=1)
    try:
        _check_cycles(case, case.model(pre, post), case.engine(pre, post), mix, "default")
    finally:
        mix.close()


def _variants(cabi):
    return {"lanes1": dict(block_lanes=1), "lanes1-no-ep": dict(block_lanes=1, block_ep=False), "blocked-from-0": dict(block_from_level=0, gs_omega=1.0),
            "host-ldlt": dict(coarse_mode=cabi.COARSE_HOST_LDLT), "device-inverse": dict(coarse_mode=cabi.COARSE_DEVICE_INVERSE),
            "graph": dict(use_graph=True), "jacobi": dict(smoother=cabi.SMOOTHER_JACOBI)}


VARIANT_PAIRS = [(v, p) for v in ("lanes1", "lanes1-no-ep", "blocked-from-0", "host-ldlt") for p in PAIRS] + \
                [(v, p) for v in ("device-inverse", "graph", "jacobi") for p in FEW_PAIRS]


@pytest.mark.parametrize("variant,pair", VARIANT_PAIRS, ids=["%s-%s" % (v, _pid(p)) for v, p in VARIANT_PAIRS])
def test_variants_match_model_cycle_by_cycle(case, cabi, oracle, variant, pair):
    """The other branch of the conditions: entry-parallel sweep and the residual from the sweep's explicit part on these small levels
    (block_lanes = 1), the block-CSR / SELL sweeps (block_ep = 0), a blocked level 0, the host coarse solve (two graphs with the host gate
    between them), the device inverse, a captured graph, weighted Jacobi.  The model takes the orderings of the fp64 engine of the variant."""
    pre, post = pair
    kw = _variants(cabi)[variant]
    P = case.P
    e64 = case.new_engine(pre, post, **kw)
    e32 = case.new_engine(pre, post, inner_precision=1, **kw)
    try:
        if variant == "blocked-from-0":
            assert e64.level_blocks(0) is not None
        if variant == "host-ldlt":
            assert e64.timing("coarse_on_device") == 0.0
        if variant == "jacobi":
            M = VcycleModel(e64, P.U, P.mass, P.lhs, oracle, e64.gs_omega, pre=pre, post=post, smoother="jacobi", jacobi_omega=0.67)
        else:
            M = VcycleModel(e64, P.U, P.mass, P.lhs, oracle, e64.gs_omega, pre=pre, post=post)
        _check_cycles(case, M, e64, e32, variant)
    finally:
        e64.close(); e32.close()


# ---------------------------------------------------------------------------------------------- (c): exact engine against the oracle itself
@pytest.mark.parametrize("pair", PAIRS, ids=_pid)
def test_exact_engine_matches_the_oracle_on_the_same_ordering(case, oracle, pair):
    """block_rows = 0, gs_omega = 1: Gauss-Seidel in colour order on every level is the reference's lexicographic sweep on P A P^T, so the oracle
    itself -- with the same pre_iters / post_iters -- is the reference.  Bounds of test_vcycle_matches_oracle_with_same_ordering."""
    pre, post = pair
    P = case.P
    eng = case.new_engine(pre, post, block_rows=0, gs_omega=1.0)
    try:
        O, order0 = colour_permuted_hierarchy(P, eng, oracle, pre_iters=pre, post_iters=post)
        for d in case.ds:
            b = case.rhs(d)
            got = eng.vcycle(b, b.copy())
            want_p = O.vcycle(b[order0], b[order0].copy())
            want = np.empty_like(want_p); want[order0] = want_p
            assert np.linalg.norm(P.lhs @ (got - want)) <= 1e-12 * case.nA * np.linalg.norm(want), d
            assert rel(got, want) <= (1e-12 if case.smoothing else 1e-6), (d, rel(got, want))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- (d): the residue the engine reports
@pytest.mark.parametrize("pair", PAIRS, ids=_pid)
def test_reported_residues_are_the_oracles_of_the_model_iterates(case, oracle, pair):
    """gmg_run_cycles: hist[i] against oracle.residual_check of the model's i-th iterate from x0 = rhs, for every norm type; and against the
    oracle's residue of the iterate the engine hands back.  The norm folded into the last colour launch (post > 0) and the separate norm launch
    (post = 0) answer to the same reference.  Bounds of tests/test_gpu_cycle_model.py."""
    pre, post = pair
    P, eng = case.P, case.engine(pre, post)
    for d in case.ds:
        b = case.rhs(d)
        xs, _ = case.chain(pre, post, d, upto=np.inf)
        for t in range(4):
            eng.load_problem(b, b)
            hist = eng.run_cycles(3, t).copy()
            xg = eng.fetch_solution()
            want = [oracle.residual_check(P.lhs, P.mass, b, xs[i], t) for i in range(3)]
            for i in range(3):
                bound = 1e-9 * want[i] + 1e-12 if case.smoothing else 1e-7
                assert abs(hist[i] - want[i]) <= bound, (d, t, i, hist[i], want[i])
            own = oracle.residual_check(P.lhs, P.mass, b, xg, t)
            assert abs(hist[2] - own) <= (1e-9 * own + 1e-12 if case.smoothing else 1e-7), (d, t, hist[2], own)


# ---------------------------------------------------------------------------------------------- (e): solves
TOLS = (1e-4, 3e-5)


def _model_solve(case, pre, post, d):
    """(tol, residues of the model's cycles up to the stop): the first of TOLS that no residue of the model's own iteration comes within 1 % of
    (a condition on the input -- the engine's residues agree with the model's to a tenth of that, so both sides take the same decision at every
    cycle); the iteration stops at the first residue <= tol or after 100 cycles."""
    _, res = case.chain(pre, post, d, upto=0.98 * min(TOLS))
    for tol in TOLS:
        stop = next((i for i, r in enumerate(res) if r <= tol), len(res) - 1)
        upto = res[:stop + 1]
        if all(abs(r - tol) > 0.01 * tol for r in upto):
            return tol, upto
    raise AssertionError(("every tolerance has a model residue within 1 %", case.name, pre, post, d, res))


@pytest.mark.parametrize("pair", [p for p in PAIRS if p != (0, 0)], ids=_pid)
def test_solve_takes_the_models_number_of_cycles(case, pair):
    pre, post = pair
    eng = case.engine(pre, post)
    for d in case.ds:
        b = case.rhs(d)
        tol, want = _model_solve(case, pre, post, d)
        x, it, res, conv = eng.solve(b, tol=tol, stop_type=2, max_iter=100)
        print("solve %s %d+%d d=%d tol=%g: model %d cycles (last %.3e), engine %d (last %.3e)" % (case.name, pre, post, d, tol, len(want), want[-1], it, res))
        assert it == len(want), (d, tol, it, len(want), conv[:, 1], want)
        if want[-1] <= tol:
            assert res <= tol
        else:                       # the model alone does not get there in 100 cycles: both sides stop at max_iter
            assert it == 100 and res > tol
        assert res == conv[-1, 1] and conv.shape == (it, 2)
        for i in range(it):
            assert abs(conv[i, 1] - want[i]) <= 1e-3 * want[i] + 1e-7, (d, i, conv[i, 1], want[i])


def test_solve_without_any_smoothing_runs_max_iter_cycles(case):
    """0 + 0: the coarse-grid correction alone does not contract.  The loop runs its max_iter cycles, reports the model's residues, and says
    "diverged" by its documented rule (above the tolerance and larger than after the first cycle)."""
    eng = case.engine(0, 0)
    for d in case.ds:
        b = case.rhs(d)
        _, want = case.chain(0, 0, d, upto=np.inf)
        assert min(want[:3]) > 1e-4 * 1.01
        x, it, res, conv = eng.solve(b, tol=1e-4, stop_type=2, max_iter=3)
        assert it == 3 and conv.shape == (3, 2) and res == conv[-1, 1]
        bound = [1e-3 * want[i] + 1e-7 for i in range(3)]
        for i in range(3):
            assert abs(conv[i, 1] - want[i]) <= bound[i], (d, i, conv[i, 1], want[i])
        # (the second and third cycle of a pure projection change the residue by rounding only: where the model's own residues do not separate
        # the first from the last cycle, the rule is applied to the residues the engine reported)
        if abs(want[2] - want[0]) > 2 * (bound[0] + bound[2]):
            grew = want[2] > want[0]
        else:
            grew = conv[2, 1] > conv[0, 1]
        assert eng.timing("diverged") == (1.0 if grew else 0.0) and eng.diverged == grew, (d, conv[:, 1], want[:3])


# ---------------------------------------------------------------------------------------------- (f): launch switches stay invisible
@pytest.mark.parametrize("pair", PAIRS, ids=_pid)
def test_head_and_fused_restriction_engage_only_with_pre_smoothing(case, pair):
    pre, post = pair
    eng = case.engine(pre, post)
    for d in case.ds:
        b = case.rhs(d)
        eng.solve(b, tol=1e-30, stop_type=2, max_iter=3)
        eng.load_problem(b, b); eng.run_cycles(2, 2)
    heads, fused = engaged(eng, "speculate_head"), engaged(eng, "fuse_restrict_sweep")
    if pre == 0:
        assert heads == 0 and fused == 0, (heads, fused)
    else:
        if case.name == "A-chain193-L3":
            assert fused > 0, fused
        if case.name == "A-chain64-L1":
            assert heads > 0, heads
    if len(case.P.U) == 1:
        assert fused == 0, fused


@pytest.mark.parametrize("pair", BITWISE_PAIRS, ids=_pid)
@pytest.mark.parametrize("switch", SWITCHES)
def test_switches_change_nothing(case, switch, pair):
    """speculate_head, fuse_restrict_sweep, uniform_slices, fine_col16 change how the cycle is launched, never what it computes: iterates,
    iteration counts and histories bit for bit with the switch on and off, at counts where the switched code takes its other branches."""
    pre, post = pair
    out = []
    for on in (1, 0):
        eng = case.new_engine(pre, post, **{switch: on})
        try:
            res = {}
            for d in case.ds:
                b = case.rhs(d)
                for name, tol, max_iter in (("to the tolerance", 1e-6, 60), ("max_iter", 1e-30, 3), ("first cycle is enough", 1e3, 100)):
                    x, it, r, conv = eng.solve(b, tol=tol, max_iter=max_iter)
                    res[(name, d)] = (x.copy(), it, r, conv[:, 1].copy())
                eng.load_problem(b, b)
                hist = eng.run_cycles(3, 2).copy()
                res[("run_cycles", d)] = (eng.fetch_solution().copy(), 3, 0.0, hist)
            ran = engaged(eng, switch)
            if not on:
                assert ran == 0, (switch, ran)
            elif pre == 0 and switch in ("speculate_head", "fuse_restrict_sweep"):
                assert ran == 0, (switch, ran)
            out.append(res)
        finally:
            eng.close()
    a, b = out
    for key in a:
        assert a[key][1] == b[key][1] and a[key][2] == b[key][2], key
        assert np.array_equal(a[key][3], b[key][3]), key
        assert np.array_equal(a[key][0], b[key][0]), key


# ---------------------------------------------------------------------------------------------- (g): gmg_profile_cycle runs ordinary cycles
@pytest.mark.parametrize("pair", [(0, 2), (2, 0), (1, 1)], ids=_pid)
def test_profile_cycle_moves_the_iterate_like_run_cycles(cabi, pair):
    """d = 3 on the smoothing torus: gmg_profile_cycle has its own copy of the condition under which the prolongation into level 0 reads the
    interleaved copy the last post-sweep of level 1 left (none without post-smoothing)."""
    pre, post = pair
    P = problems.torus_problem(96, 80, "smoothing", 30)
    assert P.rhs.shape[1] == 3

    def engine():
        e = cabi.Engine(pre_iters=pre, post_iters=post)
        e.set_prolongations(P.U); e.set_mass(P.mass); e.set_system(P.lhs); e.load_problem(P.rhs, P.rhs)
        return e
    a, b = engine(), engine()
    try:
        legs = a.profile_cycle(2, 3)
        b.run_cycles(3, 2)
        assert legs.shape == (a.num_levels + 2,)
        assert np.array_equal(a.fetch_solution(), b.fetch_solution())
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- partitioned cycle
P2P_PAIRS = [(0, 2), (1, 1), (2, 0), (3, 1), (0, 0)]


def _p2p_engine(cabi, P, world, pre, post, **kw):
    return cabi.Engine(pre_iters=pre, post_iters=post, row_align=64 * world, block_lanes=1, **kw)


def _p2p_worker(rank, world, port, q, kind, shard, partition):
    """Every pair of P2P_PAIRS on one process group: an engine with the pair's counts, connected through gmg_p2p, 3 cycles and a fetch.  No
    assertion between collectives (a rank that leaves early shows up on the others as a time-out): the parent compares."""
    try:
        sys.path.insert(0, ROOT)
        os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
        os.environ["LOCAL_WORLD_SIZE"] = str(world)
        import torch.distributed as dist
        from gravo_mg_amd import cabi
        from tests.test_gpu_p2p import _problem
        from tests.test_gpu_sweep_counts import P2P_PAIRS, _p2p_engine
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        P = _problem(kind)
        d = P.rhs.shape[1] if P.rhs.ndim == 2 else 1
        out = {}
        for pre, post in P2P_PAIRS:
            eng = _p2p_engine(cabi, P, world, pre, post, dist_shard_levels=shard)
            if partition:
                eng.dist_partition(rank, world)
            eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
            rk = cabi.P2PCycle(eng, rank, world, d)
            part1 = rk.stat("level1_partitioned")
            blobs = [None] * world
            dist.all_gather_object(blobs, rk.export())
            rk.connect(blobs=blobs)
            dist.barrier()
            rk.load(P.rhs, P.rhs)
            hist = rk.cycles(3, 2)
            x = rk.fetch()
            dist.barrier()
            out[(pre, post)] = (np.array(hist), np.array(x), part1)
            del rk
            eng.close()
        q.put((rank, out, None))
        dist.destroy_process_group()
    except Exception as e:              # noqa: BLE001
        import traceback
        q.put((rank, None, traceback.format_exc() + repr(e)))


@pytest.mark.parametrize("world,kind,shard,partition", [(2, "poisson", 2, False), (3, "poisson", 1, False), (3, "smoothing-d3", 2, False), (2, "smoothing-d3", 1, False),
                                                        (2, "cloud", 2, False), (3, "cloud", 1, False), (3, "poisson", 2, True)])
def test_partitioned_cycle_at_other_sweep_counts(cabi, world, kind, shard, partition):
    """The partitioned cycle carries its own copies of the sweep-count logic (p2p_smooth_level1: ping-pong, first sweep fused with the restriction,
    residual from the last sweep; p2p_smooth; the sharded coarse cycle).  As in test_processes_through_ipc_handles: histories to 1e-12 and iterates
    bit for bit against one handle doing everything with the same counts -- which the checks above hold to the model (block_lanes = 1 among them)."""
    import torch.multiprocessing as mp
    from tests.test_gpu_p2p import _problem
    P = _problem(kind)
    want = {}
    for pre, post in P2P_PAIRS:
        ref = _p2p_engine(cabi, P, world, pre, post)
        ref.set_prolongations(P.U); ref.set_mass(P.mass); ref.set_system(P.lhs)
        ref.load_problem(P.rhs, P.rhs)
        hist = ref.run_cycles(3, 2).copy()
        want[(pre, post)] = (hist, ref.fetch_solution().copy())
        ref.close()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_p2p_worker, args=(r, world, port, q, kind, shard, partition)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(60)
    errs = [f"rank {rank}: {err}" for rank, out, err in got if err is not None]
    assert not errs, "\n".join(sorted(errs, key=lambda e: "timed out" in e))
    for rank, out, err in got:
        for pair in P2P_PAIRS:
            hist, x, part1 = out[pair]
            assert part1 == (1.0 if shard == 2 else 0.0), (rank, pair)
            np.testing.assert_allclose(hist, want[pair][0], rtol=1e-12, err_msg=str((rank, pair)))
            assert np.array_equal(x, want[pair][1]), (rank, pair)
