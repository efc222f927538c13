"""Level 0's 16-bit column codes where a slice needs more than one window (gmgs::compress_cols, kernels.hip.hpp::row_dot_sel): every branch
of the set-up -- several windows of 8 192 columns, the second format of 32 windows of 2 048, a prefix of uncovered slices, uncovered slices
flagged one by one, the recode 8 -> 32, codes dropped -- on the synthetic operators of tests/colcode_cases.py.

Per case, for the operator and both transfers: the window bases and code words copied back from the device (Engine.debug_col16) equal the
plain model's (tests/colcode_model.py, fed with the device's own SELL arrays) exactly, and so do the timing keys; every level-0 operator and
the cycle give the bits of a handle on 32-bit indices (gmg_config::fine_col16 = 0: "the same columns in the same order"), and the operators
agree with scipy in float64 to the 1e-13 that tests/test_gpu_boundary_shapes.py asks of them.

Out of scope here: the multi-rank kernels that read codes (gs_color_push, partitioned handles); the fault knob's own tests
(tests/test_gpu_setup.py), which stay as they are; and the streamed variant of the code-reading kernels (non-temporal loads, the kernels'
C16 = 1 / 2), which needs more than 160 MB of fine operators -- these shapes keep their operators resident (asserted: fine_operators_resident
== 1), so they run C16 = 3 / 4 and leave the C16 = 1 / 2 instantiations of the multi-window decode untested."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import colcode_cases as cc
from tests import colcode_model as cm
from tests import problems
from tests.parity_checks import rel

pytestmark = pytest.mark.gpu

KEYS = {0: "col16_l0", 3: "col16_P_l0", 4: "col16_R_l0"}
DS = (1, 2, 3, 4, 5, 8)                     # both DotGroup widths and the column chunks of the launches


def _engine(cabi, P, lhs=None, **kw):
    e = cabi.Engine(**kw)
    e.set_prolongations(P.U); e.set_mass(P.mass); e.set_system(P.lhs if lhs is None else lhs)
    return e


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def model_of(eng, lhs, which, uniform_slices=True):
    """The model's verdict for a level-0 layout of eng, from the device's own SELL arrays (and, for the operator, the rows' stored lengths)."""
    s = eng.debug_sell(0, which)
    if which == 0:
        assert s["lpr"] == 1
        new2old, _ = eng.level_ordering(0)
        length = np.diff(sp.csr_matrix(lhs).indptr) - 1          # stored off-diagonal entries of a row (the diagonal is stored), zeros included
        real = cm.real_of_operator(s["slice_ptr"], np.where(new2old >= 0, length[np.maximum(new2old, 0)], 0))
    else:
        real = cm.real_of_transfer(s["val"])
    return cm.model(s["slice_ptr"], s["col"], real, uniform_slices)


def check_device_equals_model(eng, m, which):
    got = eng.debug_col16(which)
    key = KEYS[which]
    assert (got["windows"], got["mode"], got["uniform_width"]) == (m["windows"], m["mode"], m["uniform_width"]), (which, got, cc.describe(m))
    assert got["from"] == m["from"], (which, got["from"], m["from"])
    assert eng.timing(key) == (1.0 if m["windows"] else 0.0)
    assert eng.timing(key + "_failed_slices") == m["failed"] and eng.timing(key + "_mode") == m["mode"]
    assert eng.timing(key + "_windows") == m["windows"] and eng.timing(key + "_uniform_width") == m["uniform_width"]
    if m["windows"]:
        assert np.array_equal(got["win_base"], m["win_base"]), (which, np.flatnonzero((got["win_base"] != m["win_base"]).any(axis=1))[:8])
        w = m["written"]
        assert np.array_equal(got["col16"][w], m["words"][w]), (which, np.flatnonzero(got["col16"][w] != m["words"][w])[:8])
    else:
        assert got["col16"] is None and got["win_base"] is None
    return got


class Pair:
    def __init__(self, cabi, name):
        self.name, self.kw = name, cc.engine_settings(name)
        self.P = cc.problem(name)
        self.a = _engine(cabi, self.P, **self.kw)
        self.b = _engine(cabi, self.P, fine_col16=0, **self.kw)
        self.A = sp.csr_matrix(self.P.lhs)
        self.U = sp.csr_matrix(self.P.U[0])

    def close(self):
        self.a.close(); self.b.close()


@pytest.fixture(scope="module", params=list(cc.CASES))
def pair(request, cabi):
    assert cabi.device_count() > 0, "gpu tests need a HIP device"
    p = Pair(cabi, request.param)
    yield p
    p.close()          # (one case's handles at a time)


def test_set_up_equals_the_model_and_takes_the_cases_branch(pair):
    a, b = pair.a, pair.b
    assert a.timing("fine_operators_resident") == 1.0          # (the kernels' C16 = 3 / 4; see the module docstring)
    branch = {}
    for which in (0, 3, 4):
        m = model_of(a, pair.P.lhs, which)
        check_device_equals_model(a, m, which)
        branch[which] = cc.describe(m)
        assert b.timing(KEYS[which]) == 0.0 and b.debug_col16(which)["windows"] == 0
        if which == 0:
            cc.check_branch(pair.name, m)
    print(f"\n[branch] {pair.name}: A {branch[0]}  R {branch[4]}  P {branch[3]}")
    if pair.name == "span-edge":
        m = model_of(a, pair.P.lhs, 0)
        s = a.debug_sell(0, 0)
        H = cc.span_edge_half()
        wb = m["win_base"]
        cols1 = s["col"][s["slice_ptr"][1]:s["slice_ptr"][2]]
        assert list(m["needed"][:4]) == [9, 1, 2, 8]
        assert wb[1, 0] == H + 63 and cols1.max() == wb[1, 0] + 8191 and wb[1, 1] == wb[1, 0]      # a real column at base + span - 1 stays in its window
        assert wb[2, 1] == wb[2, 0] + 8192                                                        # a window opened at exactly base + span
    if pair.name in ("blocked-lane1",):
        assert a.level_blocks(0) is not None and branch[0]["windows"] > 0
    for which, what in EXPECT_TRANSFER.get(pair.name, ()):
        assert what(branch[which]), (pair.name, which, branch[which])


@pytest.mark.parametrize("d", DS)
def test_operators_give_the_32_bit_handles_bits_and_agree_with_scipy(pair, oracle, d):
    """spmv, residual, restrict, prolong_add, smooth (1 and 2 sweeps), smooth_residual (from zero and not), residual_norm types 0 .. 3: bit for
    bit the handle on 32-bit indices; the linear operators against scipy in float64 within 1e-13 relative, the residual of smooth_residual within
    1e-13 (|A||x| + |b|), the norms within the 1e-12 of tests/test_gpu_boundary_shapes.py::test_norms."""
    P, a, b, A, U = pair.P, pair.a, pair.b, pair.A, pair.U
    rng = np.random.default_rng(100 + d)
    n, n1 = P.n, U.shape[1]
    x = rng.standard_normal((n, d)); rhs = rng.standard_normal((n, d)); e1 = rng.standard_normal((n1, d))
    ya = a.spmv(0, x)
    assert same(ya, b.spmv(0, x)) and rel(ya, A @ x) <= 1e-13
    ra = a.residual(0, rhs, x)
    assert same(ra, b.residual(0, rhs, x)) and rel(ra, rhs - A @ x) <= 1e-13
    ca = a.restrict(0, x)
    assert same(ca, b.restrict(0, x)) and rel(ca, U.T @ x) <= 1e-13
    pa = a.prolong_add(0, e1, x)
    assert same(pa, b.prolong_add(0, e1, x)) and rel(pa, x + U @ e1) <= 1e-13
    for iters in (1, 2):
        assert same(a.smooth(0, rhs, x, iters), b.smooth(0, rhs, x, iters)), iters
        for from_zero in (False, True):
            xa, rra = a.smooth_residual(0, rhs, None if from_zero else x, iters, from_zero=from_zero)
            xb, rrb = b.smooth_residual(0, rhs, None if from_zero else x, iters, from_zero=from_zero)
            assert same(xa, xb) and same(rra, rrb), (iters, from_zero)
            scale = abs(A) @ abs(xa) + abs(rhs)
            assert np.abs(rra - (rhs - A @ xa)).max() <= 1e-13 * scale.max(), (iters, from_zero)
    for t in (0, 1, 2, 3):
        got = a.residual_norm(P.rhs[:, :d], x, t)
        assert got == b.residual_norm(P.rhs[:, :d], x, t), t
        want = oracle.residual_check(P.lhs, P.mass, P.rhs[:, :d], x, t)
        assert abs(got - want) <= 1e-12 * abs(want), t


# the transfers take whatever the level-1 numbering gives (made at hierarchy time; the planner entry of the host tests does not see it): the cases
# that are relied on for R in the format of 32 windows and for P with several windows in a slice
EXPECT_TRANSFER = {
    "flagged-32": ((4, lambda b: b["windows"] == 32 and b["max_used"] > 8 and b["mode"] == 1), (3, lambda b: b["max_used"] >= 2)),
    "dropped": ((4, lambda b: b["windows"] == 32 and b["mode"] == 2 and b["failed"] > 0), (3, lambda b: b["mode"] == 2 and b["max_used"] >= 2)),
    "prefix": ((4, lambda b: b["max_used"] >= 2), (3, lambda b: b["max_used"] >= 2)),
    "fused-restrict": ((4, lambda b: b["windows"] > 0 and b["max_used"] >= 2),),
}


VARIANTS = {"plain": dict(), "fp32-inner": dict(inner_precision=1), "graph": dict(use_graph=True), "no-speculation": dict(speculate_head=0)}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_cycles_give_the_32_bit_handles_bits(pair, cabi, variant):
    """run_cycles(3, 2) and the iterate, d = 1, 3, 4 (at d > 1 the transfers take the interleaved source): the code-reading handle against the
    32-bit one, also with the fp32 twins in the inner cycle, replayed from a captured graph, and without the speculative head."""
    P = pair.P
    if variant == "plain":
        a, b, made = pair.a, pair.b, []
    else:
        a = _engine(cabi, P, **dict(pair.kw, **VARIANTS[variant])); b = _engine(cabi, P, fine_col16=0, **dict(pair.kw, **VARIANTS[variant]))
        made = [a, b]
    try:
        fused0 = a.timing("restrict_sweeps_fused")
        for d in (1, 3, 4):
            hist = []
            for e in (a, b):
                e.load_problem(P.rhs[:, :d], P.rhs[:, :d])
                hist.append((e.run_cycles(3, 2), e.fetch_solution()))
            assert same(hist[0][0], hist[1][0]) and same(hist[0][1], hist[1][1]), d
            assert np.all(np.isfinite(hist[0][0])) and hist[0][0][-1] < hist[0][0][0]
        if pair.name == "fused-restrict" and variant != "graph":
            # level 1 has more than 65 536 rows: one lane per row, the entry-parallel sweep, and a restriction in the quad layout whose slices need
            # several windows (asserted with the set-up) -- restrict_sweep0<.., C16>; the other fused form does not take a coded restriction
            assert a.timing("restrict_sweeps_fused") > fused0 and a.debug_col16(4)["windows"] > 0
    finally:
        for e in made:
            e.close()


def test_solve_returns_the_32_bit_handles_iterate_and_count(pair, oracle):
    P = pair.P
    rhs = P.rhs[:, :3]
    xa, ita, resa, _ = pair.a.solve(rhs, tol=1e-8, stop_type=2, max_iter=100)
    xb, itb, resb, _ = pair.b.solve(rhs, tol=1e-8, stop_type=2, max_iter=100)
    assert ita == itb and same(xa, xb) and _bits(resa) == _bits(resb)
    assert resa <= 1e-8 and ita < 100
    assert abs(oracle.residual_check(P.lhs, P.mass, rhs, xa, 2) - resa) <= 1e-3 * resa + 1e-7


@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
def test_pointwise_smoothers_read_the_codes_too(pair, cabi, smoother):
    """The Jacobi sweep and cheby_step<.., C16> on level 0 against their twins on 32-bit indices: sweeps and cycles, d = 1 and 3."""
    if pair.name not in ("two-window", "flagged-8", "flagged-32"):
        return
    P = pair.P
    kw = dict(pair.kw, smoother=cabi.SMOOTHER_JACOBI if smoother == "jacobi" else cabi.SMOOTHER_CHEBYSHEV)
    a, b = _engine(cabi, P, **kw), _engine(cabi, P, fine_col16=0, **kw)
    try:
        # (a pointwise smoother keeps level 0 in its own order: another layout, and other windows, than the colour-major handle's)
        m = model_of(a, P.lhs, 0)
        got = check_device_equals_model(a, m, 0)
        assert got["windows"] > 0 and m["used"].max() >= 2
        print(f"\n[branch] {pair.name} {smoother}: A {cc.describe(m)}")
        rng = np.random.default_rng(8)
        for d in (1, 3):
            x = rng.standard_normal((P.n, d)); rhs = rng.standard_normal((P.n, d))
            for iters in (1, 2, 3):
                assert same(a.smooth(0, rhs, x, iters), b.smooth(0, rhs, x, iters)), (d, iters)
            for e in (a, b):
                e.load_problem(P.rhs[:, :d], P.rhs[:, :d])
            assert same(a.run_cycles(3, 2), b.run_cycles(3, 2)) and same(a.fetch_solution(), b.fetch_solution())
    finally:
        a.close(); b.close()


def _refreshed_values(lhs, seed=21):
    """New symmetric values on the pattern of lhs, a tenth of the stored off-diagonal entries exactly 0.0 (stored, not removed)."""
    A = sp.csc_matrix(lhs).copy()
    coo = A.tocoo()                                                     # (walks the CSC storage order)
    lo, hi = np.minimum(coo.row, coo.col).astype(np.int64), np.maximum(coo.row, coo.col).astype(np.int64)
    h = (lo * 2654435761 + hi * 40503 + seed) % 1000 / 1000.0          # the same number for (i, j) and (j, i)
    factor = np.where(lo == hi, 1.0, np.where(h < 0.1, 0.0, 0.6 + 0.4 * h))      # (off-diagonals shrink: still diagonally dominant)
    A.data = coo.data * factor
    assert (A.data == 0.0).sum() > 0 and A.nnz == sp.csc_matrix(lhs).nnz and abs(A - A.T).max() == 0.0
    return A


def test_values_only_refresh_keeps_the_codes_and_stored_zeros_stay_real(pair, cabi):
    """New symmetric values on the live pattern with stored off-diagonal zeros, through set_system (on two-window also through
    set_system_values_device): the refresh is values-only, the window bases and code words do not change -- a zero value does not turn a real
    entry of the operator into padding --, and operators and cycles give the bits of a fresh handle on 32-bit indices."""
    P, a = pair.P, pair.a
    lhs2 = _refreshed_values(P.lhs)
    before = {which: a.debug_col16(which) for which in (0, 3, 4)}
    fresh = None
    try:
        routes = ["set_system"] + (["device"] if pair.name == "two-window" else [])
        fresh = _engine(cabi, P, lhs=lhs2, fine_col16=0, **pair.kw)
        cold = _engine(cabi, P, lhs=lhs2, **pair.kw)          # a cold set-up on the values with zeros codes the same entries: what is real is not a value's business
        try:
            check_device_equals_model(cold, model_of(cold, lhs2, 0), 0)
            if before[0]["windows"]:
                got = cold.debug_col16(0)
                assert np.array_equal(got["win_base"], before[0]["win_base"]) and got["windows"] == before[0]["windows"]
        finally:
            cold.close()
        for route in routes:
            if route == "set_system":
                a.set_system(lhs2)
            else:
                import torch
                a.set_system(P.lhs)
                vals = torch.tensor(lhs2.data, device="cuda:0")
                torch.cuda.synchronize()
                a.set_system_values_device(vals.data_ptr(), vals.numel())
            assert a.timing("setup_values_only") == 1.0, route
            for which in (0, 3, 4):
                now = a.debug_col16(which)
                assert {k: now[k] for k in ("windows", "mode", "from", "uniform_width")} == {k: before[which][k] for k in ("windows", "mode", "from", "uniform_width")}
                if now["windows"]:
                    assert np.array_equal(now["win_base"], before[which]["win_base"])
                check_device_equals_model(a, model_of(a, lhs2, which), which)
            rng = np.random.default_rng(9)
            for d in (1, 3):
                x = rng.standard_normal((P.n, d)); rhs = rng.standard_normal((P.n, d))
                assert same(a.spmv(0, x), fresh.spmv(0, x)) and rel(a.spmv(0, x), sp.csr_matrix(lhs2) @ x) <= 1e-13
                assert same(a.smooth(0, rhs, x, 2), fresh.smooth(0, rhs, x, 2)) and same(a.residual(0, rhs, x), fresh.residual(0, rhs, x))
                assert a.residual_norm(rhs, x, 2) == fresh.residual_norm(rhs, x, 2)
                for e in (a, fresh):
                    e.load_problem(P.rhs[:, :d], P.rhs[:, :d])
                assert same(a.run_cycles(3, 2), fresh.run_cycles(3, 2)) and same(a.fetch_solution(), fresh.fetch_solution())
    finally:
        if fresh is not None:
            fresh.close()
        a.set_system(P.lhs)          # the case's handle goes back to its own system


# ---- one handle through all verdicts ------------------------------------------------------------------------------------------------
N_WALK = 120000


def _walk_links(step):
    n = N_WALK
    if step == "two-window":
        return np.arange(n - 9001), np.arange(n - 9001) + 9001
    if step == "prefix":
        rng = np.random.default_rng(11)
        return np.repeat(rng.choice(n, 5, replace=False), 40), rng.integers(0, n, 200)
    return cc.CASES[step][0]()[2:]


# (at this n the offset graphs all end on 32 windows, so the step back to 8 windows is the hub graph: a 32-bit prefix of one slice after the
# flagged 32-window system -- offset bits 11 -> 13, mode 2 -> 1, from 1 782 -> 1)
WALK = (("two-window", (8, 1)), ("dropped", (0, 0)), ("recode-32", (32, 1)), ("flagged-32", (32, 2)), ("prefix", (8, 1)), ("dropped", (0, 0)))


def test_one_handle_through_all_verdicts(cabi):
    """A single handle, n fixed, takes patterns whose operator ends on 8 windows / no codes / 32 windows mode 1 / 32 windows flagged / 8 windows
    behind a 32-bit prefix / no codes again: after every set_system its keys, copied-out arrays and cycle bits are those of a fresh handle (no stale window
    bases, offset bits, prefix length or uniform width)."""
    sizes = [N_WALK, N_WALK // 4, N_WALK // 40]          # (piecewise-constant prolongations, three levels: every laid-out level keeps rows the device builder takes)
    systems = {}
    for step, _ in WALK:
        if step not in systems:
            a, b = _walk_links(step)
            systems[step] = problems.synthetic_problem(("links", N_WALK, False, a, b), sizes, kind="smoothing", prolong=("pc",), d=3)
    first = systems[WALK[0][0]]
    walker = cabi.Engine(**cc.PINNED)
    walker.set_prolongations(first.U); walker.set_mass(first.mass)
    try:
        for step, (windows, mode) in WALK:
            P = systems[step]
            walker.set_system(P.lhs)
            fresh = cabi.Engine(**cc.PINNED)
            fresh.set_prolongations(first.U); fresh.set_mass(first.mass); fresh.set_system(P.lhs)      # (one mass for the whole walk: the norms weigh with it)
            try:
                for which in (0, 3, 4):
                    m = model_of(fresh, P.lhs, which)
                    if which == 0:
                        assert (m["windows"], m["mode"]) == (windows, mode) and (step != "prefix" or m["from"] > 0), (step, cc.describe(m))
                    got = check_device_equals_model(walker, m, which)
                    ref = fresh.debug_col16(which)
                    assert {k: got[k] for k in ("windows", "mode", "from", "uniform_width")} == {k: ref[k] for k in ("windows", "mode", "from", "uniform_width")}, (step, which)
                hist = []
                for e in (walker, fresh):
                    e.load_problem(P.rhs, P.rhs)
                    hist.append((e.run_cycles(2, 2), e.fetch_solution()))
                assert same(hist[0][0], hist[1][0]) and same(hist[0][1], hist[1][1]), step
            finally:
                fresh.close()
    finally:
        walker.close()


def test_a_set_up_that_falls_back_to_the_host_planner_reports_no_codes(cabi):
    """The prefix graph with smoothed prolongations: the hubs' level-1 rows have more than the 96 entries the device layout builder takes, the
    set-up is redone by the host planner, and host-planned layouts have no codes.  The keys must say so -- not what the abandoned device layout
    of the same call, or of an earlier system on the handle, had found -- and the handle computes what the 32-bit one does."""
    P = cc.problem(cc.FALLBACK, d=3)
    a, b = _engine(cabi, P, **cc.PINNED), _engine(cabi, P, fine_col16=0, **cc.PINNED)
    try:
        for which in (0, 3, 4):
            assert model_of(a, P.lhs, which)["windows"] > 0                       # (the device set-up WOULD code these layouts)
            assert a.debug_col16(which)["windows"] == 0 and a.debug_sell(0, which)["n_slices"] > 0
            for sfx in ("", "_failed_slices", "_mode", "_windows", "_uniform_width"):
                assert a.timing(KEYS[which] + sfx) == 0.0, (which, sfx)
        rng = np.random.default_rng(6)
        x = rng.standard_normal(P.rhs.shape)
        assert same(a.spmv(0, x), b.spmv(0, x)) and rel(a.spmv(0, x), sp.csr_matrix(P.lhs) @ x) <= 1e-13
        for e in (a, b):
            e.load_problem(P.rhs, P.rhs)
        assert same(a.run_cycles(3, 2), b.run_cycles(3, 2)) and same(a.fetch_solution(), b.fetch_solution())
    finally:
        a.close(); b.close()


def test_uniform_slices_on_and_off_on_the_ring(cabi):
    """ring-uniform: every row has four off-diagonal entries and no colour class is padded, so every slice is four entries wide and the kernels
    skip the slice pointers (gmg_config::uniform_slices) -- with slices of two windows.  Same bits with the switch off; the key says 4 and 0."""
    P = cc.problem("ring-uniform")
    on, off = _engine(cabi, P, uniform_slices=1, **cc.PINNED), _engine(cabi, P, uniform_slices=0, **cc.PINNED)
    try:
        assert on.timing("col16_l0_uniform_width") == 4.0 and off.timing("col16_l0_uniform_width") == 0.0
        assert on.debug_col16(0)["uniform_width"] == 4 and off.debug_col16(0)["uniform_width"] == 0
        for which in (0, 3, 4):
            check_device_equals_model(off, model_of(off, P.lhs, which, uniform_slices=False), which)
        assert model_of(on, P.lhs, 0)["used"].max() == 2
        rng = np.random.default_rng(4)
        for d in (1, 3, 8):
            x = rng.standard_normal((P.n, d)); rhs = rng.standard_normal((P.n, d))
            assert same(on.spmv(0, x), off.spmv(0, x)) and same(on.smooth(0, rhs, x, 2), off.smooth(0, rhs, x, 2))
            assert same(on.restrict(0, x), off.restrict(0, x)) and on.residual_norm(rhs, x, 2) == off.residual_norm(rhs, x, 2)
        for e in (on, off):
            e.load_problem(P.rhs, P.rhs)
        assert same(on.run_cycles(3, 2), off.run_cycles(3, 2)) and same(on.fetch_solution(), off.fetch_solution())
    finally:
        on.close(); off.close()
