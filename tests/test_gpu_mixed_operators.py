"""The fp32 inner cycle's kernels, operator by operator: every <float> instantiation the way down and the way up launch, run alone through
gmg_debug_f32_op (the cycle's own launch code on the fp32 twin arrays) and compared componentwise with tests/mixed_model.py -- the same
operation in float64 on the float32 operands, with a derived bound, and bit for bit on the exact twins (integer operators, power-of-two
diagonal), where float32 commits no rounding.  Catalogue and engine variants: tests/mixed_cases.py.  All inputs are float32 numbers, so the
conversions around the hooks are exact.

Per level, operation, number of right-hand sides and sweep count: every component inside the bound; equality where the model has verified
exactness; from_zero on and off; the fused restriction + first sweep against the unfused handle, bit for bit; one column alone against that
column of a block, bit for bit; residual_from_sweep as the fp64 hook reports it on the twin handle."""
import numpy as np
import pytest

from tests import colcode_cases
from tests import mixed_cases as mc
from tests import mixed_model as mm
from tests.parity_checks import engaged

pytestmark = pytest.mark.gpu

RATIOS = {}          # operation -> largest observed |device - model| / bound (reported by the last test; DESIGN.md quotes it)

OPERATOR_RUNS = [(c, v) for c, v in mc.runs() if not v.startswith("coarse-")]
COARSE_RUNS = [(c, v) for c in mc.CASES for v in (("default", "coarse-host", "coarse-triangle") if (c.all_variants or c.name.startswith("coarsest")) else ("default",))]


def _engine(cabi, P, **kw):
    eng = cabi.Engine(**kw)
    eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
    return eng


def _settings(case, variant):
    kw = dict(case.kw, **mc.VARIANTS[variant])
    if case.exact:
        kw["gs_omega"] = 1.0
    return kw


class Run:
    def __init__(self, cabi, case, variant):
        self.cabi, self.case, self.variant, self.kw = cabi, case, variant, _settings(case, variant)
        self.P = case.problem()
        self.eng = _engine(cabi, self.P, inner_precision=1, **self.kw)
        self.twin = _engine(cabi, self.P, **self.kw)                     # the same settings in fp64
        self.jacobi = self.kw.get("smoother") == cabi.SMOOTHER_JACOBI
        self.M = mm.MixedModel.from_engine(self.eng, self.P.U, "jacobi" if self.jacobi else "gs")
        self.L = len(self.P.U)

    def n(self, k):
        return self.M.A[k].shape[0]

    def close(self):
        self.eng.close(); self.twin.close()


@pytest.fixture(scope="module", params=OPERATOR_RUNS, ids=["%s-%s" % (c.name, v) for c, v in OPERATOR_RUNS])
def run(request, cabi):
    assert cabi.device_count() > 0, "gpu tests need a HIP device"
    r = Run(cabi, *request.param)
    yield r
    r.close()


def _check(got, res, op, ctx, must_be_exact=False):
    """Every component inside the model's bound; equality where the model verified exactness (must_be_exact: and it has to have)."""
    got = np.asarray(got)
    value = np.asarray(res.value)
    err = np.abs(got - value).astype(np.float64)
    bound = np.asarray(res.bound, np.float64)
    pos = bound > 0
    if pos.any():
        RATIOS[op] = max(RATIOS.get(op, 0.0), float((err[pos] / bound[pos]).max()))
    assert np.all(err <= bound), (op, ctx, float((err - bound).max()), np.argwhere(err > bound)[:4].tolist())
    if must_be_exact:
        assert res.exact, (op, ctx, "the model cannot verify exactness here")
    if res.exact:
        assert np.array_equal(got, value.astype(np.float64)), (op, ctx, np.argwhere(got != value)[:4].tolist())


def _last_column_alone(fn, args, block, ctx):
    """fn on the last column alone == that column of fn on the block, bit for bit (args: the n x d inputs)."""
    d = args[0].shape[1]
    if d > 1:
        alone = fn(*[a[:, d - 1:d] for a in args])
        alone = alone if isinstance(alone, tuple) else (alone,)
        block = block if isinstance(block, tuple) else (block,)
        for a, b in zip(alone, block):
            assert np.array_equal(a, b[:, d - 1:d]), ctx


def test_layout_is_the_one_the_variant_is_here_for(run):
    eng, v = run.eng, run.variant
    for k in range(run.L):
        blocked = eng.level_blocks(k) is not None
        if v == "multicolour" or run.jacobi:
            assert not blocked, k
        elif v == "blocked-fine" or k > 0:
            assert blocked, k
    if run.case.name == "clique65":
        assert eng.level_blocks(0) is None and eng.level_info(0)["n_colors"] == 65
    if run.case.name == "diagonal100":
        assert all(eng.level_info(k)["n_colors"] == 1 for k in range(run.L))
    if run.case.name.endswith("hub48x40"):
        A1 = eng.level_operator(1)
        assert np.diff(A1.indptr).max() == A1.shape[0] > 16          # (one level-1 row denser than kEpW)


def test_products(run):
    """launch_spmv<float> (modes 0 and 1), launch_restrict<float>, launch_prolong_add<float> on every level."""
    eng, M, case = run.eng, run.M, run.case
    rng = np.random.default_rng(31)
    for k in range(run.L):
        n, nc = run.n(k), run.n(k + 1)
        for d in case.ds:
            b, x, e = case.block(rng, n, d), case.block(rng, n, d), case.block(rng, nc, d)
            ctx = (case.name, run.variant, k, d)
            for op, fn, args, res in (("spmv", lambda x_: eng.spmv_f32(k, x_), (x,), M.spmv(k, x)),
                                      ("residual", lambda b_, x_: eng.residual_f32(k, b_, x_), (b, x), M.residual(k, b, x)),
                                      ("restrict", lambda r_: eng.restrict_f32(k, r_), (b,), M.restrict(k, b)),
                                      ("prolong_add", lambda e_, x_: eng.prolong_add_f32(k, e_, x_), (e, x), M.prolong_add(k, e, x))):
                got = fn(*args)
                _check(got, res, op, ctx, must_be_exact=case.exact)
                _last_column_alone(fn, args, got, (op,) + ctx)


def _must_be_exact(run, k, iters):
    return (run.case.exact and k == 0 and not run.jacobi and iters in mc.EXACT_FINE_SWEEPS[run.case.name])


def test_sweeps(run):
    """launch_smooth<float> on every level at 1 and 2 sweeps: gs_color<float>, the block sweeps (gs_block_ep / gs_block_csrout / gs_block4 /
    gs_block with fp32 values), jacobi_sweep<float>."""
    eng, M, case = run.eng, run.M, run.case
    rng = np.random.default_rng(32)
    for k in range(run.L):
        n = run.n(k)
        for d in case.ds:
            b, x = case.block(rng, n, d), case.block(rng, n, d)
            for iters in mc.ITERS:
                ctx = (case.name, run.variant, k, d, iters)
                got = eng.smooth_f32(k, b, x, iters)
                _check(got, M.smooth(k, b, x, iters), "smooth", ctx, must_be_exact=_must_be_exact(run, k, iters))
                _last_column_alone(lambda b_, x_: eng.smooth_f32(k, b_, x_, iters), (b, x), got, ctx)


def test_smooth_and_residual(run):
    """What the way down does on one level, in <float>: the sweeps (from the iterate, or from zero without a zero vector), then the residual
    from the sweep's explicit part (launch_residual_delta<float>) or from launch_spmv<float>, chosen as the fp64 hook chooses on the twin."""
    eng, twin, M, case = run.eng, run.twin, run.M, run.case
    rng = np.random.default_rng(33)
    from_sweep_seen = 0
    for k in range(run.L):
        n = run.n(k)
        for d in case.ds:
            b, x0 = case.block(rng, n, d), case.block(rng, n, d)
            for iters in mc.ITERS:
                for from_zero in (False, True):
                    ctx = (case.name, run.variant, k, d, iters, from_zero)
                    x, r = eng.smooth_residual_f32(k, b, x0, iters, from_zero=from_zero)
                    from_sweep = eng.timing("residual_from_sweep")
                    twin.smooth_residual(k, b, None if from_zero else x0, iters, from_zero=from_zero)
                    assert from_sweep == twin.timing("residual_from_sweep"), ctx
                    from_sweep_seen += int(from_sweep)
                    start = np.zeros_like(b) if from_zero else x0
                    assert np.array_equal(x, eng.smooth_f32(k, b, start, iters)), ctx
                    swept = M.smooth(k, b, start, iters, from_zero=from_zero)
                    _check(x, swept, "smooth", ctx, must_be_exact=_must_be_exact(run, k, iters))
                    _check(r, M.residual_behind(k, b, x, swept, from_sweep == 1.0), "residual_from_sweep" if from_sweep else "residual_behind_sweeps", ctx)
    if run.variant in ("lanes1-bcsr", "lanes4-rows128", "multicolour", "jacobi") or run.L < 2:
        assert from_sweep_seen == 0          # (only the entry-parallel sweep's storage has the explicit part; level 0 never takes it)
    if run.variant == "lanes1-ep":
        assert from_sweep_seen > 0


def test_restriction_with_first_pre_sweeps(run, cabi):
    """The restriction of r_k into level k + 1, that level's pre-smoothing from zero and its residual, as enqueue_down does through
    restrict_into -- restrict_sweep0<float> / gs_block4<float, .., FR> where fuse_restrict_sweep engages -- against the model stage by stage,
    and against a handle with the fusion switched off, bit for bit."""
    eng, M, case = run.eng, run.M, run.case
    if run.L < 2:
        return
    rng = np.random.default_rng(34)
    unfused = _engine(cabi, run.P, inner_precision=1, **dict(run.kw, fuse_restrict_sweep=False))
    try:
        before = engaged(eng, "fuse_restrict_sweep")
        for k in range(run.L - 1):
            n = run.n(k)
            for d in case.ds:
                r = case.block(rng, n, d)
                for iters in mc.ITERS:
                    ctx = (case.name, run.variant, k, d, iters)
                    b1, x1, r1 = eng.restrict_sweeps_f32(k, r, iters)
                    for a, u in zip((b1, x1, r1), unfused.restrict_sweeps_f32(k, r, iters)):
                        assert np.array_equal(a, u), ctx
                    _check(b1, M.restrict(k, r), "restrict", ctx, must_be_exact=case.exact)
                    assert np.array_equal(b1, eng.restrict_f32(k, r)), ctx
                    # (the sweeps start from the right-hand side the device formed: a float32 block, so the stages are checked one by one)
                    swept = M.smooth(k + 1, b1, None, iters, from_zero=True)
                    _check(x1, swept, "smooth", ctx)
                    assert np.array_equal(x1, eng.smooth_residual_f32(k + 1, b1, None, iters, from_zero=True)[0]), ctx
                    from_sweep = eng.timing("residual_from_sweep") == 1.0
                    _check(r1, M.residual_behind(k + 1, b1, x1, swept, from_sweep), "residual_from_sweep" if from_sweep else "residual_behind_sweeps", ctx)
        ran = engaged(eng, "fuse_restrict_sweep") - before
        assert engaged(unfused, "fuse_restrict_sweep") == 0
        if run.variant in ("unfused", "jacobi", "multicolour"):
            assert ran == 0, ran
        if case.name == "chain193-L3" and run.variant == "default":
            assert ran > 0, "the fused restriction + first sweep must engage on this shape"
    finally:
        unfused.close()


def test_defect_and_correction(run):
    """The fp64 steps around the inner cycle: residual_norm_slices<D, 1, C16> (b - A x in fp64, rounded into b32, and the norm sums of the same
    residual) and add_correction."""
    eng, twin, M, case = run.eng, run.twin, run.M, run.case
    rng = np.random.default_rng(35)
    n = run.n(0)
    for d in case.ds:
        b, x = rng.standard_normal((n, d)), rng.standard_normal((n, d))          # (fp64 inputs: this step is the fp64 one)
        res = M.defect(b, x)
        for t in (0, 1, 2, 3):
            b32, nrm = eng.defect_f32(b, x, t)
            assert np.array_equal(b32, mm.f32(b32)), (d, t)
            _check(b32.astype(np.longdouble), res, "defect", (case.name, run.variant, d, t))
            want = twin.residual_norm(b, x, t)
            assert abs(nrm - want) <= 1e-12 * abs(want), (d, t, nrm, want)
        e = mc.f32_block(rng, n, d)
        assert np.array_equal(eng.correct_f32(e, x), M.correct(e, x)), d


@pytest.mark.parametrize("case,variant", COARSE_RUNS, ids=["%s-%s" % (c.name, v) for c, v in COARSE_RUNS])
def test_coarse_conversions(cabi, case, variant):
    """enqueue_coarse_device<float> / coarse_host_roundtrip<float>: the solve is the fp64 one, so the result is float32 of the fp64 hook's
    result from the same float32 right-hand side, bit for bit -- dense inverse, its triangle, host LDL^T."""
    P = case.problem()
    kw = _settings(case, variant)
    eng, twin = _engine(cabi, P, inner_precision=1, **kw), _engine(cabi, P, **kw)
    try:
        want_device = 0.0 if variant == "coarse-host" else 1.0
        assert eng.timing("coarse_on_device") == want_device and twin.timing("coarse_on_device") == want_device
        rng = np.random.default_rng(36)
        nl = P.U[-1].shape[1]
        for d in case.ds:
            rc = case.block(rng, nl, d)
            got = eng.coarse_solve_f32(rc)
            assert np.array_equal(got, mm.f32(twin.coarse_solve(rc))), (case.name, variant, d)
            assert np.array_equal(eng.coarse_solve_f32(rc[:, d - 1:d]), got[:, d - 1:d]), (case.name, variant, d)
    finally:
        eng.close(); twin.close()


def test_level0_with_16_bit_column_codes(cabi):
    """The smallest multi-window case of tests/colcode_cases.py with inner_precision = 1: the C16 instantiations of the fp32 level-0 kernels
    (gs_color, spmv_full, transfer) and of residual_norm_slices<D, 1, C16>."""
    name = "two-window"
    assert min((colcode_cases.CASES[c][0]()[0], c) for c, v in colcode_cases.CASES.items() if v[3] and v[3].get("multi"))[1] == name
    P = colcode_cases.problem(name)
    eng = _engine(cabi, P, inner_precision=1, **colcode_cases.engine_settings(name))
    try:
        assert engaged(eng, "fine_col16") > 0
        M = mm.MixedModel.from_engine(eng, P.U)
        rng = np.random.default_rng(37)
        n, n1 = P.n, P.U[0].shape[1]
        for d in (1, 3):
            b, x, e = mc.f32_block(rng, n, d), mc.f32_block(rng, n, d), mc.f32_block(rng, n1, d)
            ctx = (name, d)
            _check(eng.spmv_f32(0, x), M.spmv(0, x), "spmv", ctx)
            _check(eng.residual_f32(0, b, x), M.residual(0, b, x), "residual", ctx)
            _check(eng.restrict_f32(0, b), M.restrict(0, b), "restrict", ctx)
            _check(eng.prolong_add_f32(0, e, x), M.prolong_add(0, e, x), "prolong_add", ctx)
            for iters in mc.ITERS:
                _check(eng.smooth_f32(0, b, x, iters), M.smooth(0, b, x, iters), "smooth", ctx + (iters,))
            b64, x64 = rng.standard_normal((n, d)), rng.standard_normal((n, d))
            _check(eng.defect_f32(b64, x64, 2)[0].astype(np.longdouble), M.defect(b64, x64), "defect", ctx)
    finally:
        eng.close()


def test_fused_restriction_into_an_entry_parallel_level(cabi):
    """restrict_sweep0<float>: the restriction fused with the first sweep of a level that runs the entry-parallel block sweep.  The default
    layout takes that sweep only on a level of more than 65 536 rows (one lane per row) below a quad-layout restriction: the "fused-restrict"
    shape of tests/colcode_cases.py, whose restriction also carries 16-bit column codes.  Against the unfused handle bit for bit, and against
    the model stage by stage."""
    name = "fused-restrict"
    P = colcode_cases.problem(name)
    kw = colcode_cases.engine_settings(name)
    eng = _engine(cabi, P, inner_precision=1, **kw)
    unfused = _engine(cabi, P, inner_precision=1, fuse_restrict_sweep=False, **kw)
    try:
        M = mm.MixedModel.from_engine(eng, P.U)
        rng = np.random.default_rng(38)
        for d in (1, 3):
            r = mc.f32_block(rng, P.n, d)
            for iters in mc.ITERS:
                ctx = (name, d, iters)
                before = engaged(eng, "fuse_restrict_sweep")
                b1, x1, r1 = eng.restrict_sweeps_f32(0, r, iters)
                assert engaged(eng, "fuse_restrict_sweep") == before + 1, ctx
                for a, u in zip((b1, x1, r1), unfused.restrict_sweeps_f32(0, r, iters)):
                    assert np.array_equal(a, u), ctx
                from_sweep = eng.timing("residual_from_sweep") == 1.0
                assert from_sweep, ctx                       # (the entry-parallel storage: the residual comes from the sweep's explicit part)
                _check(b1, M.restrict(0, r), "restrict", ctx)
                swept = M.smooth(1, b1, None, iters, from_zero=True)
                _check(x1, swept, "smooth", ctx)
                _check(r1, M.residual_behind(1, b1, x1, swept, True), "residual_from_sweep", ctx)
        assert engaged(unfused, "fuse_restrict_sweep") == 0
    finally:
        eng.close(); unfused.close()


def test_hooks_refuse_an_fp64_handle_and_bad_arguments(cabi):
    case = mc.BY_NAME["chain65-L2"]
    P = case.problem()
    x = np.ones((P.n, 1))
    eng = _engine(cabi, P)
    try:
        with pytest.raises(cabi.GmgError) as ei:
            eng.spmv_f32(0, x)
        assert ei.value.code == cabi.GMG_ERR_STATE
    finally:
        eng.close()
    eng = _engine(cabi, P, inner_precision=1)
    try:
        for call in (lambda: eng.spmv_f32(2, x), lambda: eng._f32_op(99, 0, x), lambda: eng.restrict_sweeps_f32(1, np.ones((eng.level_info(1)["n"], 1)), 1),
                     lambda: eng._f32_op(eng.F32_RESIDUAL, 0, x)):
            with pytest.raises(cabi.GmgError) as ei:
                call()
            assert ei.value.code == cabi.GMG_ERR_INVALID
        assert np.array_equal(eng.spmv_f32(0, x), mm.f32(eng.spmv_f32(0, x)))
    finally:
        eng.close()


def test_report_largest_error_to_bound_ratios():
    """Not a check of its own (every comparison above asserts ratio <= 1): prints what the run observed."""
    for op in sorted(RATIOS):
        print("largest |device - model| / bound, %-24s %.3f" % (op, RATIOS[op]))
        assert RATIOS[op] <= 1.0
