"""The model behind tests/test_gpu_mixed_operators.py, checked on the host (no GPU): an honest float32 evaluation of every operation stays
inside the model's bounds on every catalogue case, in stored order and reversed; the exact twins pass the exactness condition at the sweep
counts the GPU test uses and float32 then reproduces the model's bits; a float32 evaluation with one injected defect leaves the bound or
breaks the equality.  Level orderings come from the host planner (gmg_host_plan_level), operators from the host Galerkin product."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from tests import mixed_cases as mc
from tests import mixed_model as mm

D = 2


def _default_omega(cabi):
    cfg = cabi.GmgConfig()
    assert cabi.lib().gmg_config_default(C.byref(cfg)) == 0
    return float(cfg.gs_omega)


def host_model(cabi, P, fine="colour", coarse="block", smoother="gs", omega=None):
    """The model on the host planner's layouts: level 0 colour-major or in 64-row blocks, the Galerkin levels likewise."""
    A = [sp.csc_matrix(P.lhs)]
    for u in P.U:
        A.append(cabi.host_galerkin(A[-1], sp.csc_matrix(u)))
    layouts = []
    for k in range(len(P.U)):
        if (fine if k == 0 else coarse) == "colour":
            plan = cabi.host_plan_level(A[k], mode=0)
            layouts.append(mm.layout_from_plan(plan["new2old"], plan["color_begin"]))
        else:
            plan = cabi.host_plan_level(A[k], mode=1, block_rows=64)
            layouts.append(mm.layout_from_plan(plan["new2old"], None, (plan["blk_begin"], plan["row_color"])))
    return mm.MixedModel(A, P.U, layouts, _default_omega(cabi) if omega is None else omega, smoother)


def _inside(got, res, what):
    err = np.abs(got - res.value)
    assert np.all(err <= res.bound), (what, float((err - res.bound).max()))


def _delta_residual_f32(sw, x_old, x_new, reverse):
    """The residual straight after a block sweep as residual_delta_ep forms it: the couplings that read the sweep's input, applied to
    x_old - x_new, in float32."""
    r, c, v = sw.entries
    keep = ~sw.reads_new
    E = sp.csr_matrix((v[keep], (r[keep], c[keep])), shape=(len(sw.diag),) * 2)
    diff = x_old.astype(np.float32) - x_new.astype(np.float32)
    return mm.product_f32(E, diff.astype(np.float64), reverse=reverse)


LAYOUTS = [("colour", "block", "gs"), ("block", "block", "gs"), ("colour", "colour", "gs"), ("colour", "block", "jacobi")]


@pytest.mark.parametrize("case", mc.CASES, ids=[c.name for c in mc.CASES])
def test_float32_stays_inside_every_bound(cabi, case):
    P = case.problem()
    rng = np.random.default_rng(21)
    for li, (fine, coarse, smoother) in enumerate(LAYOUTS if case.all_variants else LAYOUTS[:1]):
        M = host_model(cabi, P, fine, coarse, smoother)
        for reverse in (False, True):
            for k in range(M.L):
                n, nc = M.A[k].shape[0], M.A[k + 1].shape[0]
                b, x, e = case.block(rng, n, D), case.block(rng, n, D), case.block(rng, nc, D)
                if li == 0:
                    _inside(mm.product_f32(M.A[k], x, reverse=reverse), M.spmv(k, x), ("spmv", k))
                    _inside(mm.product_f32(M.A[k], x, add=b, sign=-1.0, reverse=reverse), M.residual(k, b, x), ("residual", k))
                    _inside(mm.product_f32(M.UT[k], b, reverse=reverse), M.restrict(k, b), ("restrict", k))
                    _inside(mm.product_f32(M.U[k], e, add=x, reverse=reverse), M.prolong_add(k, e, x), ("prolong_add", k))
                sw = M.sweeps[k]
                for iters in mc.ITERS:
                    for from_zero in (False, True):
                        x0 = np.zeros_like(x) if from_zero else x
                        swept = M.smooth(k, b, x0, iters, from_zero=from_zero)
                        got = mm.smooth_f32(sw, b, x0, iters, reverse=reverse)
                        _inside(got, swept, ("smooth", fine, coarse, smoother, k, iters, from_zero, reverse))
                        r32 = mm.product_f32(M.A[k], got, add=b, sign=-1.0, reverse=reverse)
                        _inside(r32, M.residual_behind(k, b, got, swept, False), ("residual behind", k, iters))
                        if M.layouts[k][0] == "block" and smoother == "gs":
                            before = mm.smooth_f32(sw, b, x0, iters - 1, reverse=reverse)
                            _inside(_delta_residual_f32(sw, before, got, reverse), M.residual_behind(k, b, got, swept, True),
                                    ("residual from the sweep", k, iters, from_zero))
            if li == 0:
                b, x = rng.standard_normal((P.n, D)), rng.standard_normal((P.n, D))
                A0 = M.A64[0]
                cols, _ = mm._padded(A0, reverse)          # (the fp64 residual, row sums in stored order or reversed, then rounded to float32)
                acc = np.zeros_like(b)
                for j in range(cols.shape[1]):
                    acc += _entry(A0, reverse, j) * x[cols[:, j]]
                _inside(mm.f32(b - acc).astype(np.longdouble), M.defect(b, x), ("defect", reverse))


def _entry(A, reverse, j):
    """Column j of the padded float64 values of A's rows (stored order or reversed), n x 1."""
    cnt = np.diff(A.indptr)
    src = A.indptr[:-1] + (cnt - 1 - j if reverse else j)
    ok = j < cnt
    return np.where(ok, A.data[np.where(ok, src, 0)], 0.0)[:, None]


EXACT = [c for c in mc.CASES if c.exact]


@pytest.mark.parametrize("case", EXACT, ids=[c.name for c in EXACT])
def test_exact_twins_pass_the_exactness_condition(cabi, case):
    """Products on every level and level-0 sweeps at the catalogued counts, on the colour-major and on the blocked level 0: the model verifies
    the condition, and float32 in either order gives the model's bits."""
    P = case.problem()
    assert np.array_equal(P.lhs.data, np.round(P.lhs.data)) and np.all(np.frexp(P.lhs.diagonal())[0] == 0.5)
    rng = np.random.default_rng(22)
    for fine in ("colour", "block"):
        M = host_model(cabi, P, fine, "block", omega=1.0)          # (the GPU test creates the exact twins' engines with gs_omega = 1)
        for k in range(M.L):
            n, nc = M.A[k].shape[0], M.A[k + 1].shape[0]
            assert np.array_equal(M.A[k].data, np.round(M.A[k].data)) and np.array_equal(M.A[k].data, M.A64[k].data)
            b, x, e = case.block(rng, n, D), case.block(rng, n, D), case.block(rng, nc, D)
            for reverse in (False, True):
                for res, got in ((M.spmv(k, x), mm.product_f32(M.A[k], x, reverse=reverse)),
                                 (M.residual(k, b, x), mm.product_f32(M.A[k], x, add=b, sign=-1.0, reverse=reverse)),
                                 (M.restrict(k, b), mm.product_f32(M.UT[k], b, reverse=reverse)),
                                 (M.prolong_add(k, e, x), mm.product_f32(M.U[k], e, add=x, reverse=reverse))):
                    assert res.exact and np.array_equal(got, res.value), (fine, k, reverse)
        b, x = case.block(rng, P.n, D), case.block(rng, P.n, D)
        for iters in mc.EXACT_FINE_SWEEPS[case.name]:
            for from_zero in (False, True):
                x0 = np.zeros_like(x) if from_zero else x
                swept = M.smooth(0, b, x0, iters, from_zero=from_zero)
                assert swept.exact, (fine, iters, from_zero)
                for reverse in (False, True):
                    assert np.array_equal(mm.smooth_f32(M.sweeps[0], b, x0, iters, reverse=reverse), swept.value), (fine, iters, from_zero, reverse)


def test_the_model_refuses_to_call_an_inexact_stage_exact(cabi):
    """Non-integer inputs, a diagonal that is no power of two (the Galerkin levels), a relaxed sweep, and a sweep count past what float32
    holds: `exact` is False in each."""
    case = mc.BY_NAME["exact-chain193"]
    P = case.problem()
    M = host_model(cabi, P)
    rng = np.random.default_rng(23)
    b, x = case.block(rng, P.n, D), case.block(rng, P.n, D)
    assert M.sweeps[0].omega != 1.0 and not M.smooth(0, b, x, 1).exact            # (the default engine over-relaxes level 0)
    M.sweeps[0].omega = 1.0
    assert M.smooth(0, b, x, 2).exact and not M.smooth(0, b, x, 6).exact
    assert not M.smooth(0, b, x + 2.0 ** -30, 1).exact
    assert not M.residual(0, b, x + 2.0 ** -30).exact and not M.residual(0, b, mc.f32_block(rng, P.n, D)).exact
    n1 = M.A[1].shape[0]
    assert not np.all(np.frexp(M.A[1].diagonal())[0] == 0.5)
    assert not M.smooth(1, case.block(rng, n1, D), case.block(rng, n1, D), 1).exact


DEFECT_CASES = [c for c in mc.CASES if c.all_variants]


@pytest.mark.parametrize("kind", ["drop_last", "stale", "shift_col"])
@pytest.mark.parametrize("case", DEFECT_CASES, ids=[c.name for c in DEFECT_CASES])
def test_injected_defects_are_detected(cabi, case, kind):
    """One defect in a float32 evaluation -- a row that drops its last entry, one in-block lower entry that reads the stale value, one column
    shifted by one -- leaves the model's bound in the row it touches (and on an exact twin breaks the equality) in every sweep and, where it
    applies, every product of every level."""
    P = case.problem()
    rng = np.random.default_rng(24)
    for fine in ("colour", "block"):
        M = host_model(cabi, P, fine, "block", omega=1.0 if case.exact else None)          # (exact twins: engines with gs_omega = 1)
        for k in range(M.L):
            n = M.A[k].shape[0]
            for seed in range(3):
                b, x = case.block(rng, n, D), case.block(rng, n, D)
                if case.exact:          # (integers that differ between any two columns one or two apart, none of them zero: no defect cancels)
                    x = (np.arange(n) % 3 + 1.0)[:, None] + 3.0 * rng.integers(0, 2, (n, D))
                    b = (np.arange(n) % 3 + 1.0)[:, None] + 3.0 * rng.integers(0, 2, (n, D))
                # (right-hand sides of the size of the diagonal: the updated values are then as far apart as the inputs, and a coupling that reads
                # the wrong one of them changes its row by more than the row's rounding)
                b = M.sweeps[k].diag[:, None] * b
                made = mm.with_defect(M.sweeps[k], kind, seed)
                if made is None:
                    assert kind == "stale"              # (a level of one colour has no coupling that reads an updated value)
                    continue
                bad, row = made
                swept = M.smooth(k, b, x, 1)
                got = mm.smooth_f32(bad, b, x, 1)
                assert np.any(np.abs(got - swept.value) > swept.bound), (fine, k, kind, row)
                if k == 0 and 1 in mc.EXACT_FINE_SWEEPS.get(case.name, ()):
                    assert swept.exact and not np.array_equal(got, swept.value)
                if kind != "stale":
                    for Mx, v, res in ((M.A[k], x, M.spmv(k, x)), (M.UT[k], b, M.restrict(k, b))):
                        if Mx.shape[1] < 2:
                            continue
                        badM, row = mm.matrix_with_defect(Mx, kind, seed)
                        v = v.copy()
                        v[:, 0] += np.arange(len(v))   # (no two neighbouring entries equal: a shifted column changes the row's value)
                        res = mm.product(Mx, v)
                        got = mm.product_f32(badM, v)
                        assert np.any(np.abs(got - res.value)[row] > res.bound[row]), (fine, k, kind, row)
