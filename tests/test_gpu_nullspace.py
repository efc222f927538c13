"""gmg_config::nullspace = 1 on a real device: symmetric positive semi-definite systems with the null space span{1} -- the pure
stiffness matrix S of a torus, no mass term.

What is held here:
  * the coarsest solve is the pseudo-inverse, entry by entry: gmg_coarse_solve on the columns of the identity against numpy.linalg.pinv of
    gmg_get_level_operator(L), all four coarse modes, fp64 and inner_precision = 1, n_L = 61 (below 64), 170 (no multiple of 16) and 1 049
    (17 blocks of inverse_col_sums): within 1e-10 of the largest entry of the pseudo-inverse, the host factor's bound
    (tests/test_nullspace_host.py); the fp32 twin as tests/test_gpu_mixed_operators.py holds the regular inverse: float32 of the fp64 result,
    bit for bit;
  * the set-up's claim check: the row-sum keys, the failing inputs and their codes, the values-only refresh on the host and from device memory;
  * solves on every kind of handle against the numpy model (tests/nullspace_model.py around tests/vcycle_model.py / tests/chebyshev_model.py
    with the engine's orderings): the iteration counts are the model's, x has zero mass-weighted mean, A x is the projected b to the reported
    residue, nullspace_rhs_defect is numpy's, and single cycles from identical input agree after centring within the bounds
    tests/test_gpu_parity.py / tests/test_gpu_chebyshev.py use on their well-conditioned system (backward 1e-12 |A| |x|, forward 1e-11);
  * PCG to 1e-8 against the dense least-squares solution: within 1e-6;
  * the columns of a d = 5 solve are those of d = 1 solves; a nullspace = 0 handle on S + M is untouched by a nullspace = 1 handle beside it."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import nullspace_model as nm
from tests import problems
from tests.chebyshev_model import ChebyshevModel
from tests.vcycle_model import VcycleModel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHEBYSHEV, JACOBI = 2, 1
SHAPES = {"torus37x29": (37, 29, 60), "torus24x20": (24, 20, 60), "three-level": (52, 46, 60), "big-coarse": (88, 72, 1000)}


def _problem(shape):
    n1, n2, lb = SHAPES[shape]
    return problems.torus_problem(n1=n1, n2=n2, lower_bound=lb)


@functools.lru_cache(maxsize=None)
def _S(shape):
    S = sp.csc_matrix(_problem(shape).S)
    S.sort_indices()
    return S


def _make(cabi, shape, lhs=None, mass=True, **kw):
    P = _problem(shape)
    eng = cabi.Engine(**kw)
    eng.set_prolongations(P.U)
    if mass:
        eng.set_mass(P.mass)
    eng.set_system(_S(shape) if lhs is None else lhs)
    return eng


@functools.lru_cache(maxsize=None)
def _engine(shape, cfg=()):
    from gravo_mg_amd import cabi
    return _make(cabi, shape, nullspace=1, **dict(cfg))


@functools.lru_cache(maxsize=None)
def _rhs(shape, d):
    """random with a constant added: 1^T b is far from zero"""
    P = _problem(shape)
    rhs = np.asfortranarray(P.mass[:, None] * np.random.default_rng(500 + d).standard_normal((P.n, d)) + 0.01 * (1.0 + np.arange(d)))
    rhs.setflags(write=False)
    return rhs


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---- the coarsest operator, entry by entry ----------------------------------------------------------------------------------------------

COARSE_CASES = ([(s, m, p) for s in ("three-level", "torus37x29") for m in (0, 1, 2, 3) for p in (0, 1)]
                + [("big-coarse", m, 0) for m in (0, 1, 2, 3)] + [("big-coarse", 3, 1)])


@pytest.mark.parametrize("shape,mode,prec", COARSE_CASES, ids=[f"{s}-mode{m}-prec{p}" for s, m, p in COARSE_CASES])
def test_coarse_solve_is_the_pseudo_inverse(cabi, shape, mode, prec):
    eng = _make(cabi, shape, nullspace=1, coarse_mode=mode, inner_precision=prec)
    try:
        L = eng.num_levels
        A = eng.level_operator(L)
        nl = A.shape[0]
        assert nl == {"three-level": 61, "torus37x29": 170, "big-coarse": 1049}[shape] and L == (2 if shape == "three-level" else 1)
        assert eng.timing("coarse_on_device") == (0.0 if mode == 0 else 1.0) and eng.timing("coarse_triangle") == (1.0 if mode == 3 else 0.0)
        ref = np.linalg.pinv(np.asarray(A.todense()), hermitian=True)
        scale = float(np.abs(ref).max())
        I = np.eye(nl)
        X = np.hstack([eng.coarse_solve(np.asfortranarray(I[:, c:c + 128])) for c in range(0, nl, 128)])
        err = float(np.abs(X - ref).max())
        print(f"NULLSPACE_COARSE {shape} mode {mode} prec {prec}: n_L = {nl}, max |X - pinv| = {err:.2e} of max |pinv| = {scale:.2e}; "
              f"pinned pivot {eng.timing('nullspace_pinned_pivot'):.2e}")
        assert err <= 1e-10 * scale
        assert np.abs(X.sum(axis=0)).max() <= 1e-10 * scale * nl and np.abs(X - X.T).max() <= 1e-10 * scale
        assert np.array_equal(_bits(eng.coarse_solve(np.asfortranarray(I[:, 5:6]))), _bits(np.asfortranarray(X[:, 5:6])))      # a column alone, a second call
        if prec:
            rc = np.asfortranarray(np.random.default_rng(8).standard_normal((nl, 3)).astype(np.float32).astype(np.float64))
            assert np.array_equal(eng.coarse_solve_f32(rc), eng.coarse_solve(rc).astype(np.float32).astype(np.float64))
    finally:
        eng.close()


# ---- set-up ---------------------------------------------------------------------------------------------------------------------------

def test_setup_keys(cabi):
    """The two row-sum figures are below the bound and of the model's magnitude (rounding of a row: below 100 eps), the replaced pivot is noise
    beside the pivots of A11; a nullspace = 0 handle writes none of the keys."""
    eng = _engine("torus37x29")
    f0, fc, piv = eng.timing("nullspace_rowsum_l0"), eng.timing("nullspace_rowsum_coarse"), eng.timing("nullspace_pinned_pivot")
    m0, mc = nm.rowsum_figure(_S("torus37x29")), nm.rowsum_figure(eng.level_operator(eng.num_levels))
    print(f"NULLSPACE_KEYS rowsum l0 {f0:.2e} (numpy {m0:.2e}) coarse {fc:.2e} (numpy {mc:.2e}) pinned pivot {piv:.2e}")
    assert eng.timing("nullspace") == 1
    assert f0 <= nm.ROWSUM_MAX and fc <= nm.ROWSUM_MAX and f0 <= 2.3e-14 and fc <= 2.3e-14
    assert abs(f0 - m0) <= 2.3e-14 and abs(fc - mc) <= 1e-15 and abs(piv) <= 1e-9
    P = _problem("torus37x29")
    plain = _make(cabi, "torus37x29", lhs=(P.S + sp.diags(P.mass)).tocsc())
    try:
        for key in ("nullspace", "nullspace_rowsum_l0", "nullspace_rowsum_coarse", "nullspace_pinned_pivot", "nullspace_rhs_defect"):
            with pytest.raises(cabi.GmgError):
                plain.timing(key)
    finally:
        plain.close()


def test_failing_inputs_leave_no_system(cabi):
    """A level 0 with a mass term: GMG_ERR_INVALID; prolongations with one row scaled by 1.01: GMG_ERR_NUMERIC; after either the handle has no
    system (GMG_ERR_STATE from a solve), and a good system afterwards works -- also when the bad one came as a values-only refresh."""
    P = _problem("torus37x29")
    rhs = _rhs("torus37x29", 1)
    eng = cabi.Engine(nullspace=1)
    try:
        eng.set_prolongations(P.U); eng.set_mass(P.mass)
        with pytest.raises(cabi.GmgError) as ei:
            eng.set_system((P.S + 1e-3 * sp.diags(P.mass)).tocsc())
        assert ei.value.code == cabi.GMG_ERR_INVALID and "A 1 != 0" in str(ei.value)
        with pytest.raises(cabi.GmgError) as ei:
            eng.solve(rhs)
        assert ei.value.code == cabi.GMG_ERR_STATE
        eng.set_system(_S("torus37x29"))
        assert eng.solve(rhs, tol=1e-4)[2] <= 1e-4
        with pytest.raises(cabi.GmgError) as ei:          # the same pattern: the values-only refresh repeats the check
            eng.set_system((P.S + 1e-3 * sp.diags(P.mass)).tocsc())
        assert ei.value.code == cabi.GMG_ERR_INVALID
        with pytest.raises(cabi.GmgError) as ei:
            eng.solve(rhs)
        assert ei.value.code == cabi.GMG_ERR_STATE
        U = [sp.csr_matrix(u).copy() for u in P.U]
        row = U[0].shape[0] // 2
        U[0].data[U[0].indptr[row]:U[0].indptr[row + 1]] *= 1.01
        eng.set_prolongations([sp.csc_matrix(u) for u in U]); eng.set_mass(P.mass)
        with pytest.raises(cabi.GmgError) as ei:
            eng.set_system(_S("torus37x29"))
        assert ei.value.code == cabi.GMG_ERR_NUMERIC and "preserve constants" in str(ei.value)
        with pytest.raises(cabi.GmgError) as ei:
            eng.solve(rhs)
        assert ei.value.code == cabi.GMG_ERR_STATE
    finally:
        eng.close()


def test_workaround_system_is_refused(cabi):
    """S + 1e-6 M on a nullspace = 1 handle is refused with GMG_ERR_INVALID at the bound of 1e-9 and leaves no system; S of the same mesh is
    accepted afterwards.  The mesh is the torus (37, 29) in units ten times larger (tests/test_nullspace_host.py::workaround_system says why: S
    does not change with the unit, the masses do, and on the unit torus 1e-6 M is 1.3e-10 of a row -- below what this bound can see)."""
    from tests.test_nullspace_host import workaround_system
    S, mass, lhs = workaround_system()
    P = _problem("torus37x29")              # (the same vertices and graph: its prolongations are this mesh's)
    rhs = _rhs("torus37x29", 1)
    eng = cabi.Engine(nullspace=1)
    try:
        eng.set_prolongations(P.U); eng.set_mass(mass)
        with pytest.raises(cabi.GmgError) as ei:
            eng.set_system(lhs)
        assert ei.value.code == cabi.GMG_ERR_INVALID and "A 1 != 0" in str(ei.value)
        with pytest.raises(cabi.GmgError) as ei:
            eng.solve(rhs)
        assert ei.value.code == cabi.GMG_ERR_STATE
        eng.set_system(S)
        assert eng.timing("nullspace_rowsum_l0") <= 2.3e-14 and eng.solve(rhs, tol=1e-4)[2] <= 1e-4
    finally:
        eng.close()


@pytest.mark.parametrize("mode", [0, 2, 3])
def test_refresh_with_twice_the_matrix_halves_the_solution(cabi, mode):
    """2 S as a values-only refresh through gmg_set_system and through gmg_set_system_values_device: check and centring are repeated, the
    solution from half the initial guess is half the first one (scaling by two is exact in every step, so to the bits; the stopping rule sees
    the same residues)."""
    torch = pytest.importorskip("torch")
    shape = "torus37x29"
    S = _S(shape)
    rhs = _rhs(shape, 3)
    eng = _make(cabi, shape, nullspace=1, coarse_mode=mode)
    try:
        x1, it1, res1, _ = eng.solve(rhs, x0=rhs, tol=1e-8, stop_type=2, max_iter=30)
        S2 = (2.0 * S).tocsc()
        eng.set_system(S2)
        assert eng.timing("setup_values_only") == 1 and eng.timing("nullspace_rowsum_l0") <= 2.3e-14
        x2, it2, res2, _ = eng.solve(rhs, x0=0.5 * rhs, tol=1e-8, stop_type=2, max_iter=30)
        assert it2 == it1 and _bits(res2) == _bits(res1) and np.array_equal(_bits(2.0 * x2), _bits(x1))
        vals = torch.tensor(np.ascontiguousarray(4.0 * S.data), device=DEV)
        torch.cuda.synchronize()
        eng.set_system_values_device(vals.data_ptr(), vals.numel())
        assert eng.timing("setup_values_only") == 1
        x4, it4, res4, _ = eng.solve(rhs, x0=0.25 * rhs, tol=1e-8, stop_type=2, max_iter=30)
        assert it4 == it1 and np.array_equal(_bits(4.0 * x4), _bits(x1))
        bad = torch.tensor(np.ascontiguousarray((S + 1e-3 * sp.diags(_problem(shape).mass)).tocsc().data), device=DEV)
        torch.cuda.synchronize()
        with pytest.raises(cabi.GmgError) as ei:
            eng.set_system_values_device(bad.data_ptr(), bad.numel())
        assert ei.value.code == cabi.GMG_ERR_INVALID
        with pytest.raises(cabi.GmgError) as ei:
            eng.solve(rhs)
        assert ei.value.code == cabi.GMG_ERR_STATE
    finally:
        eng.close()


# ---- solves ---------------------------------------------------------------------------------------------------------------------------

CHEB = (("smoother", CHEBYSHEV),)
SOLVE_CASES = {
    "default": (), "exact-gs": (("block_rows", 0), ("gs_omega", 1.0)), "chebyshev": CHEB, "jacobi": (("smoother", JACOBI),),
    "accelerate3": (("accelerate", 3),), "pcg": CHEB + (("pcg", 1),), "pcg-zero-guess": CHEB + (("pcg", 1), ("zero_guess_step", 1)),
    "graph": (("use_graph", True),), "mixed": (("inner_precision", 1),), "host-ldlt": (("coarse_mode", 0),), "triangle": CHEB + (("coarse_mode", 3),),
}


def _cycle_model(eng, shape, cfg, oracle):
    """The numpy model of the handle's cycle on S with the pseudo-inverse as its coarsest solve, with the engine's orderings."""
    P = _problem(shape)
    kw = dict(cfg)
    if kw.get("smoother") == CHEBYSHEV:
        M = ChebyshevModel(None, P.U, P.mass, _S(shape), oracle, eng.timing("cheby_ratio"))
    elif kw.get("smoother") == JACOBI:
        M = VcycleModel(eng, P.U, P.mass, _S(shape), oracle, 1.0, smoother="jacobi", jacobi_omega=0.67)
    else:
        M = VcycleModel(eng, P.U, P.mass, _S(shape), oracle, eng.gs_omega)
    return nm.with_pinv_coarse(M)


def _loop_of(cfg):
    kw = dict(cfg)
    return ("pcg", 0) if kw.get("pcg") else (("accelerate", kw["accelerate"]) if kw.get("accelerate") else ("plain", 0))


# every kind of handle on the 1 073-vertex torus; the three loops on their plainest handles on the other two shapes
SOLVE_RUNS = [(c, "torus37x29") for c in SOLVE_CASES] + [(c, s) for s in ("torus24x20", "three-level") for c in ("default", "chebyshev", "pcg")]


@pytest.mark.parametrize("case,shape", SOLVE_RUNS, ids=[f"{c}-{s}" for c, s in SOLVE_RUNS])
def test_solve_follows_the_model(cabi, oracle, case, shape):
    """d = 3, x0 = rhs, stop type 2, tol 1e-4 (1e-8 for the two PCG handles).  The count is the model's; the returned x has zero mass-weighted mean;
    A x is the projected b to the reported residue; the defect key is numpy's; x agrees with the model's after centring within 1e-6 of its
    largest entry (the bound tests/test_gpu_parity.py puts on a cycle of the regular Poisson system; measured on an MI355X: 6e-15 .. 4e-14 in
    fp64, 2.5e-11 with the fp32 inner cycle)."""
    cfg = SOLVE_CASES[case]
    P = _problem(shape)
    S = _S(shape)
    rhs = _rhs(shape, 3)
    eng = _engine(shape, cfg)
    loop, depth = _loop_of(cfg)
    tol = 1e-8 if loop == "pcg" else 1e-4
    x, it, res, conv = eng.solve(rhs, tol=tol, stop_type=2, max_iter=40)
    x = x.reshape(rhs.shape)
    M = _cycle_model(eng, shape, cfg, oracle)
    mx, mit, mres, _ = nm.nullspace_solve(S, P.mass, M.vcycle, rhs, rhs, 2, tol, 40, loop=loop, depth=depth)
    b = nm.project_rhs(rhs)
    r = b - S @ x
    chk = float(np.sqrt(((P.mass[:, None] * r * r).sum(axis=0) / (P.mass[:, None] * b * b).sum(axis=0)).max()))
    mean = float((np.abs(P.mass @ x) / (P.mass @ np.abs(x))).max())
    dev = _rel(x, mx)
    print(f"NULLSPACE_SOLVE {shape} {case}: {it} iterations (model {mit}), residue {res:.3e} (numpy {chk:.3e}, model {mres[-1]:.3e}), "
          f"|m^T x| / |m|^T |x| = {mean:.2e}, x against the model {dev:.2e}, defect {eng.timing('nullspace_rhs_defect'):.6e}")
    assert not eng.diverged and res <= tol
    assert it == mit
    assert mean <= 1e-12
    assert abs(chk - res) <= 1e-6 * res + 1e-13
    assert abs(eng.timing("nullspace_rhs_defect") - nm.rhs_defect(rhs)) <= 1e-12
    assert dev <= (2e-5 if case == "mixed" else 1e-6)          # (the fp32 inner cycle: the bound of tests/test_gpu_chebyshev.py for it)
    assert _bits(res) == _bits(conv[-1, 1])


@pytest.mark.parametrize("case", ["default", "exact-gs", "chebyshev", "jacobi", "host-ldlt"])
def test_single_cycles_match_the_model_after_centring(cabi, oracle, case):
    """Three consecutive cycles from identical input -- a solve of one iteration from the model's previous iterate -- against the model's cycle
    on the projected right-hand side, both centred: backward error within 1e-12 |A| |x| and forward error within 1e-11, the bounds of
    test_default_engine_vcycles_match_model_per_cycle / test_cycles_match_the_model -- the forward one that of their WELL-conditioned system
    (the smoothing problem), not the 1e-6 of S + 1e-6 M: on the complement of the constants S has a condition number of a few hundred, which is
    the point of the feature.  Measured on an MI355X: backward 7e-17, forward 1e-14 .. 2e-14."""
    shape = "torus37x29"
    cfg = SOLVE_CASES[case]
    P, S, rhs = _problem(shape), _S(shape), _rhs(shape, 3)
    eng = _engine(shape, cfg)
    M = _cycle_model(eng, shape, cfg, oracle)
    b = nm.project_rhs(rhs)
    nA = spla.norm(S)
    xm = np.array(rhs, order="F")
    worst = (0.0, 0.0)
    for cyc in range(3):
        xg = eng.solve(rhs, x0=xm, tol=0.0, stop_type=2, max_iter=1)[0].reshape(rhs.shape)
        xm = nm.centre(M.vcycle(b, xm), P.mass)
        back, fwd = float(np.linalg.norm(S @ (xg - xm)) / (nA * np.linalg.norm(xm))), _rel(xg, xm)
        worst = (max(worst[0], back), max(worst[1], fwd))
        assert back <= 1e-12 and fwd <= 1e-11, (cyc, back, fwd)
    print(f"NULLSPACE_CYCLE {case}: backward {worst[0]:.2e} forward {worst[1]:.2e}")


@pytest.mark.parametrize("shape", ["torus37x29", "three-level"])
def test_pcg_reaches_the_least_squares_solution(cabi, shape):
    """PCG to 1e-8 against the dense least-squares solution after centring: within 1e-6 of its largest entry (the model gives 1e-9 .. 4e-9; the
    margin covers the conditioning of S on the complement of the constants, a few hundred on these tori)."""
    P, S, rhs = _problem(shape), _S(shape), _rhs(shape, 3)
    eng = _engine(shape, SOLVE_CASES["pcg"])
    x, it, res, _ = eng.solve(rhs, tol=1e-8, stop_type=2, max_iter=40)
    ref = nm.least_squares_solution(S, nm.project_rhs(rhs), P.mass)
    dev = _rel(x.reshape(rhs.shape), ref)
    print(f"NULLSPACE_LSQ {shape}: {it} iterations, residue {res:.3e}, against least squares {dev:.3e}, guards {eng.timing('pcg_guard_steps'):.0f}")
    assert res <= 1e-8 and dev <= 1e-6 and eng.timing("pcg_guard_steps") == 0


@pytest.mark.parametrize("case", ["default", "chebyshev", "pcg"])
def test_columns_of_a_block_are_solved_as_if_alone(cabi, case):
    """d = 5 (two column groups) at a fixed iteration count against five d = 1 solves: every column within 1e-7 of its own solve, the bound
    tests/test_gpu_parity.py::test_more_than_four_right_hand_sides puts on the same comparison (the kernels of one column and of a group of
    four add in different orders: no bits are demanded there either); each column's mean is removed separately."""
    shape = "torus37x29"
    P, rhs = _problem(shape), _rhs(shape, 5)
    eng = _engine(shape, SOLVE_CASES[case])
    kw = dict(tol=0.0, stop_type=2, max_iter=6)
    xa = eng.solve(rhs, **kw)[0].reshape(rhs.shape)
    assert (np.abs(P.mass @ xa) / (P.mass @ np.abs(xa))).max() <= 1e-12
    for c in (0, 3, 4):
        x1 = eng.solve(np.asfortranarray(rhs[:, c:c + 1]), **kw)[0].reshape(-1)
        assert _rel(xa[:, c], x1) <= 1e-7, c
    assert eng.timing("nullspace_rhs_defect") == pytest.approx(nm.rhs_defect(rhs[:, 4:5]), abs=1e-12)       # (the last solve: one column)


def test_entry_points_give_the_same_bits(cabi):
    """gmg_solve with an explicit x0 = rhs, gmg_solve_x0_rhs and gmg_solve_device from torch tensors: the same projections, the same bits; without
    a mass the iterate is centred with unit weights."""
    torch = pytest.importorskip("torch")
    shape = "torus37x29"
    rhs = _rhs(shape, 3)
    n, d = rhs.shape
    for cfg in (SOLVE_CASES["default"], SOLVE_CASES["pcg"], SOLVE_CASES["mixed"]):
        eng = _engine(shape, cfg)
        kw = dict(tol=1e-9, stop_type=2, max_iter=6)
        x_a, it_a, res_a, conv_a = eng.solve(rhs, **kw)
        x_b, it_b, res_b, _ = eng.solve(rhs, x0=rhs.copy(), **kw)
        assert it_a == it_b and _bits(res_a) == _bits(res_b) and np.array_equal(_bits(x_a), _bits(x_b))
        b = torch.tensor(np.ascontiguousarray(rhs), device=DEV)
        x = torch.full((n, d), float("nan"), dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        it, res, conv = eng.solve_device(b.data_ptr(), b.stride(), x.data_ptr(), x.stride(), d, **kw)
        assert it == it_a and _bits(res) == _bits(res_a) and np.array_equal(_bits(conv[:, 1]), _bits(conv_a[:, 1]))
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(np.ascontiguousarray(x_a.reshape(rhs.shape))))
        assert np.array_equal(_bits(b.cpu().numpy()), _bits(np.ascontiguousarray(rhs)))          # the caller's right-hand side is not projected in place
    eng = _make(cabi, shape, mass=False, nullspace=1)
    try:
        x = eng.solve(rhs, tol=1e-6, stop_type=0, max_iter=30)[0].reshape(rhs.shape)
        assert (np.abs(x.sum(axis=0)) / np.abs(x).sum(axis=0)).max() <= 1e-12
    finally:
        eng.close()


def test_cycles_outside_the_solve_project_nothing(cabi):
    """gmg_vcycle and gmg_load_problem / gmg_run_cycles / gmg_fetch_solution on a nullspace = 1 handle leave b and x alone: a cycle on b + c 1 from
    x + c' 1 is the cycle on b + c 1 (no projection) -- its result differs from the cycle on the projected b."""
    shape = "torus37x29"
    rhs = _rhs(shape, 1)
    eng = _engine(shape)
    v1 = eng.vcycle(rhs, rhs)
    eng.load_problem(rhs, rhs)
    eng.run_cycles(1, 2)
    v2 = eng.fetch_solution()
    assert np.array_equal(_bits(v1), _bits(v2))
    vp = eng.vcycle(nm.project_rhs(rhs), rhs)
    assert _rel(v1, vp) > 1e-6


def test_a_regular_handle_is_untouched(cabi):
    """A nullspace = 0 handle on S + M: the bits of a handle from gmg_config_default untouched, with and without a nullspace = 1 handle alive
    and solving beside it."""
    shape = "torus37x29"
    P = _problem(shape)
    lhs = (P.S + sp.diags(P.mass)).tocsc()
    lhs.sort_indices()
    rhs = _rhs(shape, 3)
    kw = dict(tol=1e-9, stop_type=2, max_iter=6)
    a = _make(cabi, shape, lhs=lhs)
    try:
        ra = a.solve(rhs, **kw)
        other = _engine(shape)
        other.solve(rhs, **kw)
        b = _make(cabi, shape, lhs=lhs, nullspace=0)
        try:
            rb = b.solve(rhs, **kw)
            other.solve(rhs, **kw)
            ra2 = a.solve(rhs, **kw)
        finally:
            b.close()
        for r in (rb, ra2):
            assert r[1] == ra[1] and _bits(r[2]) == _bits(ra[2]) and np.array_equal(_bits(r[0]), _bits(ra[0])) and np.array_equal(_bits(r[3][:, 1]), _bits(ra[3][:, 1]))
    finally:
        a.close()


def test_multi_rank_entry_points_refuse_it(cabi):
    eng = _engine("torus37x29")
    with pytest.raises(cabi.GmgError) as ei:
        eng._chk(cabi.lib().gmg_p2p_prepare(eng._h, 0, 2, 1))
    assert ei.value.code == cabi.GMG_ERR_UNSUPPORTED and "nullspace" in str(ei.value)
    with pytest.raises(cabi.GmgError) as ei:
        eng._chk(cabi.lib().gmg_dist_setup(eng._h, 0, 2))
    assert ei.value.code == cabi.GMG_ERR_UNSUPPORTED
    fresh = cabi.Engine(nullspace=1, row_align=128)
    try:
        with pytest.raises(cabi.GmgError) as ei:
            fresh._chk(cabi.lib().gmg_dist_partition(fresh._h, 0, 2))
        assert ei.value.code == cabi.GMG_ERR_UNSUPPORTED
        fresh._chk(cabi.lib().gmg_dist_partition(fresh._h, 0, 1))
    finally:
        fresh.close()


def test_tiny_systems(cabi):
    """The 2-vertex path and a triangle under a one-to-one transfer level (the set-up wants one level): the centred solutions.  The 1-vertex
    system [0] is refused by the set-up as before -- level 0 is smoothed, and a smoother divides by the diagonal (GMG_ERR_NUMERIC: zero
    diagonal); the factor's own 1 x 1 case is tests/test_nullspace_host.py's."""
    eng = cabi.Engine(nullspace=1)
    try:
        eng.set_prolongations([sp.identity(1, format="csc")])
        with pytest.raises(cabi.GmgError) as ei:
            eng.set_system(sp.csc_matrix((np.zeros(1), np.zeros(1, dtype=np.int32), np.array([0, 1], dtype=np.int32)), shape=(1, 1)))
        assert ei.value.code == cabi.GMG_ERR_NUMERIC and "diagonal" in str(ei.value)
    finally:
        eng.close()
    tri = np.array([[2.0, -1.0, -1.0], [-1.0, 2.0, -1.0], [-1.0, -1.0, 2.0]])
    for n, A, b, want in ((2, np.array([[1.0, -1.0], [-1.0, 1.0]]), np.array([[3.0], [1.0]]), np.array([[0.5], [-0.5]])),
                          (3, tri, np.array([[4.0], [1.0], [1.0]]), np.array([[2.0 / 3.0], [-1.0 / 3.0], [-1.0 / 3.0]]))):
        eng = cabi.Engine(nullspace=1)
        try:
            eng.set_prolongations([sp.identity(n, format="csc")])
            eng.set_system(sp.csc_matrix(A))
            x, it, res, _ = eng.solve(np.asfortranarray(b), tol=1e-12, stop_type=0, max_iter=20)
            print(f"NULLSPACE_TINY n = {n}: {it} iterations, residue {res}, x = {np.asarray(x).ravel()}")
            assert np.all(np.isfinite(x)) and np.abs(np.asarray(x).reshape(want.shape) - want).max() <= 1e-14
        finally:
            eng.close()
