"""gmg_config::accelerate on a real device: the solve loop with truncated GCR around the V-cycle (engine.hip::solve_common, accel_kernels.hip.hpp).

The reference is a numpy restatement of the recombination (tests/accelerate_model.py): its cycle is `vcycle(b, x)` of a SECOND handle created with
accelerate = 0 (existing code), its A x is scipy's, everything fp64.  The model differs from the device only in the order of its sums.

Measured on an MI355X over the eighteen model-comparison cases below (eight dependent iterations each), deviations taken relative to the
largest entry (max |got - model| / max |model|, for the residue history as for x):

  residue history   4.5e-8 at most (torus d = 3, m = 4); 2.7e-9 on the point cloud, 2.2e-9 with Jacobi, 1.3e-13 on the Bilaplacian
  x                 9.1e-8 at most (point cloud); 3.1e-8 with Jacobi, <= 2.0e-8 on the torus Poisson cases, 5.8e-10 on the Bilaplacian

Both are above the 1e-8 that the recombination's own rounding would give at these sizes, and so is the ENTRY-WISE relative deviation of the residues
(printed by the test, not asserted: 4e-10 in the first iteration, 0.13 - 0.27 in iterations 6 - 8 of the torus cases, 1.3e-4 on the point cloud).
One cause, and it is in the systems, not in the recombination: the Poisson systems are S + 1e-6 M, the constant vector is almost in the kernel
(condition number about 1e9) and the solution is a constant of size 1.6e4 plus the interesting part.  Every evaluation of b - A x -- scipy's in the
model, the residual kernel's on the device, in different summation orders -- carries eps |A| |x| whatever the residue is.  That is the accuracy
floor these histories reach in six iterations (6e-9 .. 4e-8 of ||b||, the `last` column of the printed lines): up to there the two sides agree to
1e-9 .. 6e-10 of the first residue, on the floor they differ by a fraction (10 - 30 %) of the floor itself, which is the 4.5e-8; and the near-kernel
part of that error is amplified by the condition number into x.  The Bilaplacian case (solution of size 1, eight iterations far above its floor)
shows the recombination's own rounding: 3.7e-11 (m = 3) and 2.6e-11 (m = 4) entry-wise on the residues, 5.8e-10 on x -- those two cases are also held to ENTRYWISE_TOL entry-wise.  So the histories are compared relative to their
largest entry, and the tolerance is MODEL_TOL = 1e-6 = 100 x the 1e-8 bound for both -- not 100 x the larger measured figures."""
import functools
import os
import sys

import numpy as np
import pytest

from tests import problems
from tests.accelerate_model import accelerated_loop

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "gravo_mg_amd", "dropin")
DEV = "cuda:0"

MODEL_TOL = 1e-6
ENTRYWISE_TOL = 1e-8          # every residue of a history that stays far above its floor (the Bilaplacian): the issue's bound for plain rounding
NONINCREASING = 1.0 + 1e-10


def _problem(name):
    if name == "torus":
        return problems.torus_problem(n1=37, n2=29, lower_bound=60)          # 1 073 rows: not a multiple of 64
    if name == "bilaplacian":
        return problems.torus_problem(n1=37, n2=29, kind="bilaplacian", lower_bound=60)      # the hard system
    return problems.pointcloud_problem(n=3000)                              # level 0 on the block sweep


@functools.lru_cache(maxsize=None)
def _engine(name, accelerate, cfg=()):
    from gravo_mg_amd import cabi
    P = _problem(name)
    eng = cabi.Engine(accelerate=accelerate, **dict(cfg))
    eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
    return eng


@functools.lru_cache(maxsize=None)
def _rhs(name, d):
    P = _problem(name)
    rhs = np.asfortranarray(P.mass[:, None] * np.random.default_rng(300 + d).standard_normal((P.n, d)))
    rhs.setflags(write=False)
    return rhs


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _model(name, cfg, rhs, x0, m, stop_type, tol, max_iter):
    """tests/accelerate_model.accelerated_loop with the cycle of a second handle (accelerate = 0): (x, iterations, residues, guarded steps)."""
    P = _problem(name)
    return accelerated_loop(P.lhs, P.mass, _engine(name, 0, cfg).vcycle, rhs, x0, m, stop_type, tol, max_iter)[:4]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


MODEL_CASES = (
    [("torus", d, m, 2, ()) for d in (1, 3, 5) for m in (1, 2, 4)]
    + [("torus", 3, 2, t, ()) for t in (0, 1, 3)]
    + [("bilaplacian", 3, 3, 2, ()), ("bilaplacian", 3, 4, 2, ()), ("pointcloud", 3, 3, 2, ())]
    + [("torus", 3, 2, 2, (("use_graph", True),)), ("torus", 3, 2, 2, (("coarse_mode", 0),)), ("torus", 3, 2, 2, (("smoother", 1),))]
)


@pytest.mark.parametrize("name,d,m,stop_type,cfg", MODEL_CASES,
                         ids=["-".join([c[0], f"d{c[1]}", f"m{c[2]}", f"type{c[3]}"] + [f"{k}{int(v)}" for k, v in c[4]]) for c in MODEL_CASES])
def test_eight_iterations_follow_the_model(cabi, name, d, m, stop_type, cfg):
    """tol = 0, max_iter = 8: all eight iterations run and the window wraps for every depth.  The residue history and the final x agree with the
    model to MODEL_TOL (module docstring); the residues do not grow; the last one is the confirmed one."""
    assert cabi.COARSE_HOST_LDLT == 0 and cabi.SMOOTHER_JACOBI == 1
    rhs = _rhs(name, d)
    eng = _engine(name, m, cfg)
    x, it, res, conv = eng.solve(rhs, tol=0.0, stop_type=stop_type, max_iter=8)
    x = x.reshape(rhs.shape)
    mx, mit, mres, _ = _model(name, cfg, rhs, rhs, m, stop_type, 0.0, 8)
    dev_res, dev_x = _rel(conv[:, 1], mres), _rel(x, mx)
    print(f"ACCEL_DEV {name} d={d} m={m} type={stop_type} cfg={dict(cfg)}: residues {dev_res:.3e} (entry-wise {float(np.max(np.abs(conv[:, 1] - mres) / mres)):.3e}) "
          f"x {dev_x:.3e}  first {conv[0, 1]:.3e} last {conv[-1, 1]:.3e}")
    print("   per iteration: " + "  ".join(f"{g:.3e}/{abs(g - w) / w:.1e}" for g, w in zip(conv[:, 1], mres)))
    assert it == mit == 8 and conv.shape[0] == 8
    assert eng.timing("accelerate") == m and eng.timing("accel_confirmations") == 1
    assert np.all(conv[1:-1, 1] <= conv[:-2, 1] * NONINCREASING), conv[:, 1]
    assert res == conv[-1, 1]
    assert dev_res <= MODEL_TOL and dev_x <= MODEL_TOL
    if name == "bilaplacian":          # eight iterations far above the floor (4.5 of 2 400): every residue, all three ring slots in use at m = 4
        assert float(np.max(np.abs(conv[:, 1] - mres) / mres)) <= ENTRYWISE_TOL and conv[-1, 1] > 1e-4 * conv[0, 1]


@pytest.mark.parametrize("name", ["torus", "bilaplacian", "pointcloud"])
def test_first_step_is_no_worse_than_the_plain_cycle(cabi, name):
    """alpha = 1, beta = 0 is admissible: the first accelerated residue cannot exceed the plain loop's first residue from the same x0."""
    rhs = _rhs(name, 3)
    _, _, _, plain = _engine(name, 0).solve(rhs, tol=0.0, stop_type=2, max_iter=2)
    for m in (1, 3):
        _, _, _, acc = _engine(name, m).solve(rhs, tol=0.0, stop_type=2, max_iter=2)
        print(f"{name} m={m}: first residue {acc[0, 1]:.6e} (plain {plain[0, 1]:.6e})")
        assert acc[0, 1] <= plain[0, 1] * NONINCREASING


@pytest.mark.parametrize("stop_type", [0, 1, 2, 3])
def test_reported_residue_is_that_of_the_returned_iterate(cabi, stop_type):
    """The residue a caller gets has the bits of residual_norm(rhs, x returned): the same kernel on the same vectors."""
    rhs = _rhs("torus", 3)
    eng = _engine("torus", 2)
    for tol, max_iter in ((0.0, 5), (1e-6, 40)):
        x, it, res, conv = eng.solve(rhs, tol=tol, stop_type=stop_type, max_iter=max_iter)
        assert _bits(res) == _bits(eng.residual_norm(rhs, x, stop_type)) and _bits(conv[-1, 1]) == _bits(res)


def test_two_runs_give_the_same_bits(cabi):
    rhs = _rhs("pointcloud", 3)
    eng = _engine("pointcloud", 3)
    a = eng.solve(rhs, tol=1e-9, stop_type=2, max_iter=12)
    b = eng.solve(rhs, tol=1e-9, stop_type=2, max_iter=12)
    assert a[1] == b[1] and _bits(a[2]) == _bits(b[2])
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[3][:, 1]), _bits(b[3][:, 1]))


def test_entry_points_give_the_same_bits(cabi):
    """solve with an explicit x0, solve (x0 = rhs) and solve_device from torch tensors (contiguous, and a strided view): d = 3, m = 2."""
    torch = pytest.importorskip("torch")
    rhs = _rhs("torus", 3)
    eng = _engine("torus", 2)
    kw = dict(tol=1e-9, stop_type=2, max_iter=6)
    x_a, it_a, res_a, conv_a = eng.solve(rhs, **kw)
    x_b, it_b, res_b, conv_b = eng.solve(rhs, x0=rhs.copy(), **kw)
    assert it_a == it_b and _bits(res_a) == _bits(res_b) and np.array_equal(_bits(x_a), _bits(x_b)) and np.array_equal(_bits(conv_a[:, 1]), _bits(conv_b[:, 1]))
    n, d = rhs.shape
    for layout in ("contiguous", "view"):
        if layout == "view":
            own = torch.full((n, d + 3), float("nan"), dtype=torch.float64, device=DEV)
            own[:, 1:1 + d] = torch.tensor(np.ascontiguousarray(rhs), device=DEV)
            b = own[:, 1:1 + d]
            x = torch.full((n, d + 2), float("nan"), dtype=torch.float64, device=DEV)[:, 1:1 + d]
        else:
            b = torch.tensor(np.ascontiguousarray(rhs), device=DEV)
            x = torch.full((n, d), float("nan"), dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        it, res, conv = eng.solve_device(b.data_ptr(), b.stride(), x.data_ptr(), x.stride(), d, **kw)
        assert it == it_a and _bits(res) == _bits(res_a) and np.array_equal(_bits(conv[:, 1]), _bits(conv_a[:, 1]))
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(np.ascontiguousarray(x_a.reshape(rhs.shape))))


def test_accelerate_zero_is_the_default_handle(cabi):
    rhs = _rhs("torus", 3)
    a = cabi.Engine()
    P = _problem("torus")
    a.set_prolongations(P.U); a.set_mass(P.mass); a.set_system(P.lhs)
    b = _engine("torus", 0)
    ra, rb = a.solve(rhs, tol=1e-9, stop_type=2, max_iter=6), b.solve(rhs, tol=1e-9, stop_type=2, max_iter=6)
    assert ra[1] == rb[1] and _bits(ra[2]) == _bits(rb[2]) and np.array_equal(_bits(ra[0]), _bits(rb[0])) and np.array_equal(_bits(ra[3][:, 1]), _bits(rb[3][:, 1]))
    assert b.timing("accelerate") == 0 and b.timing("accel_confirmations") == 0 and b.timing("accel_guard_steps") == 0
    a.close()


def test_stops_where_the_model_stops(cabi):
    """tol = 1e-6, max_iter = 40, depth 3 on the three problems: the returned residue is below the tolerance and the count is the model's.  A case
    whose model residue comes within 1e-6 relative of the tolerance at the deciding iteration is reported and skipped (at most one)."""
    tol, skipped = 1e-6, []
    for name in ("torus", "bilaplacian", "pointcloud"):
        rhs = _rhs(name, 3)
        x, it, res, conv = _engine(name, 3).solve(rhs, tol=tol, stop_type=2, max_iter=40)
        mx, mit, mres, _ = _model(name, (), rhs, rhs, 3, 2, tol, 40)
        _, pit, pres, _ = _engine(name, 0).solve(rhs, tol=tol, stop_type=2, max_iter=40)
        print(f"{name}: plain loop {pit} cycles (residue {pres:.3e}), accelerated {it} (residue {res:.3e}), model {mit} (residue {mres[-1]:.3e})")
        # (the deciding iterations: the one the model stops at and the one before it)
        if any(abs(v - tol) <= 1e-6 * tol for v in mres[-2:]):
            skipped.append(name)
            continue
        assert it == mit, (name, it, mit, res)
        if name == "bilaplacian":                     # only what the model says: it may need more than 40 iterations
            assert (res <= tol) == (mres[-1] <= tol), (name, res, mres[-1])
        else:
            assert res <= tol, (name, it, res)
    print("skipped (model residue at the tolerance):", skipped)
    assert len(skipped) <= 1


def test_zero_column_takes_the_guard(cabi):
    """d = 2, stop type 3, the second column of rhs and of x0 all zero: s = <q, q> = 0 there in every iteration."""
    rhs = np.array(_rhs("torus", 2))
    rhs[:, 1] = 0.0
    eng = _engine("torus", 3)
    x, it, res, conv = eng.solve(rhs, x0=rhs.copy(), tol=0.0, stop_type=3, max_iter=6)
    x = x.reshape(rhs.shape)
    mx, mit, mres, mguards = _model("torus", (), rhs, rhs, 3, 3, 0.0, 6)
    assert np.all(x[:, 1] == 0.0)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(conv)) and np.isfinite(res)
    assert it == mit == 6
    assert _rel(x[:, 0], mx[:, 0]) <= MODEL_TOL and _rel(conv[:, 1], mres) <= MODEL_TOL
    assert eng.timing("accel_guard_steps") > 0 and eng.timing("accel_guard_steps") == mguards


def test_refusals(cabi):
    with pytest.raises(cabi.GmgError) as ei:
        cabi.Engine(accelerate=5)
    assert ei.value.code == cabi.GMG_ERR_INVALID
    with pytest.raises(cabi.GmgError) as ei:
        cabi.Engine(accelerate=2, inner_precision=1)
    assert ei.value.code == cabi.GMG_ERR_UNSUPPORTED
    with pytest.raises(cabi.GmgError) as ei:
        cabi.P2PCycle(_engine("torus", 2), 0, 1, d=1)
    assert ei.value.code == cabi.GMG_ERR_UNSUPPORTED and "accelerate" in str(ei.value)


def test_multi_rank_set_up_is_refused(cabi):
    """gmg_dist_setup with world > 1 on an accelerated handle with a system: refused; world = 1 is not."""
    eng = _engine("torus", 2)
    with pytest.raises(cabi.GmgError) as ei:
        eng.dist_setup(0, 2)
    assert ei.value.code == cabi.GMG_ERR_UNSUPPORTED and "accelerate" in str(ei.value)
    eng.dist_setup(0, 1)


def test_run_cycles_is_unchanged_on_an_accelerated_handle(cabi):
    rhs = _rhs("torus", 3)
    out = []
    for m in (0, 3):
        eng = _engine("torus", m)
        eng.load_problem(rhs, rhs)
        res = eng.run_cycles(4, 2)
        out.append((res, eng.fetch_solution()))
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])) and np.array_equal(_bits(out[0][1]), _bits(out[1][1]))


def test_dropin_option(cabi):
    """set_engine_option("accelerate", 3) followed by solve() on the torus smoothing system: a solution within the tolerance."""
    import glob
    if not glob.glob(os.path.join(DROPIN, "gravomg_bindings*.so")):
        import __graft_entry__
        __graft_entry__.build()
    if DROPIN not in sys.path:
        sys.path.insert(0, DROPIN)
    import gravomg
    import scipy.sparse as sp
    from gravo_mg_amd import meshgen
    V, F = meshgen.torus_mesh(37, 29)
    S, mass = meshgen.cotan_laplacian(V, F)
    lhs, rhs = meshgen.smoothing_system(S, mass, V)
    solver = gravomg.MultigridSolver(V, gravomg.neighbors_from_stiffness(S), sp.diags(mass).tocsr(), lower_bound=60, tolerance=1e-6, max_iter=40)
    solver.set_engine_option("accelerate", 3)
    x = solver.solve(lhs, rhs)
    assert solver.residual(lhs, rhs, x, 2) <= 1e-6
