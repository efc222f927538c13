"""gmg_config::precond_precision = 1 on a real device: the CG loop of gmg_config::pcg with its preconditioner applied as
z = (double) cycle32(fl32(r)) -- the fp32 cycle on the fp32 twins -- and everything else of the loop in fp64 (engine.hip::solve_common,
pcg_kernels.hip.hpp: the float instantiations of pcg_dot / pcg_direction and the pcg_update that writes fl32(r)).

The reference is tests/pcg_model.pcg_loop with, as its cycle, `vcycle(r, 0)` of a SECOND handle created with pcg = 0, inner_precision = 1 and
otherwise the same configuration (existing code): from x = 0 that call is exactly (double) cycle32(fl32(r)).  The two sides run the same fp32
cycle; they differ in the order of the fp64 sums and in which entries of r round the other way in fl32(r) once r differs in its last bits.

MEASURED_RES / MEASURED_X below are the largest deviations measured on an MI355X over the model-comparison cases (eight dependent iterations
each, relative to the largest entry; the tests print them as PRECOND_DEV lines); each comparison is bounded at 10 x that figure, and the figure
itself must stay below 2e-5, the project's bound for ONE fp32 cycle against the fp64 model (tests/test_gpu_chebyshev.py): two sides that both
use the same fp32 cycle must agree better than fp32 and fp64 do.

Measured on an MI355X (max |got - model| / max |model|, residue history / x):

  smoothing torus M + 1e-3 S   d = 1: 1.5e-14 / 3.7e-16   d = 3: 1.9e-14 / 5.0e-16   d = 5: 5.4e-12 / 5.9e-16 (stop types 0 and 2 alike);
                               Jacobi 3.1e-14 / 6.6e-14; use_graph, coarse_mode = 0, zero_guess_step = 1: the figures of d = 3, digit for digit
  Bilaplacian (tau = 1)        2.3e-14 / 2.5e-14
  stiffness, nullspace = 1     3.3e-13 / 2.1e-13 (Jacobi 2.4e-12 / 2.1e-12; the other configurations: the same figures)
  point cloud                  3.8e-06 / 4.3e-08  <- the largest: MEASURED_RES, MEASURED_X

The point cloud is S + 1e-6 M, the system on which tests/test_gpu_pcg.py explains why <p, q> is only known to eps x 1e10: there a rounding of
fl32(r) that falls the other way is amplified as that docstring describes (the fp64 loop against its model: 2.5e-7 / 4.7e-8 on the same input);
everywhere else the two sides agree to 1e-11 or better, i.e. they round the same entries the same way for eight iterations.

Iterations to 1e-4 (d = 1, x0 = rhs, stop type 2), fp32 cycle / its model / fp64 cycle (precond_precision = 0):
  torus Poisson 7 / 7 / 5    torus Bilaplacian 35 / 35 / 35    sphere 10 / 10 / 7    point cloud 8 / 8 / 7
To 1e-6: torus Poisson 9 / 7 (fp32 / fp64 cycle), sphere 13 / 10.  To 1e-8 on the Bilaplacian torus: 52 with the fp32 cycle, 52 with the fp64 cycle.  The issue asks for the 1e-8 run "on the torus"; on the
torus POISSON system S + 1e-6 M neither handle gets there (1 000 iterations: 2.5e-8 with precond_precision = 0, 2.9e-8 with 1 -- the fp64
accuracy floor of that system, condition number about 1e9), so a count of the precond_precision = 0 handle to double does not exist and the run
is made on the torus Bilaplacian, the system the CG loop exists for.  The three S + 1e-6 M systems need 1 - 3 more iterations with the fp32
cycle: their residual is dominated by the near-null constant, which fl32(r) perturbs by 6e-8 of its size each iteration.
One iteration on the smoothing torus: |x32 - x64| / |x64| = 8.2e-8."""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import nullspace_model as nm
from tests import problems
from tests.pcg_model import pcg_loop

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "gravo_mg_amd", "dropin")
DEV = "cuda:0"
CHEBYSHEV, JACOBI = 2, 1
FP32_CYCLE_TOL = 2e-5          # one fp32 cycle against the fp64 model (tests/test_gpu_chebyshev.py)
MEASURED_RES = 3.803e-6       # residue history: the point cloud
MEASURED_X = 4.327e-8         # x: the point cloud
assert MEASURED_RES < FP32_CYCLE_TOL and MEASURED_X < FP32_CYCLE_TOL


@functools.lru_cache(maxsize=None)
def _problem(name):
    if name == "smoothing":
        return problems.torus_problem(n1=37, n2=29, kind="smoothing", lower_bound=60)      # M + 1e-3 S, 1 073 rows: not a multiple of 64
    if name in ("torus", "stiffness"):
        return problems.torus_problem(n1=37, n2=29, lower_bound=60)                        # S + 1e-6 M; "stiffness": its S alone
    if name == "bilaplacian":
        return problems.torus_problem(n1=37, n2=29, kind="bilaplacian", lower_bound=60)
    if name == "sphere":
        return problems.sphere_problem(n=6000)
    return problems.pointcloud_problem(n=3000)


@functools.lru_cache(maxsize=None)
def _lhs(name):
    P = _problem(name)
    if name != "stiffness":
        return P.lhs
    S = sp.csc_matrix(P.S)
    S.sort_indices()
    return S


def _make(name, **kw):
    from gravo_mg_amd import cabi
    P = _problem(name)
    kw.setdefault("smoother", CHEBYSHEV)
    if name == "stiffness":
        kw["nullspace"] = 1
    eng = cabi.Engine(**kw)
    eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(_lhs(name))
    return eng


@functools.lru_cache(maxsize=None)
def _engine(name, kind, cfg=()):
    """kind "fp32": pcg = 1, precond_precision = 1; "fp64": pcg = 1 alone; "cycle32": pcg = 0, inner_precision = 1 (the model's cycle); "plain": pcg = 0."""
    how = {"fp32": dict(pcg=1, precond_precision=1), "fp64": dict(pcg=1), "cycle32": dict(inner_precision=1), "plain": dict()}[kind]
    return _make(name, **how, **dict(cfg))


@functools.lru_cache(maxsize=None)
def _rhs(name, d):
    P = _problem(name)
    rhs = np.asfortranarray(P.mass[:, None] * np.random.default_rng(300 + d).standard_normal((P.n, d)))
    rhs.setflags(write=False)
    return rhs


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _model(name, cfg, rhs, x0, stop_type, tol, max_iter):
    """(x, iterations, residues) of the model loop around the fp32 cycle of the second handle; on the stiffness matrix the nullspace = 1 solve."""
    P = _problem(name)
    cycle = _engine(name, "cycle32", cfg).vcycle
    if name == "stiffness":
        return nm.nullspace_solve(_lhs(name), P.mass, cycle, rhs, x0, stop_type, tol, max_iter, loop="pcg")[:3]
    x, it, res, guards, restarts = pcg_loop(_lhs(name), P.mass, cycle, rhs, x0, stop_type, tol, max_iter)[:5]
    assert guards == 0 and restarts == 0
    return x, it, res


CONFIGS = [(), (("smoother", JACOBI),), (("use_graph", True),), (("coarse_mode", 0),), (("zero_guess_step", 1),)]
MODEL_CASES = (
    [("smoothing", d, t, ()) for d in (1, 3, 5) for t in (0, 2)]
    + [("bilaplacian", 3, 2, ()), ("pointcloud", 3, 2, ())]
    + [("smoothing", 3, 2, cfg) for cfg in CONFIGS[1:]]
    + [("stiffness", 3, 2, cfg) for cfg in CONFIGS]
)


@pytest.mark.parametrize("name,d,stop_type,cfg", MODEL_CASES,
                         ids=["-".join([c[0], f"d{c[1]}", f"type{c[2]}"] + [f"{k}{int(v)}" for k, v in c[3]]) for c in MODEL_CASES])
def test_eight_iterations_follow_the_model(cabi, name, d, stop_type, cfg):
    """tol = 0, max_iter = 8: all eight iterations run, one confirmation, no guards, no restarts; the residue history and the final x agree with
    the model within 10 x the measured deviations (module docstring), and the last residue is the confirmed one."""
    assert cabi.COARSE_HOST_LDLT == 0 and cabi.SMOOTHER_JACOBI == JACOBI and cabi.SMOOTHER_CHEBYSHEV == CHEBYSHEV
    rhs = _rhs(name, d)
    eng = _engine(name, "fp32", cfg)
    x, it, res, conv = eng.solve(rhs, tol=0.0, stop_type=stop_type, max_iter=8)
    x = x.reshape(rhs.shape)
    mx, mit, mres = _model(name, cfg, rhs, rhs, stop_type, 0.0, 8)
    dev_res, dev_x = _rel(conv[:, 1], mres), _rel(x, mx)
    print(f"PRECOND_DEV {name} d={d} type={stop_type} cfg={dict(cfg)}: residues {dev_res:.3e} x {dev_x:.3e}  first {conv[0, 1]:.3e} last {conv[-1, 1]:.3e}")
    print("   per iteration: " + "  ".join(f"{g:.3e}/{abs(g - w) / w:.1e}" for g, w in zip(conv[:, 1], mres)))
    assert it == mit == 8 and conv.shape[0] == 8
    assert eng.timing("pcg") == 1 and eng.timing("precond_precision") == 1 and eng.timing("pcg_confirmations") == 1
    assert eng.timing("pcg_guard_steps") == 0 and eng.timing("pcg_restarts") == 0
    assert res == conv[-1, 1]
    assert dev_res <= 10.0 * MEASURED_RES and dev_x <= 10.0 * MEASURED_X


@pytest.mark.parametrize("name", ["torus", "bilaplacian", "sphere", "pointcloud"])
def test_converges_to_a_residue_the_fp64_check_confirms(cabi, name):
    """d = 1, x0 = rhs, stop type 2, tol 1e-4, max_iter 60: within the tolerance in at most the model's count + 1 (the margin tests/test_gpu_pcg.py
    gives the fp64 loop over its model), the reported residue that of the returned iterate bit for bit.  On the torus also tol = 1e-8 within twice
    the iterations of the precond_precision = 0 handle on the same input: an fp32 preconditioner that doubles the count has no point.  That torus
    is the Bilaplacian (module docstring: 1e-8 is below the fp64 floor of S + 1e-6 M for both handles)."""
    P = _problem(name)
    rhs = np.asfortranarray(P.rhs)
    eng, ref = _engine(name, "fp32"), _engine(name, "fp64")
    x, it, res, _ = eng.solve(rhs, tol=1e-4, stop_type=2, max_iter=60)
    mit = _model(name, (), rhs, rhs, 2, 1e-4, 60)[1]
    _, it64, res64, _ = ref.solve(rhs, tol=1e-4, stop_type=2, max_iter=60)
    print(f"PRECOND_CONV {name} tol 1e-4: fp32 cycle {it} iterations (residue {res:.3e}), model {mit}; fp64 cycle {it64} iterations (residue {res64:.3e})")
    assert not eng.diverged and res <= 1e-4
    assert _bits(res) == _bits(eng.residual_norm(rhs, x, 2))
    assert it <= mit + 1
    # what the fp32 cycle costs in iterations is pinned, not only printed: never twice the precond_precision = 0 handle's count (the issue's
    # rule for the 1e-8 run), at 1e-4 on every system and at 1e-6 on the two S + 1e-6 M meshes, where it costs the most
    assert it <= 2 * it64
    if name in ("torus", "sphere"):
        _, jt64, s64, _ = ref.solve(rhs, tol=1e-6, stop_type=2, max_iter=100)
        _, jt, s32, _ = eng.solve(rhs, tol=1e-6, stop_type=2, max_iter=100)
        print(f"PRECOND_CONV {name} tol 1e-6: fp32 cycle {jt} iterations (residue {s32:.3e}); fp64 cycle {jt64} iterations (residue {s64:.3e})")
        assert s64 <= 1e-6 and s32 <= 1e-6 and jt <= 2 * jt64
    if name == "bilaplacian":
        _, it64, res64, _ = ref.solve(rhs, tol=1e-8, stop_type=2, max_iter=200)
        x, it, res, _ = eng.solve(rhs, tol=1e-8, stop_type=2, max_iter=2 * it64)
        print(f"PRECOND_CONV {name} tol 1e-8: fp32 cycle {it} iterations (residue {res:.3e}); fp64 cycle {it64} iterations (residue {res64:.3e})")
        assert res64 <= 1e-8
        assert not eng.diverged and res <= 1e-8 and _bits(res) == _bits(eng.residual_norm(rhs, x, 2))


def test_the_fp32_cycle_ran_and_zero_is_the_parent(cabi):
    """After one iteration on the smoothing torus x differs in bits from the precond_precision = 0 handle's, by at most 2e-5 |x|; the key is
    written by the new handle only; a handle with the field at 0 gives the bits of a handle that never set it."""
    rhs = _rhs("smoothing", 3)
    e32, e64 = _engine("smoothing", "fp32"), _engine("smoothing", "fp64")
    x32 = e32.solve(rhs, tol=0.0, stop_type=2, max_iter=1)[0]
    x64 = e64.solve(rhs, tol=0.0, stop_type=2, max_iter=1)[0]
    diff = float(np.linalg.norm(x32 - x64) / np.linalg.norm(x64))
    print(f"PRECOND_ONE_ITERATION |x32 - x64| / |x64| = {diff:.3e}")
    assert not np.array_equal(_bits(x32), _bits(x64)) and 0.0 < diff <= FP32_CYCLE_TOL
    assert e32.timing("precond_precision") == 1
    with pytest.raises(Exception):
        e64.timing("precond_precision")
    zero = _make("smoothing", pcg=1, precond_precision=0)
    try:
        kw = dict(tol=0.0, stop_type=2, max_iter=6)
        a, b = zero.solve(rhs, **kw), e64.solve(rhs, **kw)
        assert a[1] == b[1] == 6 and _bits(a[2]) == _bits(b[2]) and np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[3][:, 1]), _bits(b[3][:, 1]))
        with pytest.raises(Exception):
            zero.timing("precond_precision")
    finally:
        zero.close()


@pytest.mark.parametrize("cfg", [(), (("use_graph", True),)], ids=["stream", "graph"])
def test_cycles_outside_the_solve_stay_fp64(cabi, cfg):
    """gmg_vcycle (and gmg_run_cycles) on a precond_precision = 1 handle, after a solve that ran the fp32 cycle -- under a graph too --, give the
    bits of a pcg = 0 fp64 handle of the same configuration."""
    rhs = _rhs("smoothing", 3)
    out = []
    for kind in ("plain", "fp32"):
        eng = _engine("smoothing", kind, cfg)
        eng.solve(rhs, tol=0.0, stop_type=2, max_iter=3)
        v = eng.vcycle(rhs, rhs)
        eng.load_problem(rhs, rhs)
        res = eng.run_cycles(4, 2)
        out.append((v, res, eng.fetch_solution()))
        eng.solve(rhs, tol=0.0, stop_type=2, max_iter=3)
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(_bits(a), _bits(b))


CHAINS = (1, 2, 5, 63, 64, 65, 129)


@pytest.mark.parametrize("d", [1, 5])
@pytest.mark.parametrize("n", CHAINS)
def test_boundary_shapes(cabi, n, d):
    """Chains of 1 .. 129 rows as tests/test_gpu_pcg.py::test_boundary_shapes, tol = 1e-12, max_iter = 25: status no worse than the plain loop's,
    every value finite, the residue at most 4.5 x the plain loop's after the same count.  With tol = -1 all 25 iterations run, stay finite, and
    the reported residue is the confirmed one."""
    P = problems.synthetic_problem(graph=("chain", n), sizes=[n, max(1, n // 4)], kind="poisson", prolong=("pc",), d=d)
    rhs = np.asfortranarray(P.rhs)
    kw = dict(smoother=CHEBYSHEV)
    eng, plain = cabi.Engine(pcg=1, precond_precision=1, **kw), cabi.Engine(pcg=0, **kw)
    try:
        for e in (eng, plain):
            e.set_prolongations(P.U); e.set_mass(P.mass); e.set_system(P.lhs)
        x, it, res, conv = eng.solve(rhs, tol=1e-12, stop_type=2, max_iter=25)
        diverged, guards = eng.diverged, eng.timing("pcg_guard_steps")
        plain.solve(rhs, tol=1e-12, stop_type=2, max_iter=25)
        plain_diverged = plain.diverged
        _, pit, pres, _ = plain.solve(rhs, tol=0.0, stop_type=2, max_iter=it)
        print(f"PRECOND_SHAPE chain{n} d={d}: {it} iterations, residue {res:.3e} (guards {guards:.0f}, restarts {eng.timing('pcg_restarts'):.0f}, "
              f"confirmations {eng.timing('pcg_confirmations'):.0f}); plain loop after {pit}: {pres:.3e}")
        assert not (diverged and not plain_diverged)
        assert np.all(np.isfinite(x)) and np.all(np.isfinite(conv)) and np.isfinite(res)
        assert pit == it or pres == 0.0
        assert res <= 4.5 * pres
        x2, it2, res2, conv2 = eng.solve(rhs, tol=-1.0, stop_type=2, max_iter=25)
        print(f"   all 25 iterations: residue {res2:.3e}, largest reported {conv2[:, 1].max():.3e} (guards {eng.timing('pcg_guard_steps'):.0f}, restarts {eng.timing('pcg_restarts'):.0f})")
        assert it2 == 25 and np.all(np.isfinite(x2)) and np.all(np.isfinite(conv2))
        assert _bits(res2) == _bits(eng.residual_norm(rhs, x2, 2)) and _bits(res2) == _bits(conv2[-1, 1])
    finally:
        eng.close(); plain.close()


def test_two_runs_give_the_same_bits(cabi):
    rhs = _rhs("pointcloud", 3)
    eng = _engine("pointcloud", "fp32")
    a = eng.solve(rhs, tol=1e-9, stop_type=2, max_iter=12)
    b = eng.solve(rhs, tol=1e-9, stop_type=2, max_iter=12)
    assert a[1] == b[1] and _bits(a[2]) == _bits(b[2])
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[3][:, 1]), _bits(b[3][:, 1]))


def test_entry_points_give_the_same_bits(cabi):
    """solve with an explicit x0, solve (x0 = rhs: gmg_solve_x0_rhs) and solve_device from torch tensors (contiguous, and a strided view), d = 3; then
    d = 5 and d = 1 on one handle (the level vectors, fp32 ones included, and the loop's own are re-sized) against fresh handles; then a values-only
    set_system(3 lhs) and a gmg_set_system_values_device with the same values -- both must refresh the fp32 twins -- against a handle set up with
    those values."""
    torch = pytest.importorskip("torch")
    rhs = _rhs("smoothing", 3)
    eng = _engine("smoothing", "fp32")
    kw = dict(tol=0.0, stop_type=2, max_iter=6)
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
    P = _problem("smoothing")
    how = dict(pcg=1, precond_precision=1)
    fresh, live = _make("smoothing", **how), _make("smoothing", **how)
    live.solve(_rhs("smoothing", 3), **kw)
    live.solve(_rhs("smoothing", 5), **kw)
    live.solve(_rhs("smoothing", 1), **kw)
    for dd in (1, 5):
        a, b = live.solve(_rhs("smoothing", dd), **kw), fresh.solve(_rhs("smoothing", dd), **kw)
        assert a[1] == b[1] and _bits(a[2]) == _bits(b[2]) and np.array_equal(_bits(a[0]), _bits(b[0]))
    lhs2 = (P.lhs * 3.0).tocsc()
    lhs2.sort_indices()
    live.set_system(lhs2)
    other = cabi.Engine(smoother=CHEBYSHEV, **how)
    other.set_prolongations(P.U); other.set_mass(P.mass); other.set_system(lhs2)
    a, b = live.solve(_rhs("smoothing", 3), **kw), other.solve(_rhs("smoothing", 3), **kw)
    assert a[1] == b[1] and _bits(a[2]) == _bits(b[2]) and np.array_equal(_bits(a[0]), _bits(b[0]))
    # gmg_set_system_values_device refreshes the twins too: the same values from device memory on a handle that holds lhs
    vals = torch.tensor(lhs2.data, device=DEV)
    torch.cuda.synchronize()
    fresh.set_system_values_device(vals.data_ptr(), vals.numel())
    assert fresh.timing("setup_values_only") == 1.0
    c = fresh.solve(_rhs("smoothing", 3), **kw)
    assert c[1] == b[1] and _bits(c[2]) == _bits(b[2]) and np.array_equal(_bits(c[0]), _bits(b[0]))
    for e in (fresh, live, other):
        e.close()


def test_dropin_option(cabi):
    """set_engine_option("pcg", 1) and ("precond_precision", 1) with the Chebyshev smoother, then solve() on the torus smoothing system: a solution
    within the tolerance by solver.residual, and the engine that computed it says precond_precision = 1."""
    import glob
    if not glob.glob(os.path.join(DROPIN, "gravomg_bindings*.so")):
        import __graft_entry__
        __graft_entry__.build()
    if DROPIN not in sys.path:
        sys.path.insert(0, DROPIN)
    import gravomg
    from gravo_mg_amd import meshgen
    V, F = meshgen.torus_mesh(37, 29)
    S, mass = meshgen.cotan_laplacian(V, F)
    lhs, rhs = meshgen.smoothing_system(S, mass, V)
    solver = gravomg.MultigridSolver(V, gravomg.neighbors_from_stiffness(S), sp.diags(mass).tocsr(), lower_bound=60, tolerance=1e-6, max_iter=40)
    solver.set_engine_option("smoother", CHEBYSHEV)
    solver.set_engine_option("pcg", 1)
    solver.set_engine_option("precond_precision", 1)
    x = solver.solve(lhs, rhs)
    assert solver.residual(lhs, rhs, x, 2) <= 1e-6
    eng = cabi.Engine.borrow(solver.solver.engine_handle())
    assert eng.timing("pcg") == 1 and eng.timing("precond_precision") == 1 and eng.timing("pcg_confirmations") >= 1
