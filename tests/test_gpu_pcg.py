"""gmg_config::pcg on a real device: conjugate gradients with the V-cycle as the preconditioner (engine.hip::solve_common, pcg_kernels.hip.hpp).

The reference is a numpy restatement of the loop (tests/pcg_model.py): its cycle is `vcycle(b, x)` of a SECOND handle created with pcg = 0 and
otherwise the same configuration (existing code), its A x is scipy's, everything fp64.  The model differs from the device only in the order of its
sums.  Histories and x are compared relative to their largest entry against MODEL_TOL = 1e-6 of tests/test_gpu_accelerate.py (the same kind of
comparison: 100 x the 1e-8 rounding bound); on the Bilaplacian, whose eight iterations stay far above any accuracy floor, every residue is held
entry-wise to that file's ENTRYWISE_TOL = 1e-8.

Measured on an MI355X over the eleven model-comparison cases (eight dependent iterations each; the tests print them as PCG_DEV lines),
deviations relative to the largest entry (max |got - model| / max |model|):

  residue history   2.5e-7 at most (point cloud); torus Poisson 1.0e-7 .. 2.3e-7 (2.0e-8 with stop type 3), Jacobi 1.0e-7, Bilaplacian 8.7e-13
  x                 4.7e-8 at most (point cloud); torus Poisson 1.5e-8 .. 3.6e-8, Jacobi 9.0e-9, Bilaplacian 2.2e-10

The Bilaplacian (tau = 1: solution of size 1, eight iterations far above its floor) shows the loop's own rounding: 9.0e-12 entry-wise on the
residues.  The Poisson systems are S + 1e-6 M: the constant vector is almost in the kernel (condition number about 1e9), p carries a large
constant part, and q = A p is what is left of row sums that cancel on it: |p|^T |A| |p| / p^T A p = 1.1e10 in the first iteration of the torus
case, and forming q in extended precision instead of fp64 moves <p, q> by 7.7e-9 (reordering the dot product alone: 1e-14).  So <p, q> is
known to eps x 1e10 at best, to scipy's product in the model as to the SpMV kernel (fused multiply-adds, another order) on the device.  alpha
carries that, so the residues differ by 1e-7 .. 1.1e-6 entry-wise from the
FIRST iteration on (accelerate's <q, q> has no such cancellation: 4e-10 there), and by 4e-4 .. 2e-2 in the eighth, which is on the accuracy floor
(1.3e-7 .. 1.7e-7 of |b|).  The iteration counts to 1e-4 are the model's (Bilaplacian 35, sphere 7).

The boundary shapes: the issue asks for pcg_guard_steps > 0 on the 1-row chain at tol = 1e-12.  There the first iteration solves the system (the
cycle of a 1 x 1 system is exact, alpha = 1), the confirmed residue is 0 (d = 1) or 2e-16 (d = 5) and the loop ends after ONE iteration, before any
guard can be taken -- by the algorithm as stated, on the model as on the device (tests/pcg_model.py gives 1 iteration, 0 guards).  The guard on that
shape is therefore asked for where it can occur: the same shapes with a NEGATIVE tolerance, which makes all 25 iterations run from a residue of
exactly zero on; everything else of that test is held at tol = 1e-12 as stated."""
import functools
import os
import sys

import numpy as np
import pytest

from tests import problems
from tests.pcg_model import pcg_loop
from tests.test_gpu_accelerate import ENTRYWISE_TOL, MODEL_TOL, NONINCREASING

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "gravo_mg_amd", "dropin")
DEV = "cuda:0"
CHEBYSHEV, JACOBI = 2, 1


def _problem(name):
    if name == "torus":
        return problems.torus_problem(n1=37, n2=29, lower_bound=60)          # 1 073 rows: not a multiple of 64
    if name == "bilaplacian":
        return problems.torus_problem(n1=37, n2=29, kind="bilaplacian", lower_bound=60)      # the hard system
    if name == "sphere":
        return problems.sphere_problem(n=6000)
    return problems.pointcloud_problem(n=3000)


@functools.lru_cache(maxsize=None)
def _engine(name, pcg, cfg=()):
    """A handle on the problem: Chebyshev 2 + 2 unless cfg says otherwise."""
    from gravo_mg_amd import cabi
    P = _problem(name)
    eng = cabi.Engine(pcg=pcg, **dict((("smoother", CHEBYSHEV),) + tuple(cfg)))
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


def _model(name, cfg, rhs, x0, stop_type, tol, max_iter):
    """tests/pcg_model.pcg_loop with the cycle of a second handle (pcg = 0): (x, iterations, residues, guarded steps, restarts, steps, iterates)."""
    P = _problem(name)
    return pcg_loop(P.lhs, P.mass, _engine(name, 0, cfg).vcycle, rhs, x0, stop_type, tol, max_iter)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


MODEL_CASES = (
    [("torus", d, 2, ()) for d in (1, 3, 5)]
    + [("torus", 3, t, ()) for t in (0, 1, 3)]
    + [("bilaplacian", 3, 2, ()), ("pointcloud", 3, 2, ())]
    + [("torus", 3, 2, (("smoother", JACOBI),)), ("torus", 3, 2, (("use_graph", True),)), ("torus", 3, 2, (("coarse_mode", 0),))]
)


@pytest.mark.parametrize("name,d,stop_type,cfg", MODEL_CASES,
                         ids=["-".join([c[0], f"d{c[1]}", f"type{c[2]}"] + [f"{k}{int(v)}" for k, v in c[3]]) for c in MODEL_CASES])
def test_eight_iterations_follow_the_model(cabi, name, d, stop_type, cfg):
    """tol = 0, max_iter = 8: all eight iterations run.  The residue history and the final x agree with the model to MODEL_TOL (module docstring);
    the last residue is the confirmed one."""
    assert cabi.COARSE_HOST_LDLT == 0 and cabi.SMOOTHER_JACOBI == JACOBI and cabi.SMOOTHER_CHEBYSHEV == CHEBYSHEV
    rhs = _rhs(name, d)
    eng = _engine(name, 1, cfg)
    x, it, res, conv = eng.solve(rhs, tol=0.0, stop_type=stop_type, max_iter=8)
    x = x.reshape(rhs.shape)
    mx, mit, mres, mguards, mrestarts = _model(name, cfg, rhs, rhs, stop_type, 0.0, 8)[:5]
    dev_res, dev_x = _rel(conv[:, 1], mres), _rel(x, mx)
    entry = float(np.max(np.abs(conv[:, 1] - mres) / mres))
    print(f"PCG_DEV {name} d={d} type={stop_type} cfg={dict(cfg)}: residues {dev_res:.3e} (entry-wise {entry:.3e}) x {dev_x:.3e}  first {conv[0, 1]:.3e} last {conv[-1, 1]:.3e}")
    print("   per iteration: " + "  ".join(f"{g:.3e}/{abs(g - w) / w:.1e}" for g, w in zip(conv[:, 1], mres)))
    assert it == mit == 8 and conv.shape[0] == 8
    assert eng.timing("pcg") == 1 and eng.timing("pcg_confirmations") == 1
    assert eng.timing("pcg_guard_steps") == mguards == 0 and eng.timing("pcg_restarts") == mrestarts == 0
    assert res == conv[-1, 1]
    assert dev_res <= MODEL_TOL and dev_x <= MODEL_TOL
    if name == "bilaplacian":          # eight iterations far above the floor: every residue
        assert entry <= ENTRYWISE_TOL and conv[-1, 1] > 1e-4 * conv[0, 1]


def test_converges_on_the_bilaplacian_where_the_plain_loop_does_not(cabi):
    """The feature's point.  Bilaplacian torus, d = 1, x0 = rhs, stop type 2, tol 1e-4, max_iter 60: GMG_OK and a residue within the tolerance in
    at most the model's count + 1, while the pcg = 0 handle of the same configuration is above 1e-2 after 60 cycles."""
    P = _problem("bilaplacian")
    rhs = np.asfortranarray(P.rhs)
    eng = _engine("bilaplacian", 1)
    x, it, res, conv = eng.solve(rhs, tol=1e-4, stop_type=2, max_iter=60)
    mit = _model("bilaplacian", (), rhs, rhs, 2, 1e-4, 60)[1]
    plain = _engine("bilaplacian", 0)
    _, pit, pres, _ = plain.solve(rhs, tol=1e-4, stop_type=2, max_iter=60)
    print(f"bilaplacian: PCG {it} iterations (residue {res:.3e}), model {mit}; plain Chebyshev loop {pit} cycles, residue {pres:.3e}")
    assert not eng.diverged and res <= 1e-4 and it <= mit + 1
    assert _bits(res) == _bits(eng.residual_norm(rhs, x, 2))
    assert pit == 60 and pres > 1e-2


def test_needs_no_more_iterations_than_the_plain_loop_on_the_sphere(cabi):
    P = _problem("sphere")
    rhs = np.asfortranarray(P.rhs)
    eng = _engine("sphere", 1)
    x, it, res, _ = eng.solve(rhs, tol=1e-4, stop_type=2, max_iter=60)
    mit = _model("sphere", (), rhs, rhs, 2, 1e-4, 60)[1]
    _, pit, pres, _ = _engine("sphere", 0).solve(rhs, tol=1e-4, stop_type=2, max_iter=60)
    print(f"sphere: PCG {it} iterations (residue {res:.3e}), model {mit}; plain Chebyshev loop {pit} cycles, residue {pres:.3e}")
    assert not eng.diverged and res <= 1e-4 and it <= mit + 1 and it <= pit


@pytest.mark.parametrize("stop_type", [0, 1, 2, 3])
def test_reported_residue_is_that_of_the_returned_iterate(cabi, stop_type):
    """The residue a caller gets has the bits of residual_norm(rhs, x returned): the same kernel on the same vectors."""
    rhs = _rhs("torus", 3)
    eng = _engine("torus", 1)
    for tol, max_iter in ((0.0, 5), (1e-6, 40)):
        x, it, res, conv = eng.solve(rhs, tol=tol, stop_type=stop_type, max_iter=max_iter)
        assert _bits(res) == _bits(eng.residual_norm(rhs, x, stop_type)) and _bits(conv[-1, 1]) == _bits(res)
        assert eng.timing("pcg_confirmations") >= 1


@pytest.mark.parametrize("name", ["torus", "bilaplacian"])
def test_energy_norm_of_the_error_does_not_grow(cabi, name):
    """b = A x* for a known x*: |x_k - x*|_A after max_iter = 1 .. 6 (and of x0 = b) does not grow -- CG's own invariant: a wrong alpha or a stale p
    breaks it."""
    P = _problem(name)
    A = P.lhs.tocsr()
    xs = np.random.default_rng(11).standard_normal((P.n, 3))
    rhs = np.asfortranarray(A @ xs)
    eng = _engine(name, 1)

    def energy(x):
        e = np.asarray(x).reshape(xs.shape) - xs
        return np.sqrt((e * (A @ e)).sum(axis=0))
    hist = [energy(rhs)] + [energy(eng.solve(rhs, tol=0.0, stop_type=2, max_iter=k)[0]) for k in range(1, 7)]
    print(f"{name}: A-norm of the error per column, x0 and iterations 1 .. 6:\n" + "\n".join("   " + " ".join(f"{v:.6e}" for v in h) for h in hist))
    for a, b in zip(hist[:-1], hist[1:]):
        assert np.all(b <= a * NONINCREASING), (a, b)
    assert np.all(hist[-1] < 0.5 * hist[0])


CHAINS = (1, 2, 5, 63, 64, 65, 129)


@pytest.mark.parametrize("d", [1, 5])
@pytest.mark.parametrize("n", CHAINS)
def test_boundary_shapes(cabi, n, d):
    """Chains of 1 .. 129 rows (level 0 smaller than a 64-row slice, one slice, just over one, three), tol = 1e-12, max_iter = 25: the Krylov space
    is exhausted and the floor is reached.  Status no worse than the plain loop's, every value finite, the residue at most 4.5 x the plain loop's
    after the same count (the bound of the accelerated loop's boundary test).  The guards (module docstring): with a negative
    tolerance all 25 iterations run; everything stays finite and where it was, and the 1-row shape takes guards."""
    P = problems.synthetic_problem(graph=("chain", n), sizes=[n, max(1, n // 4)], kind="poisson", prolong=("pc",), d=d)
    rhs = np.asfortranarray(P.rhs)
    kw = dict(smoother=CHEBYSHEV)
    eng, plain = cabi.Engine(pcg=1, **kw), cabi.Engine(pcg=0, **kw)
    try:
        for e in (eng, plain):
            e.set_prolongations(P.U); e.set_mass(P.mass); e.set_system(P.lhs)
        x, it, res, conv = eng.solve(rhs, tol=1e-12, stop_type=2, max_iter=25)
        pcg_diverged, guards = eng.diverged, eng.timing("pcg_guard_steps")
        plain.solve(rhs, tol=1e-12, stop_type=2, max_iter=25)
        plain_diverged = plain.diverged
        _, pit, pres, _ = plain.solve(rhs, tol=0.0, stop_type=2, max_iter=it)
        print(f"PCG_SHAPE chain{n} d={d}: {it} iterations, residue {res:.3e} (guards {guards:.0f}, restarts {eng.timing('pcg_restarts'):.0f}, "
              f"confirmations {eng.timing('pcg_confirmations'):.0f}); plain loop after {pit}: {pres:.3e}")
        assert not (pcg_diverged and not plain_diverged)
        assert np.all(np.isfinite(x)) and np.all(np.isfinite(conv)) and np.isfinite(res)
        assert pit == it or pres == 0.0
        assert res <= 4.5 * pres
        # past the exhausted Krylov space
        x2, it2, res2, conv2 = eng.solve(rhs, tol=-1.0, stop_type=2, max_iter=25)
        guards2 = eng.timing("pcg_guard_steps")
        print(f"   all 25 iterations: residue {res2:.3e}, largest reported {conv2[:, 1].max():.3e} (guards {guards2:.0f}, restarts {eng.timing('pcg_restarts'):.0f})")
        assert it2 == 25 and np.all(np.isfinite(x2)) and np.all(np.isfinite(conv2))
        assert _bits(res2) == _bits(eng.residual_norm(rhs, x2, 2))
        if n == 1:
            assert guards2 > 0 and res2 <= 1e-15
    finally:
        eng.close(); plain.close()


def test_two_runs_give_the_same_bits(cabi):
    rhs = _rhs("pointcloud", 3)
    eng = _engine("pointcloud", 1)
    a = eng.solve(rhs, tol=1e-9, stop_type=2, max_iter=12)
    b = eng.solve(rhs, tol=1e-9, stop_type=2, max_iter=12)
    assert a[1] == b[1] and _bits(a[2]) == _bits(b[2])
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[3][:, 1]), _bits(b[3][:, 1]))


def test_entry_points_give_the_same_bits(cabi):
    """solve with an explicit x0, solve (x0 = rhs: gmg_solve_x0_rhs) and solve_device from torch tensors (contiguous, and a strided view), d = 3; then
    d = 5 and d = 1 on the same handle (the level vectors and the loop's own are re-sized) against a fresh handle."""
    torch = pytest.importorskip("torch")
    rhs = _rhs("torus", 3)
    eng = _engine("torus", 1)
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
    P = _problem("torus")
    fresh = cabi.Engine(pcg=1, smoother=CHEBYSHEV)
    fresh.set_prolongations(P.U); fresh.set_mass(P.mass); fresh.set_system(P.lhs)
    live = cabi.Engine(pcg=1, smoother=CHEBYSHEV)
    live.set_prolongations(P.U); live.set_mass(P.mass); live.set_system(P.lhs)
    live.solve(_rhs("torus", 1), **kw)
    live.solve(_rhs("torus", 5), **kw)
    for dd in (1, 5):
        a, b = live.solve(_rhs("torus", dd), **kw), fresh.solve(_rhs("torus", dd), **kw)
        assert a[1] == b[1] and _bits(a[2]) == _bits(b[2]) and np.array_equal(_bits(a[0]), _bits(b[0]))
    # a values-only refresh: the same pattern with other values, against a handle set up with them
    lhs2 = (P.lhs * 3.0).tocsc()
    lhs2.sort_indices()
    live.set_system(lhs2)
    other = cabi.Engine(pcg=1, smoother=CHEBYSHEV)
    other.set_prolongations(P.U); other.set_mass(P.mass); other.set_system(lhs2)
    a, b = live.solve(_rhs("torus", 3), **kw), other.solve(_rhs("torus", 3), **kw)
    assert a[1] == b[1] and _bits(a[2]) == _bits(b[2]) and np.array_equal(_bits(a[0]), _bits(b[0]))
    for e in (fresh, live, other):
        e.close()


def test_pcg_zero_is_the_default_handle(cabi):
    """A pcg = 0 handle writes the four keys as zeros and computes what a handle from gmg_config_default untouched computes, bit for bit."""
    rhs = _rhs("torus", 3)
    P = _problem("torus")
    a = cabi.Engine()
    b = cabi.Engine(pcg=0)
    for e in (a, b):
        e.set_prolongations(P.U); e.set_mass(P.mass); e.set_system(P.lhs)
    ra, rb = a.solve(rhs, tol=1e-9, stop_type=2, max_iter=6), b.solve(rhs, tol=1e-9, stop_type=2, max_iter=6)
    assert ra[1] == rb[1] and _bits(ra[2]) == _bits(rb[2]) and np.array_equal(_bits(ra[0]), _bits(rb[0])) and np.array_equal(_bits(ra[3][:, 1]), _bits(rb[3][:, 1]))
    for e in (a, b, _engine("torus", 0)):
        if e is not a and e is not b:
            e.solve(rhs, tol=1e-9, stop_type=2, max_iter=3)
        for key in ("pcg", "pcg_confirmations", "pcg_guard_steps", "pcg_restarts"):
            assert e.timing(key) == 0, key
    a.close(); b.close()


@pytest.mark.parametrize("cfg", [(), (("use_graph", True),)], ids=["stream", "graph"])
def test_cycles_outside_the_solve_are_unchanged_on_a_pcg_handle(cabi, cfg):
    """gmg_vcycle and gmg_run_cycles after a PCG solve on the same handle -- whose loop ran the cycle on its own vectors, under a graph too --
    give the bits of the pcg = 0 handle."""
    rhs = _rhs("torus", 3)
    out = []
    for pcg in (0, 1):
        eng = _engine("torus", pcg, cfg)
        eng.solve(rhs, tol=0.0, stop_type=2, max_iter=3)
        v = eng.vcycle(rhs, rhs)
        eng.load_problem(rhs, rhs)
        res = eng.run_cycles(4, 2)
        out.append((v, res, eng.fetch_solution()))
        eng.solve(rhs, tol=0.0, stop_type=2, max_iter=3)
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(_bits(a), _bits(b))


def test_dropin_option(cabi):
    """set_engine_option("pcg", 1) with the Chebyshev smoother, then solve() on the torus smoothing system: a solution within the tolerance, and
    the engine that computed it says pcg = 1."""
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
    solver.set_engine_option("smoother", CHEBYSHEV)
    solver.set_engine_option("pcg", 1)
    x = solver.solve(lhs, rhs)
    assert solver.residual(lhs, rhs, x, 2) <= 1e-6
    eng = cabi.Engine.borrow(solver.solver.engine_handle())
    assert eng.timing("pcg") == 1 and eng.timing("pcg_confirmations") >= 1
