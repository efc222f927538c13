"""gmg_solve_device / gmg_set_system_values_device on a real device: the solve loop and the values-only refresh fed from caller-owned device
memory (torch tensors) must give the bits of the host entry points on a second handle fed the same data from the host -- the permutation only
moves doubles, everything behind it is the same code, so every comparison here is exact."""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import problems

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "gravo_mg_amd", "dropin")
DEV = "cuda:0"
TOL, MAX_ITER = 1e-9, 6          # a handful of cycles: the loop's decisions (tolerance / max_iter) are part of what is compared
LAYOUTS = ("contiguous", "colmajor", "view", "alias")


def _torus():
    return problems.torus_problem(n1=37, n2=29, lower_bound=60)          # 1 073 rows: not a multiple of 64, 17 wavefronts


def _problem(name):
    if name == "torus":
        return _torus()
    if name == "bilaplacian":
        return problems.torus_problem(n1=37, n2=29, kind="bilaplacian", lower_bound=60)
    return problems.pointcloud_problem(n=3000)


@functools.lru_cache(maxsize=None)
def _engines(name, cfg):
    """(device-fed handle, host-fed handle) with the same configuration and system."""
    from gravo_mg_amd import cabi
    P = _problem(name)
    out = []
    for _ in range(2):
        eng = cabi.Engine(**dict(cfg))
        eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
        out.append(eng)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _data(name, d):
    """(rhs, x0) as host arrays, n x d; x0 differs from rhs in every entry."""
    P = _problem(name)
    rng = np.random.default_rng(100 + d)
    rhs = P.mass[:, None] * rng.standard_normal((P.n, d))
    x0 = 0.5 * rhs + 1e-3 * rng.standard_normal((P.n, d))
    rhs.setflags(write=False); x0.setflags(write=False)
    return rhs, x0


@functools.lru_cache(maxsize=None)
def _host_reference(name, cfg, d, with_x0):
    """gmg_solve_x0_rhs / gmg_solve on the host-fed handle: (x, iterations, residue, residues per cycle)."""
    rhs, x0 = _data(name, d)
    x, it, res, conv = _engines(name, cfg)[1].solve(rhs, x0=x0 if with_x0 else None, tol=TOL, stop_type=2, max_iter=MAX_ITER)
    x = np.ascontiguousarray(x.reshape(rhs.shape))
    x.setflags(write=False)
    return x, it, res, conv[:, 1].copy()


def _place(torch, a, layout):
    """a (n x d, host) as a device tensor in the given layout; returns (tensor that owns the memory, n x d view)."""
    n, d = a.shape
    if layout == "colmajor":
        own = torch.tensor(np.ascontiguousarray(a.T), device=DEV)
        return own, own.T
    if layout == "view":                                   # columns 1 .. d of a wider tensor whose other columns must stay as they are
        own = torch.full((n, d + 3), float("nan"), dtype=torch.float64, device=DEV)
        own[:, 1:1 + d] = torch.tensor(a, device=DEV)
        return own, own[:, 1:1 + d]
    own = torch.tensor(np.ascontiguousarray(a), device=DEV)
    return own, own


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _compare(torch, name, cfg, d, layout, with_x0):
    eng = _engines(name, cfg)[0]
    rhs, x0 = _data(name, d)
    want_x, want_it, want_res, want_conv = _host_reference(name, cfg, d, with_x0)
    _, b = _place(torch, rhs, "contiguous" if layout == "alias" else layout)
    g = _place(torch, x0, layout if layout != "alias" else "colmajor")[1] if with_x0 else None
    if layout == "alias":
        x_own = x = b                                       # x IS rhs: same pointer, same strides
    else:
        x_own, x = _place(torch, np.full(rhs.shape, np.nan), layout)
    assert tuple(b.shape) == (rhs.shape[0], d) and (layout != "view" or b.stride() == (d + 3, 1))
    assert layout != "colmajor" or d == 1 or b.stride() == (1, rhs.shape[0])              # (torch reports a one-column tensor as contiguous)
    torch.cuda.synchronize()
    it, res, conv = eng.solve_device(b.data_ptr(), b.stride(), x.data_ptr(), x.stride(), d, x0_ptr=0 if g is None else g.data_ptr(),
                                     x0_strides=(0, 0) if g is None else g.stride(), tol=TOL, stop_type=2, max_iter=MAX_ITER)
    got = x.cpu().numpy()
    print(f"{name} d={d} {layout} x0={'given' if with_x0 else 'rhs'}: iterations {it} / {want_it}, residue {res!r} / {want_res!r}, "
          f"differing entries {int((_bits(got) != _bits(want_x)).sum())}")
    assert np.array_equal(_bits(got), _bits(want_x))
    assert it == want_it and _bits(res) == _bits(want_res)
    assert np.array_equal(_bits(conv[:, 1]), _bits(want_conv))
    assert not eng.diverged
    if layout == "view":                                    # nothing outside the d columns was written
        other = torch.cat([x_own[:, :1], x_own[:, 1 + d:]], dim=1)
        assert bool(torch.isnan(other).all())
    if layout != "alias":                                   # ... and the inputs were only read
        assert np.array_equal(_bits(b.cpu().numpy()), _bits(rhs))
    if g is not None:
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(x0))


@pytest.mark.parametrize("with_x0", [False, True], ids=["x0_rhs", "x0_given"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", [1, 3, 4, 5])
def test_bitwise_parity_with_the_host_path(cabi, d, layout, with_x0):
    """d = 1, 3, 4 take the compile-time paths of the two permutation kernels, d = 5 the run-time one; every layout, x aliasing rhs included."""
    import torch
    _compare(torch, "torus", (), d, layout, with_x0)


@pytest.mark.parametrize("name,cfg", [
    ("torus", (("inner_precision", 1),)),
    ("torus", (("use_graph", True),)),
    ("torus", (("smoother", 1),)),
    ("torus", (("speculate_head", False),)),
    ("pointcloud", ()),
    ("bilaplacian", ()),
], ids=["inner_precision", "use_graph", "jacobi", "no_speculated_head", "pointcloud_blocked_level0", "bilaplacian"])
def test_bitwise_parity_in_other_configurations(cabi, name, cfg):
    import torch
    if name == "pointcloud":
        assert _engines(name, cfg)[0].level_blocks(0) is not None, "the point cloud's level 0 should run the block sweep (gmg_config::block_fine)"
    for with_x0 in (False, True):
        _compare(torch, name, cfg, 3, "view", with_x0)


def test_solve_is_ordered_behind_the_stream_that_made_rhs(cabi):
    """gmg_set_stream at a non-default torch stream, rhs computed by torch operations on that stream behind a long-running product, no
    synchronisation before the call."""
    import torch
    eng = _engines("torus", ())[0]
    rhs, _ = _data("torus", 3)
    host_rhs = rhs * 3.0 + 0.25                                                   # one multiply, one add per entry: rounds as the two torch kernels do
    want, want_it, want_res, _ = _engines("torus", ())[1].solve(host_rhs, tol=TOL, stop_type=2, max_iter=MAX_ITER)
    base = torch.tensor(rhs, device=DEV)
    big = torch.randn(4096, 4096, device=DEV)
    x = torch.full(rhs.shape, float("nan"), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    eng.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            for _ in range(8):
                big = big @ big * 1e-3                                              # some milliseconds of work in front of rhs
            b = base * 3.0 + 0.25
            it, res, _ = eng.solve_device(b.data_ptr(), b.stride(), x.data_ptr(), x.stride(), 3, tol=TOL, stop_type=2, max_iter=MAX_ITER)
    finally:
        eng.set_stream(0)
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(want.reshape(rhs.shape)))
    assert it == want_it and _bits(res) == _bits(want_res)


def test_rows_further_apart_than_2_to_31_elements(cabi):
    """row_stride * n past 2^31: the kernels' offsets are 64 bits wide.  One 18 GB allocation of which 2 x 1 073 x 2 doubles are touched."""
    import torch
    eng = _engines("torus", ())[0]
    rhs, _ = _data("torus", 2)
    n = rhs.shape[0]
    rs = 2_100_000
    assert (n - 1) * rs > 2**31
    try:
        big = torch.empty((n - 1) * rs + 8, dtype=torch.float64, device=DEV)
    except torch.OutOfMemoryError:
        pytest.skip("no 18 GB of device memory free")
    b = big.as_strided((n, 2), (rs, 1))
    x = big[4:].as_strided((n, 2), (rs, 1))
    b.copy_(torch.tensor(rhs, device=DEV))
    torch.cuda.synchronize()
    want, want_it, _, _ = _host_reference("torus", (), 2, False)
    it, _, _ = eng.solve_device(b.data_ptr(), b.stride(), x.data_ptr(), x.stride(), 2, tol=TOL, stop_type=2, max_iter=MAX_ITER)
    assert it == want_it and np.array_equal(_bits(x.cpu().numpy()), _bits(want))
    del b, x, big
    torch.cuda.empty_cache()


def _mass_stiffness_values(P):
    """(indptr, indices, m, s): M and S of the problem as value arrays over ONE sorted CSC pattern (that of S, which holds every diagonal entry)."""
    S = sp.csc_matrix(P.S)
    S.sort_indices()
    n = S.shape[0]
    col = np.repeat(np.arange(n), np.diff(S.indptr))
    assert (np.bincount(col[S.indices == col], minlength=n) == 1).all()
    m = np.where(S.indices == col, P.mass[col], 0.0)
    return S.indptr.astype(np.int32), S.indices.astype(np.int32), m, S.data.astype(np.float64)


def test_values_refresh_from_device_memory(cabi):
    import torch
    P = _torus()
    indptr, indices, m, s = _mass_stiffness_values(P)

    def system(tau):
        return sp.csc_matrix((m + tau * s, indices, indptr), shape=(P.n, P.n))      # one multiply, one add per entry

    engs = []
    for tau in (1e-3, 5e-3):
        eng = cabi.Engine()
        eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(system(tau))
        engs.append(eng)
    dev, ref = engs
    m_t, s_t = torch.tensor(m, device=DEV), torch.tensor(s, device=DEV)
    vals = m_t + 5e-3 * s_t
    assert np.array_equal(_bits(vals.cpu().numpy()), _bits(system(5e-3).data))
    torch.cuda.synchronize()
    dev.set_system_values_device(vals.data_ptr(), vals.numel())
    assert dev.timing("setup_values_only") == 1.0
    for k in range(dev.num_levels + 1):
        a, b = dev.level_operator(k), ref.level_operator(k)
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices), k
        print(f"level {k}: {int((_bits(a.data) != _bits(b.data)).sum())} of {a.nnz} values differ")
        assert np.array_equal(_bits(a.data), _bits(b.data)), k
    rhs, _ = _data("torus", 3)
    want, want_it, want_res, _ = ref.solve(rhs, tol=TOL, stop_type=2, max_iter=MAX_ITER)
    b = torch.tensor(rhs, device=DEV)
    x = torch.empty_like(b)
    it, res, _ = dev.solve_device(b.data_ptr(), b.stride(), x.data_ptr(), x.stride(), 3, tol=TOL, stop_type=2, max_iter=MAX_ITER)
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(want.reshape(rhs.shape))) and it == want_it and _bits(res) == _bits(want_res)


def test_values_refresh_keeps_the_sign_test_of_a_blocked_level0(cabi):
    """Level 0 of the point cloud runs the block sweep because its values pass the sign test; values with one positive off-diagonal entry
    are refused before anything is copied, and the old system goes on solving."""
    import torch
    P = _problem("pointcloud")
    A = sp.csc_matrix(P.lhs)
    A.sort_indices()
    eng = cabi.Engine()
    eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(A)
    assert eng.level_blocks(0) is not None
    rhs, _ = _data("pointcloud", 3)
    want, want_it, want_res, _ = _host_reference("pointcloud", (), 3, False)
    col = np.repeat(np.arange(P.n), np.diff(A.indptr))
    p = int(np.nonzero(A.indices != col)[0][A.nnz // 3])
    bad = A.data.copy()
    bad[p] = abs(bad[p]) + 1.0
    vals = torch.tensor(bad, device=DEV)
    torch.cuda.synchronize()
    with pytest.raises(cabi.GmgError) as ei:
        eng.set_system_values_device(vals.data_ptr(), vals.numel())
    assert ei.value.code == cabi.GMG_ERR_STATE and "full set-up" in str(ei.value)
    b = torch.tensor(rhs, device=DEV)
    x = torch.empty_like(b)
    it, res, _ = eng.solve_device(b.data_ptr(), b.stride(), x.data_ptr(), x.stride(), 3, tol=TOL, stop_type=2, max_iter=MAX_ITER)
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(want)) and it == want_it and _bits(res) == _bits(want_res)
    # ... and values that pass it are taken
    good = torch.tensor(A.data * 2.0, device=DEV)
    torch.cuda.synchronize()
    eng.set_system_values_device(good.data_ptr(), good.numel())
    assert eng.timing("setup_values_only") == 1.0 and eng.level_blocks(0) is not None


def test_error_paths_launch_nothing(cabi):
    import ctypes as C
    import torch
    P = _torus()
    b = torch.tensor(_data("torus", 1)[0], device=DEV)
    x = torch.empty_like(b)
    vals = torch.zeros(16, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    args = (b.data_ptr(), b.stride(), x.data_ptr(), x.stride(), 1)
    # before any system
    fresh = cabi.Engine()
    fresh.set_prolongations(P.U)
    for call in (lambda: fresh.set_system_values_device(vals.data_ptr(), vals.numel()), lambda: fresh.solve_device(*args)):
        with pytest.raises(cabi.GmgError) as ei:
            call()
        assert ei.value.code == cabi.GMG_ERR_STATE
    eng = _engines("torus", ())[0]
    with pytest.raises(cabi.GmgError) as ei:
        eng.set_system_values_device(vals.data_ptr(), vals.numel())               # not the live system's nnz
    assert ei.value.code == cabi.GMG_ERR_STATE
    it, res = C.c_int(), C.c_double()
    assert cabi.lib().gmg_solve_device(eng._h, None, 1, TOL, 2, MAX_ITER, C.byref(it), C.byref(res), None) == cabi.GMG_ERR_INVALID       # v == NULL
    for bad in ((b.data_ptr(), b.stride(), 0, x.stride(), 1),                     # x == NULL
                (0, b.stride(), x.data_ptr(), x.stride(), 1),                     # rhs == NULL
                (b.data_ptr(), b.stride(), x.data_ptr(), x.stride(), 0),          # d == 0
                (b.data_ptr(), (0, 1), x.data_ptr(), x.stride(), 1),              # row stride 0
                (b.data_ptr(), b.stride(), x.data_ptr(), (0, 1), 1),
                (b.data_ptr(), b.stride(), x.data_ptr(), (-1, 1), 1)):
        with pytest.raises(cabi.GmgError) as ei:
            eng.solve_device(*bad)
        assert ei.value.code == cabi.GMG_ERR_INVALID, bad
    with pytest.raises(cabi.GmgError) as ei:
        eng.solve_device(*args, x0_ptr=b.data_ptr(), x0_strides=(0, 1))           # x0 given: its row stride counts
    assert ei.value.code == cabi.GMG_ERR_INVALID
    # the handle is none the worse for it
    want, want_it, _, _ = _host_reference("torus", (), 1, False)
    it2, _, _ = eng.solve_device(*args, tol=TOL, stop_type=2, max_iter=MAX_ITER)
    assert it2 == want_it and np.array_equal(_bits(x.cpu().numpy()), _bits(want))


# ---- the drop-in: gravomg.MultigridSolver.solve_device ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gravomg(cabi):
    import glob
    if not glob.glob(os.path.join(DROPIN, "gravomg_bindings*.so")):
        import __graft_entry__
        __graft_entry__.build()
    if DROPIN not in sys.path:
        sys.path.insert(0, DROPIN)
    import gravomg as g
    return g


def _dropin_solver(gravomg):
    from gravo_mg_amd import meshgen
    V, F = meshgen.torus_mesh(37, 29)
    S, mass = meshgen.cotan_laplacian(V, F)
    solver = gravomg.MultigridSolver(V, gravomg.neighbors_from_stiffness(S), sp.diags(mass).tocsr(), lower_bound=60, tolerance=TOL, max_iter=MAX_ITER)
    solver.set_engine_option("coarse_mode", 2)              # both objects of a comparison on the same engine options
    return solver, V, problems.Problem(V, S, mass, None, S, None, "dropin-torus")           # (lhs = S: only its shape is used, Problem.n)


def test_dropin_flow_steps_from_resident_tensors(cabi, gravomg):
    """Three steps of the demos' loop (lhs = M + tau S, rhs = M V, V = solve(lhs, rhs), V rescaled): scipy lhs on step 1, a values tensor on
    steps 2 and 3, against three solve() calls of a second object; then solve() on the FIRST object with the first matrix -- whose digest its
    pybind mirror still remembers as "the live system" -- must return that matrix's solution."""
    import torch
    dev, V, P = _dropin_solver(gravomg)
    ref, _, _ = _dropin_solver(gravomg)
    indptr, indices, m, s = _mass_stiffness_values(P)
    taus = (1e-3, 5e-3, 2e-2)
    lhs = [sp.csc_matrix((m + tau * s, indices, indptr), shape=(P.n, P.n)) for tau in taus]
    m_t, s_t, mass_t = torch.tensor(m, device=DEV), torch.tensor(s, device=DEV), torch.tensor(P.mass, device=DEV)
    Vh, Vd = V.copy(), torch.tensor(V, device=DEV)
    host_steps = []
    for k, tau in enumerate(taus):
        rhs_h = P.mass[:, None] * Vh
        Vh = ref.solve(lhs[k], rhs_h) * 0.75
        host_steps.append((rhs_h, Vh))
        rhs_d = mass_t[:, None] * Vd
        out = dev.solve_device(lhs[0] if k == 0 else m_t + tau * s_t, rhs_d)
        assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (P.n, 3) and out.data_ptr() != rhs_d.data_ptr()
        assert dev.device_info["iterations"] >= 1 and np.isfinite(dev.device_info["residue"]) and dev.device_info["diverged"] is False
        Vd = out * 0.75
        print(f"step {k}: {int((_bits(Vd.cpu().numpy()) != _bits(Vh)).sum())} entries differ, {dev.device_info}")
        assert np.array_equal(_bits(Vd.cpu().numpy()), _bits(Vh)), k
    # lhs = None keeps the live system (tau = 2e-2); x0 given
    rhs_h, _ = host_steps[2]
    again = dev.solve_device(None, torch.tensor(rhs_h, device=DEV), x0=torch.tensor(rhs_h, device=DEV))
    assert np.array_equal(_bits(again.cpu().numpy() * 0.75), _bits(host_steps[2][1]))
    # the stale-generation trap
    rhs_h, want = host_steps[0]
    got = dev.solve(lhs[0], rhs_h) * 0.75
    assert np.array_equal(_bits(got), _bits(want))


def test_dropin_rejects_wrong_tensors_before_the_engine_is_called(cabi, gravomg):
    import torch
    solver, V, P = _dropin_solver(gravomg)
    indptr, indices, m, s = _mass_stiffness_values(P)
    lhs = sp.csc_matrix((m + 1e-3 * s, indices, indptr), shape=(P.n, P.n))
    good = torch.tensor(P.mass[:, None] * V, device=DEV)
    with pytest.raises(TypeError, match="rhs"):
        solver.solve_device(lhs, good.cpu())
    with pytest.raises(TypeError, match="rhs"):
        solver.solve_device(lhs, good.float())
    with pytest.raises(TypeError, match="rhs"):
        solver.solve_device(lhs, P.mass[:, None] * V)                              # numpy is solve()'s business
    with pytest.raises(TypeError, match="x0"):
        solver.solve_device(lhs, good, x0=good.cpu())
    with pytest.raises(TypeError, match="lhs"):
        solver.solve_device(torch.tensor(lhs.data), good)                          # a CPU tensor of values
    with pytest.raises(TypeError, match="lhs"):
        solver.solve_device(torch.tensor(lhs.data, device=DEV).float(), good)
    with pytest.raises(ValueError, match="rhs"):
        solver.solve_device(lhs, good[:-1])
    with pytest.raises(ValueError, match="x0"):
        solver.solve_device(lhs, good, x0=good[:, :2])
    # none of these calls got as far as the engine: the one the constructor made still holds no system
    handle = solver.solver.engine_handle()
    if handle:
        with pytest.raises(cabi.GmgError) as ei:
            cabi.Engine.borrow(handle).level_info(0)
        assert ei.value.code == cabi.GMG_ERR_STATE
    with pytest.raises(RuntimeError, match="no system set|no live system"):
        solver.solve_device(torch.tensor(lhs.data, device=DEV), good)              # values before any system
    out = solver.solve_device(lhs, good)                                           # ... and the object is none the worse for it
    assert tuple(out.shape) == (P.n, 3) and 1 <= solver.device_info["iterations"] <= MAX_ITER
