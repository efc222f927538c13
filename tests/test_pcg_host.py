"""gmg_config::pcg, the part that needs no device: the configuration mirror, the refusals gmg_create makes before it looks for a device, the
drop-in's option, the scalar decisions of the loop (gravo_mg_amd/csrc/pcg_scalars.hpp, the code the reducing kernels call) run from a
stand-alone program built with AddressSanitizer + UBSan, and the numpy model of the loop (tests/pcg_model.py) -- against scipy's CG, and on the
system the feature is for: the Bilaplacian on which the plain loop around the same cycle does not converge.

Measured with the model (ChebyshevModel cycle, ratio 8, 2 + 2, x0 = rhs, stop type 2, one right-hand side) on the Bilaplacian torus: 35 iterations
to 1e-4; 60 plain cycles of the same model end at a residue of 1.7."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import problems
from tests.accelerate_model import plain_loop
from tests.chebyshev_model import ChebyshevModel
from tests.pcg_model import pcg_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "gravo_mg_amd", "dropin")


def test_config_mirror_has_pcg_in_front_of_accelerate(cabi):
    """In front of device_coloring, the field added before it (tests/test_jp_coloring_host.py pins that one next to accelerate): accelerate stays
    the last field and the size changes, so a binding built against the parent's header is refused."""
    names = [f[0] for f in cabi.GmgConfig._fields_]
    assert names[-3:] == ["pcg", "device_coloring", "accelerate"] and cabi.GmgConfig._fields_[-3] == ("pcg", C.c_int)
    assert C.sizeof(cabi.GmgConfig) == cabi.lib().gmg_config_size()
    cfg = cabi.GmgConfig()
    cfg.pcg = 7
    assert cabi.lib().gmg_config_default(C.byref(cfg)) == 0 and cfg.pcg == 0 and cfg.accelerate == 0


def _refused(cabi, **kw):
    with pytest.raises(cabi.GmgError) as ei:
        cabi.Engine(**kw)
    return ei.value


def test_create_refuses_without_a_device(cabi):
    """Every refusal comes before the device is looked for: the same codes on a box without a GPU."""
    assert cabi.SMOOTHER_JACOBI == 1 and cabi.SMOOTHER_CHEBYSHEV == 2
    for bad in (-1, 2, 100):
        assert _refused(cabi, pcg=bad, smoother=cabi.SMOOTHER_CHEBYSHEV).code == cabi.GMG_ERR_INVALID
    unsupported = [
        dict(pcg=1),                                                                        # the default smoother: Gauss-Seidel
        dict(pcg=1, smoother=cabi.SMOOTHER_MULTICOLOR_GS),
        dict(pcg=1, smoother=cabi.SMOOTHER_CHEBYSHEV, pre_iters=2, post_iters=1),
        dict(pcg=1, smoother=cabi.SMOOTHER_JACOBI, pre_iters=1, post_iters=3),
        dict(pcg=1, smoother=cabi.SMOOTHER_CHEBYSHEV, pre_iters=0, post_iters=0),
        dict(pcg=1, smoother=cabi.SMOOTHER_CHEBYSHEV, accelerate=2),
        dict(pcg=1, smoother=cabi.SMOOTHER_CHEBYSHEV, inner_precision=1),
    ]
    for kw in unsupported:
        e = _refused(cabi, **kw)
        assert e.code == cabi.GMG_ERR_UNSUPPORTED and "pcg" in str(e), (kw, str(e))
    # what is allowed: both pointwise smoothers, any equal degree; and pcg = 0 handles are unaffected
    allowed = [dict(pcg=1, smoother=cabi.SMOOTHER_CHEBYSHEV), dict(pcg=1, smoother=cabi.SMOOTHER_JACOBI, pre_iters=1, post_iters=1),
               dict(pcg=1, smoother=cabi.SMOOTHER_CHEBYSHEV, pre_iters=3, post_iters=3, use_graph=True),
               dict(pcg=0), dict(pcg=0, pre_iters=2, post_iters=1), dict(pcg=0, accelerate=2), dict(pcg=0, inner_precision=1),
               dict(pcg=0, smoother=cabi.SMOOTHER_CHEBYSHEV, pre_iters=2, post_iters=1)]
    for kw in allowed:
        try:
            cabi.Engine(**kw).close()
        except cabi.GmgError as e:
            assert cabi.device_count() == 0 and e.code == cabi.GMG_ERR_NO_DEVICE, (kw, str(e))
    # a refusal's message does not outlive the next gmg_create of the thread
    e = _refused(cabi, accelerate=9)
    assert e.code == cabi.GMG_ERR_INVALID and "pcg" not in str(e)


def test_dropin_accepts_the_option(cabi):
    import glob
    if not glob.glob(os.path.join(DROPIN, "gravomg_bindings*.so")):
        import __graft_entry__
        __graft_entry__.build()
    if DROPIN not in sys.path:
        sys.path.insert(0, DROPIN)
    import gravomg
    from gravo_mg_amd import meshgen
    V, F = meshgen.torus_mesh(24, 20)
    S, mass = meshgen.cotan_laplacian(V, F)
    solver = gravomg.MultigridSolver(V, gravomg.neighbors_from_stiffness(S), sp.diags(mass).tocsr(), lower_bound=40)
    solver.set_engine_option("pcg", 1)
    with pytest.raises(Exception):
        solver.set_engine_option("pcg_more", 1)
    assert "pcg" in gravomg.MultigridSolver.set_engine_option.__doc__


_SCALARS_MAIN = r"""
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>
#include "pcg_scalars.hpp"
using namespace gmg;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double tiny = std::numeric_limits<double>::denorm_min(), huge = std::numeric_limits<double>::max();
    // normal values
    PcgStep st = pcg_step(4.0, 2.0, 1.0, 0.0);
    EXPECT(!st.guarded && st.alpha == 0.5);
    st = pcg_step(4.0, -2.0, 1.0, 0.0);                      // a negative rho is no guard: the step still minimises the energy along p
    EXPECT(!st.guarded && st.alpha == -0.5);
    st = pcg_step(4.0, 0.0, 1.0, 0.0);                       // rho = 0: no guard, the step is empty by itself
    EXPECT(!st.guarded && st.alpha == 0.0);
    st = pcg_step(tiny, tiny, 1.0, 0.0);                     // a denormal is positive: it divides
    EXPECT(!st.guarded && st.alpha == 1.0);
    st = pcg_step(huge, 1.0, 1.0, 0.0);
    EXPECT(!st.guarded && st.alpha == 1.0 / huge);
    EXPECT(pcg_beta(6.0, 3.0, false) == 2.0 && pcg_beta(-6.0, 3.0, false) == -2.0 && pcg_beta(0.0, 3.0, false) == 0.0);
    // the first iteration, the iteration after a guard or after a recomputed residual: beta = 0 whatever the sums are
    for (double prev : {3.0, 0.0, inf, nan, tiny}) EXPECT(pcg_beta(6.0, prev, true) == 0.0);
    EXPECT(pcg_beta(nan, 3.0, true) == 0.0 && pcg_beta(inf, nan, true) == 0.0);
    // a previous rho that cannot be divided by, a rho that is not finite: beta = 0, never a NaN or an infinity
    for (double prev : {0.0, -0.0, inf, -inf, nan}) EXPECT(pcg_beta(6.0, prev, false) == 0.0);
    for (double rho : {inf, -inf, nan}) EXPECT(pcg_beta(rho, 3.0, false) == 0.0);
    EXPECT(pcg_beta(tiny, tiny, false) == 1.0);
    // <p, q> zero, negative, not finite: the guard, alpha = 0, whatever rho is
    for (double pq : {0.0, -0.0, -1.0, -tiny, -huge, inf, -inf, nan})
        for (double rho : {0.0, 1.0, -1.0, inf, nan}) {
            st = pcg_step(pq, rho, 1.0, 0.0);
            EXPECT(st.guarded == 1 && st.alpha == 0.0 && !std::signbit(st.alpha));
        }
    // rho not finite with a usable <p, q>: the guard
    for (double rho : {inf, -inf, nan}) {
        st = pcg_step(2.0, rho, 1.0, 0.0);
        EXPECT(st.guarded == 1 && st.alpha == 0.0);
    }
    // the floor: sum w r^2 at or below 1e-25 <b, b> freezes the column; <b, b> of 0, below 0 or NaN means "not known" -- no floor
    const double f4 = accel_floor(4.0);
    EXPECT(f4 == kAccelFloorRel2 * 4.0);
    st = pcg_step(4.0, 2.0, f4, f4);                          // on the floor: the comparison includes it
    EXPECT(st.guarded == 1 && st.alpha == 0.0);
    st = pcg_step(4.0, 2.0, 0.5 * f4, f4);
    EXPECT(st.guarded == 1 && st.alpha == 0.0);
    st = pcg_step(4.0, 2.0, 0.0, f4);                         // an exactly solved column
    EXPECT(st.guarded == 1);
    st = pcg_step(4.0, 2.0, 2.0 * f4, f4);                    // above it: an ordinary step
    EXPECT(!st.guarded && st.alpha == 0.5);
    st = pcg_step(4.0, 2.0, 0.0, accel_floor(0.0));           // no floor known (the first iteration): rr is not looked at
    EXPECT(!st.guarded && st.alpha == 0.5);
    st = pcg_step(4.0, 2.0, 0.0, accel_floor(nan));
    EXPECT(!st.guarded);
    st = pcg_step(4.0, 2.0, 0.0, accel_floor(-1.0));
    EXPECT(!st.guarded);
    st = pcg_step(4.0, 2.0, nan, f4);                         // a NaN residual sum compares false: the residue test of the loop sees it
    EXPECT(!st.guarded);
    st = pcg_step(4.0, 2.0, 1.0, accel_floor(inf));           // <b, b> not finite: everything is below it
    EXPECT(st.guarded == 1);
    std::printf(fails ? "%d checks failed\n" : "all checks passed\n", fails);
    return fails ? 1 : 0;
}
"""


def test_scalar_decisions_under_address_and_ub_sanitizers(tmp_path):
    """alpha / beta and the guards on normal values, zeros, negative values, infinities and NaNs, the floor and the first iteration: header-only
    code shared with the kernels, run from a stand-alone program under -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "pcg_scalars_main.cpp"
    src.write_text(_SCALARS_MAIN)
    exe = tmp_path / "pcg_scalars_main"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gravo_mg_amd", "csrc"),
                            str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout + run.stderr


def test_model_converges_on_the_bilaplacian_where_the_plain_loop_does_not(oracle):
    """The premise of the feature: torus Bilaplacian (tau M + S M^-1 S, tau = 1), ChebyshevModel cycle (ratio 8, 2 + 2), x0 = rhs, stop type 2.
    PCG reaches 1e-4 in at most 40 iterations (35 measured); 60 plain cycles of the same model stay above 1 (1.7 measured)."""
    P = problems.torus_problem(n1=37, n2=29, kind="bilaplacian", lower_bound=60)
    M = ChebyshevModel(None, P.U, P.mass, P.lhs, oracle, 8.0, pre=2, post=2)
    x, it, res, guards, restarts, steps, _ = pcg_loop(P.lhs, P.mass, M.vcycle, P.rhs, P.rhs, 2, 1e-4, 60)
    _, pit, pres = plain_loop(P.lhs, P.mass, M.vcycle, P.rhs, P.rhs, 2, 1e-4, 60)
    print(f"bilaplacian torus: PCG {it} iterations (residue {res[-1]:.3e}, guards {guards}, restarts {restarts}); plain loop {pit} cycles, residue {pres[-1]:.3e}")
    assert it <= 40 and res[-1] <= 1e-4 and guards == 0
    assert steps[-1]["confirmed"] and all(not s["confirmed"] for s in steps[:-1]) and restarts == 0
    r = P.rhs - P.lhs @ x
    assert abs(np.sqrt((P.mass[:, None] * r * r).sum() / (P.mass[:, None] * P.rhs ** 2).sum()) - res[-1]) <= 1e-12 * res[-1]
    assert pit == 60 and pres[-1] > 1.0


def test_model_follows_scipy_cg(oracle):
    """The first 6 iterates of the model are those of scipy.sparse.linalg.cg with the same cycle as its preconditioner, x0 = rhs, to 1e-10 of the
    largest entry.  The system: the torus' S + M (tau = 1: condition number of a few hundred after preconditioning nothing -- both sides carry
    rounding of 1e-16 times a small factor) with b = A y, y ~ N(0, 1): a solution of size 1."""
    P = problems.torus_problem(n1=37, n2=29, lower_bound=60)
    lhs = (P.S + sp.diags(P.mass)).tocsc()
    lhs.sort_indices()
    y = np.random.default_rng(7).standard_normal((P.n, 1))
    rhs = lhs @ y
    M = ChebyshevModel(None, P.U, P.mass, lhs, oracle, 8.0, pre=2, post=2)
    _, it, res, guards, restarts, _, iterates = pcg_loop(lhs, P.mass, M.vcycle, rhs, rhs, 2, 0.0, 6)
    assert it == 6 and guards == 0 and restarts == 0
    B = spla.LinearOperator(lhs.shape, matvec=lambda v: M.vcycle(np.asarray(v, dtype=np.float64).reshape(-1, 1), np.zeros((P.n, 1))).ravel(), dtype=np.float64)
    seen = []
    kw = dict(x0=rhs.ravel().copy(), maxiter=6, M=B, callback=lambda xk: seen.append(np.array(xk, copy=True)), atol=0.0)
    try:
        spla.cg(lhs.tocsr(), rhs.ravel(), rtol=0.0, **kw)
    except TypeError:          # (older scipy: the relative tolerance is called tol)
        seen.clear()
        spla.cg(lhs.tocsr(), rhs.ravel(), tol=0.0, **kw)
    assert len(seen) == 6
    scale = float(np.abs(y).max())
    devs = [float(np.abs(a.ravel() - b).max()) / scale for a, b in zip(iterates, seen)]
    print("model against scipy, per iteration:", " ".join(f"{v:.2e}" for v in devs), " residues", " ".join(f"{v:.2e}" for v in res))
    assert 1.0 < scale < 10.0 and max(devs) <= 1e-10
    assert res[-1] < 1e-3 * res[0]          # six iterations that do something
