"""gmg_config::accelerate, the part that needs no device: the configuration mirrors, the refusals gmg_create makes before it looks for a
device, the drop-in's option, and the scalar decisions of the accelerated loop (gravo_mg_amd/csrc/accel_scalars.hpp, the code the reducing
kernels call) run from a stand-alone program built with AddressSanitizer + UBSan."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "gravo_mg_amd", "dropin")


def test_config_mirror_ends_with_accelerate(cabi):
    assert cabi.GmgConfig._fields_[-1] == ("accelerate", C.c_int)
    assert C.sizeof(cabi.GmgConfig) == cabi.lib().gmg_config_size()
    cfg = cabi.GmgConfig()
    cfg.accelerate = 7
    assert cabi.lib().gmg_config_default(C.byref(cfg)) == 0 and cfg.accelerate == 0
    assert cabi.GmgConfig.accelerate.offset + C.sizeof(C.c_int) <= C.sizeof(cabi.GmgConfig)
    assert len(cabi.SIGNATURES) == 75          # the feature adds no entry point


def test_create_refuses_bad_depths_without_a_device(cabi):
    """The two checks come before the device is looked for: the same codes on a box without a GPU."""
    for depth in (-1, 5, 100):
        with pytest.raises(cabi.GmgError) as ei:
            cabi.Engine(accelerate=depth)
        assert ei.value.code == cabi.GMG_ERR_INVALID
    with pytest.raises(cabi.GmgError) as ei:
        cabi.Engine(accelerate=1, inner_precision=1)
    assert ei.value.code == cabi.GMG_ERR_UNSUPPORTED
    if cabi.device_count() == 0:
        try:
            cabi.Engine(accelerate=4).close()
        except cabi.GmgError as e:
            assert e.code == cabi.GMG_ERR_NO_DEVICE
    else:
        for depth in range(5):
            cabi.Engine(accelerate=depth).close()


def test_partition_for_several_ranks_is_refused(cabi):
    """gmg_dist_partition with world > 1 on an accelerated handle: refused before any device work; world = 1 and an unaccelerated handle are not."""
    try:
        eng, plain = cabi.Engine(accelerate=2, row_align=128), cabi.Engine(row_align=128)
    except cabi.GmgError as e:
        assert e.code == cabi.GMG_ERR_NO_DEVICE
        return
    with pytest.raises(cabi.GmgError) as ei:
        eng.dist_partition(0, 2)
    assert ei.value.code == cabi.GMG_ERR_UNSUPPORTED and "accelerate" in str(ei.value)
    eng.dist_partition(0, 1)
    plain.dist_partition(1, 2)
    eng.close(); plain.close()


def test_dropin_accepts_the_option(cabi):
    import glob
    if not glob.glob(os.path.join(DROPIN, "gravomg_bindings*.so")):
        import __graft_entry__
        __graft_entry__.build()
    if DROPIN not in sys.path:
        sys.path.insert(0, DROPIN)
    import gravomg
    import scipy.sparse as sp
    from gravo_mg_amd import meshgen
    V, F = meshgen.torus_mesh(24, 20)
    S, mass = meshgen.cotan_laplacian(V, F)
    solver = gravomg.MultigridSolver(V, gravomg.neighbors_from_stiffness(S), sp.diags(mass).tocsr(), lower_bound=40)
    solver.set_engine_option("accelerate", 2)
    with pytest.raises(Exception):
        solver.set_engine_option("accelerate_more", 2)
    assert "accelerate" in gravomg.MultigridSolver.set_engine_option.__doc__


_SCALARS_MAIN = r"""
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>
#include "accel_scalars.hpp"
using namespace gmg;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double tiny = std::numeric_limits<double>::denorm_min(), huge = std::numeric_limits<double>::max();
    static_assert(kAccelMaxDepth == 4 && kAccelMaxStored == 3, "depths");
    // the floor guard: <q, q> at or below 1e-25 <b, b> is noise; <b, b> of 0, below 0 or NaN means "not known" -- no floor
    static_assert(kAccelFloorRel2 == 1e-25, "the floor");
    EXPECT(accel_floor(4.0) == kAccelFloorRel2 * 4.0 && accel_floor(0.0) == 0.0 && accel_floor(-1.0) == 0.0 && accel_floor(nan) == 0.0 && std::isinf(accel_floor(inf)));
    AccelStep st = accel_step(accel_floor(4.0), 2e-25, accel_floor(4.0));                     // on the floor: the comparison includes it
    EXPECT(st.guarded == 1 && st.alpha == 1.0 && st.s_store == 0.0);
    st = accel_step(2.0 * accel_floor(4.0), 0.5 * accel_floor(4.0), accel_floor(4.0));      // above it: an ordinary step
    EXPECT(!st.guarded && st.alpha == 0.25 && st.s_store == 2.0 * accel_floor(4.0));
    st = accel_step(tiny, tiny, accel_floor(4.0));
    EXPECT(st.guarded == 1 && st.s_store == 0.0);
    st = accel_step(tiny, tiny, accel_floor(0.0));                         // no floor known (the first iteration): only the old guard
    EXPECT(!st.guarded && st.alpha == 1.0);
    st = accel_step(tiny, tiny, nan);                                      // a NaN floor compares false
    EXPECT(!st.guarded);
    st = accel_step(1.0, 1.0, accel_floor(inf));                           // <b, b> not finite: everything is below it
    EXPECT(st.guarded == 1);
    st = accel_step(nan, 1.0, accel_floor(4.0));
    EXPECT(st.guarded == 1 && st.alpha == 1.0);
    EXPECT(accel_beta(123.0, accel_step(1e-26, 1.0, accel_floor(1.0)).s_store) == 0.0);      // a direction on the floor is never divided by later
    // normal values
    st = accel_step(4.0, 2.0);
    EXPECT(!st.guarded && st.alpha == 0.5 && st.s_store == 4.0);
    st = accel_step(4.0, -2.0);
    EXPECT(!st.guarded && st.alpha == -0.5 && st.s_store == 4.0);
    st = accel_step(3.0, 0.0);
    EXPECT(!st.guarded && st.alpha == 0.0 && st.s_store == 3.0);
    st = accel_step(tiny, tiny);                       // a denormal is not zero: it divides
    EXPECT(!st.guarded && st.alpha == 1.0 && st.s_store == tiny);
    st = accel_step(huge, 1.0);
    EXPECT(!st.guarded && st.alpha == 1.0 / huge && st.s_store == huge);
    EXPECT(accel_beta(6.0, 3.0) == 2.0 && accel_beta(-6.0, 3.0) == -2.0 && accel_beta(0.0, 3.0) == 0.0);
    // zeros: the guard
    for (double s : {0.0, -0.0}) {
        st = accel_step(s, 5.0);
        EXPECT(st.guarded == 1 && st.alpha == 1.0 && st.s_store == 0.0 && !std::signbit(st.s_store));
        st = accel_step(s, 0.0);
        EXPECT(st.guarded == 1 && st.alpha == 1.0 && st.s_store == 0.0);
        EXPECT(accel_beta(5.0, s) == 0.0 && accel_beta(nan, s) == 0.0 && accel_beta(inf, s) == 0.0);
    }
    // infinities and NaNs in s: the guard, whatever rho is
    for (double s : {inf, -inf, nan}) {
        for (double rho : {0.0, 1.0, inf, nan}) {
            st = accel_step(s, rho);
            EXPECT(st.guarded == 1 && st.alpha == 1.0 && st.s_store == 0.0);
        }
        EXPECT(accel_beta(1.0, s) == 0.0);
        EXPECT(!accel_usable(s));
    }
    // a usable s with a rho that is not finite: no guard (the issue guards on s), the step carries it and the loop's own residue test sees it
    st = accel_step(2.0, inf);
    EXPECT(!st.guarded && std::isinf(st.alpha) && st.s_store == 2.0);
    st = accel_step(2.0, nan);
    EXPECT(!st.guarded && std::isnan(st.alpha));
    EXPECT(std::isnan(accel_beta(nan, 2.0)) && std::isinf(accel_beta(inf, 2.0)));
    // what the ring stores for a guarded direction switches that direction off for the column later on
    st = accel_step(0.0, 1.0);
    EXPECT(accel_beta(123.0, st.s_store) == 0.0);
    EXPECT(accel_usable(1.0) && accel_usable(-1.0) && accel_usable(tiny) && !accel_usable(0.0));
    std::printf(fails ? "%d checks failed\n" : "all checks passed\n", fails);
    return fails ? 1 : 0;
}
"""


def test_scalar_decisions_under_address_and_ub_sanitizers(tmp_path):
    """alpha / beta and the guard on normal values, zeros, infinities and NaNs: header-only code shared with the kernels, run from a stand-alone
    program under -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "accel_scalars_main.cpp"
    src.write_text(_SCALARS_MAIN)
    exe = tmp_path / "accel_scalars_main"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gravo_mg_amd", "csrc"),
                            str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout + run.stderr
