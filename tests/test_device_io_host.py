"""Device-resident entry points (gmg_solve_device, gmg_set_system_values_device), the part that needs no device: the boundary's tables, the
struct mirror, the loud failure on a box without a GPU, the drop-in method without torch, and the host-only argument checks
(gravo_mg_amd/csrc/device_io_check.hpp) run from a stand-alone program built with AddressSanitizer + UBSan."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

from tests import problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "gravo_mg_amd", "dropin")


def test_both_entry_points_are_in_the_boundary_tables(cabi):
    assert "gmg_solve_device" in cabi.SIGNATURES and "gmg_set_system_values_device" in cabi.SIGNATURES
    assert len(cabi.SIGNATURES) == 75
    lib = cabi.lib()
    assert lib.gmg_solve_device.argtypes[1] == C.POINTER(cabi.GmgDeviceVectors)


def test_struct_mirror_is_three_pointer_stride_triples(cabi):
    assert C.sizeof(cabi.GmgDeviceVectors) == 72
    assert [f[0] for f in cabi.GmgDeviceVectors._fields_] == ["rhs", "rhs_row_stride", "rhs_col_stride", "x0", "x0_row_stride", "x0_col_stride",
                                                              "x", "x_row_stride", "x_col_stride"]
    assert cabi.GmgDeviceVectors.x.offset == 48 and cabi.GmgDeviceVectors.x0_col_stride.offset == 40


def test_entry_points_fail_loudly_without_a_gpu(cabi):
    """No CPU fallback: GMG_ERR_NO_DEVICE from both entry points (before any argument is looked at), or from the handle's creation."""
    if cabi.device_count() > 0:
        pytest.skip("a HIP device is present")
    try:
        eng = cabi.Engine()
    except cabi.GmgError as e:
        assert e.code == cabi.GMG_ERR_NO_DEVICE
        return
    P = problems.torus_problem(24, 20, "poisson", 20)
    eng.set_prolongations(P.U)
    with pytest.raises(cabi.GmgError) as ei:
        eng.solve_device(0, (1, 1), 0, (1, 1), 1)
    assert ei.value.code == cabi.GMG_ERR_NO_DEVICE
    with pytest.raises(cabi.GmgError) as ei:
        eng.set_system_values_device(0, 0)
    assert ei.value.code == cabi.GMG_ERR_NO_DEVICE
    v = cabi.GmgDeviceVectors()
    assert cabi.lib().gmg_solve_device(eng._h, C.byref(v), 1, 1e-4, 2, 10, None, None, None) == cabi.GMG_ERR_NO_DEVICE
    assert cabi.lib().gmg_solve_device(None, C.byref(v), 1, 1e-4, 2, 10, None, None, None) == cabi.GMG_ERR_INVALID


def test_dropin_imports_and_documents_solve_device_without_torch(cabi):
    """`import gravomg` must not import torch; solve_device imports it inside the call only."""
    import glob
    if not glob.glob(os.path.join(DROPIN, "gravomg_bindings*.so")):
        import __graft_entry__
        __graft_entry__.build()
    code = ("import sys; sys.path.insert(0, %r); import gravomg; assert 'torch' not in sys.modules, 'import gravomg imported torch'; "
            "doc = gravomg.MultigridSolver.solve_device.__doc__; assert doc and 'torch' in doc and 'stream' in doc; "
            "assert 'torch' not in sys.modules; print('ok')" % DROPIN)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


_CHECK_MAIN = r"""
#include <cstdio>
#include <cstring>
#include "device_io_check.hpp"
using namespace gmg;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
int main() {
    double buf[4];                       // never dereferenced by the checks: only the pointer values matter
    int64_t e = -1;
    EXPECT(strided_extent(1073, 3, 3, 1, &e) && e == 1072 * 3 + 2);
    EXPECT(strided_extent(1073, 3, 1, 1073, &e) && e == 1072 + 2 * 1073);
    EXPECT(strided_extent(1, 1, 7, 0, &e) && e == 0);
    EXPECT(strided_extent(3000000, 5, (int64_t)1 << 20, 1, &e) && e == 2999999 * ((int64_t)1 << 20) + 4);     // past 2^31, fine in 64 bits
    EXPECT(!strided_extent(0, 1, 1, 1, &e) && !strided_extent(4, 0, 1, 1, &e));
    EXPECT(!strided_extent(4, 2, -1, 1, &e) && !strided_extent(4, 2, 1, -4, &e));
    EXPECT(!strided_extent(INT32_MAX, 2, INT64_MAX / 2, 1, &e));                  // the product overflows
    EXPECT(!strided_extent(2, 2, INT64_MAX / 2, INT64_MAX / 2 + 2, &e));          // the sum overflows
    EXPECT(!strided_extent(2, 1, INT64_MAX / 8, 1, &e));                          // the byte offset would
    gmg_device_vectors v;
    std::memset(&v, 0, sizeof(v));
    EXPECT(device_vectors_fault(nullptr, 10, 1) != nullptr);
    v.rhs = buf; v.rhs_row_stride = 1; v.rhs_col_stride = 10;
    EXPECT(device_vectors_fault(&v, 10, 1) != nullptr);                          // x is NULL
    v.x = buf; v.x_row_stride = 1; v.x_col_stride = 10;
    EXPECT(device_vectors_fault(&v, 10, 1) == nullptr);
    EXPECT(device_vectors_fault(&v, 10, 3) == nullptr);
    EXPECT(device_vectors_fault(&v, 10, 0) != nullptr && device_vectors_fault(&v, 10, -2) != nullptr);
    v.rhs = nullptr;
    EXPECT(device_vectors_fault(&v, 10, 1) != nullptr);
    v.rhs = buf; v.rhs_row_stride = 0;
    EXPECT(device_vectors_fault(&v, 10, 1) != nullptr);
    v.rhs_row_stride = 1; v.x_row_stride = 0;
    EXPECT(device_vectors_fault(&v, 10, 1) != nullptr);
    v.x_row_stride = 3; v.x_col_stride = 0;
    EXPECT(device_vectors_fault(&v, 10, 1) == nullptr && device_vectors_fault(&v, 10, 3) != nullptr);       // columns of x on top of each other
    v.x_col_stride = 1;
    v.x0 = buf; v.x0_row_stride = 0; v.x0_col_stride = 1;
    EXPECT(device_vectors_fault(&v, 10, 3) != nullptr);                          // x0 given: its row stride counts
    v.x0_row_stride = 3;
    EXPECT(device_vectors_fault(&v, 10, 3) == nullptr);
    v.x0_col_stride = -1;
    EXPECT(device_vectors_fault(&v, 10, 3) != nullptr);
    v.x0 = nullptr;
    EXPECT(device_vectors_fault(&v, 10, 3) == nullptr);                          // x0 == NULL: its strides are not looked at
    v.rhs_col_stride = 0;
    EXPECT(device_vectors_fault(&v, 10, 3) == nullptr);                          // a broadcast rhs may be read
    std::printf(fails ? "%d checks failed\n" : "all checks passed\n", fails);
    return fails ? 1 : 0;
}
"""


def test_argument_checks_under_address_and_ub_sanitizers(tmp_path):
    """The shape checks of gmg_solve_device are header-only host code: a stand-alone program calls them with boundary strides (64-bit products,
    overflow, zero, negative) under -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "check_main.cpp"
    src.write_text(_CHECK_MAIN)
    exe = tmp_path / "check_main"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gravo_mg_amd", "csrc"),
                            str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout + run.stderr
