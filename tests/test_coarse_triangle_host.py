"""GMG_COARSE_DEVICE_TRIANGLE, the part that needs no device: the value in the header and its Python mirror, the unchanged surface (75 entry
points), the drop-in's docstring, and the index arithmetic of the packed triangle (gravo_mg_amd/csrc/coarse_triangle.hpp, the code the set-up, the
product kernels and this test share) run from a stand-alone program built with AddressSanitizer + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "gravo_mg_amd", "dropin")


def test_the_value_and_the_unchanged_surface(cabi):
    assert cabi.COARSE_DEVICE_TRIANGLE == 3
    assert (cabi.COARSE_HOST_LDLT, cabi.COARSE_DEVICE_INVERSE, cabi.COARSE_AUTO) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "gravomg_hip.h")).read()
    assert re.search(r"\bGMG_COARSE_DEVICE_TRIANGLE\s*=\s*3\b", header)
    assert len(cabi.SIGNATURES) == 75                       # the mode adds no entry point ...
    cfg = cabi.GmgConfig()
    assert cabi.lib().gmg_config_default(C.byref(cfg)) == 0 and cfg.coarse_mode == cabi.COARSE_AUTO          # ... and moves no default


def test_create_accepts_the_mode_without_a_device(cabi):
    """The value is a placement, not a refusal: on a box without a GPU gmg_create fails for the missing device, not for the argument."""
    try:
        cabi.Engine(coarse_mode=cabi.COARSE_DEVICE_TRIANGLE).close()
    except cabi.GmgError as e:
        assert cabi.device_count() == 0 and e.code == cabi.GMG_ERR_NO_DEVICE


def test_dropin_docstring_names_the_mode(cabi):
    import glob
    if not glob.glob(os.path.join(DROPIN, "gravomg_bindings*.so")):
        import __graft_entry__
        __graft_entry__.build()
    if DROPIN not in sys.path:
        sys.path.insert(0, DROPIN)
    import gravomg
    doc = gravomg.MultigridSolver.set_engine_option.__doc__
    assert "GMG_COARSE_DEVICE_TRIANGLE" in doc and "3 the packed lower triangle" in doc


_INDEX_MAIN = r"""
#include <cstdio>
#include <vector>
#include "coarse_triangle.hpp"
using namespace gmg;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { if (fails < 20) std::printf("FAILED line %d (nb = %d): %s\n", __LINE__, nb, #c); ++fails; } } while (0)
int main() {
    static_assert(kTriBlock == 64 && kTriBlockDoubles == 4096 && kTriRun >= 1 && kTriCols == 4, "layout");
    std::printf("R = %d\n", kTriRun);
    for (int nb = 1; nb <= 40; ++nb) {
        EXPECT(tri_blocks(64 * nb) == nb && tri_blocks(64 * nb - 63) == nb && tri_blocks(64 * nb + 1) == nb + 1);
        const int64_t nblk = tri_block_count(nb);
        EXPECT(nblk == (int64_t)nb * (nb + 1) / 2);
        // the block offsets are a bijection onto [0, nb (nb + 1) / 2), block row after block row
        std::vector<int> hit((size_t)nblk, 0);
        int64_t next = 0;
        for (int bi = 0; bi < nb; ++bi)
            for (int bj = 0; bj <= bi; ++bj) {
                const int64_t o = tri_block_offset(bi, bj);
                EXPECT(o == next);
                ++next;
                if (o >= 0 && o < nblk) ++hit[(size_t)o]; else EXPECT(false);
            }
        for (int64_t o = 0; o < nblk; ++o) EXPECT(hit[(size_t)o] == 1);
        // the items cover every block exactly once, in runs of at most R that stay inside one block row
        const int64_t nitems = tri_item_count(nb);
        std::vector<int> covered((size_t)nblk, 0);
        int64_t t_expected = 0;
        for (int bi = 0; bi < nb; ++bi) {
            EXPECT(tri_item_first(bi) == t_expected);
            EXPECT(tri_runs_of_row(bi) == (bi + 1 + kTriRun - 1) / kTriRun);
            t_expected += tri_runs_of_row(bi);
        }
        EXPECT(t_expected == nitems);
        for (int64_t t = 0; t < nitems; ++t) {
            const TriItem it = tri_item(t);
            EXPECT(it.bi >= 0 && it.bi < nb && it.bj0 >= 0 && it.len >= 1 && it.len <= kTriRun);
            EXPECT(it.bj0 % kTriRun == 0 && it.bj0 + it.len <= it.bi + 1);                      // no run crosses its block row
            EXPECT(t == tri_item_first(it.bi) + it.bj0 / kTriRun);
            EXPECT(it.len == kTriRun || it.bj0 + it.len == it.bi + 1);                          // only a row's last run is short
            if (!(it.bi >= 0 && it.bi < nb && it.bj0 >= 0 && it.bj0 + it.len <= it.bi + 1)) continue;
            for (int q = 0; q < it.len; ++q) ++covered[(size_t)tri_block_offset(it.bi, it.bj0 + q)];
        }
        for (int64_t o = 0; o < nblk; ++o) EXPECT(covered[(size_t)o] == 1);
        // every output block's list names each of its partials once, row partials (run order) first, then column partials (ascending bi)
        std::vector<int> row_used((size_t)nitems, 0), col_used((size_t)nblk, 0);
        for (int b = 0; b < nb; ++b) {
            const int cnt = tri_partial_count(nb, b);
            EXPECT(cnt == tri_runs_of_row(b) + nb - 1 - b);
            int64_t last_row = -1, last_col = -1;
            bool seen_col = false;
            for (int k = 0; k < cnt; ++k) {
                bool col = false;
                const int64_t slot = tri_partial_slot(b, k, &col);
                if (col) {
                    seen_col = true;
                    EXPECT(slot > last_col && slot >= 0 && slot < nblk);
                    last_col = slot;
                    const int bi = b + 1 + (k - tri_runs_of_row(b));
                    EXPECT(bi > b && bi < nb && slot == tri_block_offset(bi, b));
                    if (slot >= 0 && slot < nblk) ++col_used[(size_t)slot];
                } else {
                    EXPECT(!seen_col && slot > last_row && slot >= 0 && slot < nitems);
                    last_row = slot;
                    if (slot >= 0 && slot < nitems) { EXPECT(tri_item(slot).bi == b); ++row_used[(size_t)slot]; }
                }
            }
        }
        for (int64_t t = 0; t < nitems; ++t) EXPECT(row_used[(size_t)t] == 1);
        for (int bi = 0; bi < nb; ++bi)
            for (int bj = 0; bj <= bi; ++bj) EXPECT(col_used[(size_t)tri_block_offset(bi, bj)] == (bi != bj ? 1 : 0));
        // the scratch holds one slot of kTriCols x 64 doubles per item / per block
        EXPECT(tri_row_scratch_doubles(nb) == nitems * 256 && tri_col_scratch_doubles(nb) == nblk * 256);
    }
    std::printf(fails ? "%d checks failed\n" : "all checks passed\n", fails);
    return fails ? 1 : 0;
}
"""


def test_index_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    """Block offsets, items and reduction lists for 1 .. 40 block rows and the compiled run length: header-only code shared with the kernels, run
    from a stand-alone program under -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "coarse_triangle_main.cpp"
    src.write_text(_INDEX_MAIN)
    exe = tmp_path / "coarse_triangle_main"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gravo_mg_amd", "csrc"),
                            str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout + run.stderr
