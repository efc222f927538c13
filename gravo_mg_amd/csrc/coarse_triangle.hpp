// coarse_triangle.hpp -- index arithmetic of GMG_COARSE_DEVICE_TRIANGLE, shared by the set-up (setup_kernels.hip.hpp::pack_lower_blocks,
// engine_system.hip.hpp), the product kernels (kernels.hip.hpp::tri_symv_items / tri_symv_reduce) and a stand-alone host test
// (tests/test_coarse_triangle_host.py).  Plain C++: no HIP header is needed to include it.
//
// The lower triangle of the symmetric A_L^-1 (factor's numbering, zero-padded to nb = ceil(n / 64) block rows) is stored as 64 x 64 blocks, each
// row-major and contiguous (kTriBlockDoubles doubles = 32 KB), in the order (0,0) (1,0) (1,1) (2,0) ... over bi >= bj: block row after block
// row, so the blocks of a row are neighbours in memory.  A diagonal block holds both of its triangles.
//
// The product y = T x is dealt out as ITEMS: block row bi cut into runs of at most kTriRun consecutive bj (the last run of a row may be
// shorter).  Items are numbered row after row, run after run.  An item adds its blocks' row parts into one 64-row partial (slot = item
// number); every block below the diagonal also leaves one 64-row column partial (slot = block offset).  Output block b is then
//     the row partials of b's items in run order, followed by the column partials of the blocks (bi, b), bi = b + 1 .. nb - 1, ascending:
// one fixed order for every output value, whatever the device schedules.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GMG_TRI_HD __host__ __device__ inline
#else
#define GMG_TRI_HD inline
#endif

namespace gmg {

constexpr int kTriBlock = 64;                                 // rows and columns of a block
constexpr int kTriBlockDoubles = kTriBlock * kTriBlock;
constexpr int kTriRun = 4;                                    // R: blocks of an item at most (timing key "coarse_triangle_run_blocks")
constexpr int kTriCols = 4;                                   // columns of a partial slot (the column groups of the cycle: for_col_chunks)

GMG_TRI_HD int tri_blocks(int n) { return (n + kTriBlock - 1) / kTriBlock; }
GMG_TRI_HD int64_t tri_block_count(int nb) { return (int64_t)nb * (nb + 1) / 2; }
// position of block (bi, bj), bi >= bj, in the packed order
GMG_TRI_HD int64_t tri_block_offset(int bi, int bj) { return (int64_t)bi * (bi + 1) / 2 + bj; }
GMG_TRI_HD int tri_runs_of_row(int bi) { return bi / kTriRun + 1; }                        // = ceil((bi + 1) / R)
// number of the first item of block row bi (= items of the rows above it): rows g R .. g R + R - 1 have g + 1 runs each
GMG_TRI_HD int64_t tri_item_first(int bi) {
    const int64_t g = bi / kTriRun;
    return (int64_t)kTriRun * g * (g + 1) / 2 + (int64_t)(bi - g * kTriRun) * (g + 1);
}
GMG_TRI_HD int64_t tri_item_count(int nb) { return tri_item_first(nb); }
// item t -> its block row, first block column and number of blocks
struct TriItem { int bi, bj0, len; };
GMG_TRI_HD TriItem tri_item(int64_t t) {
    int64_t g = 0;
    while ((int64_t)kTriRun * (g + 1) * (g + 2) / 2 <= t) ++g;
    const int64_t u = t - (int64_t)kTriRun * g * (g + 1) / 2;
    TriItem it;
    it.bi = (int)(g * kTriRun + u / (g + 1));
    it.bj0 = (int)(u % (g + 1)) * kTriRun;
    it.len = it.bi + 1 - it.bj0 < kTriRun ? it.bi + 1 - it.bj0 : kTriRun;
    return it;
}
// the partials of output block b in the order of their summation: tri_partial_count of them, the k-th one in slot tri_partial_slot of the row
// scratch (*col = false) or of the column scratch (*col = true)
GMG_TRI_HD int tri_partial_count(int nb, int b) { return tri_runs_of_row(b) + (nb - 1 - b); }
GMG_TRI_HD int64_t tri_partial_slot(int b, int k, bool* col) {
    const int runs = tri_runs_of_row(b);
    *col = k >= runs;
    return k < runs ? tri_item_first(b) + k : tri_block_offset(b + 1 + (k - runs), b);
}
// doubles of the two scratch arrays the product needs for one group of kTriCols columns
GMG_TRI_HD int64_t tri_row_scratch_doubles(int nb) { return tri_item_count(nb) * kTriCols * kTriBlock; }
GMG_TRI_HD int64_t tri_col_scratch_doubles(int nb) { return tri_block_count(nb) * kTriCols * kTriBlock; }

}  // namespace gmg
