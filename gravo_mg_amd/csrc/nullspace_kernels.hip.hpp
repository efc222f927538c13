// nullspace_kernels.hip.hpp -- the two projections at the ends of a solve on a gmg_config::nullspace = 1 handle (engine.hip::solve_common;
// DESIGN.md 5f): the system is symmetric positive semi-definite with the null space span{1}, so
//
//   after the load     b <- b - (1^T b / n) 1             the orthogonal projection onto range(A): unit weights
//   before the fetch   x <- x - (m^T x / m^T 1) 1         the solution of zero mass-weighted mean: m the handle's mass, unit weights without one
//
// on level-0 vectors in device numbering (n_pad x d column-major, padding rows zero in every vector and left zero), for one group of <= 4
// columns:
//
//   nullspace_sums     partial sums of sum_i w_i v_i and sum_i v_i^2 per column, and of sum_i w_i, over the REAL rows (real[i] >= 0: the
//                      level's new2old; the device copy of the mass carries weight 1 in padding rows)
//   nullspace_reduce   s_c = sum w v / sum w per column; the sums themselves are kept for the timing key "nullspace_rhs_defect"
//   nullspace_shift    v_i -= s_c on the real rows only
//
// Same form as pcg_kernels.hip.hpp, whose helpers are used: every kernel streams each vector once, two rows (16 bytes) per lane, on a fixed
// grid-stride map; block partials are added by ONE block in index order: no floating-point atomics, the same input gives the same bits.
#pragma once

#include "accel_kernels.hip.hpp"

namespace gmgk {

// partials[block][c] = share of sum w v of column c, [DC + c] = share of sum v^2, [2 DC] = share of sum w (w == nullptr: unit weights)
template <int DC>
__global__ __launch_bounds__(kAccelBlock) void nullspace_sums(const double* __restrict__ v, const double* __restrict__ w, const int* __restrict__ real, int ld,
                                                              int n_pairs, double* __restrict__ partials) {
    double acc[2 * DC + 1];
#pragma unroll
    for (int k = 0; k < 2 * DC + 1; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * kAccelBlock + threadIdx.x; i < n_pairs; i += gridDim.x * kAccelBlock) {
        const int2 rl = *reinterpret_cast<const int2*>(real + 2 * (int64_t)i);
        double2 wv = w ? accel_ld2(w, 2 * (int64_t)i) : make_double2(1.0, 1.0);
        if (rl.x < 0) wv.x = 0.0;
        if (rl.y < 0) wv.y = 0.0;
        acc[2 * DC] += wv.x + wv.y;
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            const double2 vv = accel_ld2(v, 2 * (int64_t)i + (int64_t)c * ld);
            acc[c] += wv.x * vv.x + wv.y * vv.y;
            acc[DC + c] += vv.x * vv.x + vv.y * vv.y;
        }
    }
    accel_block_store<2 * DC + 1>(acc, 2 * DC + 1, partials);
}

// out[c] = sum w v / sum w (0 where sum w is not positive), out[d_all + c] = sum w v, out[2 d_all + c] = sum v^2 of column c, from the partials
__global__ __launch_bounds__(kReduceBlock) void nullspace_reduce(const double* __restrict__ partials, int n_blocks, int dc, int d_all, double* __restrict__ out) {
    __shared__ double tot[kAccelMaxComp];
    accel_block_total(partials, n_blocks, 2 * dc + 1, tot);
    const int c = threadIdx.x;
    if (c < dc) {
        const double sw = tot[2 * dc];
        out[c] = sw > 0.0 ? tot[c] / sw : 0.0;
        out[d_all + c] = tot[c];
        out[2 * d_all + c] = tot[dc + c];
    }
}

// v_i -= shift[c] on the real rows of column c; padding rows keep their zeros
template <int DC>
__global__ __launch_bounds__(kAccelBlock) void nullspace_shift(double* __restrict__ v, const double* __restrict__ shift, const int* __restrict__ real, int ld,
                                                               int n_pairs) {
    double sh[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) sh[c] = shift[c];
    for (int i = blockIdx.x * kAccelBlock + threadIdx.x; i < n_pairs; i += gridDim.x * kAccelBlock) {
        const int2 rl = *reinterpret_cast<const int2*>(real + 2 * (int64_t)i);
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            const int64_t at = 2 * (int64_t)i + (int64_t)c * ld;
            double2 vv = accel_ld2(v, at);
            if (rl.x >= 0) vv.x -= sh[c];
            if (rl.y >= 0) vv.y -= sh[c];
            accel_st2(v, at, vv);
        }
    }
}

}  // namespace gmgk
