// pcg_kernels.hip.hpp -- the vector steps of the preconditioned CG solve loop (gmg_config::pcg, engine.hip::solve_common): conjugate gradients
// with the V-cycle as the preconditioner.  Per iteration, on level-0 vectors in device numbering (n_pad x d column-major, padding rows zero in
// every vector and left zero), for one group of <= 4 columns, z = cycle(rhs = r, x = 0) being there already:
//
//   pcg_rz          partial sums of rho = <r, z>                              -> pcg_reduce_beta:  beta = rho / rho_prev (0: a fresh recurrence)
//   pcg_direction   p = z + beta p (beta = 0: p = z, the old p is not read);  z = 0 (the next cycle's zero guess; not with gmg_config::zero_guess_step)
//   (q = A p: the level-0 product, engine_cycle.hip.hpp::launch_spmv)
//   pcg_pq          partial sums of <p, q>                                    -> pcg_reduce_alpha: alpha = rho / <p, q> or the guard (alpha = 0)
//   pcg_update      x += alpha p,  r -= alpha q (alpha = 0: neither p nor q is read),  partial sums of w r^2, w b^2 (the residual check's)
//
// gmg_config::precond_precision = 1: z is the fp32 cycle's result (float) and pcg_update also writes fl32(r), that cycle's next right-hand side;
// x, r, p, q, every sum and every scalar stay fp64 (the float instantiations below).
//
// <r, z> and <p, q> are plain Euclidean sums over the rows, PER COLUMN; the check's sums carry the stop type's weights.  Same form as
// accel_kernels.hip.hpp, whose helpers are used: every kernel streams each vector once, two rows (16 bytes) per lane, on a fixed grid-stride map;
// block partials are added by ONE block in index order (gmgk::reduce_partials for the check's sums): no floating-point atomics, the same input gives
// the same bits.  rho, beta, alpha and the guard's word stay in device memory (pcg_scalars.hpp decides them); the host sees the check's sums only.
#pragma once

#include "accel_kernels.hip.hpp"
#include "pcg_scalars.hpp"

namespace gmgk {

// gmg_config::precond_precision = 1: z comes out of the fp32 cycle (level 0's x32) and the cycle's right-hand side is fl32(r) (level 0's b32).
// The kernels below then read z as float -- one 8-byte load beside the 16-byte ones, widened exactly -- on the SAME map and in the same
// order of operations: a z that is exactly representable in fp32 gives the bits the all-fp64 instantiations give.
__device__ __forceinline__ double2 pcg_ld2(const double* p, int64_t at) { return accel_ld2(p, at); }
__device__ __forceinline__ double2 pcg_ld2(const float* p, int64_t at) {
    const float2 v = *reinterpret_cast<const float2*>(p + at);
    return make_double2((double)v.x, (double)v.y);
}
__device__ __forceinline__ void pcg_st2(double* p, int64_t at, double2 v) { accel_st2(p, at, v); }
__device__ __forceinline__ void pcg_st2(float* p, int64_t at, double2 v) { *reinterpret_cast<float2*>(p + at) = make_float2((float)v.x, (float)v.y); }

// partials[block][c] = this block's share of <u, v> in column c (TV = float: v is the fp32 cycle's z)
template <int DC, class TV = double>
__global__ __launch_bounds__(kAccelBlock) void pcg_dot(const double* __restrict__ u, const TV* __restrict__ v, int ld, int n_pairs,
                                                       double* __restrict__ partials) {
    double acc[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) acc[c] = 0.0;
    for (int i = blockIdx.x * kAccelBlock + threadIdx.x; i < n_pairs; i += gridDim.x * kAccelBlock) {
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            const int64_t at = 2 * (int64_t)i + (int64_t)c * ld;
            const double2 uv = accel_ld2(u, at), vv = pcg_ld2(v, at);
            acc[c] += uv.x * vv.x + uv.y * vv.y;
        }
    }
    accel_block_store<DC>(acc, DC, partials);
}

// p = z + beta p (a column with beta = 0 writes p = z without reading p: what is there may be anything); ZERO_Z: z = 0 afterwards -- without it
// z is only read (three vector passes instead of four): the next cycle starts from zero by itself (gmg_config::zero_guess_step).
// TZ = float: z is the fp32 cycle's (p = (double) z + beta p; ZERO_Z zeroes the fp32 vector, padding rows included: they stay zero)
template <int DC, bool ZERO_Z = true, class TZ = double>
__global__ __launch_bounds__(kAccelBlock) void pcg_direction(TZ* __restrict__ z, double* __restrict__ p, const double* __restrict__ beta, int ld,
                                                             int n_pairs) {
    double bt[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) bt[c] = beta[c];
    for (int i = blockIdx.x * kAccelBlock + threadIdx.x; i < n_pairs; i += gridDim.x * kAccelBlock) {
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            const int64_t at = 2 * (int64_t)i + (int64_t)c * ld;
            double2 pn = pcg_ld2(z, at);
            if (bt[c] != 0.0) {
                const double2 po = accel_ld2(p, at);
                pn.x += bt[c] * po.x; pn.y += bt[c] * po.y;
            }
            accel_st2(p, at, pn);
            if constexpr (ZERO_Z) pcg_st2(z, at, make_double2(0.0, 0.0));
        }
    }
}

// x += alpha p, r -= alpha q; a column with alpha = 0 (the guard, pcg_scalars.hpp) keeps x and r and reads neither p nor q.
// partials[block][2 c] = share of sum w r^2, [2 c + 1] = share of sum w b^2: the residual check's sums (gmgk::norm_term), for reduce_partials.
// R32 (gmg_config::precond_precision = 1): where r is written, fl32(r) -- the next fp32 cycle's right-hand side -- is written to r32 from the same
// registers: no conversion pass over r.  A guarded column writes neither, so r32 must still hold what the previous iteration (or the fresh
// residual's conversion) left there.  It does: no leg of the fp32 cycle writes level 0's right-hand side -- the smoother steps, the zero-guess
// step and the residual product take it as a const operand (engine_cycle.hip.hpp: enqueue_down / enqueue_up reach level 0's b32 through
// Prec<float>::b as the `b` of launch_smooth and launch_spmv only), a restriction writes the b32 of level k + 1 >= 1, and the coarsest solve's
// conversions touch level L >= 1 (gmg_set_system refuses a hierarchy without a transfer level).
// Padding rows: r is zero there and stays zero (p, q are), so r32 is written zero or not at all.
template <int DC, bool R32 = false>
__global__ __launch_bounds__(kAccelBlock) void pcg_update(double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
                                                          const double* __restrict__ q, const double* __restrict__ alpha, const double* __restrict__ b,
                                                          const double* __restrict__ w, int ld, int n_pairs, double* __restrict__ partials,
                                                          float* __restrict__ r32 = nullptr) {
    double al[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) al[c] = alpha[c];
    double acc[2 * DC];
#pragma unroll
    for (int k = 0; k < 2 * DC; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * kAccelBlock + threadIdx.x; i < n_pairs; i += gridDim.x * kAccelBlock) {
        const double2 wv = w ? accel_ld2(w, 2 * (int64_t)i) : make_double2(1.0, 1.0);
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            const int64_t at = 2 * (int64_t)i + (int64_t)c * ld;
            double2 rn = accel_ld2(r, at);
            const double2 bv = accel_ld2(b, at);
            if (al[c] != 0.0) {
                const double2 xv = accel_ld2(x, at), pv = accel_ld2(p, at), qv = accel_ld2(q, at);
                accel_st2(x, at, make_double2(xv.x + al[c] * pv.x, xv.y + al[c] * pv.y));
                rn = make_double2(rn.x - al[c] * qv.x, rn.y - al[c] * qv.y);
                accel_st2(r, at, rn);
                if constexpr (R32) pcg_st2(r32, at, rn);
            }
            acc[2 * c] += norm_term(rn.x, wv.x) + norm_term(rn.y, wv.y);
            acc[2 * c + 1] += norm_term(bv.x, wv.x) + norm_term(bv.y, wv.y);
        }
    }
    accel_block_store<2 * DC>(acc, 2 * DC, partials);
}

// rho[c] = <r, z> from the partials of pcg_dot (on entry: the previous iteration's), beta[c] = pcg_beta.  first: the first iteration of the solve;
// fresh_all: r was recomputed from the iterate (a confirmation that did not hold): every column starts a new recurrence; restart[c] != 0: the
// column took a guard in the last iteration.  *restarts counts the (iteration, column) pairs after the first iteration that started one (one
// block, launches in stream order: a plain add).
__global__ __launch_bounds__(kReduceBlock) void pcg_reduce_beta(const double* __restrict__ partials, int n_blocks, int dc, double* __restrict__ rho,
                                                                double* __restrict__ beta, const double* __restrict__ restart, int first, int fresh_all,
                                                                double* __restrict__ restarts) {
    __shared__ double tot[kAccelMaxComp];
    __shared__ int flag[4];
    accel_block_total(partials, n_blocks, dc, tot);
    const int c = threadIdx.x;
    if (c < dc) {
        const bool fresh = first || fresh_all || restart[c] != 0.0;
        beta[c] = gmg::pcg_beta(tot[c], rho[c], fresh);
        rho[c] = tot[c];
        flag[c] = !first && fresh;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int k = 0; k < dc; ++k) n += flag[k];
        if (n) *restarts += (double)n;
    }
}

// alpha[c], restart[c] (pcg_step) from the partials of pcg_dot(p, q).  sums: the check's sums of the column group as the last update or
// confirmation left them ([2 c]: sum w r^2, [2 c + 1]: sum w b^2; null in the first iteration of a solve: not known, no floor guard).
// *guard_steps counts the guarded (iteration, column) steps of the solve.
__global__ __launch_bounds__(kReduceBlock) void pcg_reduce_alpha(const double* __restrict__ partials, int n_blocks, int dc, const double* __restrict__ rho,
                                                                 double* __restrict__ alpha, double* __restrict__ restart, const double* sums,
                                                                 double* __restrict__ guard_steps) {
    __shared__ double tot[kAccelMaxComp];
    __shared__ int flag[4];
    accel_block_total(partials, n_blocks, dc, tot);
    const int c = threadIdx.x;
    if (c < dc) {
        const double rr = sums ? sums[2 * c] : 0.0, floor2 = sums ? gmg::accel_floor(sums[2 * c + 1]) : 0.0;
        const gmg::PcgStep st = gmg::pcg_step(tot[c], rho[c], rr, floor2);
        alpha[c] = st.alpha;
        restart[c] = st.guarded ? 1.0 : 0.0;
        flag[c] = st.guarded;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int k = 0; k < dc; ++k) n += flag[k];
        if (n) *guard_steps += (double)n;
    }
}

}  // namespace gmgk
