// accel_kernels.hip.hpp -- the recombination step of the accelerated solve loop (gmg_config::accelerate, engine.hip::solve_common):
// truncated GCR around the V-cycle.  Per iteration, on level-0 vectors in device numbering (n_pad x d column-major, padding rows zero in
// every vector and left zero), for one group of <= 4 columns:
//
//   accel_form     z0 = x~ - x_k,  q0 = r - r~ (in place of r~),  partial sums of <q0, q_j> for the stored directions j
//   accel_orth     z = z0 - sum beta_j z_j,  q = q0 - sum beta_j q_j  (into the ring slot that is dropped),  partial sums of <q, q>, <r, q>
//   accel_update   x = x_k + alpha z (also the next x_k),  r -= alpha q,  partial sums of w r^2, w b^2 (the residual check's)
//
// <u, v> = sum over rows of w u v with the stop type's weights, PER COLUMN.  Every kernel streams each vector once, two rows (16 bytes) per
// lane, on a fixed grid-stride map; block partials are added by ONE block in index order (accel_reduce_beta / accel_reduce_alpha here,
// gmgk::reduce_partials for the check's sums): no floating-point atomics, the same input gives the same bits.  beta, alpha and the stored
// s_j = <q_j, q_j> stay in device memory (accel_scalars.hpp decides them); the host sees the check's sums only.
#pragma once

#include "accel_scalars.hpp"

namespace gmgk {

using gmg::kAccelMaxStored;
constexpr int kAccelBlock = 256;              // 4 waves
constexpr int kAccelMaxBlocks = 2048;         // partials per launch: 8 blocks per CU, grid-stride beyond
constexpr int kAccelMaxComp = kAccelMaxStored * 4;      // sums per launch: 3 stored directions x 4 columns (reduce_partials' 8 do not hold them)

// The stored directions of one column group (entries j >= the number stored are not read).
// INVARIANT the kernels rely on: a slot's z_j, q_j are valid for a column only where its s_j (engine_cycle.hip.hpp: s_slot[j * d_all + c]) is usable.
// In a GUARDED column accel_orth still writes the direction it formed into the slot -- entries that may be NaN or Inf -- and accel_reduce_alpha stores
// s_j = 0 for it.  accel_form goes on reading that column's q_j into its partial sums (which may then be NaN), but accel_beta returns 0 for s_j = 0
// whatever the numerator is, and accel_orth does not look at a slot whose beta is 0: nothing of an unusable column reaches z, q, x or r.
struct AccelRing {
    const double* z[kAccelMaxStored];
    const double* q[kAccelMaxStored];
};

__device__ __forceinline__ double2 accel_ld2(const double* p, int64_t at) { return *reinterpret_cast<const double2*>(p + at); }
__device__ __forceinline__ void accel_st2(double* p, int64_t at, double2 v) { *reinterpret_cast<double2*>(p + at) = v; }

// the block's sums -> partials[blockIdx.x][ncomp]: shuffle tree inside the wave, then the four wave sums in index order (all threads call it)
template <int NC>
__device__ __forceinline__ void accel_block_store(const double (&sums)[NC], int ncomp, double* __restrict__ partials) {
    __shared__ double red[kAccelBlock / 64][NC];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (c >= ncomp) break;
        double v = sums[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) red[wave][c] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < ncomp) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < kAccelBlock / 64; ++w) v += red[w][threadIdx.x];
        partials[(int64_t)blockIdx.x * ncomp + threadIdx.x] = v;
    }
}

// z0 = x - xk, q0 = r - rt (written over rt); partials[block][j * DC + c] = this block's share of <q0, q_j> in column c, j < ns
template <int DC>
__global__ __launch_bounds__(kAccelBlock) void accel_form(const double* __restrict__ x, const double* __restrict__ xk, const double* __restrict__ r,
                                                          double* __restrict__ rt_q0, double* __restrict__ z0, AccelRing ring, int ns,
                                                          const double* __restrict__ w, int ld, int n_pairs, double* __restrict__ partials) {
    double acc[kAccelMaxStored * DC];
#pragma unroll
    for (int k = 0; k < kAccelMaxStored * DC; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * kAccelBlock + threadIdx.x; i < n_pairs; i += gridDim.x * kAccelBlock) {
        const double2 wv = w ? accel_ld2(w, 2 * (int64_t)i) : make_double2(1.0, 1.0);
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            const int64_t at = 2 * (int64_t)i + (int64_t)c * ld;
            const double2 xv = accel_ld2(x, at), kv = accel_ld2(xk, at), rv = accel_ld2(r, at), tv = accel_ld2(rt_q0, at);
            const double2 z = make_double2(xv.x - kv.x, xv.y - kv.y), q = make_double2(rv.x - tv.x, rv.y - tv.y);
            accel_st2(z0, at, z);
            accel_st2(rt_q0, at, q);
#pragma unroll
            for (int j = 0; j < kAccelMaxStored; ++j) {
                if (j >= ns) break;
                const double2 qj = accel_ld2(ring.q[j], at);
                acc[j * DC + c] += (q.x * wv.x) * qj.x + (q.y * wv.y) * qj.y;
            }
        }
    }
    if (ns > 0) accel_block_store<kAccelMaxStored * DC>(acc, ns * DC, partials);
}

// z = z0 - sum beta_j z_j, q = q0 - sum beta_j q_j -> zw, qw (the ring slot being replaced: may BE one of the slots read -- every element is
// read before it is written, by the same lane; nullptr at depth 1: nothing is stored, z0 / q0 are the direction).
// beta[j * d_all + c]; partials[block][2 c] = share of s = <q, q>, [2 c + 1] = share of rho = <r, q>
template <int DC>
__global__ __launch_bounds__(kAccelBlock) void accel_orth(const double* z0, const double* q0, const double* __restrict__ r, AccelRing ring, int ns,
                                                          double* zw, double* qw, const double* __restrict__ beta, int d_all,
                                                          const double* __restrict__ w, int ld, int n_pairs, double* __restrict__ partials) {
    double bt[kAccelMaxStored][DC];
#pragma unroll
    for (int j = 0; j < kAccelMaxStored; ++j)
#pragma unroll
        for (int c = 0; c < DC; ++c) bt[j][c] = j < ns ? beta[j * d_all + c] : 0.0;
    double acc[2 * DC];
#pragma unroll
    for (int k = 0; k < 2 * DC; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * kAccelBlock + threadIdx.x; i < n_pairs; i += gridDim.x * kAccelBlock) {
        const double2 wv = w ? accel_ld2(w, 2 * (int64_t)i) : make_double2(1.0, 1.0);
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            const int64_t at = 2 * (int64_t)i + (int64_t)c * ld;
            double2 z = accel_ld2(z0, at), q = accel_ld2(q0, at);
            const double2 rv = accel_ld2(r, at);
#pragma unroll
            for (int j = 0; j < kAccelMaxStored; ++j) {
                if (j >= ns) break;
                // (beta = 0: a direction this column never stored -- its entries are not looked at)
                if (bt[j][c] != 0.0) {
                    const double2 zj = accel_ld2(ring.z[j], at), qj = accel_ld2(ring.q[j], at);
                    z.x -= bt[j][c] * zj.x; z.y -= bt[j][c] * zj.y;
                    q.x -= bt[j][c] * qj.x; q.y -= bt[j][c] * qj.y;
                }
            }
            if (zw) { accel_st2(zw, at, z); accel_st2(qw, at, q); }
            acc[2 * c] += (q.x * wv.x) * q.x + (q.y * wv.y) * q.y;
            acc[2 * c + 1] += (rv.x * wv.x) * q.x + (rv.y * wv.y) * q.y;
        }
    }
    accel_block_store<2 * DC>(acc, 2 * DC, partials);
}

// x = xk + alpha z (written to x and to xk), r -= alpha q; in a guarded column (guarded[c] != 0, alpha = 1) z0 / q0 take the place of z / q.
// partials[block][2 c] = share of sum w r^2, [2 c + 1] = share of sum w b^2: the residual check's sums (gmgk::norm_term), for reduce_partials
template <int DC>
__global__ __launch_bounds__(kAccelBlock) void accel_update(double* __restrict__ xk, double* __restrict__ x, double* __restrict__ r, const double* zp,
                                                            const double* qp, const double* z0, const double* q0, const double* __restrict__ alpha,
                                                            const double* __restrict__ guarded, const double* __restrict__ b,
                                                            const double* __restrict__ w, int ld, int n_pairs, double* __restrict__ partials) {
    double al[DC];
    const double* zs[DC];
    const double* qs[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) {
        al[c] = alpha[c];
        const bool g = guarded[c] != 0.0;
        zs[c] = g ? z0 : zp;
        qs[c] = g ? q0 : qp;
    }
    double acc[2 * DC];
#pragma unroll
    for (int k = 0; k < 2 * DC; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * kAccelBlock + threadIdx.x; i < n_pairs; i += gridDim.x * kAccelBlock) {
        const double2 wv = w ? accel_ld2(w, 2 * (int64_t)i) : make_double2(1.0, 1.0);
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            const int64_t at = 2 * (int64_t)i + (int64_t)c * ld;
            const double2 kv = accel_ld2(xk, at), zv = accel_ld2(zs[c], at), rv = accel_ld2(r, at), qv = accel_ld2(qs[c], at), bv = accel_ld2(b, at);
            const double2 xn = make_double2(kv.x + al[c] * zv.x, kv.y + al[c] * zv.y);
            const double2 rn = make_double2(rv.x - al[c] * qv.x, rv.y - al[c] * qv.y);
            accel_st2(x, at, xn);
            accel_st2(xk, at, xn);
            accel_st2(r, at, rn);
            acc[2 * c] += norm_term(rn.x, wv.x) + norm_term(rn.y, wv.y);
            acc[2 * c + 1] += norm_term(bv.x, wv.x) + norm_term(bv.y, wv.y);
        }
    }
    accel_block_store<2 * DC>(acc, 2 * DC, partials);
}

// tot[c] = sum over blocks of partials[block][c], c < ncomp <= kAccelMaxComp: reduce_partials' order (thread-strided sums, wave shuffles, the 16
// wave sums in index order) for up to 12 sums, result in LDS for the block's own use.  All threads of the kReduceBlock-thread block call it.
__device__ __forceinline__ void accel_block_total(const double* __restrict__ partials, int n_blocks, int ncomp, double (&tot)[kAccelMaxComp]) {
    __shared__ double red[kReduceBlock / 64][kAccelMaxComp];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double v[kAccelMaxComp];
#pragma unroll
    for (int c = 0; c < kAccelMaxComp; ++c) v[c] = 0.0;
    for (int i = threadIdx.x; i < n_blocks; i += kReduceBlock)
#pragma unroll
        for (int c = 0; c < kAccelMaxComp; ++c) v[c] += c < ncomp ? partials[(int64_t)i * ncomp + c] : 0.0;
#pragma unroll
    for (int c = 0; c < kAccelMaxComp; ++c) {
        if (c >= ncomp) break;
        double t = v[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
        if (lane == 0) red[wave][c] = t;
    }
    __syncthreads();
    if ((int)threadIdx.x < ncomp) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kReduceBlock / 64; ++w) t += red[w][threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
}

// beta[j * d_all + c] = <q0, q_j> / s_j (accel_beta) from the partials of accel_form; s_slot[j * d_all + c] = s_j
__global__ __launch_bounds__(kReduceBlock) void accel_reduce_beta(const double* __restrict__ partials, int n_blocks, int ns, int dc,
                                                                  const double* __restrict__ s_slot, int d_all, double* __restrict__ beta) {
    __shared__ double tot[kAccelMaxComp];
    accel_block_total(partials, n_blocks, ns * dc, tot);
    const int t = threadIdx.x;
    if (t < ns * dc) {
        const int j = t / dc, c = t % dc;
        beta[j * d_all + c] = gmg::accel_beta(tot[t], s_slot[j * d_all + c]);
    }
}

// alpha[c], guarded[c] (accel_step) from the partials of accel_orth; s_store (may be null: depth 1) receives what the ring keeps as s_j of
// the direction just formed; *guard_steps counts the guarded (iteration, column) steps of the solve (one block, launches in stream order: a plain add)
// bb[c] = <b, b> of the column for the floor guard (gmg::accel_floor; 0 in the first iteration of a solve: not known yet, accel_reduce_bb)
__global__ __launch_bounds__(kReduceBlock) void accel_reduce_alpha(const double* __restrict__ partials, int n_blocks, int dc, double* __restrict__ alpha,
                                                                   double* __restrict__ guarded, double* __restrict__ s_store, double* __restrict__ guard_steps,
                                                                   const double* __restrict__ bb) {
    __shared__ double tot[kAccelMaxComp];
    __shared__ int flag[4];
    accel_block_total(partials, n_blocks, 2 * dc, tot);
    const int c = threadIdx.x;
    if (c < dc) {
        const gmg::AccelStep st = gmg::accel_step(tot[2 * c], tot[2 * c + 1], gmg::accel_floor(bb[c]));
        alpha[c] = st.alpha;
        guarded[c] = st.guarded ? 1.0 : 0.0;
        if (s_store) s_store[c] = st.s_store;
        flag[c] = st.guarded;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int k = 0; k < dc; ++k) n += flag[k];
        if (n) *guard_steps += (double)n;
    }
}

// bb[c] = <b, b> of column c from the partials of accel_update ([2 c + 1]: the check's sums of w b^2), once per solve after its first update
__global__ __launch_bounds__(kReduceBlock) void accel_reduce_bb(const double* __restrict__ partials, int n_blocks, int dc, double* __restrict__ bb) {
    __shared__ double tot[kAccelMaxComp];
    accel_block_total(partials, n_blocks, 2 * dc, tot);
    if ((int)threadIdx.x < dc) bb[threadIdx.x] = tot[2 * threadIdx.x + 1];
}

}  // namespace gmgk
