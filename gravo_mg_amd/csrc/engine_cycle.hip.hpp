// engine_cycle.hip.hpp -- part of libgravomg_hip.so's single translation unit (included by engine.hip, in this order:
// engine_state, engine_setup, engine_cycle).  Kernel launch helpers and the V-cycle legs.
#pragma once

namespace {

// ---- launch helpers (all on h->stream; column chunks of <= 4) ----------------------------------------

#define DISPATCH_D(dc, ...)              \
    switch (dc) {                        \
        case 1: { constexpr int D = 1; __VA_ARGS__; } break; \
        case 2: { constexpr int D = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int D = 3; __VA_ARGS__; } break; \
        default: { constexpr int D = 4; __VA_ARGS__; } break; \
    }

// level 0 with 16-bit column codes (DevSell::col16) runs the C16 instantiation of its kernels
#define DISPATCH_C16(mode, ...)          \
    switch (mode) {                      \
        case 1: { constexpr int C16 = 1; __VA_ARGS__; } break; \
        case 2: { constexpr int C16 = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int C16 = 3; __VA_ARGS__; } break; \
        case 4: { constexpr int C16 = 4; __VA_ARGS__; } break; \
        default: { constexpr int C16 = 0; __VA_ARGS__; } break; \
    }

// a run-time flag as a compile-time one (kernel template arguments that are a bool, or an int / enum with two values in use)
#define DISPATCH_FLAG(NAME, cond, ...)   \
    { if (cond) { constexpr bool NAME = true; __VA_ARGS__; } else { constexpr bool NAME = false; __VA_ARGS__; } }

// ... and an int with three values in use: NAME = A or B where v equals one of them, C otherwise
#define DISPATCH_ONE_OF(NAME, v, A, B, C, ...)   \
    { if ((v) == (A)) { constexpr int NAME = A; __VA_ARGS__; } else if ((v) == (B)) { constexpr int NAME = B; __VA_ARGS__; } else { constexpr int NAME = C; __VA_ARGS__; } }

// the groups of <= 4 columns a kernel launch covers: f(first column, columns in the group)
template <class F>
inline void for_col_chunks(int d, F&& f) {
    for (int c0 = 0; c0 < d; c0 += 4) f(c0, std::min(4, d - c0));
}

// Precision selector: the fp64 arrays, or their fp32 twins (same layout, same index arrays).
template <class T> struct Prec;
template <> struct Prec<double> {
    static const double* val(const DevSell& s) { return s.val; }
    static const double* diag(const Level& l) { return l.diag; }
    static const double* bcval(const Level& l) { return l.bc_val; }
    static const double* epval(const Level& l) { return l.ep_val; }
    static const double* eeval(const Level& l) { return l.ee_val; }
    static double* x(Level& l) { return l.x; }
    static double* b(Level& l) { return l.b; }
    static double* r(Level& l) { return l.r; }
    static double* tmp(Level& l) { return l.tmp; }
};
template <> struct Prec<float> {
    static const float* val(const DevSell& s) { return s.val32; }
    static const float* diag(const Level& l) { return l.diag32; }
    static const float* bcval(const Level& l) { return l.bc_val32; }
    static const float* epval(const Level& l) { return l.ep_val32; }
    static const float* eeval(const Level& l) { return l.ee_val32; }
    static float* x(Level& l) { return l.x32; }
    static float* b(Level& l) { return l.b32; }
    static float* r(Level& l) { return l.r32; }
    static float* tmp(Level& l) { return l.tmp32; }
};

// What the launches around a level's smoothing hand to one another travels as values: a request goes down with launch_smooth, a result comes back
// (empty where the smoother cannot serve a part of the request -- Jacobi and Chebyshev serve none: the caller then enqueues the ordinary launch).
template <class T>
struct SmoothAsk {
    bool from_zero = false;       // the iterate is the zero vector: the first block sweep takes no input (and the caller skipped the memset)
    bool first_done = false;      // ... and the restriction's launch already ran that sweep: its result is in tmp (restrict_into)
    int head_done = 0;            // level 0: the first colour launch is already in the stream (enqueue_head; HEAD_FOLDED: the first two)
    T* res_out = nullptr;         // level-0 pre-smoothing: where the last colour launch may write the residual of its rows (fold_residual) ...
    bool res_il = false;          // ... as an interleaved multi-vector
    int norm_type = -1;           // level-0 post-smoothing: the residual check the cycle ends with, which the last colour launch may join (fold_norm)
    T* il_out = nullptr;          // level-1 post-smoothing: where the last block sweep may write an interleaved copy of the level's x
};
template <class T>
struct SmoothDone {
    int res_from = 0;             // first slice whose residual the last colour launch wrote (0: it wrote none)
    int norm_blocks = 0;          // partial-sum blocks of the residual check the last colour launch produced (0: none)
    const T* prev = nullptr;      // the iterate the last block sweep started from (nullptr: the zero vector) ...
    bool prev_valid = false;      // ... where launch_residual_delta may use it
    bool il_written = false;      // the interleaved copy asked for is in il_out
};

// The last colour launch of the cycle's last level-0 sweep also forms its rows' share of the residual check (gs_color_norm) when the cycle being
// enqueued ends with one (type >= 0: SmoothAsk::norm_type): fp64, one group of <= 4 columns, >= 2 colours.  Its partial sums go behind the ones
// the norm kernel will write for the rows of the other colours (launch_norm).  Returns their number of blocks, 0 where the launch is not folded.
template <class T>
int fold_norm(gmg_handle, Level&, int, bool, int, int, int) { return 0; }
template <>
int fold_norm<double>(gmg_handle h, Level& l, int d, bool last_launch, int sb, int se, int type) {
    if (!last_launch || type < 0 || &l != &h->lv[0] || d > 4 || l.ord.n_colors < 2 || se != l.Aoff.n_slices) return 0;
    const double* w = type == 1 ? h->d_minv : (type == 2 ? h->d_mass : nullptr);
    const int nblk = grid_for(se - sb), first = norm_grid(sb);
    if ((size_t)(first + nblk) > (size_t)h->partial_blocks) return 0;
    DISPATCH_D(d, DISPATCH_C16(l.Aoff.c16_sel(), hipLaunchKernelGGL((gmgk::gs_color_norm<D, C16>), dim3(nblk), dim3(gmgk::kBlock), 0, h->stream, l.Aoff.slice_ptr,
                                     l.Aoff.col, l.Aoff.val, l.diag, l.b, l.x, l.n_pad, sb, se, h->cfg.gs_omega, w, h->d_partials + (size_t)first * 2 * d,
                                     l.Aoff.col16, l.Aoff.win_base, l.Aoff.c16_arg())));
    return nblk;
}

// ... and the last colour launch of the level-0 PRE-smoothing writes the residual of its rows to `out` (gs_color_residual) when the way down
// asks for it (SmoothAsk::res_out, res_il); launch_spmv then covers the slices in front of that colour only.  Returns the first slice the
// launch covered, 0 where it is not folded.
template <class T>
int fold_residual(gmg_handle, Level&, int, bool, int, int, T*, bool) { return 0; }
template <>
int fold_residual<double>(gmg_handle h, Level& l, int d, bool last_launch, int sb, int se, double* out, bool il) {
    if (!last_launch || !out || &l != &h->lv[0] || d > 4 || l.ord.n_colors < 2 || se != l.Aoff.n_slices || sb <= 0) return 0;
    DISPATCH_D(d, DISPATCH_C16(l.Aoff.c16_sel(), DISPATCH_FLAG(YI, il, hipLaunchKernelGGL((gmgk::gs_color_residual<D, C16, (YI && D > 1)>), dim3(grid_for(se - sb)),
                                     dim3(gmgk::kBlock), 0, h->stream, l.Aoff.slice_ptr, l.Aoff.col, l.Aoff.val, l.diag, l.b, l.x, out, l.n_pad, sb, se,
                                     h->cfg.gs_omega, l.Aoff.col16, l.Aoff.win_base, l.Aoff.c16_arg()))));
    return sb;
}

inline bool polled(gmg_handle h);

// over-relaxation on the finest level only (gmg_config::gs_omega)
template <class T>
T level_omega(gmg_handle h, const Level& l) { return &l == &h->lv[0] ? (T)h->cfg.gs_omega : (T)1.0; }

// one colour launch of a sweep over level l (columns c0 .. c0 + dc), slices [sb, se); plain_rows (level 0, fp64: the hybrid smoother of the
// distributed code), go: see gmgk::gs_color
template <class T>
void launch_gs_color(gmg_handle h, Level& l, int c0, int dc, int sb, int se, T omega, const unsigned long long* plain_rows = nullptr, const int* go = nullptr) {
    const int ld = l.n_pad;
    T* x = Prec<T>::x(l);
    const T* b = Prec<T>::b(l);
    if (&l == &h->lv[0]) {           // FINE = 1 + C16 (c16_sel: 0 32-bit columns, 1 / 2 streamed codes, 3 / 4 a fine level that stays on the chip)
        DISPATCH_D(dc, DISPATCH_C16(l.Aoff.c16_sel(), DISPATCH_FLAG(OM, plain_rows != nullptr, hipLaunchKernelGGL((gmgk::gs_color<T, D, C16 + 1, (OM && sizeof(T) == 8)>),
                                          dim3(grid_for(se - sb)), dim3(gmgk::kBlock), 0, h->stream, l.Aoff.slice_ptr, l.Aoff.col, Prec<T>::val(l.Aoff), Prec<T>::diag(l),
                                          b + (size_t)c0 * ld, x + (size_t)c0 * ld, ld, sb, se, 1, omega, l.Aoff.col16, l.Aoff.win_base, l.Aoff.c16_arg(), plain_rows, go))));
    } else {
        DISPATCH_D(dc, hipLaunchKernelGGL((gmgk::gs_color<T, D, 0>), dim3(grid_for(se - sb)), dim3(gmgk::kBlock), 0, h->stream,
                                          l.Aoff.slice_ptr, l.Aoff.col, Prec<T>::val(l.Aoff), Prec<T>::diag(l), b + (size_t)c0 * ld,
                                          x + (size_t)c0 * ld, ld, sb, se, 1, omega));
    }
}

inline int first_color(const Level& l) {
    for (int c = 0; c < l.ord.n_colors; ++c)
        if (l.ord.color_begin[c + 1] / 64 > l.ord.color_begin[c] / 64) return c;
    return -1;
}

// Head of the next cycle: may the first colour launch of the level-0 pre-smoothing be enqueued ahead of the solve loop's decision?  Stream
// launches with the polled check (the reduction publishes the decision), fp64, colour-major level 0 with a colour class in front of the one the
// residual rides on, one group of columns, the whole system on this device.  The loop that enqueues a head (enqueue_head) tells the next
// cycle so (vcycle_resident's head_done -> SmoothAsk::head_done): its level-0 pre-smoothing then starts with its second launch.
inline bool head_eligible(gmg_handle h, int d) {
    return h->cfg.speculate_head && polled(h) && !h->cfg.inner_precision && h->cfg.smoother == GMG_SMOOTHER_MULTICOLOR_GS && h->cfg.pre_iters > 0 && h->L >= 1 &&
           !h->lv[0].ord.blocked && h->lv[0].ord.n_colors >= 2 && first_color(h->lv[0]) >= 0 && first_color(h->lv[0]) < h->lv[0].ord.n_colors - 1 && d >= 1 && d <= 4 &&
           !h->partitioned && h->part_world <= 1 && h->d_watch && !h->prof_on;
}
// The folded head (gmg_config::fold_head): the residual check in front of the head computes the first colour's update as well -- it holds every
// operand -- and stores it to the side vector (residual_norm_slices_head); the launch enqueued ahead of the decision is then the SECOND colour
// launch, which gathers the first colour's columns from the side vector and commits it to x (gs_color_commit).  One launch and one pass over
// the first colour's rows less per cycle; speculation stays one launch deep.  Asked per iteration (wait_flag may switch polling off in
// mid-solve): where today's head goes, with a second non-empty colour class whose launch of the first pre-sweep is a plain one (not the
// sweep's last launch, which carries the residual: fold_residual) and the side vector in place.
inline int second_color(const Level& l) {
    for (int c = first_color(l) + 1; c > 0 && c < l.ord.n_colors; ++c)
        if (l.ord.color_begin[c + 1] / 64 > l.ord.color_begin[c] / 64) return c;
    return -1;
}
inline bool fold_eligible(gmg_handle h, int d) {
    if (!h->cfg.fold_head || h->cfg.accelerate != 0 || !head_eligible(h, d)) return false;
    const Level& l = h->lv[0];
    const int c1 = first_color(l), c2 = second_color(l);
    return c2 > 0 && (c2 < l.ord.n_colors - 1 || h->cfg.pre_iters >= 2) && l.xh &&
           l.xh_rows == (l.ord.color_begin[c1 + 1] / 64 - l.ord.color_begin[c1] / 64) * 64 && d <= h->dcap;
}
// What of the coming cycle is in the stream, enqueued ahead of the loop's decision: nothing, its first colour launch, or (folded) its first
// two -- what the caller hands to that cycle (vcycle_resident's head_done -> SmoothAsk::head_done)
enum { HEAD_NONE = 0, HEAD_FIRST = 1, HEAD_FOLDED = 2 };
// (folded: the check in front was asked for the side vector, CycleWatch::fold)
inline int enqueue_head(gmg_handle h, int d, bool folded = false) {
    Level& l = h->lv[0];
    const int c = first_color(l);
    const int* go = reinterpret_cast<const int*>(h->d_watch + 1);
    h->timing["heads_enqueued"] += 1.0;
    if (!folded) {
        launch_gs_color<double>(h, l, 0, d, l.ord.color_begin[c] / 64, l.ord.color_begin[c + 1] / 64, level_omega<double>(h, l), nullptr, go);
        return HEAD_FIRST;
    }
    const int c2 = second_color(l);
    const int hb = l.ord.color_begin[c] / 64, he = l.ord.color_begin[c + 1] / 64, sb = l.ord.color_begin[c2] / 64, se = l.ord.color_begin[c2 + 1] / 64;
    const int n_work = grid_for(se - sb), n_copy = ((he - hb) * 32 + gmgk::kBlock - 1) / gmgk::kBlock;      // (the commit moves two rows per lane)
    DISPATCH_D(d, DISPATCH_C16(l.Aoff.c16_sel(), hipLaunchKernelGGL((gmgk::gs_color_commit<D, C16>), dim3(n_work + n_copy), dim3(gmgk::kBlock), 0, h->stream,
                                     l.Aoff.slice_ptr, l.Aoff.col, l.Aoff.val, l.diag, l.b, l.x, l.n_pad, sb, se, n_work, level_omega<double>(h, l), l.Aoff.col16,
                                     l.Aoff.win_base, l.Aoff.c16_arg(), l.xh.get(), hb, he, go)));
    h->timing["heads_folded"] += 1.0;
    return HEAD_FOLDED;
}

template <class T>
SmoothDone<T> launch_gs_sweeps(gmg_handle h, Level& l, int d, int iters, const SmoothAsk<T>& ask) {
    SmoothDone<T> done;
    // (the first launch of this cycle is already in the stream: enqueue_head -- the first two where the head was folded)
    const int c_head = ask.head_done ? first_color(l) : -1, c_head2 = ask.head_done == HEAD_FOLDED ? second_color(l) : -1;
    for (int it = 0; it < iters; ++it)
        for_col_chunks(d, [&](int c0, int dc) {
            for (int c = 0; c < l.ord.n_colors; ++c) {
                int sb = l.ord.color_begin[c] / 64, se = l.ord.color_begin[c + 1] / 64;
                if (se <= sb) continue;
                if (it == 0 && c0 == 0 && (c == c_head || c == c_head2)) continue;
                const bool last_launch = it == iters - 1 && c == l.ord.n_colors - 1;
                if (const int nblk = fold_norm<T>(h, l, d, last_launch, sb, se, ask.norm_type)) { done.norm_blocks = nblk; continue; }
                if (const int from = fold_residual<T>(h, l, d, last_launch, sb, se, ask.res_out, ask.res_il)) { done.res_from = from; continue; }
                launch_gs_color<T>(h, l, c0, dc, sb, se, level_omega<T>(h, l));
            }
        });
    return done;
}

// The factor of a pointwise smoother's first step on a zero iterate, x = c * (b / diag) (gmgk::zero_step_row): Jacobi's damping, or the second
// coefficient of Chebyshev step 0 on this level (its first multiplies a p that does not exist yet).
template <class T>
T zero_step_coeff(gmg_handle h, const Level& l) {
    if (h->cfg.smoother == GMG_SMOOTHER_JACOBI) return (T)h->cfg.jacobi_omega;
    return (T)cheby_step_coeffs(l.cheby_lambda, cheby_ratio(h), 0).c2;
}

// That step as a launch of its own (gmg_config::zero_guess_step): tmp = c * (b / diag) over all n_pad rows, for Chebyshev the direction p (the
// level's residual vector: launch_cheby_steps) too.  It writes where the generic first step writes, so the sweeps behind it ping-pong as ever.
template <class T>
void launch_zero_step(gmg_handle h, Level& l, int d) {
    const int ld = l.n_pad;
    const T c = zero_step_coeff<T>(h, l);
    ++h->zero_steps;
    for_col_chunks(d, [&](int c0, int dc) {
        DISPATCH_D(dc, DISPATCH_FLAG(WRITE_P, h->cfg.smoother == GMG_SMOOTHER_CHEBYSHEV, hipLaunchKernelGGL((gmgk::pointwise_zero_step<T, D, WRITE_P>),
                                          dim3((ld + gmgk::kBlock - 1) / gmgk::kBlock), dim3(gmgk::kBlock), 0, h->stream, Prec<T>::diag(l), Prec<T>::b(l) + (size_t)c0 * ld,
                                          Prec<T>::tmp(l) + (size_t)c0 * ld, Prec<T>::r(l) + (size_t)c0 * ld, ld, ld, c)));
    });
}

// ask.from_zero (both pointwise smoothers): the iterate is the zero vector and x holds anything -- the first step is the zero step, enqueued here
// unless the restriction into the level computed it (ask.first_done); either way its result is in tmp and the second step reads it there
template <class T>
void launch_jacobi_sweeps(gmg_handle h, Level& l, int d, int iters, const SmoothAsk<T>& ask = {}) {
    const int ld = l.n_pad;
    T* in = Prec<T>::x(l); T* out = Prec<T>::tmp(l);
    const T* b = Prec<T>::b(l);
    int it0 = 0;
    if (ask.from_zero) {
        if (!ask.first_done) launch_zero_step<T>(h, l, d);
        std::swap(in, out);
        it0 = 1;
    }
    for (int it = it0; it < iters; ++it) {
        for_col_chunks(d, [&](int c0, int dc) {
            DISPATCH_D(dc, hipLaunchKernelGGL((gmgk::jacobi_sweep<T, D>), dim3(grid_for(l.Aoff.n_slices)), dim3(gmgk::kBlock), 0, h->stream,
                                              l.Aoff.slice_ptr, l.Aoff.col, Prec<T>::val(l.Aoff), Prec<T>::diag(l), b + (size_t)c0 * ld,
                                              (in ? in + (size_t)c0 * ld : nullptr), out + (size_t)c0 * ld, ld, l.Aoff.n_slices, (T)h->cfg.jacobi_omega, 1));
        });
        std::swap(in, out);
    }
    if (in != Prec<T>::x(l)) (void)hipMemcpyAsync(Prec<T>::x(l), in, sizeof(T) * (size_t)ld * d, hipMemcpyDeviceToDevice, h->stream);
}

// `iters` steps of a Chebyshev polynomial that starts here (cheby_coeffs.hpp): one launch per step and group of columns, the step's two
// coefficients as kernel arguments.  x ping-pongs between the level's x and tmp like the Jacobi sweeps; p lives in the level's residual vector,
// which is dead while the level is smoothed (the way down forms b - A x after the pre-smoothing, the restriction has consumed it before the
// post-smoothing, and the accelerated loop writes it anew after the cycle).
template <class T>
void launch_cheby_steps(gmg_handle h, Level& l, int d, int iters, const SmoothAsk<T>& ask = {}) {
    const int ld = l.n_pad;
    T* in = Prec<T>::x(l); T* out = Prec<T>::tmp(l);
    const T* b = Prec<T>::b(l);
    T* p = Prec<T>::r(l);
    const int c16 = &l == &h->lv[0] ? l.Aoff.c16_sel() : 0;
    const double ratio = cheby_ratio(h);
    int it0 = 0;
    if (ask.from_zero) {                               // (see launch_jacobi_sweeps; the zero step wrote p as well)
        if (!ask.first_done) launch_zero_step<T>(h, l, d);
        std::swap(in, out);
        it0 = 1;
    }
    for (int it = it0; it < iters; ++it) {
        const ChebyStep st = cheby_step_coeffs(l.cheby_lambda, ratio, it);
        for_col_chunks(d, [&](int c0, int dc) {
            DISPATCH_D(dc, DISPATCH_C16(c16, DISPATCH_FLAG(FIRST, it == 0, hipLaunchKernelGGL((gmgk::cheby_step<T, D, FIRST, C16>), dim3(grid_for(l.Aoff.n_slices)),
                                              dim3(gmgk::kBlock), 0, h->stream, l.Aoff.slice_ptr, l.Aoff.col, Prec<T>::val(l.Aoff), Prec<T>::diag(l), b + (size_t)c0 * ld,
                                              in + (size_t)c0 * ld, out + (size_t)c0 * ld, p + (size_t)c0 * ld, ld, l.Aoff.n_slices, (T)st.c1, (T)st.c2, 1, l.Aoff.col16,
                                              l.Aoff.win_base, l.Aoff.c16_arg()))));
        });
        std::swap(in, out);
    }
    if (in != Prec<T>::x(l)) (void)hipMemcpyAsync(Prec<T>::x(l), in, sizeof(T) * (size_t)ld * d, hipMemcpyDeviceToDevice, h->stream);
}

// Does the entry-parallel block sweep of level l STREAM its operator (non-temporal loads)?  Yes when the operator's chunks (12 B per explicit,
// 10 B per lower entry in fp64) are more than the memory-side cache (256 MB on MI355X) holds beside the cycle's vectors between two of the
// launches that read them: level 0 of a point cloud (300 MB) -- measured 0.634 ms per cycle streamed, 0.699 with ordinary loads; the 506 k-row
// level 1 of the 3 M mesh (76 MB, five readers per cycle): 140 us per cycle streamed, 125 not.
constexpr int64_t kEpResidentBytes = (int64_t)128 << 20;
inline bool ep_streams(const Level& l) { return l.ee_nnz * 12 + l.ep_nnz * 10 > kEpResidentBytes; }

// block-hybrid Gauss-Seidel: one launch per sweep, ping-pong between x and tmp
// One block-hybrid sweep in -> out over blocks [b0, b0 + nb) of a blocked level (in == nullptr: the iterate is the zero vector).
// The kernels find their rows through blk_begin[block]: a sub-range is the same launch on offset block tables.
template <class T>
void launch_block_sweep_range(gmg_handle h, Level& l, int d, const T* in, T* out, int b0, int nb, const int* begin_table = nullptr,
                              const int* ncolors_table = nullptr, T* out_il = nullptr) {
    const int ld = l.n_pad;
    const T* b = Prec<T>::b(l);
    // (begin_table / ncolors_table: an explicit list of nb blocks instead of a range -- entry-parallel sweep only, which reads
    // nothing but the first row of its block from the table)
    const int* blk_begin = begin_table ? begin_table : l.d_blk_begin + b0;
    const int* blk_ncolors = ncolors_table ? ncolors_table : l.d_blk_ncolors + b0;
    if (nb <= 0) return;
    for_col_chunks(d, [&](int c0, int dc) {
        if (l.use_ep) {
            // one block per workgroup (persistent workgroups, grid < vgrid, measured the same or worse: profiles/r04/b_*); a multiple of 8: the
            // kernel's XCD-aware block map is a bijection onto [0, vgrid).  The kernel takes its blocks from b0 on unless it is given a list
            const int vgrid = (nb + 7) / 8 * 8;
            DISPATCH_D(dc, DISPATCH_FLAG(STREAM, ep_streams(l), hipLaunchKernelGGL((gmgk::gs_block_ep<T, D, STREAM>), dim3(vgrid), dim3(64),
                                              gmgk::ep_lds_bytes<T>(D, l.ep_cap_e, l.ep_cap_l), h->stream, begin_table, blk_ncolors, l.d_row_color, l.ep_ptr, l.ep_col,
                                              Prec<T>::epval(l), l.ee_ptr, l.ee_col, Prec<T>::eeval(l), Prec<T>::diag(l), b + (size_t)c0 * ld,
                                              (in ? in + (size_t)c0 * ld : nullptr), out + (size_t)c0 * ld, ld, l.ep_cap_e, l.ep_cap_l, nb, b0, vgrid, out_il)));
        } else if (l.use_bcsr && d > 1) {
            DISPATCH_D(dc, hipLaunchKernelGGL((gmgk::gs_block_csrout<T, D, (D == 1 ? 32 : 24)>), dim3(nb), dim3(64),
                                              (size_t)l.bc_cap * (sizeof(T) + sizeof(int)) + (size_t)D * 64 * sizeof(T), h->stream, blk_begin,
                                              blk_ncolors, l.d_row_color, l.Ain.slice_ptr, l.ain_col16, Prec<T>::val(l.Ain), l.bc_ptr, l.bc_col,
                                              Prec<T>::bcval(l), Prec<T>::diag(l), b + (size_t)c0 * ld, (in ? in + (size_t)c0 * ld : nullptr), out + (size_t)c0 * ld,
                                              ld, l.bc_cap));
        } else if (l.Ain.lpr == 4) {
            DISPATCH_D(dc, hipLaunchKernelGGL((gmgk::gs_block4<T, D, 8>), dim3(nb), dim3(4 * h->cfg.block_rows), 0, h->stream, blk_begin,
                                              blk_ncolors, l.d_row_color, l.Ain.slice_ptr, l.ain_col16, Prec<T>::val(l.Ain), l.Aout.slice_ptr,
                                              l.Aout.col, Prec<T>::val(l.Aout), Prec<T>::diag(l), b + (size_t)c0 * ld, (in ? in + (size_t)c0 * ld : nullptr),
                                              out + (size_t)c0 * ld, ld));
        } else {
            DISPATCH_D(dc, hipLaunchKernelGGL((gmgk::gs_block<T, D, (D == 1 ? 32 : 24)>), dim3(nb), dim3(h->cfg.block_rows), 0, h->stream, blk_begin,
                                              blk_ncolors, l.d_row_color, l.Ain.slice_ptr, l.ain_col16, Prec<T>::val(l.Ain), l.Aout.slice_ptr,
                                              l.Aout.col, Prec<T>::val(l.Aout), Prec<T>::diag(l), b + (size_t)c0 * ld, (in ? in + (size_t)c0 * ld : nullptr),
                                              out + (size_t)c0 * ld, ld));
        }
    });
}

template <class T>
SmoothDone<T> launch_block_sweeps(gmg_handle h, Level& l, int d, int iters, const SmoothAsk<T>& ask) {
    SmoothDone<T> done;
    const int ld = l.n_pad;
    const int nb = l.ord.n_blocks();
    // from_zero: the iterate is the zero vector (the coarse correction's initial guess, multigrid_solver.cpp:1072-1073): the
    // first sweep gets no input vector -- it neither reads x nor gathers the off-block couplings (all zero) -- and the
    // caller skips the memset
    T* in = ask.from_zero ? nullptr : Prec<T>::x(l); T* out = Prec<T>::tmp(l);
    const T* before_last = nullptr;      // the iterate the last sweep started from (nullptr: the zero vector)
    bool last_known = false;
    int it0 = 0;
    if (ask.from_zero && ask.first_done) {         // the restriction into this level already ran the first sweep (launch_restrict_sweep0): its result is in tmp
        before_last = nullptr; last_known = true;
        in = out; out = Prec<T>::x(l);
        it0 = 1;
    }
    for (int it = it0; it < iters; ++it) {
        // (il_out: the last sweep also writes the level's x as an interleaved multi-vector)
        const bool with_il = ask.il_out && it == iters - 1 && l.use_ep && d > 1 && d <= 4;
        launch_block_sweep_range<T>(h, l, d, in, out, 0, nb, nullptr, nullptr, with_il ? ask.il_out : nullptr);
        if (with_il) done.il_written = true;
        before_last = in; last_known = true;
        if (it == 0 && ask.from_zero) { in = out; out = Prec<T>::x(l); }      // the result of sweep 1 is in tmp; ping-pong from there
        else std::swap(in, out);
    }
    if (in != Prec<T>::x(l)) (void)hipMemcpyAsync(Prec<T>::x(l), in, sizeof(T) * (size_t)ld * d, hipMemcpyDeviceToDevice, h->stream);
    // what residual_delta_ep needs: the last sweep went before_last -> x (the copy above, if any, does not touch before_last)
    done.prev_valid = last_known && before_last != (const T*)Prec<T>::x(l);
    done.prev = before_last;
    return done;
}

// r = b - A x of a blocked level with the unpadded block storage, straight after its block sweeps (swept: their result -- the iterate the
// last sweep started from): the sweep's explicit part applied to x_old - x_new (kernels.hip.hpp::residual_delta_ep)
// (begin_table / nb_list: an explicit list of blocks -- a rank's blocks of a partitioned level -- instead of all of them)
template <class T>
bool launch_residual_delta(gmg_handle h, Level& l, int d, T* r, const SmoothDone<T>& swept, const int* begin_table = nullptr, int nb_list = 0) {
    if (!l.use_ep || !swept.prev_valid || pointwise_smoother(h->cfg)) return false;
    const int ld = l.n_pad, nb = begin_table ? nb_list : l.ord.n_blocks();
    if (nb <= 0) return true;
    const int grid = (nb + 7) / 8 * 8;
    const T* x_old = swept.prev;
    const T* x_new = Prec<T>::x(l);
    for_col_chunks(d, [&](int c0, int dc) {
        DISPATCH_D(dc, DISPATCH_FLAG(STREAM, ep_streams(l), hipLaunchKernelGGL((gmgk::residual_delta_ep<T, D, STREAM>), dim3(grid), dim3(64),
                                          gmgk::ep_lds_bytes<T>(0, l.ep_cap_e, 0), h->stream, begin_table, l.ee_ptr, l.ee_col, Prec<T>::eeval(l),
                                          (x_old ? x_old + (size_t)c0 * ld : nullptr), x_new + (size_t)c0 * ld, r + (size_t)c0 * ld, ld, nb)));
    });
    return true;
}

// true when smoothing level l from a zero iterate needs no materialised zero vector: block sweeps, or a pointwise smoother with
// gmg_config::zero_guess_step (launch_zero_step) -- at least one sweep / step either way
inline bool smooth_from_zero_ok(gmg_handle h, const Level& l, int iters) {
    if (pointwise_smoother(h->cfg)) return iters > 0 && h->cfg.zero_guess_step != 0;
    return iters > 0 && l.ord.blocked;
}

template <class T = double>
SmoothDone<T> launch_smooth(gmg_handle h, Level& l, int d, int iters, const SmoothAsk<T>& ask = {}) {
    if (iters <= 0) return {};
    if (h->cfg.smoother == GMG_SMOOTHER_JACOBI) launch_jacobi_sweeps<T>(h, l, d, iters, ask);
    else if (h->cfg.smoother == GMG_SMOOTHER_CHEBYSHEV) launch_cheby_steps<T>(h, l, d, iters, ask);
    else if (l.ord.blocked) return launch_block_sweeps<T>(h, l, d, iters, ask);
    else return launch_gs_sweeps<T>(h, l, d, iters, ask);
    return {};
}

// y = A x (mode 0) or y = b - A x (mode 1) on the slices [sb, se) of level l
// y_il: the residual as an interleaved multi-vector (level 0, one lane per row, d = 2 .. 4: what the restriction gathers from)
template <class T, int LPR>
void launch_spmv_lpr(gmg_handle h, Level& l, int d, int mode, const T* b, const T* x, T* y, int sb, int se, bool y_il = false) {
    const int ld = l.n_pad;
    const bool il = y_il && mode == 1 && LPR == 1 && d > 1 && d <= 4;
    for_col_chunks(d, [&](int c0, int dc) {
        // (the 16-bit column codes belong to the one-lane-per-row layout of level 0: the quad layout has the plain instantiation only)
        DISPATCH_D(dc, DISPATCH_C16(l.Aoff.c16_sel(), DISPATCH_FLAG(RES, mode == 1, DISPATCH_FLAG(YI, il,
                       hipLaunchKernelGGL((gmgk::spmv_full<T, D, (RES ? 1 : 0), LPR, (LPR == 1 ? C16 : 0), (YI && RES && LPR == 1 && D > 1)>), dim3(grid_for(se - sb)),
                                          dim3(gmgk::kBlock), 0, h->stream, l.Aoff.slice_ptr, l.Aoff.col, Prec<T>::val(l.Aoff), Prec<T>::diag(l),
                                          (RES ? b + (size_t)c0 * ld : nullptr), x + (size_t)c0 * ld, y + (size_t)c0 * ld, ld, sb, se, 1, l.Aoff.col16,
                                          l.Aoff.win_base, l.Aoff.c16_arg())))));
    });
}
// the same on a LIST of slices (a rank's rows of a level partitioned by blocks), mode 1
template <class T>
void launch_spmv_list(gmg_handle h, Level& l, int d, const T* b, const T* x, T* y, const int* slices, int n_list) {
    const int ld = l.n_pad;
    for_col_chunks(d, [&](int c0, int dc) {
        DISPATCH_D(dc, DISPATCH_FLAG(QUAD, l.Aoff.lpr == 4, hipLaunchKernelGGL((gmgk::spmv_full_list<T, D, 1, (QUAD ? 4 : 1)>), dim3(grid_for(n_list)), dim3(gmgk::kBlock), 0,
                                          h->stream, l.Aoff.slice_ptr, l.Aoff.col, Prec<T>::val(l.Aoff), Prec<T>::diag(l), b + (size_t)c0 * ld, x + (size_t)c0 * ld,
                                          y + (size_t)c0 * ld, ld, slices, n_list)));
    });
}
// the first n_slices slices (all of them by default)
template <class T>
void launch_spmv(gmg_handle h, Level& l, int d, int mode, const T* b, const T* x, T* y, int n_slices = -1, bool y_il = false) {
    if (n_slices < 0) n_slices = l.Aoff.n_slices;
    if (l.Aoff.lpr == 4) launch_spmv_lpr<T, 4>(h, l, d, mode, b, x, y, 0, n_slices);
    else launch_spmv_lpr<T, 1>(h, l, d, mode, b, x, y, 0, n_slices, y_il);
}

// coarse.b = U^T fine.r   (src_il: the source is an interleaved multi-vector, d = 2 .. 4)
template <class T, int LPR>
void launch_restrict_lpr(gmg_handle h, Level& fine, Level& coarse, int d, const T* src, T* dst, bool src_il = false) {
    const bool il = src_il && d > 1 && d <= 4;
    for_col_chunks(d, [&](int c0, int dc) {
        DISPATCH_D(dc, DISPATCH_C16(fine.R.c16_sel(), DISPATCH_FLAG(XI, il, hipLaunchKernelGGL((gmgk::transfer<T, D, 0, LPR, C16, (XI && D > 1)>), dim3(grid_for(fine.R.n_slices)),
                                          dim3(gmgk::kBlock), 0, h->stream, fine.R.slice_ptr, fine.R.col, Prec<T>::val(fine.R), fine.R.row_of, src + (size_t)c0 * fine.n_pad,
                                          fine.n_pad, dst + (size_t)c0 * coarse.n_pad, coarse.n_pad, 0, fine.R.n_slices, 1, fine.R.col16, fine.R.win_base, fine.R.c16_arg()))));
    });
}
// the same on a LIST of the restriction's slices (a rank's rows of a coarse level partitioned by blocks; 32-bit columns, column-major source)
template <class T>
void launch_restrict_list(gmg_handle h, Level& fine, Level& coarse, int d, const T* src, T* dst, const int* slices, int n_list) {
    for_col_chunks(d, [&](int c0, int dc) {
        DISPATCH_D(dc, DISPATCH_FLAG(QUAD, fine.R.lpr == 4, hipLaunchKernelGGL((gmgk::transfer_list<T, D, 0, (QUAD ? 4 : 1)>), dim3(grid_for(n_list)), dim3(gmgk::kBlock), 0,
                                          h->stream, fine.R.slice_ptr, fine.R.col, Prec<T>::val(fine.R), fine.R.row_of, src + (size_t)c0 * fine.n_pad, fine.n_pad,
                                          dst + (size_t)c0 * coarse.n_pad, coarse.n_pad, slices, n_list)));
    });
}
template <class T>
void launch_restrict(gmg_handle h, Level& fine, Level& coarse, int d, const T* src, T* dst, bool src_il = false) {
    if (fine.R.lpr == 4) launch_restrict_lpr<T, 4>(h, fine, coarse, d, src, dst, src_il);
    else launch_restrict_lpr<T, 1>(h, fine, coarse, d, src, dst, src_il);
}

// Pointwise smoothers (gmg_config::zero_guess_step): may the restriction into `coarse` compute that level's zero step for the rows it writes
// (transfer<.., STEP0>)?  The one rule: the level is smoothed from zero (smooth_from_zero_ok: a pointwise smoother with the field set and
// pre_iters >= 1; the caller keeps the coarsest level out) and all columns are one chunk (d <= 4) -- with more, the separate zero step runs
// (launch_zero_step), as it does on the coarsest-but-one level of a caller that restricts by hand.  Every layout of the restriction qualifies:
// one or four lanes per row, with or without an output-row map, 16-bit codes or not, interleaved or column-major source.
inline bool restrict_step0_ok(gmg_handle h, const Level& coarse, int d) {
    return pointwise_smoother(h->cfg) && smooth_from_zero_ok(h, coarse, h->cfg.pre_iters) && d <= 4;
}
// coarse.b = U^T fine.r, and coarse.tmp (Chebyshev: and p) = the zero step on it, in one launch
template <class T, int LPR>
void launch_restrict_step0_lpr(gmg_handle h, Level& fine, Level& coarse, int d, const T* src, bool src_il) {
    const bool il = src_il && d > 1 && d <= 4;
    const T c = zero_step_coeff<T>(h, coarse);
    DISPATCH_D(d, DISPATCH_C16(fine.R.c16_sel(), DISPATCH_FLAG(XI, il, DISPATCH_FLAG(CHEB, h->cfg.smoother == GMG_SMOOTHER_CHEBYSHEV,
                  hipLaunchKernelGGL((gmgk::transfer<T, D, 0, LPR, C16, (XI && D > 1), (CHEB ? 2 : 1)>), dim3(grid_for(fine.R.n_slices)), dim3(gmgk::kBlock), 0, h->stream,
                                     fine.R.slice_ptr, fine.R.col, Prec<T>::val(fine.R), fine.R.row_of, src, fine.n_pad, Prec<T>::b(coarse), coarse.n_pad, 0, fine.R.n_slices, 1,
                                     fine.R.col16, fine.R.win_base, fine.R.c16_arg(), Prec<T>::diag(coarse), Prec<T>::tmp(coarse), Prec<T>::r(coarse), c)))));
}
template <class T>
void launch_restrict_step0(gmg_handle h, Level& fine, Level& coarse, int d, const T* src, bool src_il) {
    if (fine.R.lpr == 4) launch_restrict_step0_lpr<T, 4>(h, fine, coarse, d, src, src_il);
    else launch_restrict_step0_lpr<T, 1>(h, fine, coarse, d, src, src_il);
}

// coarse.b = U^T fine.r AND the first pre-sweep of the coarse level from the zero iterate, in one launch (kernels.hip.hpp::restrict_sweep0), where the
// layouts allow it: the coarse level runs the entry-parallel block sweep on blocks b = rows 64 b .., its restriction has the quad layout with
// 64-row sorting windows (a workgroup's four slices = one block), and the level's pre-smoothing starts from zero.  The coarse level's
// launch_block_sweeps then starts with its second sweep (SmoothAsk::first_done, from restrict_into's return value).
// which fused form the restriction into `coarse` takes: 0 none, 1 restrict_sweep0 (entry-parallel sweep), 2 gs_block4<.., FR = true> (quad layout)
template <class T>
int restrict_sweep0_kind(gmg_handle h, const Level& fine, const Level& coarse, int d, bool src_il) {
    if (!h->cfg.fuse_restrict_sweep || pointwise_smoother(h->cfg) || h->cfg.pre_iters <= 0 || d > 4) return 0;
    if (!coarse.ord.blocked || fine.R.lpr != 4 || !(h->cfg.restrict_sigma == 0 || h->cfg.restrict_sigma == 64)) return 0;
    if (coarse.use_ep) return (coarse.n_pad == 64 * coarse.ord.n_blocks() && fine.R.n_slices == 4 * coarse.ord.n_blocks()) ? 1 : 0;      // (block b = rows 64 b .. 64 b + 63)
    // quad layout: a wave of the block sweep covers the 16 rows of one restriction slice; plain 32-bit restriction, column-major source
    if (!(coarse.use_bcsr && d > 1) && coarse.Ain.lpr == 4 && fine.R.c16_mode == 0 && !src_il && fine.R.n_slices * 16 == coarse.n_pad) return 2;
    return 0;
}
// blk_list / nb_list: the coarse blocks of ONE rank of a level partitioned by blocks instead of all of them (kind 1 only)
template <class T>
void launch_restrict_sweep0(gmg_handle h, Level& fine, Level& coarse, int d, const T* src, bool src_il, int kind, const int* blk_list = nullptr, int nb_list = 0) {
    const int nb = blk_list ? nb_list : coarse.ord.n_blocks();
    if (kind == 2) {
        DISPATCH_D(d, hipLaunchKernelGGL((gmgk::gs_block4<T, D, 8, true>), dim3(nb), dim3(4 * h->cfg.block_rows), 0, h->stream, coarse.d_blk_begin, coarse.d_blk_ncolors,
                                         coarse.d_row_color, coarse.Ain.slice_ptr, coarse.ain_col16, Prec<T>::val(coarse.Ain), coarse.Aout.slice_ptr, coarse.Aout.col,
                                         Prec<T>::val(coarse.Aout), Prec<T>::diag(coarse), (const T*)nullptr, (const T*)nullptr, Prec<T>::tmp(coarse), coarse.n_pad,
                                         fine.R.slice_ptr, fine.R.col, Prec<T>::val(fine.R), fine.R.row_of, src, fine.n_pad, Prec<T>::b(coarse)));
        return;
    }
    const int vgrid = (nb + 7) / 8 * 8;
    const size_t lds_sweep = gmgk::ep_lds_bytes<T>(d, 0, coarse.ep_cap_l);
    const size_t lds = lds_sweep + (size_t)d * 64 * sizeof(T);
    // (the result of a from-zero first sweep lives in tmp: launch_block_sweeps)
    DISPATCH_D(d, DISPATCH_C16(fine.R.c16_sel(), DISPATCH_FLAG(STREAM, ep_streams(coarse), DISPATCH_FLAG(XI, src_il,
                  hipLaunchKernelGGL((gmgk::restrict_sweep0<T, D, STREAM, C16, (XI && D > 1)>), dim3(vgrid), dim3(256), lds, h->stream, fine.R.slice_ptr, fine.R.col,
                                     Prec<T>::val(fine.R), fine.R.row_of, src, fine.n_pad, fine.R.col16, fine.R.win_base, fine.R.c16_arg(), Prec<T>::b(coarse),
                                     coarse.d_blk_ncolors, coarse.d_row_color, coarse.ep_ptr, coarse.ep_col, Prec<T>::epval(coarse), Prec<T>::diag(coarse),
                                     Prec<T>::tmp(coarse), coarse.n_pad, nb, vgrid, (int)lds_sweep, blk_list)))));
}

// fine.x += U coarse.x on the slices [sb, se) of the fine level (se < 0: all of them).  U has <= 3 entries per row: always one lane per row.
// src_il: the source is an interleaved multi-vector (d = 2 .. 4); c16: the kernels' C16 argument (< 0: what the layout of U asks for)
template <class T>
void launch_prolong_add(gmg_handle h, Level& fine, Level& coarse, int d, const T* src, T* dst, bool src_il = false, int sb = 0, int se = -1, int c16 = -1) {
    const bool il = src_il && d > 1 && d <= 4;
    if (se < 0) se = fine.P.n_slices;
    if (c16 < 0) c16 = fine.P.c16_sel();
    for_col_chunks(d, [&](int c0, int dc) {
        DISPATCH_D(dc, DISPATCH_C16(c16, DISPATCH_FLAG(XI, il, hipLaunchKernelGGL((gmgk::transfer<T, D, 1, 1, C16, (XI && D > 1)>), dim3(grid_for(se - sb)), dim3(gmgk::kBlock), 0,
                                          h->stream, fine.P.slice_ptr, fine.P.col, Prec<T>::val(fine.P), (const int*)nullptr, src + (size_t)c0 * coarse.n_pad, coarse.n_pad,
                                          dst + (size_t)c0 * fine.n_pad, fine.n_pad, sb, se, 1, fine.P.col16, fine.P.win_base, fine.P.c16_arg()))));
    });
}
// the same on a LIST of the prolongation's slices (32-bit columns, column-major source)
template <class T>
void launch_prolong_add_list(gmg_handle h, Level& fine, Level& coarse, int d, const T* src, T* dst, const int* slices, int n_list) {
    for_col_chunks(d, [&](int c0, int dc) {
        DISPATCH_D(dc, hipLaunchKernelGGL((gmgk::transfer_list<T, D, 1, 1>), dim3(grid_for(n_list)), dim3(gmgk::kBlock), 0, h->stream, fine.P.slice_ptr, fine.P.col,
                                          Prec<T>::val(fine.P), (const int*)nullptr, src + (size_t)c0 * coarse.n_pad, coarse.n_pad, dst + (size_t)c0 * fine.n_pad,
                                          fine.n_pad, slices, n_list));
    });
}

// Polled completion.  Slot 0: residual-norm sums in h_norm; slot 1: the coarsest right-hand side in h_pinned.
// The polled words and the data they announce are written by a kernel and read by the host while the stream is still
// busy: that needs fine-grained (coherent) pinned memory, requested explicitly -- what hipHostMallocDefault gives depends on
// the ROCm version and on HIP_HOST_COHERENT.
constexpr unsigned kPolledHostFlags = hipHostMallocCoherent | hipHostMallocMapped;
inline bool polled(gmg_handle h) { return !h->cfg.use_graph && h->poll && h->h_flag; }

int wait_flag(gmg_handle h, int slot) {
    const unsigned long long want = h->flag_seq[slot];
    auto t0 = clk::now();
    double next_query_ms = 20.0;
    for (unsigned spin = 1;; ++spin) {
        if (__atomic_load_n(h->h_flag + 8 * slot, __ATOMIC_ACQUIRE) == want) return GMG_OK;
        // safety net only (the runtime's query is not free and may touch the queue): a finished stream implies the data
        // is visible, flag or not; an error state must not spin for ever
        if ((spin & 4095u) == 0 && ms_since(t0) > next_query_ms) {
            hipError_t q = hipStreamQuery(h->stream);
            if (q == hipSuccess) {
                // the stream is idle, so the data is visible -- but the flag never showed up while it ran: this host does not
                // see device writes to pinned memory in flight.  Stop polling on this handle (copy + synchronise instead)
                if (__atomic_load_n(h->h_flag + 8 * slot, __ATOMIC_ACQUIRE) != want) { h->poll = false; h->timing["poll_disabled"] = 1.0; }
                return GMG_OK;
            }
            if (q != hipErrorNotReady) HIPCHK(q);
            next_query_ms += 20.0;
        }
        __builtin_ia32_pause();
    }
}

// the result of the last launch_norm / launch_residual_to_f32 is in h_norm when this returns
int wait_norm(gmg_handle h) {
    if (polled(h)) return wait_flag(h, 0);
    HIPCHK(hipStreamSynchronize(h->stream));
    return GMG_OK;
}

// What the check's reduction needs to take the loop's decision on the device (gmgk::SolveWatch): mode 0 a fixed number of cycles, 1 the rule of
// solve_rule.hpp; cycles done including this one.  The loops that enqueue heads hand one to vcycle_resident with every cycle; nobody else does.
// fold: the check also stores the next cycle's first colour update to level 0's side vector (fold_eligible; the caller then enqueues the folded head).
struct CycleWatch { int mode; double tol; int type; int cycles_done; bool fold = false; };

// the reduction of one group of <= 4 columns: into h_norm + flag when polled, into d_norm (+ a copy later) otherwise
// (partials: whose block sums -- the norm kernels' by default; decide: also take the loop's decision, see CycleWatch)
void launch_reduce(gmg_handle h, int nblk, int dc, int c0, bool last, const double* partials = nullptr, const CycleWatch* decide = nullptr) {
    if (!partials) partials = h->d_partials;
    if (polled(h)) {
        gmgk::SolveWatch watch{nullptr, nullptr, nullptr, 0.0, 0, 0, 0, 0};
        if (decide && last && c0 == 0 && h->d_watch)         // (one group of columns: the kernel sees every sum the decision needs)
            watch = gmgk::SolveWatch{reinterpret_cast<int*>(h->d_watch + 1), h->h_flag + 1, h->d_watch, decide->tol, decide->mode, decide->type, dc, decide->cycles_done};
        hipLaunchKernelGGL(gmgk::reduce_partials, dim3(1), dim3(gmgk::kReduceBlock), 0, h->stream, partials, nblk, 2 * dc, h->h_norm + 2 * c0,
                           last ? h->h_flag : nullptr, last ? ++h->flag_seq[0] : 0ull, (int)EnvSwitches::get().publish_fenced, watch);
    }
    else
        hipLaunchKernelGGL(gmgk::reduce_partials, dim3(1), dim3(gmgk::kReduceBlock), 0, h->stream, partials, nblk, 2 * dc, h->d_norm + 2 * c0,
                           (unsigned long long*)nullptr, 0ull, 0);
}

// sums of w r^2 / w b^2 per column -> h_norm[2*d] (after wait_norm).  folded: partial-sum blocks the cycle's last colour launch already produced
// for the rows of the last colour (fold_norm; 0: none); decide: launch_reduce
int launch_norm(gmg_handle h, int d, int type, int folded = 0, const CycleWatch* decide = nullptr) {
    Level& l = h->lv[0];
    const double* w = type == 1 ? h->d_minv : (type == 2 ? h->d_mass : nullptr);
    const int n_slices = folded ? l.ord.color_begin[l.ord.n_colors - 1] / 64 : l.Aoff.n_slices;
    const int nblk = norm_grid(n_slices);                // one slice per wave, like the residual SpMV; one partial per block of 16
    const bool poll = polled(h);
    // (decide->fold: the same sums, and the next cycle's first colour update into level 0's side vector -- one group of columns, fold_eligible;
    // the first colour's slices lie in front of the last colour's, inside n_slices)
    const int c_head = decide && decide->fold && d <= 4 ? first_color(l) : -1;
    for_col_chunks(d, [&](int c0, int dc) {
        if (c_head >= 0) {
            DISPATCH_D(dc, DISPATCH_C16(l.Aoff.c16_sel(), hipLaunchKernelGGL((gmgk::residual_norm_slices_head<D, C16>), dim3(nblk), dim3(gmgk::kNormWaves * 64), 0, h->stream,
                                              l.Aoff.slice_ptr, l.Aoff.col, l.Aoff.val, l.diag, l.b.get(), l.x.get(), w, l.n_pad, n_slices, h->d_partials.get(), l.Aoff.col16,
                                              l.Aoff.win_base, l.Aoff.c16_arg(), l.xh.get(), l.ord.color_begin[c_head] / 64, l.ord.color_begin[c_head + 1] / 64,
                                              level_omega<double>(h, l))));
        } else {
            DISPATCH_D(dc, DISPATCH_C16(l.Aoff.c16_sel(), hipLaunchKernelGGL((gmgk::residual_norm_slices<D, 0, C16>), dim3(nblk), dim3(gmgk::kNormWaves * 64), 0, h->stream,
                                              l.Aoff.slice_ptr, l.Aoff.col, l.Aoff.val, l.diag, l.b + (size_t)c0 * l.n_pad, l.x + (size_t)c0 * l.n_pad, w,
                                              l.n_pad, n_slices, (float*)nullptr, h->d_partials, l.Aoff.col16, l.Aoff.win_base, l.Aoff.c16_arg())));
        }
        launch_reduce(h, nblk + folded, dc, c0, c0 + 4 >= d, nullptr, decide);
    });
    if (!poll) HIPCHK(hipMemcpyAsync(h->h_norm, h->d_norm, sizeof(double) * 2 * d, hipMemcpyDeviceToHost, h->stream));
    return GMG_OK;
}

int ensure_vectors(gmg_handle h, int d) {
    if (d <= h->dcap) return GMG_OK;
    drop_graphs(h);
    unbind_level0(h);
    h->accel = {};
    h->pcg = {};
    h->nullsp = {};
    // a zeroed n_pad x d vector of the level, or none (wanted = false): the old one goes back to the pool either way
    auto vec = [&](auto& v, const Level& l, bool wanted) -> int {
        v.reset();
        if (!wanted) return GMG_OK;
        const size_t count = (size_t)l.n_pad * d;
        int rc = dev_alloc(h, v, count);
        if (rc == GMG_OK) HIPCHK(hipMemsetAsync(v, 0, sizeof(*v.get()) * count, h->stream));
        return rc;
    };
    for (auto& l : h->lv) {
        const bool tmp = pointwise_smoother(h->cfg) || l.ord.blocked, f32 = fp32_cycle_wanted(h->cfg);
        int rc;
        if ((rc = vec(l.x, l, true)) || (rc = vec(l.b, l, true)) || (rc = vec(l.r, l, true)) || (rc = vec(l.tmp, l, tmp)) ||
            (rc = vec(l.x32, l, f32)) || (rc = vec(l.b32, l, f32)) || (rc = vec(l.r32, l, f32)) || (rc = vec(l.tmp32, l, f32 && tmp))) return rc;
    }
    {   // the side vector of the folded head (fold_eligible asks for it): the first colour's slices, d columns
        Level& l0 = h->lv[0];
        const int fc = h->cfg.fold_head && !l0.ord.blocked ? first_color(l0) : -1;
        l0.xh.reset(); l0.xh_rows = 0;
        if (fc >= 0) {
            const int rows = (l0.ord.color_begin[fc + 1] / 64 - l0.ord.color_begin[fc] / 64) * 64;
            int rc = dev_alloc(h, l0.xh, (size_t)rows * d);
            if (rc) return rc;
            l0.xh_rows = rows;
        }
    }
    Level& c = h->lv[h->L];
    size_t need = (size_t)c.n_pad * d * 2;
    if (need > h->pinned_cap) {
        if (h->h_pinned) (void)sync_hipHostFree(h->h_pinned);
        HIPCHK(hipHostMalloc((void**)&h->h_pinned, sizeof(double) * need, kPolledHostFlags));
        h->pinned_cap = need;
    }
    if (h->h_norm) (void)sync_hipHostFree(h->h_norm);
    HIPCHK(hipHostMalloc((void**)&h->h_norm, sizeof(double) * 2 * d, kPolledHostFlags));
    if (!h->h_flag) {
        HIPCHK(hipHostMalloc((void**)&h->h_flag, 256, kPolledHostFlags));
        std::memset(h->h_flag, 0, 256);
    }

    int rc;
    if ((rc = dev_alloc(h, h->d_norm, (size_t)2 * d))) return rc;
    if (!h->d_watch) {
        if ((rc = dev_alloc(h, h->d_watch, 2))) return rc;
        HIPCHK(hipMemsetAsync(h->d_watch, 0, 16, h->stream));
    }
    h->dcap = d;
    h->loaded_d = 0;
    return GMG_OK;
}

int ensure_stage(gmg_handle h, size_t n_doubles) {
    if (n_doubles <= h->stage_cap) return GMG_OK;
    int rc;
    if ((rc = dev_alloc(h, h->d_stage, n_doubles))) return rc;
    h->stage_cap = n_doubles;
    return GMG_OK;
}

// Pinned, double-buffered host staging: the caller's (pageable) vectors are copied in with a few threads and moved by
// DMA at PCIe speed (a pageable hipMemcpy of 24 MB runs at a fraction of that: 3 vectors cost ~18 ms per solve at 3 M).
int ensure_host_stage(gmg_handle h, size_t n_doubles) {
    if (n_doubles <= h->h_stage_cap) return GMG_OK;
    for (int i = 0; i < 2; ++i) {
        if (h->h_stage[i]) (void)sync_hipHostFree(h->h_stage[i]);
        h->h_stage[i] = nullptr;
        HIPCHK(hipHostMalloc((void**)&h->h_stage[i], sizeof(double) * n_doubles, hipHostMallocDefault));
        if (!h->h_stage_ev[i]) HIPCHK(hipEventCreateWithFlags(&h->h_stage_ev[i], hipEventDisableTiming));
    }
    h->h_stage_cap = n_doubles;
    return GMG_OK;
}

inline void threaded_copy(double* dst, const double* src, size_t n, int threads) {
    const int T = (int)std::min<size_t>(std::max(1, std::min(threads, 16)), n / 65536 + 1);
    if (T <= 1) { std::memcpy(dst, src, sizeof(double) * n); return; }
    parallel_ranges(T, T, [&](int t0, int t1, int) {
        for (int t = t0; t < t1; ++t) {
            size_t lo = n * t / T, hi = n * (t + 1) / T;
            std::memcpy(dst + lo, src + lo, sizeof(double) * (hi - lo));
        }
    }, 1);
}

// Vectors cross PCIe in chunks so that the host's copy between the caller's (pageable) array and the pinned staging buffer overlaps
// the DMA of the neighbouring chunk: 24 MB took ~0.35 ms of copy + ~0.5 ms of DMA one after the other.
constexpr int kXferChunks = 6;
inline size_t xfer_chunk(size_t cnt) { return std::max<size_t>((cnt + kXferChunks - 1) / kXferChunks, (size_t)1 << 17); }

// The pinned staging holds ONE column (n doubles per buffer, two buffers): an n x d block crosses column by column, alternating the buffers, so
// a first n x 3 solve pays no page-locking of a bigger staging area (16-40 ms at 3 M vertices: the demos' call, core.cpp:68-72) and the
// host copy of column c + 1 overlaps the DMA of column c.
// host natural n x d  ->  device numbering (level k) buffer
int to_device(gmg_handle h, int k, const double* src, int d, double* dst) {
    Level& l = h->lv[k];
    const size_t n = (size_t)l.n, cnt = n * d;
    int rc = ensure_stage(h, cnt);
    if (rc) return rc;
    if ((rc = ensure_host_stage(h, n))) return rc;
    const size_t ch = xfer_chunk(n);
    for (int c = 0; c < d; ++c) {
        const int f = h->h_stage_flip;
        h->h_stage_flip ^= 1;
        HIPCHK(hipEventSynchronize(h->h_stage_ev[f]));          // the previous DMA out of this staging buffer is done
        for (size_t off = 0; off < n; off += ch) {
            const size_t len = std::min(ch, n - off);
            threaded_copy(h->h_stage[f] + off, src + c * n + off, len, h->cfg.host_threads);
            HIPCHK(hipMemcpyAsync(h->d_stage + c * n + off, h->h_stage[f] + off, sizeof(double) * len, hipMemcpyHostToDevice, h->stream));
        }
        HIPCHK(hipEventRecord(h->h_stage_ev[f], h->stream));
    }
    hipLaunchKernelGGL(gmgk::permute_in, dim3((l.n_pad + 255) / 256), dim3(256), 0, h->stream, h->d_stage, l.n, l.d_new2old, dst, l.n_pad, l.n_pad, d);
    // d_stage is reused by the next call: order is guaranteed by the single stream
    return GMG_OK;
}

int to_host(gmg_handle h, int k, const double* src, int d, double* dst) {
    Level& l = h->lv[k];
    const size_t n = (size_t)l.n, cnt = n * d;
    int rc = ensure_stage(h, cnt);
    if (rc) return rc;
    if ((rc = ensure_host_stage(h, n))) return rc;
    HIPCHK(hipEventSynchronize(h->h_stage_ev[0]));
    HIPCHK(hipEventSynchronize(h->h_stage_ev[1]));
    hipLaunchKernelGGL(gmgk::permute_out, dim3((l.n_pad + 255) / 256), dim3(256), 0, h->stream, src, l.n_pad, l.n_pad, l.d_new2old, h->d_stage, l.n, d);
    const size_t ch = xfer_chunk(n);
    constexpr int kEvPerBuf = (int)(sizeof(h->h_chunk_ev) / sizeof(h->h_chunk_ev[0])) / 2;
    static_assert(kEvPerBuf >= kXferChunks, "one event per chunk and staging buffer");
    auto issue = [&](int c) -> int {                             // column c on the wire, into buffer c & 1, an event behind every chunk
        const int f = c & 1;
        int nch = 0;
        for (size_t off = 0; off < n; off += ch, ++nch) {
            const size_t len = std::min(ch, n - off);
            hipEvent_t& ev = h->h_chunk_ev[f * kEvPerBuf + nch];
            if (!ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            HIPCHK(hipMemcpyAsync(h->h_stage[f] + off, h->d_stage + c * n + off, sizeof(double) * len, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipEventRecord(ev, h->stream));
        }
        return GMG_OK;
    };
    if ((rc = issue(0))) return rc;
    for (int c = 0; c < d; ++c) {
        if (c + 1 < d && (rc = issue(c + 1))) return rc;         // (its buffer was copied out two columns ago)
        const int f = c & 1;
        int nch = 0;
        for (size_t off = 0; off < n; off += ch, ++nch) {
            const size_t len = std::min(ch, n - off);
            HIPCHK(hipEventSynchronize(h->h_chunk_ev[f * kEvPerBuf + nch]));
            threaded_copy(dst + c * n + off, h->h_stage[f] + off, len, h->cfg.host_threads);
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return GMG_OK;
}

// ---- caller-owned device memory (gmg_solve_device, gmg_set_system_values_device) ------------------------

// the column count as a template argument where the kernels have a fast path (1 .. 4), 0 = run-time d otherwise
#define DISPATCH_D_ANY(dc, ...)          \
    switch (dc) {                        \
        case 1: { constexpr int D = 1; __VA_ARGS__; } break; \
        case 2: { constexpr int D = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int D = 3; __VA_ARGS__; } break; \
        case 4: { constexpr int D = 4; __VA_ARGS__; } break; \
        default: { constexpr int D = 0; __VA_ARGS__; } break; \
    }

// `what` [0 .. extent] (doubles) must be device memory of the handle's device, inside one allocation.  Nothing but device memory may reach
// a kernel: a host pointer would fault the device.
int check_device_block(gmg_handle h, const void* p, int64_t extent, const char* what) {
    hipPointerAttribute_t attr;
    std::memset(&attr, 0, sizeof(attr));
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return fail(h, GMG_ERR_INVALID, std::string(what) + " is not device memory (unknown to the HIP runtime: a host pointer?)"); }
    if (attr.type != hipMemoryTypeDevice || attr.isManaged) return fail(h, GMG_ERR_INVALID, std::string(what) + " is not plain device memory (host, pinned or managed memory)");
    if (attr.device != h->cfg.device) return fail(h, GMG_ERR_INVALID, std::string(what) + " lives on device " + std::to_string(attr.device) + ", the handle on device " + std::to_string(h->cfg.device));
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return GMG_OK; }      // (no range to compare with: virtual-memory mappings)
    const size_t off = (size_t)((const char*)p - (const char*)base);
    if (off > size || (size_t)(extent + 1) > (size - off) / sizeof(double)) return fail(h, GMG_ERR_INVALID, std::string(what) + " with these strides does not fit the allocation it points into");
    return GMG_OK;
}

int check_device_vectors(gmg_handle h, const gmg_device_vectors& v, int n, int d) {
    int rc;
    int64_t e = 0;
    (void)strided_extent(n, d, v.rhs_row_stride, v.rhs_col_stride, &e);           // (shapes were checked: device_vectors_fault)
    if ((rc = check_device_block(h, v.rhs, e, "rhs"))) return rc;
    if (v.x0) {
        (void)strided_extent(n, d, v.x0_row_stride, v.x0_col_stride, &e);
        if ((rc = check_device_block(h, v.x0, e, "x0"))) return rc;
    }
    (void)strided_extent(n, d, v.x_row_stride, v.x_col_stride, &e);
    return check_device_block(h, v.x, e, "x");
}

// level-0 b <- rhs and x <- x0 (or rhs) in one pass over the ordering; x <- level-0 iterate
void launch_permute_in2_strided(gmg_handle h, Level& l, const gmg_device_vectors& v, int d) {
    const dim3 grid((l.n_pad + 255) / 256);
    DISPATCH_D_ANY(d, DISPATCH_FLAG(X0, v.x0 != nullptr, hipLaunchKernelGGL((gmgk::permute_in2_strided<D, X0>), grid, dim3(256), 0, h->stream, v.rhs, v.rhs_row_stride,
                                        v.rhs_col_stride, v.x0, v.x0_row_stride, v.x0_col_stride, l.d_new2old, l.b, l.x, l.n_pad, l.n_pad, d)));
}

void launch_permute_out_strided(gmg_handle h, Level& l, const gmg_device_vectors& v, int d) {
    DISPATCH_D_ANY(d, hipLaunchKernelGGL((gmgk::permute_out_strided<D>), dim3((l.n_pad + 255) / 256), dim3(256), 0, h->stream, (const double*)l.x, l.n_pad, l.n_pad,
                                         l.d_new2old, v.x, v.x_row_stride, v.x_col_stride, d));
}

// ---- V-cycle legs --------------------------------------------------------------------------------------

// gmg_profile_cycle: an event at every boundary between the legs of a cycle (2 L + 3 of them: before each level's way down, after the
// last one, at the start of the way up, after each level's way up, after the residual check)
inline void prof_mark(gmg_handle h) {
    if (!h->prof_on) return;
    if ((size_t)h->prof_n >= h->prof_ev.size()) { hipEvent_t e = nullptr; if (hipEventCreate(&e) != hipSuccess) return; h->prof_ev.push_back(e); }
    (void)hipEventRecord(h->prof_ev[h->prof_n++], h->stream);
}

// coarse.b = U_k^T r_k (:1069) into level k + 1 -- together with that level's first pre-sweep where the layouts allow the two in one launch
// (restrict_sweep0_kind).  Returns whether it did: the level's launch_block_sweeps then starts with its second sweep (SmoothAsk::first_done)
template <class T>
bool restrict_into(gmg_handle h, int k, int d, bool il) {
    Level& l = h->lv[k];
    Level& c = h->lv[k + 1];
    // (a pointwise smoother: the restriction's launch computes the level's zero step -- restrict_step0_ok; SmoothAsk::first_done means that result there)
    if (k + 1 < h->L && restrict_step0_ok(h, c, d)) {
        ++h->fused_step_restrictions;
        launch_restrict_step0<T>(h, l, c, d, Prec<T>::r(l), il);
        return true;
    }
    const int fused = (k + 1 < h->L && smooth_from_zero_ok(h, c, h->cfg.pre_iters)) ? restrict_sweep0_kind<T>(h, l, c, d, il) : 0;
    if (fused) { ++h->fused_restrictions; launch_restrict_sweep0<T>(h, l, c, d, Prec<T>::r(l), il, fused); }
    else launch_restrict<T>(h, l, c, d, Prec<T>::r(l), Prec<T>::b(c), il);
    return fused != 0;
}

// the way down from level k0.  first_done: the caller's restriction into level k0 ran that level's first pre-sweep (restrict_into's return
// value: a caller that starts below level 0 restricted into level k0 itself); head_done: level 0's first colour launch is in the stream;
// x0_zero: level 0 starts from the zero vector too and its x holds anything (level0_zero_guess: the engine's own zero guesses)
template <class T = double>
void enqueue_down(gmg_handle h, int d, int k0 = 0, bool first_done = false, int head_done = 0, bool x0_zero = false) {
    const int L = h->L;
    for (int k = k0; k < L; ++k) {
        Level& l = h->lv[k];
        prof_mark(h);
        SmoothAsk<T> ask;
        ask.from_zero = (k > 0 || x0_zero) && smooth_from_zero_ok(h, l, h->cfg.pre_iters);      // eps.setZero (:1072-1073) folded into the first sweep
        if (k > 0 && !ask.from_zero) (void)hipMemsetAsync(Prec<T>::x(l), 0, sizeof(T) * (size_t)l.n_pad * d, h->stream);
        ask.first_done = first_done; ask.head_done = k == 0 ? head_done : 0;
        // d = 2 .. 4: the level-0 residual is written as an INTERLEAVED multi-vector (n x d row-major) -- only the restriction reads it, and a
        // gathered child then costs one cache line instead of d
        const bool il = k == 0 && d > 1 && d <= 4 && l.Aoff.lpr == 1;
        // level 0, fp64: the last colour launch of the pre-smoothing also writes the residual of its rows (fold_residual)
        if (k == 0 && sizeof(T) == 8) { ask.res_out = Prec<T>::r(l); ask.res_il = il; }
        const SmoothDone<T> swept = launch_smooth<T>(h, l, d, h->cfg.pre_iters, ask);                // :1063
        const int res_slices = (k == 0 && swept.res_from > 0) ? swept.res_from : -1;
        // :1066.  Straight after block sweeps on the unpadded block storage the residual comes from the sweep's explicit part alone
        if (!(k > 0 && launch_residual_delta<T>(h, l, d, Prec<T>::r(l), swept)))
            launch_spmv<T>(h, l, d, 1, Prec<T>::b(l), Prec<T>::x(l), Prec<T>::r(l), res_slices, il);
        // :1069 (+ the first pre-sweep of level k + 1 where the layouts allow the two in one launch)
        first_done = restrict_into<T>(h, k, d, il);
    }
    prof_mark(h);
}

// the way up to level k0.  norm_type >= 0: the check the cycle ends with, which level 0's last colour launch may join; returns fold_norm's blocks
template <class T = double>
int enqueue_up(gmg_handle h, int d, int k0 = 0, int norm_type = -1) {
    prof_mark(h);
    int norm_blocks = 0;
    bool il = false;
    for (int k = h->L - 1; k >= k0; --k) {
        Level& l = h->lv[k];
        // d = 2 .. 4: level 1's last post-sweep left a second, interleaved copy of its x in its (idle) residual vector: the prolongation into
        // level 0 gathers a parent's d values from one cache line
        const T* src = il ? Prec<T>::r(h->lv[k + 1]) : Prec<T>::x(h->lv[k + 1]);
        launch_prolong_add<T>(h, l, h->lv[k + 1], d, src, Prec<T>::x(l), il);     // :1082
        SmoothAsk<T> ask;
        if (k == 1 && k0 == 0 && d > 1 && d <= 4 && h->cfg.post_iters > 0 && l.ord.blocked && l.use_ep && !pointwise_smoother(h->cfg))
            ask.il_out = Prec<T>::r(l);
        if (k == 0) ask.norm_type = norm_type;
        const SmoothDone<T> swept = launch_smooth<T>(h, l, d, h->cfg.post_iters, ask);               // :1085
        il = swept.il_written; norm_blocks = swept.norm_blocks;
        prof_mark(h);
    }
    return norm_blocks;
}

// (n = 0 -- the block-CSR of a level that is one block has no entry -- is no launch: a grid of 0 workgroups is refused, and the error it leaves
// behind would be reported by the next gmg_set_system on this thread)
inline void launch_cvt(gmg_handle h, const double* src, float* dst, size_t n) {
    if (n == 0) return;
    hipLaunchKernelGGL(gmgk::cvt_f64_to_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, src, dst, (int64_t)n);
}
inline void launch_cvt(gmg_handle h, const float* src, double* dst, size_t n) {
    if (n == 0) return;
    hipLaunchKernelGGL(gmgk::cvt_f32_to_f64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, src, dst, (int64_t)n);
}

#ifndef GMG_SYMV_ROWS
#define GMG_SYMV_ROWS 0
#endif
inline int symv_rows(int n, int d) {
    const int forced = EnvSwitches::get().symv_rows;      // (measurement: scripts/symv_sweep.py)
    if (forced == 1 || forced == 2 || forced == 4) return forced;
    if (GMG_SYMV_ROWS > 0) return GMG_SYMV_ROWS;       // (A/B builds)
    // with 16-byte loads (dense_symv_v2; profiles/r06/symv_rows_loads_sweep.txt): one row per wave while the level is small (n_L = 1 929: 11.8 us at
    // d = 1, 13.5 at d = 3; 2 968: 16.3), two beyond (4 046 at d = 3: 32.6; 6 005: 57 at d = 3, 50 at d = 1); four rows only pay with 8-byte loads
    (void)d;
    return n >= 3000 ? 2 : 1;
}
// strides of 64 columns a lane loads per trip (dense_symv's U)
inline int symv_strides(int n, int d, int rows) {
    const int forced = EnvSwitches::get().symv_strides;
    if (forced == 2 || forced == 4 || forced == 8) return forced;
    (void)n; (void)d; (void)rows;
    return 4;                                          // (2 / 4 / 8 measured: within the noise of each other except four rows x two strides at 4 046: +3 us)
}

// e = A_L^{-1} rc with the dense inverse (always applied in fp64; the fp32 cycle converts around it)
template <class T = double>
void enqueue_coarse_device(gmg_handle h, int d) {
    Level& c = h->lv[h->L];
    const size_t cnt = (size_t)c.n_pad * d;
    if (sizeof(T) == 4) launch_cvt(h, c.b32, c.b, cnt);
    if (h->coarse_triangle) {
        // GMG_COARSE_DEVICE_TRIANGLE: two launches per column group (kernels.hip.hpp::tri_symv_items / tri_symv_reduce); the groups share the scratch,
        // one after the other on the stream
        const int nb = tri_blocks(c.n);
        const bool nt = EnvSwitches::get().tri_nt;
        if (nb > 0) for_col_chunks(d, [&](int c0, int dc) {
            const double* b = c.b + (size_t)c0 * c.n_pad;
            double* x = c.x + (size_t)c0 * c.n_pad;
            DISPATCH_D(dc, DISPATCH_FLAG(NT, nt, hipLaunchKernelGGL((gmgk::tri_symv_items<D, NT>), dim3((unsigned)tri_item_count(nb)), dim3(gmgk::kBlock), 0, h->stream,
                                          (const double*)h->d_tri, (const int*)h->d_tri_perm, c.n, b, c.n_pad, h->d_tri_row, h->d_tri_col)));
            DISPATCH_D(dc, hipLaunchKernelGGL((gmgk::tri_symv_reduce<D>), dim3(nb), dim3(gmgk::kBlock), 0, h->stream, (const double*)h->d_tri_row,
                                          (const double*)h->d_tri_col, (const int*)h->d_tri_perm, c.n, nb, x, c.n_pad));
        });
        if (sizeof(T) == 4) launch_cvt(h, c.x, c.x32, cnt);
        return;
    }
    for_col_chunks(d, [&](int c0, int dc) {
        // rows per wave: the rows of a wave share the loads of the vectors (what bounds the product at d = 3 and at n_L beyond the L1's reach); a small
        // level keeps one row per wave -- it needs every wave it can get to cover the memory latency
        const int rows_per_wave = symv_rows(c.n, dc);
        const int per_block = gmgk::kWavesPerBlock * rows_per_wave;
        const dim3 grid((c.n + per_block - 1) / per_block);
        const int strides = symv_strides(c.n, dc, rows_per_wave);
        const double* b = c.b + (size_t)c0 * c.n_pad;
        double* x = c.x + (size_t)c0 * c.n_pad;
        if (EnvSwitches::get().symv_v2 && rows_per_wave <= 2 && (h->ainv_ld & 1) == 0 && (c.n_pad & 1) == 0) {      // 16-byte loads: one or two rows per wave
            DISPATCH_D(dc, DISPATCH_FLAG(TWO, rows_per_wave == 2, hipLaunchKernelGGL((gmgk::dense_symv_v2<D, (TWO ? 2 : 1), 2>), grid, dim3(gmgk::kBlock), 0, h->stream,
                                              h->d_ainv, c.n, h->ainv_ld, b, x, c.n_pad)));
        } else {
            DISPATCH_D(dc, DISPATCH_ONE_OF(R, rows_per_wave, 4, 2, 1, DISPATCH_ONE_OF(U, strides, 8, 4, 2, hipLaunchKernelGGL((gmgk::dense_symv<D, R, U>), grid,
                                              dim3(gmgk::kBlock), 0, h->stream, h->d_ainv, c.n, h->ainv_ld, b, x, c.n_pad))));
        }
    });
    if (sizeof(T) == 4) launch_cvt(h, c.x, c.x32, cnt);
}

// Host coarsest solve (:1075): rc to the host, LDL^T back-substitution per column (fp64), eps back.
// Polled handles split it in two so that the host's answer releases work that is ALREADY in the queue: coarse_host_begin enqueues
// the publication of rc, a stream wait on a host-written word (hipStreamWaitValue64) and the fetch of eps; the caller goes on
// enqueuing the way up (and the residual check); coarse_host_serve then waits for rc, solves, writes eps and the word.  Releasing
// queued work costs ~3 us after the host's store; launching it after the solve costs ~12 us for the first kernel and ~4 us for
// each of the next few (scripts/micro/wait_value.hip).
void coarse_host_solve(gmg_handle h, int d) {
    Level& c = h->lv[h->L];
    const size_t cnt = (size_t)c.n_pad * d;
    double* rc = h->h_pinned;
    double* e = h->h_pinned + cnt;
    auto t0 = clk::now();
    std::memset(e, 0, sizeof(double) * cnt);
    if (h->coarse_work.size() < (size_t)c.n * d) h->coarse_work.resize((size_t)c.n * d);
    // gmg_config::nullspace = 1: the pinned factor applies G; with the means removed on both sides this is P G P = A_L^+, the operator the
    // device modes keep as a matrix
    if (h->cfg.nullspace) remove_means(rc, (size_t)c.n_pad, c.n, d);
    h->coarse.solve_multi(rc, (size_t)c.n_pad, e, (size_t)c.n_pad, d, h->coarse_work.data(), h->coarse_helper.get());
    if (h->cfg.nullspace) remove_means(e, (size_t)c.n_pad, c.n, d);
    h->timing["coarse_host_ms"] += ms_since(t0);
}

// While one of these is alive the helper threads of the coarsest back-substitution spin (a hand-over costs ~0.2 us instead of a
// wake-up); outside they sleep and single solves run every part of the elimination tree on the calling thread.
// GMG_LDLT_THREADS = threads of a solve including the caller (default: as many as the factor has parts, at most 8); 1: no team.
struct HelperScope {
    gmg_handle h;
    // cols: right-hand sides of the solves to come (their (part, column) jobs are independent: up to 8 threads have work with d = 3)
    explicit HelperScope(gmg_handle hh, int cols = 1) : h(hh) {
        const int env_threads = EnvSwitches::get().ldlt_threads;
        // (every rank of a multi-GPU job keeps its team busy -- and this thread polls -- on the CPUs the job may use: a rank's team
        // is sized to its share of them (cpu_budget() divides by LOCAL_WORLD_SIZE) minus one CPU of slack, a throttled spinning
        // thread costs far more than it saves; ranks started without that variable are counted through the handle's world size)
        const int ranks = (h->dist_ready && EnvSwitches::get().local_world <= 1) ? std::max(1, h->world) : 1;
        const int share = cpu_budget() / ranks;
        int threads = std::min(std::min(h->coarse.parts() * std::max(1, std::min(cols, 4)), 8), share - 1);
        if (env_threads > 0) threads = std::min(threads, env_threads);
        if (h->coarse_device || threads < 2) { h = nullptr; return; }
        if (!h->coarse_helper || h->coarse_helper->helpers() != threads - 1) h->coarse_helper.reset(new SpinTeam(threads - 1));
        h->coarse_helper->stay_near_caller();
        h->coarse_helper->arm();
    }
    ~HelperScope() { if (h) h->coarse_helper->disarm(); }
    HelperScope(const HelperScope&) = delete;
    HelperScope& operator=(const HelperScope&) = delete;
};

// the host part of a pending gate (no-op without one).  The word is written even when waiting for rc failed: the stream must
// not stay blocked.
int coarse_host_serve(gmg_handle h) {
    if (!h->coarse_pending) return GMG_OK;
    h->coarse_pending = false;
    if (!h->coarse_warm) { h->coarse_warm_sink += h->coarse.warm(); h->coarse_warm = true; }      // (the device is busy with the way down)
    const int w = wait_flag(h, 1);
    if (w == GMG_OK) coarse_host_solve(h, h->coarse_pending_d);
    __atomic_store_n(h->h_flag + 16, h->flag_seq[2], __ATOMIC_RELEASE);
    if (h->gate_shared) { h->gate_shared = false; --tl_gates_held; gate_mutex().unlock_shared(); }
    return w;
}

}  // namespace
// an exception crossed a cycle: open a pending gate without an answer (the stream must not stay parked, the shared lock not stay held)
int gate_unwound(gmg_handle h) {
    if (h->coarse_pending) {
        h->coarse_pending = false;
        if (h->h_flag) __atomic_store_n(h->h_flag + 16, h->flag_seq[2], __ATOMIC_RELEASE);
    }
    if (h->gate_shared) { h->gate_shared = false; --tl_gates_held; gate_mutex().unlock_shared(); }
    return GMG_OK;
}
namespace {

template <class T = double>
int coarse_host_begin(gmg_handle h, int d) {
    Level& c = h->lv[h->L];
    const size_t cnt = (size_t)c.n_pad * d;
    double* rc = h->h_pinned;
    double* e = h->h_pinned + cnt;
    if (sizeof(T) == 4) launch_cvt(h, c.b32, c.b, cnt);          // tiny (n_L doubles): convert on the device, ship fp64
    if (polled(h)) {
        hipLaunchKernelGGL(gmgk::publish_to_host, dim3(1), dim3(gmgk::kBlock), 0, h->stream, c.b, rc, (int)cnt, h->h_flag + 8, ++h->flag_seq[1], (int)EnvSwitches::get().publish_fenced);
        const bool gate_off = h->cfg.stream_gate == 0;      // gmg_config::stream_gate
        // The gate is only used once this handle has SEEN a published right-hand side arrive while its stream was still busy: wait_flag's
        // safety net (an idle stream implies visible data) cannot fire behind a gate the host itself has to open, so on a host that does
        // not see in-flight device writes a gated first contact would spin for ever.  The first coarse solve of a handle is ungated.
        if (h->gate_ok && h->gate_proven && !gate_off) {
            // (shared lock first: from here to coarse_host_serve no thread of this process starts a device-wide synchronisation, see gate_mutex)
            if (!h->gate_shared) { gate_mutex().lock_shared(); h->gate_shared = true; ++tl_gates_held; }
            if (hipStreamWaitValue64(h->stream, h->h_flag + 16, ++h->flag_seq[2], hipStreamWaitValueGte, ~0ull) == hipSuccess) {
                // (round 4: letting the prolongation out of the coarsest level gather the answer straight from the pinned host buffer instead of this
                // copy kernel -- one launch less behind the host -- measured 0.6608 vs 0.6582 ms per cycle: the gathers over PCIe cost what the copy costs)
                hipLaunchKernelGGL(gmgk::fetch_from_host, dim3((unsigned)std::min<size_t>(8, (cnt + gmgk::kBlock - 1) / gmgk::kBlock)), dim3(gmgk::kBlock), 0, h->stream,
                                   (const double*)e, c.x, (int)cnt);
                if (sizeof(T) == 4) launch_cvt(h, c.x, c.x32, cnt);
                h->coarse_pending = true; h->coarse_pending_d = d;
                return GMG_OK;
            }
            (void)hipGetLastError();
            if (h->gate_shared) { h->gate_shared = false; --tl_gates_held; gate_mutex().unlock_shared(); }
            h->gate_ok = false; --h->flag_seq[2]; h->timing["gate_disabled"] = 1.0;
        }
        int w = wait_flag(h, 1);
        if (w) return w;
        if (h->poll) h->gate_proven = true;        // the flag showed up by itself (wait_flag clears h->poll otherwise)
        if (!polled(h)) HIPCHK(hipStreamSynchronize(h->stream));
    } else {
        HIPCHK(hipMemcpyAsync(rc, c.b, sizeof(double) * cnt, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    coarse_host_solve(h, d);
    HIPCHK(hipMemcpyAsync(c.x, e, sizeof(double) * cnt, hipMemcpyHostToDevice, h->stream));
    if (sizeof(T) == 4) launch_cvt(h, c.x, c.x32, cnt);
    return GMG_OK;
}

// both halves back to back (callers that have nothing to enqueue in between)
template <class T = double>
int coarse_host_roundtrip(gmg_handle h, int d) {
    int rc = coarse_host_begin<T>(h, d);
    return rc ? rc : coarse_host_serve(h);
}

// Mixed precision: fp64 residual of the current iterate -> fp32 right-hand side of the inner cycle, plus the norm sums
// of that same residual (h_norm after the copy + sync).  type < 0: weights of type 0.
int launch_residual_to_f32(gmg_handle h, int d, int type) {
    Level& l = h->lv[0];
    const double* w = type == 1 ? h->d_minv : (type == 2 ? h->d_mass : nullptr);
    const int nblk = norm_grid(l.Aoff.n_slices);
    for_col_chunks(d, [&](int c0, int dc) {
        DISPATCH_D(dc, DISPATCH_C16(l.Aoff.c16_sel(), hipLaunchKernelGGL((gmgk::residual_norm_slices<D, 1, C16>), dim3(nblk), dim3(gmgk::kNormWaves * 64), 0, h->stream,
                                          l.Aoff.slice_ptr, l.Aoff.col, l.Aoff.val, l.diag, l.b + (size_t)c0 * l.n_pad, l.x + (size_t)c0 * l.n_pad, w, l.n_pad,
                                          l.Aoff.n_slices, l.b32 + (size_t)c0 * l.n_pad, h->d_partials, l.Aoff.col16, l.Aoff.win_base, l.Aoff.c16_arg())));
        launch_reduce(h, nblk, dc, c0, c0 + 4 >= d);
    });
    if (!polled(h)) HIPCHK(hipMemcpyAsync(h->h_norm, h->d_norm, sizeof(double) * 2 * d, hipMemcpyDeviceToHost, h->stream));
    return GMG_OK;
}

enum { G_DOWN = 1, G_UP = 2, G_FULL = 3 };

template <class F>
int run_graph(gmg_handle h, int key, F&& enqueue) {
    if (!h->cfg.use_graph) { enqueue(); return GMG_OK; }
    auto it = h->graphs.find(key);
    if (it == h->graphs.end()) {
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        auto tc = clk::now();
        HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        enqueue();
        HIPCHK(hipStreamEndCapture(h->stream, &g));
        h->timing["graph_capture_ms"] += ms_since(tc);
        // what this leg enqueues, counted: kernels, memsets and copies of the graph captured last (scripts/pointwise_ab.py reads a cycle's launch count here)
        { size_t nodes = 0; if (hipGraphGetNodes(g, nullptr, &nodes) == hipSuccess) h->timing["graph_nodes"] = (double)nodes; else (void)hipGetLastError(); }
        tc = clk::now();
        HIPCHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        h->timing["graph_instantiate_ms"] += ms_since(tc);
        (void)hipGraphDestroy(g);
        it = h->graphs.emplace(key, ge).first;
    }
    HIPCHK(hipGraphLaunch(it->second, h->stream));
    return GMG_OK;
}

// One V-cycle on the resident problem; norm_type >= 0 also enqueues the residual check of that type
// (result in h_norm after the stream is synchronised by the caller).
// What the loop around the cycle knows -- head_done: this cycle's first colour launch is already in the stream (enqueue_head: never under a
// graph); decide: the check's reduction also takes the loop's decision (CycleWatch; not the mixed-precision check: no head is eligible there).
// zero_guess: the caller's x of level 0 is the zero vector by construction and holds anything (the preconditioner application of the CG loop); the
// fp32 inner cycle always starts so.  Where the smoother can start without a materialised zero (level0_zero_guess) nothing zeroes or reads it.
// precond (T = float; the CG loop of gmg_config::precond_precision = 1): head, down, coarse and up only -- the caller has put the right-hand side
// into level 0's b32 and zeros into x32 (unless level0_zero_guess), takes the result from x32 and wants neither the correction added to the fp64
// iterate nor a new defect: level 0's fp64 x and b are not touched.  Such graphs need a key_salt of their own.
inline bool level0_zero_guess(gmg_handle h) { return pointwise_smoother(h->cfg) && h->L >= 1 && smooth_from_zero_ok(h, h->lv[0], h->cfg.pre_iters); }
template <class T>
int vcycle_legs(gmg_handle h, int d, int norm_type, int key_salt, int head_done, const CycleWatch* decide, bool zero_guess = false, bool precond = false) {
    int rc;
    const int nt = norm_type < 0 ? 9 : norm_type;
    constexpr bool mixed = sizeof(T) == 4;
    // the residual check's sums over the rows of the last colour come out of the last colour launch of the post-smoothing (fold_type >= 0)
    const bool foldable = !mixed && norm_type >= 0 && h->cfg.post_iters > 0 && h->cfg.smoother == GMG_SMOOTHER_MULTICOLOR_GS && !h->lv[0].ord.blocked;
    const int fold_type = foldable ? norm_type : -1;
    // mixed precision: the fp32 cycle starts from a zero guess on the defect b32 = b - A x (already in place), its
    // result is added to the fp64 iterate, and the new defect + its norms are formed in one fp64 pass
    const bool x0_zero = (mixed || zero_guess) && level0_zero_guess(h);
    auto head = [&] { if (mixed && !precond && !x0_zero) (void)hipMemsetAsync(h->lv[0].x32, 0, sizeof(float) * (size_t)h->lv[0].n_pad * d, h->stream); };
    // (folded: what the way up returned -- both in one enqueue body, which under a graph runs at capture only)
    auto tail = [&](int& err, int folded) {
        if (mixed && precond) {
        } else if (mixed) {
            const size_t cnt = (size_t)h->lv[0].n_pad * d;
            hipLaunchKernelGGL(gmgk::add_correction, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, h->lv[0].x32, h->lv[0].x, (int64_t)cnt);
            err = launch_residual_to_f32(h, d, norm_type);
        } else if (norm_type >= 0) err = launch_norm(h, d, norm_type, folded, decide);
        prof_mark(h);
    };
    if (h->coarse_device) {
        int err = GMG_OK;
        rc = run_graph(h, key_salt + G_FULL * 10000 + d * 10 + nt, [&] {
            head();
            enqueue_down<T>(h, d, /*k0*/ 0, /*first_done*/ false, head_done, x0_zero);
            enqueue_coarse_device<T>(h, d);
            tail(err, enqueue_up<T>(h, d, 0, fold_type));
        });
        return rc ? rc : err;
    }
    if ((rc = run_graph(h, key_salt + G_DOWN * 10000 + d * 10, [&] { head(); enqueue_down<T>(h, d, /*k0*/ 0, /*first_done*/ false, head_done, x0_zero); }))) return rc;
    if ((rc = coarse_host_begin<T>(h, d))) return rc;              // (polled: the way up is enqueued behind a gate the host opens in _serve)
    int err = GMG_OK;
    rc = run_graph(h, key_salt + G_UP * 10000 + d * 10 + nt, [&] { tail(err, enqueue_up<T>(h, d, 0, fold_type)); });
    const int served = coarse_host_serve(h);
    return rc ? rc : (served ? served : err);
}

int vcycle_resident(gmg_handle h, int d, int norm_type, int head_done = 0, const CycleWatch* decide = nullptr) {
    if (h->cfg.inner_precision) return vcycle_legs<float>(h, d, norm_type, 100000, head_done, decide);
    return vcycle_legs<double>(h, d, norm_type, 0, head_done, decide);
}

// ---- accelerated solve loop (gmg_config::accelerate; engine.hip::solve_common; kernels: accel_kernels.hip.hpp) ----------------------

// its vectors and scalars, for the level vectors as they are now (n_pad x dcap)
int ensure_accel(gmg_handle h) {
    auto& a = h->accel;
    const int m = h->cfg.accelerate, n_pad = h->lv[0].n_pad, D = h->dcap;
    if (a.xk && a.depth == m && a.d == D && a.n_pad == n_pad) return GMG_OK;
    a = {};
    const size_t count = (size_t)n_pad * D;
    auto vec = [&](DevBuf<double>* p) -> int {
        int rc = dev_alloc(h, *p, count);
        if (rc == GMG_OK) HIPCHK(hipMemsetAsync(*p, 0, sizeof(double) * count, h->stream));          // (padding rows: zero, and no kernel writes anything else there)
        return rc;
    };
    int rc;
    for (DevBuf<double>* p : {&a.xk, &a.r, &a.z0}) if ((rc = vec(p))) return rc;
    for (int j = 0; j < m - 1; ++j) for (DevBuf<double>* p : {&a.zs[j], &a.qs[j]}) if ((rc = vec(p))) return rc;
    if ((rc = dev_alloc(h, a.scal, (size_t)9 * D + 1)) ||          // alpha, guarded, 3 betas, 3 s_j per column; guard_steps; <b, b> per column
        (rc = dev_alloc(h, a.partials, (size_t)gmgk::kAccelMaxBlocks * gmgk::kAccelMaxComp))) return rc;
    a.depth = m; a.d = D; a.n_pad = n_pad;
    return GMG_OK;
}

// One recombination: lv[0].x holds the cycle's iterate x~, lv[0].r its residual b - A x~; `done` directions were formed in this solve before this
// one.  Leaves the new iterate in lv[0].x (and accel.xk), the recurrence residual in accel.r and the check's sums on their way to h_norm (wait_norm).
int launch_accel_step(gmg_handle h, int d, int type, int done) {
    auto& a = h->accel;
    Level& l = h->lv[0];
    const int DA = a.d, ld = l.n_pad, n_pairs = l.n_pad / 2, stored = a.depth - 1;
    const int ns = std::min(done, stored);                       // stored directions to orthogonalise against
    const int wslot = stored > 0 ? done % stored : -1;           // ring slot the new direction replaces (the oldest, or a free one)
    const int nblk = std::max(1, std::min(gmgk::kAccelMaxBlocks, (n_pairs + gmgk::kAccelBlock - 1) / gmgk::kAccelBlock));
    const double* w = type == 1 ? h->d_minv : (type == 2 ? h->d_mass : nullptr);
    double *alpha = a.scal, *guarded = a.scal + DA, *beta = a.scal + 2 * DA, *s_slot = a.scal + 5 * DA, *guard_steps = a.scal + 8 * DA,
           *bb = a.scal + 8 * DA + 1;
    for_col_chunks(d, [&](int c0, int dc) {
        const size_t off = (size_t)c0 * ld;
        gmgk::AccelRing ring{};
        for (int j = 0; j < ns; ++j) { ring.z[j] = a.zs[j] + off; ring.q[j] = a.qs[j] + off; }
        double* q0 = l.r + off;
        double* zw = wslot >= 0 ? a.zs[wslot] + off : nullptr;
        double* qw = wslot >= 0 ? a.qs[wslot] + off : nullptr;
        DISPATCH_D(dc, hipLaunchKernelGGL((gmgk::accel_form<D>), dim3(nblk), dim3(gmgk::kAccelBlock), 0, h->stream, l.x + off, a.xk + off, a.r + off, q0, a.z0 + off,
                                          ring, ns, w, ld, n_pairs, a.partials));
        if (ns > 0)
            hipLaunchKernelGGL(gmgk::accel_reduce_beta, dim3(1), dim3(gmgk::kReduceBlock), 0, h->stream, a.partials, nblk, ns, dc, s_slot + c0, DA, beta + c0);
        DISPATCH_D(dc, hipLaunchKernelGGL((gmgk::accel_orth<D>), dim3(nblk), dim3(gmgk::kAccelBlock), 0, h->stream, a.z0 + off, q0, a.r + off, ring, ns, zw, qw,
                                          beta + c0, DA, w, ld, n_pairs, a.partials));
        hipLaunchKernelGGL(gmgk::accel_reduce_alpha, dim3(1), dim3(gmgk::kReduceBlock), 0, h->stream, a.partials, nblk, dc, alpha + c0, guarded + c0,
                           wslot >= 0 ? s_slot + (size_t)wslot * DA + c0 : nullptr, guard_steps, bb + c0);
        DISPATCH_D(dc, hipLaunchKernelGGL((gmgk::accel_update<D>), dim3(nblk), dim3(gmgk::kAccelBlock), 0, h->stream, a.xk + off, l.x + off, a.r + off,
                                          zw ? zw : a.z0 + off, qw ? qw : q0, a.z0 + off, q0, alpha + c0, guarded + c0, l.b + off, w, ld, n_pairs, a.partials));
        // (the floor guard's <b, b>: kept from the first update's sums, zero until then)
        if (done == 0) hipLaunchKernelGGL(gmgk::accel_reduce_bb, dim3(1), dim3(gmgk::kReduceBlock), 0, h->stream, a.partials, nblk, dc, bb + c0);
        launch_reduce(h, nblk, dc, c0, c0 + 4 >= d, a.partials);
    });
    if (!polled(h)) HIPCHK(hipMemcpyAsync(h->h_norm, h->d_norm, sizeof(double) * 2 * d, hipMemcpyDeviceToHost, h->stream));
    return GMG_OK;
}

// ---- preconditioned CG solve loop (gmg_config::pcg; engine.hip::solve_common; kernels: pcg_kernels.hip.hpp) --------------------------

// Graphs of the cycle captured while the owners are exchanged hold the exchanged buffers: a key of their own (vcycle_legs' key_salt).  The two
// states hand lv[0].x / lv[0].b the same two pairs of buffers for as long as the level vectors live (every solve exchanges an even number of times).
constexpr int kPcgGraphSalt = 200000;
// ... and the fp32 cycle without head and tail (gmg_config::precond_precision = 1) is another graph than the inner cycle's (salt 100000)
constexpr int kPcgGraphSalt32 = 300000;

// its vectors and scalars, for the level vectors as they are now (n_pad x dcap).  gmg_config::precond_precision = 1 exchanges nothing: b (there: r)
// and p only
int ensure_pcg(gmg_handle h) {
    auto& a = h->pcg;
    const int n_pad = h->lv[0].n_pad, D = h->dcap;
    if (a.p && a.d == D && a.n_pad == n_pad) return GMG_OK;
    a = {};
    const size_t count = (size_t)n_pad * D;
    int rc;
    for (DevBuf<double>* p : {&a.x, &a.b, &a.p}) {
        if (p == &a.x && h->cfg.precond_precision) continue;
        if ((rc = dev_alloc(h, *p, count))) return rc;
        HIPCHK(hipMemsetAsync(*p, 0, sizeof(double) * count, h->stream));          // (padding rows: zero, and no kernel writes anything else there)
    }
    if ((rc = dev_alloc(h, a.scal, (size_t)4 * D + 2)) || (rc = dev_alloc(h, a.partials, (size_t)gmgk::kAccelMaxBlocks * 8))) return rc;
    a.d = D; a.n_pad = n_pad;
    return GMG_OK;
}

// lv[0].x <-> pcg.x, lv[0].b <-> pcg.b: who owns the CG iterate and the true right-hand side (gmg_solver_s::PcgState)
void pcg_exchange(gmg_handle h) {
    Level& l = h->lv[0];
    std::swap(l.x, h->pcg.x);
    std::swap(l.b, h->pcg.b);
    h->pcg.exchanged = !h->pcg.exchanged;
}

// One CG step behind the cycle.  first: the first iteration of the solve; fresh: r was recomputed from the iterate.  Who holds what:
//   fp64 cycle, owners exchanged: lv[0].b holds r, lv[0].x holds z = cycle(r, 0), pcg.x the iterate, pcg.b the true b;
//   gmg_config::precond_precision = 1, nothing exchanged: lv[0].x the iterate, lv[0].b the true b, pcg.b holds r, z is lv[0].x32 (float), and
//   pcg_update leaves fl32(r) in lv[0].b32, the next cycle's right-hand side.
// Leaves the new iterate and the recurrence residual there, zeros in z (z itself where the next cycle starts from zero without them:
// level0_zero_guess) and the check's sums on their way to h_norm (wait_norm).  The same launches in the same order for both.
template <class TZ>
int launch_pcg_step_on(gmg_handle h, int d, int type, bool first, bool fresh, double* x, double* r, TZ* z, const double* b, float* r32) {
    constexpr bool mixed = sizeof(TZ) == 4;
    auto& a = h->pcg;
    Level& l = h->lv[0];
    const int DA = a.d, ld = l.n_pad, n_pairs = l.n_pad / 2;
    const int nblk = std::max(1, std::min(gmgk::kAccelMaxBlocks, (n_pairs + gmgk::kAccelBlock - 1) / gmgk::kAccelBlock));
    const double* w = type == 1 ? h->d_minv : (type == 2 ? h->d_mass : nullptr);
    double *rho = a.scal, *beta = a.scal + DA, *alpha = a.scal + 2 * DA, *restart = a.scal + 3 * DA, *guard_steps = a.scal + 4 * DA, *restarts = a.scal + 4 * DA + 1;
    // the check's sums of the last update or confirmation, where the device reads them (launch_reduce)
    const double* sums = first ? nullptr : (polled(h) ? h->h_norm : h->d_norm.get());
    double* q = l.r;
    for_col_chunks(d, [&](int c0, int dc) {
        const size_t off = (size_t)c0 * ld;
        DISPATCH_D(dc, hipLaunchKernelGGL((gmgk::pcg_dot<D, TZ>), dim3(nblk), dim3(gmgk::kAccelBlock), 0, h->stream, r + off, z + off, ld, n_pairs, a.partials));
        hipLaunchKernelGGL(gmgk::pcg_reduce_beta, dim3(1), dim3(gmgk::kReduceBlock), 0, h->stream, a.partials, nblk, dc, rho + c0, beta + c0, restart + c0,
                           (int)first, (int)fresh, restarts);
        // (the next cycle's zero guess: written here unless that cycle starts from zero by itself)
        DISPATCH_D(dc, DISPATCH_FLAG(ZERO_Z, !level0_zero_guess(h), hipLaunchKernelGGL((gmgk::pcg_direction<D, ZERO_Z, TZ>), dim3(nblk), dim3(gmgk::kAccelBlock), 0, h->stream,
                                          z + off, a.p + off, beta + c0, ld, n_pairs)));
    });
    launch_spmv<double>(h, l, d, 0, nullptr, a.p.get(), q);
    for_col_chunks(d, [&](int c0, int dc) {
        const size_t off = (size_t)c0 * ld;
        DISPATCH_D(dc, hipLaunchKernelGGL((gmgk::pcg_dot<D>), dim3(nblk), dim3(gmgk::kAccelBlock), 0, h->stream, a.p + off, q + off, ld, n_pairs, a.partials));
        hipLaunchKernelGGL(gmgk::pcg_reduce_alpha, dim3(1), dim3(gmgk::kReduceBlock), 0, h->stream, a.partials, nblk, dc, rho + c0, alpha + c0, restart + c0,
                           sums ? sums + 2 * c0 : nullptr, guard_steps);
        DISPATCH_D(dc, hipLaunchKernelGGL((gmgk::pcg_update<D, mixed>), dim3(nblk), dim3(gmgk::kAccelBlock), 0, h->stream, x + off, r + off, a.p + off, q + off, alpha + c0,
                                          b + off, w, ld, n_pairs, a.partials, mixed ? r32 + off : nullptr));
        launch_reduce(h, nblk, dc, c0, c0 + 4 >= d, a.partials);
    });
    if (!polled(h)) HIPCHK(hipMemcpyAsync(h->h_norm, h->d_norm, sizeof(double) * 2 * d, hipMemcpyDeviceToHost, h->stream));
    return GMG_OK;
}

int launch_pcg_step(gmg_handle h, int d, int type, bool first, bool fresh) {
    auto& a = h->pcg;
    Level& l = h->lv[0];
    if (h->cfg.precond_precision) return launch_pcg_step_on<float>(h, d, type, first, fresh, l.x, a.b, l.x32.get(), l.b, l.b32);
    return launch_pcg_step_on<double>(h, d, type, first, fresh, a.x, l.b, l.x.get(), a.b, nullptr);
}

// ---- the projections of a solve on a semi-definite system (gmg_config::nullspace; engine.hip::solve_common; kernels: nullspace_kernels.hip.hpp) ----

int ensure_nullspace(gmg_handle h) {
    auto& a = h->nullsp;
    const int D = h->dcap;
    if (a.scal && a.d == D) return GMG_OK;
    a = {};
    int rc;
    if ((rc = dev_alloc(h, a.partials, (size_t)gmgk::kAccelMaxBlocks * 9)) || (rc = dev_alloc(h, a.scal, (size_t)6 * D))) return rc;
    a.d = D;
    return GMG_OK;
}

// v <- v - (w^T v / w^T 1) 1 on the real rows of a level-0 vector (n_pad x d), column by column; w == nullptr: unit weights.  slot 0: the
// right-hand side, 1: the iterate -- where nullspace_reduce leaves the shifts and the sums (NullspaceState::scal).
void launch_nullspace_project(gmg_handle h, int d, double* v, const double* w, int slot) {
    auto& a = h->nullsp;
    Level& l = h->lv[0];
    const int DA = a.d, ld = l.n_pad, n_pairs = l.n_pad / 2;
    const int nblk = std::max(1, std::min(gmgk::kAccelMaxBlocks, (n_pairs + gmgk::kAccelBlock - 1) / gmgk::kAccelBlock));
    double* out = a.scal + (size_t)slot * 3 * DA;
    const int* real = l.d_new2old;
    for_col_chunks(d, [&](int c0, int dc) {
        double* vc = v + (size_t)c0 * ld;
        DISPATCH_D(dc, hipLaunchKernelGGL((gmgk::nullspace_sums<D>), dim3(nblk), dim3(gmgk::kAccelBlock), 0, h->stream, (const double*)vc, w, real, ld, n_pairs, a.partials.get()));
        hipLaunchKernelGGL(gmgk::nullspace_reduce, dim3(1), dim3(gmgk::kReduceBlock), 0, h->stream, (const double*)a.partials, nblk, dc, DA, out + c0);
        DISPATCH_D(dc, hipLaunchKernelGGL((gmgk::nullspace_shift<D>), dim3(nblk), dim3(gmgk::kAccelBlock), 0, h->stream, vc, (const double*)(out + c0), real, ld, n_pairs));
    });
}

// ---- the solve loop (gmg_solve, gmg_solve_x0_rhs, gmg_solve_device, gmg_p2p_solve) -----------------------------------------------------
// do { one cycle; the stopping rule of solve_rule.hpp } while (it goes on).  What a cycle is, is the caller's: step(rule, residue, device_go)
// advances one cycle from the state `rule` and reports its residue -- and, where the check's reduction took the decision on the device
// (gmgk::reduce_partials, the same functions on the same sums), that word in device_go (0 / 1): the loop follows it, one decision, not two.
// conv (optional): (ms since t0, residue) pairs.  Sets the timing keys cycles, diverged, blown_up, iterations and residue and the two
// outputs; returns GMG_OK, GMG_DIVERGED or what a step failed with (< 0).
template <class Step>
int solve_loop(gmg_handle h, double tol, int max_iter, clk::time_point t0, double* conv, bool verbose, int* iters_out, double* residue_out, Step&& step) {
    SolveRule rule = rule_begin(tol, max_iter);
    bool go_on;
    do {
        double residue = 0.0; int device_go = -1;          // (-1: the host decides)
        if (const int rc = step(rule, residue, device_go)) return rc;
        rule = rule_after(rule, residue);
        if (conv) { conv[2 * rule.cycles - 2] = ms_since(t0); conv[2 * rule.cycles - 1] = residue; }
        if (verbose) std::printf("%d,%f,%.14f \n", rule.cycles, ms_since(t0), residue);
        go_on = rule_goes_on(rule);
        if (device_go >= 0) {
            if ((device_go != 0) != go_on) h->timing["head_decision_differs"] += 1.0;      // (never seen: the two sides compute the same bits)
            go_on = device_go != 0;
        }
    } while (go_on);
    h->timing["cycles"] = ms_since(t0);
    // Not contracting.  The parallel smoothers are not the reference's lexicographic Gauss-Seidel (block sweeps on the Galerkin levels take the
    // couplings between blocks from the previous sweep; nothing guarantees their convergence for every SPD matrix), so the caller is told --
    // return value GMG_DIVERGED and timing key "diverged" -- and can retry on a handle with block_rows = 0, gs_omega = 1: Gauss-Seidel in
    // colour order on every level, convergent for every SPD matrix (MultigridSolver::solve does).  x receives the last iterate either way, as
    // in the reference (multigrid_solver.cpp:1408-1419 never looks at the trend).
    const bool diverged = rule_diverged(rule);
    h->timing["diverged"] = diverged ? 1.0 : 0.0; h->timing["blown_up"] = rule.blown ? 1.0 : 0.0;           // (blown_up: stopped early)
    h->timing["iterations"] = rule.cycles; h->timing["residue"] = rule.residue;
    if (iters_out) *iters_out = rule.cycles;
    if (residue_out) *residue_out = rule.residue;
    return diverged ? GMG_DIVERGED : GMG_OK;
}

int check_level(gmg_handle h, int k, bool allow_coarsest) {
    if (h->live != LiveSystem::system) return fail(h, GMG_ERR_STATE, "no system set (call gmg_set_system first)");
    if (k < 0 || k > h->L || (!allow_coarsest && k == h->L)) return fail(h, GMG_ERR_INVALID, "level index out of range");
    return GMG_OK;
}

// entry points that read whole level operators: not on a handle that holds one rank's rows of a partitioned system
int check_whole_system(gmg_handle h) {
    if (h->partitioned) return fail(h, GMG_ERR_STATE, "this handle holds one rank's rows of a partitioned system (gmg_dist_partition): only the gmg_p2p_* / gmg_dist_* entry points run on it");
    return GMG_OK;
}

int check_norm_type(gmg_handle h, int type) {
    if (type < 0 || type > 3) return fail(h, GMG_ERR_INVALID, "residual norm type must be 0..3");
    if ((type == 1 || type == 2) && !h->d_mass) return fail(h, GMG_ERR_STATE, "mass matrix not set (gmg_set_mass) but an M-weighted norm was requested");
    return GMG_OK;
}

}  // namespace
