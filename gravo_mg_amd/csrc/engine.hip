// engine.hip -- libgravomg_hip.so: the C-ABI of include/gravomg_hip.h over the device engine.
//
// One handle = one HIP device, one stream.  The hierarchy (all A_k as SELL-64 + diagonal, all U_k / U_k^T) is built on
// the device once per system (gmg_set_system); a V-cycle is a fixed launch sequence on that stream (smooth -> residual
// -> restrict ... coarse solve ... prolong-add -> smooth), optionally captured into hipGraphs.  The coarsest operator is
// factored on the host (supernodal LDL^T, host_ldlt.hpp); per cycle it is applied as a dense inverse on the device (built on
// the device from that factor; gmg_config::coarse_mode = GMG_COARSE_AUTO, the default) or back-substituted on the host.
//
// One translation unit: engine_state.hip.hpp (memory pool, level / handle structures, helpers), engine_setup.hip.hpp
// (device-side layout construction, Galerkin products), engine_cycle.hip.hpp (launch helpers, V-cycle legs, the solve loop),
// engine_dist.hip.hpp / engine_part.hip.hpp (multi-GPU cycle, partition plan), engine_system.hip.hpp (the set-up stages
// of gmg_set_system) and this file (the extern "C" entry points).
//
// Reference call sites this replaces: gravomg/src/multigrid_solver.cpp:1059-1088 (V-cycle),
// :1194-1226 (smoother), :1228-1277 (norms), :1387-1419 (solve loop).
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <functional>
#include <future>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#if !defined(__HIP_DEVICE_COMPILE__)
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>
#endif

#include "../../include/gravomg_hip.h"
#include "../../include/gravomg_hip_internal.h"
#include "host_hierarchy.hpp"
#include "host_ldlt.hpp"
#include "host_plan.hpp"
#include "host_sparse.hpp"
#include "device_io_check.hpp"
#include "cheby_coeffs.hpp"
#include "kernels.hip.hpp"
#include "setup_kernels.hip.hpp"
#include "hierarchy_kernels.hip.hpp"
#include "accel_kernels.hip.hpp"
#include "pcg_kernels.hip.hpp"
#include "nullspace_kernels.hip.hpp"

using namespace gmg;
using clk = std::chrono::steady_clock;
static inline double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

#if !defined(__HIP_DEVICE_COMPILE__)
// Debugging aid: GMG_SEGV_BACKTRACE=1 makes a fatal signal inside the process print the native call stack of the faulting thread
// (symbol + offset; `addr2line -e libgravomg_hip.so` resolves them) before the default action takes over.
namespace {
struct sigaction gmg_prev_action[32];
void gmg_fatal_signal(int sig) {
    void* frames[48];
    const int nf = backtrace(frames, 48);          // (libgcc's unwinder was loaded at install time: no first-use allocation in here)
    const char msg[] = "[gmg] fatal signal, native stack of the faulting thread:\n";
    (void)!write(2, msg, sizeof(msg) - 1);
    backtrace_symbols_fd(frames, nf, 2);
    // hand over to whoever was installed before us (the host application's handler, or the default action)
    if (sig > 0 && sig < 32) sigaction(sig, &gmg_prev_action[sig], nullptr); else signal(sig, SIG_DFL);
    raise(sig);
}
struct GmgSignalAid {
    GmgSignalAid() {
        if (!EnvSwitches::get().segv_backtrace) return;
        void* warm[4];
        (void)backtrace(warm, 4);                  // first use loads libgcc_s (dlopen + malloc): not something to do inside a signal handler
        struct sigaction sa;
        std::memset(&sa, 0, sizeof(sa));
        sa.sa_handler = gmg_fatal_signal;
        for (int sig : {SIGSEGV, SIGBUS, SIGABRT, SIGFPE}) sigaction(sig, &sa, &gmg_prev_action[sig]);
    }
} gmg_signal_aid;
}  // namespace
#endif

#include "engine_state.hip.hpp"
#include "engine_setup.hip.hpp"
#include "engine_cycle.hip.hpp"
#include "engine_part.hip.hpp"
#include "engine_system.hip.hpp"

// =========================================================================================================
// No exception leaves the C-ABI: std::bad_alloc (a 3 M-vertex set-up allocates hundreds of MB on the host), a failed
// thread start, ... become a status code + gmg_last_error.
// (a cycle that was unwound between the two halves of its coarsest solve leaves a gate in its stream and the process-wide shared lock that
// goes with it: the handler opens both -- gate_unwound)
int gate_unwound(gmg_handle h);
#define GMG_CATCH_H                                                                                             \
    catch (const std::exception& e_) { if (h) (void)gate_unwound(h); return h ? fail(h, GMG_ERR_STATE, std::string("exception: ") + e_.what()) : GMG_ERR_STATE; } \
    catch (...) { if (h) (void)gate_unwound(h); return h ? fail(h, GMG_ERR_STATE, "unknown exception") : GMG_ERR_STATE; }
#define GMG_CATCH_0                                              \
    catch (...) { return GMG_ERR_STATE; }

void p2p_release_handle(gmg_handle h);      // engine_dist.hip.hpp


extern "C" {

int gmg_config_size(void) { return (int)sizeof(gmg_config); }

int gmg_config_default(gmg_config* cfg) try {
    if (!cfg) return GMG_ERR_INVALID;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->device = 0;
    cfg->smoother = GMG_SMOOTHER_MULTICOLOR_GS;
    cfg->jacobi_omega = 0.67;
    cfg->pre_iters = 2;       // gravomg_bindings/src/gravomg/core.py:10
    cfg->post_iters = 2;
    cfg->coarse_mode = GMG_COARSE_AUTO;
    cfg->use_graph = 0;      // measured: the cycle is not launch-bound (eager == graph per cycle) and instantiating costs ~5 ms per system
    cfg->sigma = 0;          // measured: no length sorting inside colour classes beats every window size (irregular meshes; profiles/README.md)
    cfg->row_align = 64;
    cfg->block_rows = 64;
    cfg->block_from_level = 1;
    cfg->block_lanes = 0;
    cfg->device_setup = 1;
    cfg->device_rap = 1;
    cfg->reorder_fine = 2;
    cfg->inner_precision = 0;
    cfg->block_csr = 1;
    cfg->host_threads = 0;
    cfg->verbose = 0;
    cfg->block_ep = 1;
    cfg->dist_shard_levels = 2;
    cfg->fine_col16 = 1;
    cfg->stream_gate = 1;
    cfg->prepare_structure = 1;
    cfg->fuse_restrict_sweep = 1;
    cfg->speculate_head = 1;
    cfg->precond_precision = 0; // a pcg = 1 handle applies its cycle in fp64 (1: the fp32 cycle on the fp32 twins, see gmg_config)
    cfg->nullspace = 0;       // symmetric positive definite systems (1: semi-definite with the null space span{1}, see gmg_config)
    cfg->fold_head = 1;
    cfg->uniform_slices = 1;
    cfg->color_ahead = 1;
    cfg->reorder_pointwise = 0; // a pointwise smoother keeps the caller's numbering of level 0 (1: reorder_fine applies to it too, see gmg_config)
    cfg->zero_guess_step = 0; // a pointwise smoother reads a materialised zero guess (1: its first step is c * b / diag, see gmg_config)
    cfg->pcg = 0;             // the plain solve loop (1: conjugate gradients preconditioned by a symmetric cycle, solve_common)
    cfg->device_coloring = 0; // level 0 is coloured by the host's greedy loop (1: Jones-Plassmann rounds on the device, another colouring: see gmg_config)
    cfg->dist_exchange = 0;
    cfg->block_fine = 1;      // level 0 blocked too where it pays and is safe (long rows, Stieltjes matrix): see gmg_config
    cfg->restrict_sigma = 64;
    cfg->gs_omega = 1.35;     // measured (profiles/r02/a_iteration_ab.json, f_iteration_ab_omega_scan.json): 7 -> 4 V-cycles to 1e-4 on the 3 M Poisson
                              // problem at the same cost per cycle; centre of the 1.3 - 1.4 plateau on six workloads
    cfg->accelerate = 0;      // the plain solve loop (1..4: truncated GCR around the cycle, solve_common)
    return GMG_OK;
} GMG_CATCH_0

int gmg_host_threads(void) try { return hw_threads(); } GMG_CATCH_0

int gmg_device_count(void) try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
} GMG_CATCH_0

// Why this thread's last gmg_create refused a configuration, where it says so: there is no handle to ask, gmg_last_error(NULL) returns it
static std::string& create_error() { static thread_local std::string s; return s; }
static int create_refused(int code, const char* why) { create_error() = why; return code; }

int gmg_create(const gmg_config* cfg, gmg_handle* out) try {
    if (!out) return GMG_ERR_INVALID;
    create_error().clear();
    gmg_config c;
    if (cfg) c = *cfg; else gmg_config_default(&c);
    if (c.nullspace < 0 || c.nullspace > 1) return create_refused(GMG_ERR_INVALID, "gmg_config::nullspace must be 0 or 1");
    if (c.sigma < 0 || c.sigma % 64 || c.restrict_sigma < 0 || c.restrict_sigma % 64 || c.row_align <= 0 || c.row_align % 64 || c.pre_iters < 0 || c.post_iters < 0 ||
        c.reorder_fine < 0 || c.reorder_fine > 2 || c.inner_precision < 0 || c.inner_precision > 1 || c.block_rows < 0 || c.block_rows > gmgk::kBlockRows || c.block_rows % 64 || c.block_from_level < 0 || !(c.gs_omega > 0.0 && c.gs_omega < 2.0) || c.dist_shard_levels < 1 || c.dist_shard_levels > 2 || c.block_fine < 0 || c.block_fine > 1 || c.dist_exchange < 0 || c.dist_exchange > 2 ||
        (c.block_lanes != 0 && c.block_lanes != 1 && c.block_lanes != 4) || (c.block_lanes != 1 && c.block_rows > gmgk::kQuadBlockRows)) return GMG_ERR_INVALID;
    if (c.accelerate < 0 || c.accelerate > gmg::kAccelMaxDepth) return GMG_ERR_INVALID;
    if (c.device_coloring < 0 || c.device_coloring > 1) return GMG_ERR_INVALID;
    if (c.smoother < GMG_SMOOTHER_MULTICOLOR_GS || c.smoother > GMG_SMOOTHER_CHEBYSHEV) return GMG_ERR_INVALID;
    if (c.accelerate > 0 && c.inner_precision) return GMG_ERR_UNSUPPORTED;      // the recombination is fp64 only (gmg_config::accelerate)
    if (c.reorder_pointwise < 0 || c.reorder_pointwise > 1) return create_refused(GMG_ERR_INVALID, "gmg_config::reorder_pointwise must be 0 or 1");
    if (c.zero_guess_step < 0 || c.zero_guess_step > 1) return create_refused(GMG_ERR_INVALID, "gmg_config::zero_guess_step must be 0 or 1");
    if (c.pcg < 0 || c.pcg > 1) return create_refused(GMG_ERR_INVALID, "gmg_config::pcg must be 0 or 1");
    if (c.pcg) {        // conjugate gradients need a symmetric positive definite preconditioner: a pointwise smoother, as many steps down as up (gmg_config::pcg)
        if (c.smoother != GMG_SMOOTHER_CHEBYSHEV && c.smoother != GMG_SMOOTHER_JACOBI)
            return create_refused(GMG_ERR_UNSUPPORTED, "gmg_config::pcg needs a pointwise smoother (GMG_SMOOTHER_CHEBYSHEV or GMG_SMOOTHER_JACOBI): a Gauss-Seidel cycle is not a symmetric operator");
        if (c.pre_iters != c.post_iters || c.pre_iters < 1) return create_refused(GMG_ERR_UNSUPPORTED, "gmg_config::pcg needs pre_iters == post_iters >= 1: the cycle must be a symmetric operator");
        if (c.accelerate != 0) return create_refused(GMG_ERR_UNSUPPORTED, "gmg_config::pcg and gmg_config::accelerate are two solve loops: set one of them");
        if (c.inner_precision != 0) return create_refused(GMG_ERR_UNSUPPORTED, "gmg_config::pcg is fp64 only (inner_precision = 0)");
    }
    if (c.precond_precision < 0 || c.precond_precision > 1) return create_refused(GMG_ERR_INVALID, "gmg_config::precond_precision must be 0 or 1");
    if (c.precond_precision && !c.pcg) return create_refused(GMG_ERR_UNSUPPORTED, "gmg_config::precond_precision = 1 needs gmg_config::pcg = 1: it is the precision of that loop's preconditioner cycle");
    gmg_handle h = new gmg_solver_s();
    h->cfg = c;
    h->coarse.pin_last = c.nullspace != 0;      // the coarsest factor takes its last pivot for what it is (host_ldlt.hpp)
    if (h->cfg.host_threads <= 0) h->cfg.host_threads = hw_threads();
    int ndev = gmg_device_count();
    if (ndev > 0 && c.device >= 0 && c.device < ndev && hipSetDevice(c.device) == hipSuccess &&
        hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess) {
        h->has_device = true;
        h->own_stream = h->stream;
        { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c.device) == hipSuccess && cus > 0) h->n_cus = cus; else (void)hipGetLastError(); }
        (void)hipEventCreate(&h->ev0);
        (void)hipEventCreate(&h->ev1);
        if (hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking) != hipSuccess) { h->aux_stream = nullptr; (void)hipGetLastError(); }
        if (hipEventCreateWithFlags(&h->aux_ev, hipEventDisableTiming) != hipSuccess) { h->aux_ev = nullptr; (void)hipGetLastError(); }
        if (hipMalloc((void**)&h->d_aux_err, sizeof(int)) != hipSuccess) { h->d_aux_err = nullptr; (void)hipGetLastError(); }
        h->poll = EnvSwitches::get().poll;
        (void)ensure_bounce(h);         // 2 x 16 MB pinned, once per handle (page-locking is not free: not inside gmg_set_system)
    }
    *out = h;
    return GMG_OK;     // host-only entry points work without a device; device ones report GMG_ERR_NO_DEVICE
} GMG_CATCH_0

void gmg_destroy(gmg_handle h) {
    if (!h) return;
    PoolScope pool_scope_(&h->pool);
    if (h->has_device) {
        (void)hipSetDevice(h->cfg.device);
        (void)hipStreamSynchronize(h->stream);
        p2p_release_handle(h);
        drop_system(h);
        drop_device_transfers(h);
        h->d_stage = {}; h->d_partials = {}; h->d_norm = {}; h->d_watch = {};       // (every pool block is parked before the pool is emptied and the handle deleted)
        if (h->h_pinned) (void)sync_hipHostFree(h->h_pinned);
        for (int i = 0; i < 2; ++i) { if (h->h_stage[i]) (void)sync_hipHostFree(h->h_stage[i]); if (h->h_stage_ev[i]) (void)hipEventDestroy(h->h_stage_ev[i]); }
        for (hipEvent_t& e : h->h_chunk_ev) if (e) (void)hipEventDestroy(e);
        if (h->h_norm) (void)sync_hipHostFree(h->h_norm);
        if (h->h_flag) (void)sync_hipHostFree(h->h_flag);
        if (h->ev0) (void)hipEventDestroy(h->ev0);
        if (h->ev1) (void)hipEventDestroy(h->ev1);
        if (h->aux_ev) (void)hipEventDestroy(h->aux_ev);
        if (h->aux_stream) { (void)hipStreamSynchronize(h->aux_stream); (void)sync_hipStreamDestroy(h->aux_stream); }
        if (h->d_aux_err) (void)sync_hipFree(h->d_aux_err);
        drop_rap_order(h);
        for (int i = 0; i < 2; ++i) { if (h->bounce[i]) (void)sync_hipHostFree(h->bounce[i]); if (h->bounce_ev[i]) (void)hipEventDestroy(h->bounce_ev[i]); }
        for (hipEvent_t e : h->prof_ev) (void)hipEventDestroy(e);
        (void)sync_hipStreamDestroy(h->own_stream);
        h->pool.trim();
    }
    delete h;
}

const char* gmg_last_error(gmg_handle h) { return h ? h->err.c_str() : (create_error().empty() ? "null handle" : create_error().c_str()); }

int gmg_set_num_levels(gmg_handle h, int L) try {
    if (!h || L < 0 || L > 64) return h ? fail(h, GMG_ERR_INVALID, "invalid level count") : GMG_ERR_INVALID;
    PoolScope pool_scope_(&h->pool);
    if (h->has_device) { drop_system(h); drop_device_transfers(h); }
    h->patches.clear(); h->patches_ready = false;
    h->bfs_order.clear();
    h->fine_graph.reset();
    drop_rap_order(h);
    h->L = L;
    h->ord_cache_valid = false;
    h->U.assign(L, Compressed());
    h->U_set.assign(L, 0);
    return GMG_OK;
} GMG_CATCH_H

int gmg_set_prolongation(gmg_handle h, int k, int n_fine, int n_coarse, const int* colptr, const int* rowidx, const double* val) try {
    if (!h) return GMG_ERR_INVALID;
    PoolScope pool_scope_(&h->pool);
    if (h->L < 0) return fail(h, GMG_ERR_STATE, "call gmg_set_num_levels first");
    if (k < 0 || k >= h->L || n_fine <= 0 || n_coarse <= 0 || !colptr || !rowidx || !val) return fail(h, GMG_ERR_INVALID, "bad prolongation arguments");
    for (int j = 0; j < n_coarse; ++j) if (colptr[j + 1] < colptr[j]) return fail(h, GMG_ERR_INVALID, "colptr not monotone");
    {
        std::atomic<bool> bad{false};
        parallel_ranges(colptr[n_coarse], h->cfg.host_threads, [&](int lo, int hi, int) {
            for (int p = lo; p < hi; ++p) if (rowidx[p] < 0 || rowidx[p] >= n_fine) { bad = true; return; }
        }, 1 << 18);
        if (bad) return fail(h, GMG_ERR_INVALID, "row index out of range in U");
    }
    if (h->has_device) { drop_system(h); drop_device_transfers(h); }
    h->patches.clear(); h->patches_ready = false;
    {   // (default-initialised vectors filled on all cores: 108 MB of first touches at 3 M vertices)
        Compressed& u = h->U[k];
        u.n_outer = n_coarse; u.n_inner = n_fine;
        u.ptr.assign(colptr, colptr + n_coarse + 1);
        u.idx.resize((size_t)colptr[n_coarse]); u.val.resize((size_t)colptr[n_coarse]);
        threaded_copy_bytes(u.idx.data(), rowidx, sizeof(int) * u.idx.size(), h->cfg.host_threads);
        threaded_copy_bytes(u.val.data(), val, sizeof(double) * u.val.size(), h->cfg.host_threads);
    }
    h->U_set[k] = 1;
    h->ord_cache_valid = false;
    if (k == 0) drop_rap_order(h);
    return GMG_OK;
} GMG_CATCH_H

int gmg_set_mass(gmg_handle h, int n, const double* mass_diag) try {
    if (!h || n <= 0 || !mass_diag) return h ? fail(h, GMG_ERR_INVALID, "bad mass arguments") : GMG_ERR_INVALID;
    PoolScope pool_scope_(&h->pool);
    // a live system (or the prepared structure of one) fixes n: a mass of another size could only leave the M-weighted norms on stale weights
    if (h->live != LiveSystem::none && !h->lv.empty() && h->lv[0].n != n)
        return fail(h, GMG_ERR_INVALID, "mass size does not match the system");
    h->mass.assign(mass_diag, mass_diag + n);
    // (with a system -- or the prepared structure of one: the ordering that permutes the mass exists -- it goes to the device now)
    if (h->has_device && h->live != LiveSystem::none && !h->lv.empty() && h->lv[0].n == n && h->lv[0].d_new2old) { h->mass_dirty = false; return upload_mass(h); }
    h->mass_dirty = true;
    return GMG_OK;
} GMG_CATCH_H

int gmg_set_system(gmg_handle h, int n, const int* colptr, const int* rowidx, const double* val) try {
    return set_system_impl(h, n, colptr, rowidx, val);
} GMG_CATCH_H

int gmg_num_levels(gmg_handle h) { return h ? h->L : GMG_ERR_INVALID; }

int gmg_level_info(gmg_handle h, int k, int* n, int64_t* nnz, int* n_colors, int* n_pad) try {
    if (!h) return GMG_ERR_INVALID;
    int rc = check_level(h, k, true);
    if (rc) return rc;
    Level& l = h->lv[k];
    if (n) *n = l.n;
    if (nnz) *nnz = l.nnz;
    if (n_colors) *n_colors = l.ord.n_colors;
    if (n_pad) *n_pad = l.n_pad;
    return GMG_OK;
} GMG_CATCH_H

int gmg_get_level_operator(gmg_handle h, int k, int* colptr, int* rowidx, double* val) try {
    if (!h) return GMG_ERR_INVALID;
    int rc = check_level(h, k, true);
    if (rc) return rc;
    if ((rc = check_whole_system(h))) return rc;
    {
        PoolScope pool_scope_(&h->pool);
        if ((rc = ensure_host_A(h, k, true))) return rc;
    }
    const Compressed& A = h->lv[k].A;
    if (colptr) std::memcpy(colptr, A.ptr.data(), sizeof(int) * (A.n_outer + 1));
    if (rowidx) std::memcpy(rowidx, A.idx.data(), sizeof(int) * A.nnz());
    if (val) std::memcpy(val, A.val.data(), sizeof(double) * A.nnz());
    return GMG_OK;
} GMG_CATCH_H

int gmg_get_level_ordering(gmg_handle h, int k, int* new2old, int* color_begin) try {
    if (!h) return GMG_ERR_INVALID;
    int rc = check_level(h, k, true);
    if (rc) return rc;
    const LevelOrdering& o = h->lv[k].ord;
    if (new2old) std::memcpy(new2old, o.new2old.data(), sizeof(int) * o.n_pad);
    if (color_begin) {      // colour-major levels: n_colors + 1 entries; blocked levels: {0, n_pad} (one range)
        for (int c = 0; c <= o.n_colors; ++c) color_begin[c] = c < (int)o.color_begin.size() ? o.color_begin[c] : o.n_pad;
    }
    return GMG_OK;
} GMG_CATCH_H

int gmg_get_level_blocks(gmg_handle h, int k, int* n_blocks, int* blk_begin, unsigned char* row_color) try {
    if (!h) return GMG_ERR_INVALID;
    int rc = check_level(h, k, true);
    if (rc) return rc;
    const LevelOrdering& o = h->lv[k].ord;
    if (n_blocks) *n_blocks = o.blocked ? o.n_blocks() : 0;
    if (o.blocked && blk_begin) std::memcpy(blk_begin, o.blk_begin.data(), sizeof(int) * o.blk_begin.size());
    if (o.blocked && row_color) std::memcpy(row_color, o.row_color.data(), o.row_color.size());
    return GMG_OK;
} GMG_CATCH_H

// Debug / test access to the device-resident layouts: which = 0 A (off-diagonal), 1 A_in, 2 A_out, 3 P (U), 4 R (U^T).
static DevSell* pick_sell(gmg_handle h, int k, int which) {
    Level& l = h->lv[k];
    switch (which) { case 0: return &l.Aoff; case 1: return &l.Ain; case 2: return &l.Aout; case 3: return &l.P; case 4: return &l.R; default: return nullptr; }
}

int gmg_debug_sell_info(gmg_handle h, int k, int which, int64_t* info) try {
    NEED_DEVICE();
    int rc = check_level(h, k, false);
    if (rc) return rc;
    if (which == 5) {      // block-CSR of a big blocked level: reported as n_pad "slices" of one row (lpr 64: one row_of entry per row)
        Level& l = h->lv[k];
        if (!info) return fail(h, GMG_ERR_INVALID, "bad arguments");
        info[0] = l.use_bcsr ? l.n_pad : 0; info[1] = 64; info[2] = l.use_bcsr ? l.bc_nnz : 0; info[3] = l.use_bcsr ? 1 : 0;
        return GMG_OK;
    }
    if (which == 6 || which == 7) {      // unpadded block sweep: 6 = "lower" part (local columns), 7 = "explicit" part (device columns)
        Level& l = h->lv[k];
        if (!info) return fail(h, GMG_ERR_INVALID, "bad arguments");
        info[0] = l.use_ep ? l.n_pad : 0; info[1] = 64; info[2] = l.use_ep ? (which == 6 ? l.ep_nnz : l.ee_nnz) : 0; info[3] = l.use_ep ? 1 : 0;
        return GMG_OK;
    }
    DevSell* s = pick_sell(h, k, which);
    if (!s || !info) return fail(h, GMG_ERR_INVALID, "bad arguments");
    info[0] = s->n_slices; info[1] = s->lpr; info[2] = s->stored; info[3] = s->row_of ? 1 : 0;
    return GMG_OK;
} GMG_CATCH_H

int gmg_debug_sell_copy(gmg_handle h, int k, int which, int64_t* slice_ptr, int* col, double* val, int* row_of, double* diag) try {
    NEED_DEVICE();
    int rc = check_level(h, k, false);
    if (rc) return rc;
    if ((rc = check_whole_system(h))) return rc;
    if (which == 5) {      // slice_ptr <- row_ptr (n_pad + 1), row_of <- row_mid (n_pad)
        Level& lb = h->lv[k];
        if (!lb.use_bcsr) return GMG_OK;
        HIPCHK(hipStreamSynchronize(h->stream));
        std::vector<int> tmp((size_t)lb.n_pad + 1);
        HIPCHK(hipMemcpy(tmp.data(), lb.bc_ptr, sizeof(int) * tmp.size(), hipMemcpyDeviceToHost));
        if (slice_ptr) for (size_t i = 0; i < tmp.size(); ++i) slice_ptr[i] = tmp[i];
        if (row_of) HIPCHK(hipMemcpy(row_of, lb.bc_mid, sizeof(int) * (size_t)lb.n_pad, hipMemcpyDeviceToHost));
        if (col) HIPCHK(hipMemcpy(col, lb.bc_col, sizeof(int) * (size_t)lb.bc_nnz, hipMemcpyDeviceToHost));
        if (val) HIPCHK(hipMemcpy(val, lb.bc_val, sizeof(double) * (size_t)lb.bc_nnz, hipMemcpyDeviceToHost));
        return GMG_OK;
    }
    if (which == 6 || which == 7) {      // slice_ptr <- row pointers (n_pad + 1), col <- columns, row_of[0] <- LDS capacity of that part
        Level& lb = h->lv[k];
        if (!lb.use_ep) return GMG_OK;
        HIPCHK(hipStreamSynchronize(h->stream));
        const int64_t nnz = which == 6 ? lb.ep_nnz : lb.ee_nnz;
        std::vector<int> tmp((size_t)lb.n_pad + 1);
        HIPCHK(hipMemcpy(tmp.data(), which == 6 ? lb.ep_ptr : lb.ee_ptr, sizeof(int) * tmp.size(), hipMemcpyDeviceToHost));
        if (slice_ptr) for (size_t i = 0; i < tmp.size(); ++i) slice_ptr[i] = tmp[i];
        if (row_of) { std::memset(row_of, 0, sizeof(int) * (size_t)lb.n_pad); row_of[0] = which == 6 ? lb.ep_cap_l : lb.ep_cap_e; }
        if (col && which == 6) {
            std::vector<unsigned short> c16((size_t)nnz);
            HIPCHK(hipMemcpy(c16.data(), lb.ep_col, sizeof(unsigned short) * c16.size(), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < c16.size(); ++i) col[i] = c16[i];
        } else if (col) HIPCHK(hipMemcpy(col, lb.ee_col, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToHost));
        if (val) HIPCHK(hipMemcpy(val, which == 6 ? lb.ep_val : lb.ee_val, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost));
        return GMG_OK;
    }
    DevSell* s = pick_sell(h, k, which);
    if (!s) return fail(h, GMG_ERR_INVALID, "bad arguments");
    Level& l = h->lv[k];
    HIPCHK(hipStreamSynchronize(h->stream));
    if (slice_ptr && s->slice_ptr) HIPCHK(hipMemcpy(slice_ptr, s->slice_ptr, sizeof(int64_t) * (s->n_slices + 1), hipMemcpyDeviceToHost));
    if (val && s->val) HIPCHK(hipMemcpy(val, s->val, sizeof(double) * s->stored, hipMemcpyDeviceToHost));
    if (col) {
        if (which == 1 && l.ain_col16) {
            std::vector<unsigned short> c16((size_t)s->stored);
            HIPCHK(hipMemcpy(c16.data(), l.ain_col16, sizeof(unsigned short) * s->stored, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < s->stored; ++i) col[i] = c16[i];
        } else if (s->col) HIPCHK(hipMemcpy(col, s->col, sizeof(int) * s->stored, hipMemcpyDeviceToHost));
    }
    if (row_of && s->row_of) HIPCHK(hipMemcpy(row_of, s->row_of, sizeof(int) * (size_t)s->n_slices * (64 / s->lpr), hipMemcpyDeviceToHost));
    if (diag && which == 0 && l.diag) HIPCHK(hipMemcpy(diag, l.diag, sizeof(double) * l.n_pad, hipMemcpyDeviceToHost));
    return GMG_OK;
} GMG_CATCH_H

// The 16-bit column codes of a level-0 layout as gmgs::compress_cols left them (gravomg_hip_internal.h): plain copies of arrays the handle owns.
int gmg_debug_col16_copy(gmg_handle h, int which, int64_t* info, unsigned* col16, int* win_base) try {
    NEED_DEVICE();
    int rc = check_level(h, 0, false);
    if (rc) return rc;
    if ((rc = check_whole_system(h))) return rc;
    DevSell* s = (which == 0 || which == 3 || which == 4) ? pick_sell(h, 0, which) : nullptr;
    if (!s || !info) return fail(h, GMG_ERR_INVALID, "bad arguments");
    const int nw = s->col16 ? (s->c16_dbits == 13 ? 8 : 32) : 0;
    info[0] = nw; info[1] = s->col16 ? s->c16_mode : 0; info[2] = s->c16_from; info[3] = s->uniform_w; info[4] = s->col16 ? s->stored : 0;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (col16 && s->col16) HIPCHK(hipMemcpy(col16, s->col16, sizeof(unsigned) * (size_t)s->stored, hipMemcpyDeviceToHost));
    if (win_base && s->win_base) HIPCHK(hipMemcpy(win_base, s->win_base, sizeof(int) * (size_t)s->n_slices * nw, hipMemcpyDeviceToHost));
    return GMG_OK;
} GMG_CATCH_H

int gmg_get_timing(gmg_handle h, const char* key, double* out) try {
    if (!h || !key || !out) return GMG_ERR_INVALID;
    if (std::string(key) == "device_bytes_now") { *out = (double)h->pool.live_bytes; return GMG_OK; }      // device memory the handle holds at this moment (pool blocks in use)
    if (std::string(key) == "device_blocks_now") { *out = (double)(h->pool.size_of.size() - h->pool.parked.size()); return GMG_OK; }      // ... and how many blocks that is
    if (std::string(key) == "zero_guess_steps") { *out = (double)h->zero_steps; return GMG_OK; }                   // zero-step launches enqueued so far (gmg_config::zero_guess_step)
    if (std::string(key) == "restrict_steps_fused") { *out = (double)h->fused_step_restrictions; return GMG_OK; }  // ... and restrictions that computed the step instead
    if (std::string(key) == "restrict_sweeps_fused") { *out = (double)h->fused_restrictions; return GMG_OK; }      // fused restriction + first pre-sweep launches enqueued so far (gmg_config::fuse_restrict_sweep)
    auto it = h->timing.find(key);
    if (it == h->timing.end()) return fail(h, GMG_ERR_INVALID, std::string("unknown timing key: ") + key);
    *out = it->second;
    return GMG_OK;
} GMG_CATCH_H

// ---- operators -------------------------------------------------------------------------------------------

int gmg_smooth(gmg_handle h, int k, const double* b, double* x, int d, int iters) try {
    NEED_DEVICE();
    int rc = check_level(h, k, false);
    if (rc) return rc;
    if ((rc = check_whole_system(h))) return rc;
    if (!b || !x || d <= 0 || iters < 0) return fail(h, GMG_ERR_INVALID, "bad arguments");
    if ((rc = ensure_vectors(h, d))) return rc;
    Level& l = h->lv[k];
    if ((rc = to_device(h, k, b, d, l.b))) return rc;
    if ((rc = to_device(h, k, x, d, l.x))) return rc;
    launch_smooth<double>(h, l, d, iters);
    h->loaded_d = 0;
    return to_host(h, k, l.x, d, x);
} GMG_CATCH_H

int gmg_smooth_residual(gmg_handle h, int k, const double* b, double* x, int d, int iters, int from_zero, double* r) try {
    NEED_DEVICE();
    int rc = check_level(h, k, false);
    if (rc) return rc;
    if ((rc = check_whole_system(h))) return rc;
    if (!b || !x || !r || d <= 0 || iters < 0) return fail(h, GMG_ERR_INVALID, "bad arguments");
    if ((rc = ensure_vectors(h, d))) return rc;
    Level& l = h->lv[k];
    if ((rc = to_device(h, k, b, d, l.b))) return rc;
    SmoothAsk<double> ask;                         // (a single level's sweeps: nothing ran ahead of them, nothing rides on them)
    // (a pointwise smoother's zero step serves level 0 as well: where the engine supplies the zero guess, the cycle uses it there)
    ask.from_zero = from_zero != 0 && (k > 0 || pointwise_smoother(h->cfg)) && smooth_from_zero_ok(h, l, iters);
    if (from_zero) HIPCHK(hipMemsetAsync(l.x, 0, sizeof(double) * (size_t)l.n_pad * d, h->stream));
    else if ((rc = to_device(h, k, x, d, l.x))) return rc;
    const SmoothDone<double> swept = launch_smooth<double>(h, l, d, iters, ask);
    const bool delta = k > 0 && launch_residual_delta<double>(h, l, d, l.r, swept);        // exactly what enqueue_down does
    if (!delta) launch_spmv<double>(h, l, d, 1, l.b, l.x, l.r);
    h->timing["residual_from_sweep"] = delta ? 1.0 : 0.0;
    h->loaded_d = 0;
    if ((rc = to_host(h, k, l.x, d, x))) return rc;
    return to_host(h, k, l.r, d, r);
} GMG_CATCH_H

int gmg_residual(gmg_handle h, int k, const double* b, const double* x, int d, double* r) try {
    NEED_DEVICE();
    int rc = check_level(h, k, false);
    if (rc) return rc;
    if ((rc = check_whole_system(h))) return rc;
    if (!b || !x || !r || d <= 0) return fail(h, GMG_ERR_INVALID, "bad arguments");
    if ((rc = ensure_vectors(h, d))) return rc;
    Level& l = h->lv[k];
    if ((rc = to_device(h, k, b, d, l.b))) return rc;
    if ((rc = to_device(h, k, x, d, l.x))) return rc;
    launch_spmv<double>(h, l, d, 1, l.b, l.x, l.r);
    h->loaded_d = 0;
    return to_host(h, k, l.r, d, r);
} GMG_CATCH_H

int gmg_spmv(gmg_handle h, int k, const double* x, int d, double* y) try {
    NEED_DEVICE();
    int rc = check_level(h, k, false);
    if (rc) return rc;
    if ((rc = check_whole_system(h))) return rc;
    if (!x || !y || d <= 0) return fail(h, GMG_ERR_INVALID, "bad arguments");
    if ((rc = ensure_vectors(h, d))) return rc;
    Level& l = h->lv[k];
    if ((rc = to_device(h, k, x, d, l.x))) return rc;
    launch_spmv<double>(h, l, d, 0, nullptr, l.x, l.r);
    h->loaded_d = 0;
    return to_host(h, k, l.r, d, y);
} GMG_CATCH_H

int gmg_restrict(gmg_handle h, int k, const double* r, int d, double* rc_out) try {
    NEED_DEVICE();
    int rc = check_level(h, k, false);
    if (rc) return rc;
    if ((rc = check_whole_system(h))) return rc;
    if (!r || !rc_out || d <= 0) return fail(h, GMG_ERR_INVALID, "bad arguments");
    if ((rc = ensure_vectors(h, d))) return rc;
    Level& l = h->lv[k];
    if ((rc = to_device(h, k, r, d, l.r))) return rc;
    launch_restrict<double>(h, l, h->lv[k + 1], d, l.r, h->lv[k + 1].b);
    h->loaded_d = 0;
    return to_host(h, k + 1, h->lv[k + 1].b, d, rc_out);
} GMG_CATCH_H

int gmg_prolong_add(gmg_handle h, int k, const double* e, int d, double* x) try {
    NEED_DEVICE();
    int rc = check_level(h, k, false);
    if (rc) return rc;
    if ((rc = check_whole_system(h))) return rc;
    if (!e || !x || d <= 0) return fail(h, GMG_ERR_INVALID, "bad arguments");
    if ((rc = ensure_vectors(h, d))) return rc;
    Level& l = h->lv[k];
    if ((rc = to_device(h, k + 1, e, d, h->lv[k + 1].x))) return rc;
    if ((rc = to_device(h, k, x, d, l.x))) return rc;
    launch_prolong_add<double>(h, l, h->lv[k + 1], d, h->lv[k + 1].x, l.x);
    h->loaded_d = 0;
    return to_host(h, k, l.x, d, x);
} GMG_CATCH_H

int gmg_coarse_solve(gmg_handle h, const double* rc_in, int d, double* e) try {
    NEED_DEVICE();
    int rc = check_level(h, h->L, true);
    if (rc) return rc;
    if (!rc_in || !e || d <= 0) return fail(h, GMG_ERR_INVALID, "bad arguments");
    if ((rc = ensure_vectors(h, d))) return rc;
    Level& c = h->lv[h->L];
    if ((rc = to_device(h, h->L, rc_in, d, c.b))) return rc;
    if (h->coarse_device) enqueue_coarse_device<double>(h, d);
    else if ((rc = coarse_host_roundtrip<double>(h, d))) return rc;
    h->loaded_d = 0;
    return to_host(h, h->L, c.x, d, e);
} GMG_CATCH_H

int gmg_residual_norm(gmg_handle h, const double* b, const double* x, int d, int type, double* out) try {
    NEED_DEVICE();
    int rc = check_level(h, 0, false);
    if (rc) return rc;
    if ((rc = check_whole_system(h))) return rc;
    if (!b || !x || !out || d <= 0) return fail(h, GMG_ERR_INVALID, "bad arguments");
    if ((rc = check_norm_type(h, type))) return rc;
    if ((rc = ensure_vectors(h, d))) return rc;
    Level& l = h->lv[0];
    if ((rc = to_device(h, 0, b, d, l.b))) return rc;
    if ((rc = to_device(h, 0, x, d, l.x))) return rc;
    if ((rc = launch_norm(h, d, type))) return rc;
    if ((rc = wait_norm(h))) return rc;
    h->loaded_d = 0;
    *out = norm_from_sums(h->h_norm, d, type);
    return GMG_OK;
} GMG_CATCH_H

// ---- the fp32 inner cycle's operators, one at a time (include/gravomg_hip_internal.h) ------------------------------------------

namespace {
// host fp64 -> the level's fp64 vector -> its fp32 twin, and back (exact for fp32-representable values)
int f32_in(gmg_handle h, int k, const double* src, int d, double* v64, float* v32) {
    if (const int rc = to_device(h, k, src, d, v64)) return rc;
    launch_cvt(h, v64, v32, (size_t)h->lv[k].n_pad * d);
    return GMG_OK;
}
int f32_out(gmg_handle h, int k, const float* v32, double* v64, int d, double* dst) {
    launch_cvt(h, v32, v64, (size_t)h->lv[k].n_pad * d);
    return to_host(h, k, v64, d, dst);
}
// level l's smoothing from zero or from x32 as enqueue_down enqueues it, and the residual behind it; sets residual_from_sweep
void f32_smooth_residual(gmg_handle h, int k, int d, int iters, bool from_zero, bool first_done) {
    Level& l = h->lv[k];
    SmoothAsk<float> ask;
    ask.from_zero = from_zero && (k > 0 || pointwise_smoother(h->cfg)) && smooth_from_zero_ok(h, l, iters);
    ask.first_done = first_done;
    if (from_zero && !ask.from_zero) (void)hipMemsetAsync(l.x32, 0, sizeof(float) * (size_t)l.n_pad * d, h->stream);
    const SmoothDone<float> swept = launch_smooth<float>(h, l, d, iters, ask);
    const bool delta = k > 0 && launch_residual_delta<float>(h, l, d, l.r32, swept);
    if (!delta) launch_spmv<float>(h, l, d, 1, l.b32, l.x32, l.r32);
    h->timing["residual_from_sweep"] = delta ? 1.0 : 0.0;
}
}  // namespace

int gmg_debug_f32_op(gmg_handle h, int op, int k, int d, int iters, int flag, const double* in0, const double* in1, double* out0, double* out1,
                     double* out2) try {
    NEED_DEVICE();
    if (!h->cfg.inner_precision) return fail(h, GMG_ERR_STATE, "gmg_debug_f32_op needs a handle created with inner_precision = 1");
    const bool coarse_op = op == GMG_F32_COARSE;
    int rc = check_level(h, coarse_op ? h->L : k, coarse_op);
    if (rc) return rc;
    if ((rc = check_whole_system(h))) return rc;
    if (!in0 || !out0 || d <= 0 || iters < 0) return fail(h, GMG_ERR_INVALID, "bad arguments");
    if ((rc = ensure_vectors(h, d))) return rc;
    h->loaded_d = 0;
    if (coarse_op) {
        Level& c = h->lv[h->L];
        if ((rc = f32_in(h, h->L, in0, d, c.b, c.b32))) return rc;
        if (h->coarse_device) enqueue_coarse_device<float>(h, d);
        else if ((rc = coarse_host_roundtrip<float>(h, d))) return rc;
        return f32_out(h, h->L, c.x32, c.x, d, out0);
    }
    Level& l = h->lv[k];
    Level& c = h->lv[k + 1];
    switch (op) {
    case GMG_F32_SMOOTH:                      // in0 b, in1 x -> out0 x
        if (!in1) break;
        if ((rc = f32_in(h, k, in0, d, l.b, l.b32)) || (rc = f32_in(h, k, in1, d, l.x, l.x32))) return rc;
        launch_smooth<float>(h, l, d, iters);
        return f32_out(h, k, l.x32, l.x, d, out0);
    case GMG_F32_SMOOTH_RESIDUAL:             // in0 b, in1 x (flag = from_zero: not read) -> out0 x, out1 r
        if (!out1 || (!flag && !in1)) break;
        if ((rc = f32_in(h, k, in0, d, l.b, l.b32))) return rc;
        if (!flag && (rc = f32_in(h, k, in1, d, l.x, l.x32))) return rc;
        f32_smooth_residual(h, k, d, iters, flag != 0, false);
        if ((rc = f32_out(h, k, l.x32, l.x, d, out0))) return rc;
        return f32_out(h, k, l.r32, l.r, d, out1);
    case GMG_F32_RESIDUAL:                    // in0 b, in1 x -> out0 b - A x
        if (!in1) break;
        if ((rc = f32_in(h, k, in0, d, l.b, l.b32)) || (rc = f32_in(h, k, in1, d, l.x, l.x32))) return rc;
        launch_spmv<float>(h, l, d, 1, l.b32, l.x32, l.r32);
        return f32_out(h, k, l.r32, l.r, d, out0);
    case GMG_F32_SPMV:                        // in0 x -> out0 A x
        if ((rc = f32_in(h, k, in0, d, l.x, l.x32))) return rc;
        launch_spmv<float>(h, l, d, 0, nullptr, l.x32, l.r32);
        return f32_out(h, k, l.r32, l.r, d, out0);
    case GMG_F32_RESTRICT:                    // in0 r_k -> out0 b_{k+1}
        if ((rc = f32_in(h, k, in0, d, l.r, l.r32))) return rc;
        launch_restrict<float>(h, l, c, d, l.r32, c.b32);
        return f32_out(h, k + 1, c.b32, c.b, d, out0);
    case GMG_F32_RESTRICT_SWEEPS: {           // in0 r_k -> out0 b_{k+1}, out1 x_{k+1} after `iters` pre-sweeps from zero, out2 its residual
        if (!out1 || !out2 || iters <= 0) break;
        if (k + 1 >= h->L) return fail(h, GMG_ERR_INVALID, "level k + 1 is the coarsest: it is not smoothed");
        // (d = 2 .. 4 on level 0: the way down hands the restriction an interleaved residual, which the residual launch writes -- from x = 0 it is r_k itself)
        const bool il = k == 0 && d > 1 && d <= 4 && l.Aoff.lpr == 1;
        if (il) {
            if ((rc = f32_in(h, k, in0, d, l.b, l.b32))) return rc;
            (void)hipMemsetAsync(l.x32, 0, sizeof(float) * (size_t)l.n_pad * d, h->stream);
            launch_spmv<float>(h, l, d, 1, l.b32, l.x32, l.r32, -1, true);
        } else if ((rc = f32_in(h, k, in0, d, l.r, l.r32))) return rc;
        struct PreIters { int& v; int old; ~PreIters() { v = old; } } keep{h->cfg.pre_iters, h->cfg.pre_iters};      // (restrict_into asks the configuration)
        h->cfg.pre_iters = iters;
        const bool first_done = restrict_into<float>(h, k, d, il);
        f32_smooth_residual(h, k + 1, d, iters, true, first_done);
        if ((rc = f32_out(h, k + 1, c.b32, c.b, d, out0)) || (rc = f32_out(h, k + 1, c.x32, c.x, d, out1))) return rc;
        return f32_out(h, k + 1, c.r32, c.r, d, out2);
    }
    case GMG_F32_PROLONG_ADD:                 // in0 e_{k+1}, in1 x_k -> out0 x_k + U e
        if (!in1) break;
        if ((rc = f32_in(h, k + 1, in0, d, c.x, c.x32)) || (rc = f32_in(h, k, in1, d, l.x, l.x32))) return rc;
        launch_prolong_add<float>(h, l, c, d, c.x32, l.x32);
        return f32_out(h, k, l.x32, l.x, d, out0);
    case GMG_F32_DEFECT: {                    // level 0: in0 b, in1 x (fp64) -> out0 b32 widened, out1[0] the norm of type `flag`
        if (!in1 || !out1 || k != 0) break;
        if ((rc = check_norm_type(h, flag))) return rc;
        if ((rc = to_device(h, 0, in0, d, l.b)) || (rc = to_device(h, 0, in1, d, l.x))) return rc;
        if ((rc = launch_residual_to_f32(h, d, flag)) || (rc = wait_norm(h))) return rc;
        out1[0] = norm_from_sums(h->h_norm, d, flag);
        return f32_out(h, 0, l.b32, l.r, d, out0);
    }
    case GMG_F32_CORRECT: {                   // level 0: in0 an fp32 vector, in1 x (fp64) -> out0 x + in0
        if (!in1 || k != 0) break;
        if ((rc = f32_in(h, 0, in0, d, l.r, l.x32)) || (rc = to_device(h, 0, in1, d, l.x))) return rc;
        const size_t cnt = (size_t)l.n_pad * d;
        hipLaunchKernelGGL(gmgk::add_correction, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, l.x32, l.x, (int64_t)cnt);
        return to_host(h, 0, l.x, d, out0);
    }
    default:
        return fail(h, GMG_ERR_INVALID, "unknown operation");
    }
    return fail(h, GMG_ERR_INVALID, "bad arguments");
} GMG_CATCH_H

// ---- resident problem: load / run / fetch ------------------------------------------------------------------

int gmg_load_problem(gmg_handle h, const double* b, const double* x0, int d) try {
    NEED_DEVICE();
    int rc = check_level(h, 0, false);
    if (rc) return rc;
    if (!b || !x0 || d <= 0) return fail(h, GMG_ERR_INVALID, "bad arguments");
    auto tl = clk::now();
    if ((rc = ensure_vectors(h, d))) return rc;
    h->timing["load_vectors"] = ms_since(tl); tl = clk::now();
    Level& l = h->lv[0];
    // The reference's Python API always starts from x0 = rhs (gravomg_bindings/src/cpp/core.cpp:69): when the initial guess IS
    // the right-hand side (same buffer, or the same content -- one threaded comparison, far cheaper than a second trip over
    // PCIe), it is copied on the device instead of being uploaded again.  The comparison runs beside the upload of b.
    bool same = x0 == b;
    std::future<bool> compared;
    if (!same) {
        const size_t cnt = (size_t)l.n * d;
        const int threads = std::min(h->cfg.host_threads, 16);
        compared = std::async(std::launch::async, [b, x0, cnt, threads] {
            std::atomic<bool> differ{false};
            parallel_ranges((int)std::min<size_t>(cnt >> 12, 1 << 20) + 1, threads, [&](int lo, int hi, int) {
                const size_t a = (size_t)lo << 12, e = std::min(cnt, (size_t)hi << 12);
                if (a < e && !differ.load(std::memory_order_relaxed) && std::memcmp(b + a, x0 + a, sizeof(double) * (e - a)) != 0) differ = true;
            }, 2);
            return !differ.load();
        });
    }
    rc = to_device(h, 0, b, d, l.b);
    if (compared.valid()) same = compared.get();          // (joined before any return: the task reads the caller's arrays)
    if (rc) return rc;
    h->timing["load_b"] = ms_since(tl); tl = clk::now();
    if (same) HIPCHK(hipMemcpyAsync(l.x, l.b, sizeof(double) * (size_t)l.n_pad * d, hipMemcpyDeviceToDevice, h->stream));
    else if ((rc = to_device(h, 0, x0, d, l.x))) return rc;
    h->timing["load_x"] = ms_since(tl); tl = clk::now();
    if (h->cfg.inner_precision && (rc = launch_residual_to_f32(h, d, -1))) return rc;    // defect of the initial guess -> b32
    HIPCHK(hipStreamSynchronize(h->stream));
    h->timing["load_sync"] = ms_since(tl);
    h->loaded_d = d;
    return GMG_OK;
} GMG_CATCH_H

namespace {
// does a loop over cycles enqueue heads (head_eligible, where the loop wants them)?  Its two timing keys exist from then on.  Such a loop hands
// every cycle a CycleWatch and whether the cycle's head is in the stream: its own locals, so nothing of them outlives it.
inline bool loop_enqueues_heads(gmg_handle h, int d, bool wanted) {
    if (!wanted || !head_eligible(h, d)) return false;
    h->timing["heads_enqueued"] += 0.0; h->timing["head_decision_differs"] += 0.0; h->timing["heads_folded"] += 0.0;
    return true;
}
}  // namespace

int gmg_run_cycles(gmg_handle h, int n_cycles, int stop_type, double* residues) try {
    NEED_DEVICE();
    if (h->loaded_d <= 0) return fail(h, GMG_ERR_STATE, "no problem loaded (gmg_load_problem)");
    if (n_cycles < 0) return fail(h, GMG_ERR_INVALID, "bad cycle count");
    int rc;
    if ((rc = check_whole_system(h))) return rc;
    if (stop_type >= 0 && (rc = check_norm_type(h, stop_type))) return rc;
    const int d = h->loaded_d;
    HelperScope helper_scope(h, d);
    // (a fixed number of cycles: the first colour launch of the next one goes into the stream before the host has seen this one's norm,
    // as in the solve loop -- there the check's reduction decides on the device whether that launch does anything, solve_common)
    const bool heads = loop_enqueues_heads(h, d, stop_type >= 0);
    CycleWatch watch{0, 0.0, stop_type, 0};
    int head_done = HEAD_NONE;       // this cycle's first colour launch is in the stream (HEAD_FOLDED: its first two)
    for (int i = 0; i < n_cycles; ++i) {
        watch.cycles_done = i + 1;
        const bool head = heads && i + 1 < n_cycles;
        watch.fold = head && fold_eligible(h, d);       // (the check then also computes the head's values: asked anew every cycle)
        if ((rc = vcycle_resident(h, d, stop_type, head_done, heads ? &watch : nullptr))) return rc;
        if (stop_type >= 0) {
            head_done = head ? enqueue_head(h, d, watch.fold) : HEAD_NONE;
            if ((rc = wait_norm(h))) return rc;
            if (residues) residues[i] = norm_from_sums(h->h_norm, d, stop_type);
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return GMG_OK;
} GMG_CATCH_H

// Where the time of a cycle goes, leg by leg: `reps` V-cycles + residual checks on the resident problem with an event at every leg boundary.
// ms_out[k], k < L: level k (way down: pre-smoothing, residual, restriction; way up: prolongation, post-smoothing); ms_out[L]: the coarsest
// solve (publication of the right-hand side, host back-substitution, fetch: GPU idle time included); ms_out[L + 1]: the residual check.
// The events cost a little (the sum is reported against the unprofiled cycle by the caller).
int gmg_profile_cycle(gmg_handle h, int stop_type, int reps, double* ms_out, int n_out) try {
    NEED_DEVICE();
    if (h->loaded_d <= 0) return fail(h, GMG_ERR_STATE, "no problem loaded (gmg_load_problem)");
    const int L = h->L;
    if (!ms_out || n_out < L + 2 || reps <= 0) return fail(h, GMG_ERR_INVALID, "bad arguments (ms_out needs levels + 2 entries)");
    if (h->cfg.use_graph) return fail(h, GMG_ERR_UNSUPPORTED, "leg profiling needs stream launches (use_graph = 0)");
    int rc;
    if ((rc = check_whole_system(h))) return rc;
    if ((rc = check_norm_type(h, stop_type))) return rc;
    const int d = h->loaded_d;
    HelperScope helper_scope(h, d);
    std::vector<double> acc((size_t)L + 2, 0.0);
    for (int i = 0; i < reps; ++i) {
        h->prof_on = true; h->prof_n = 0;
        rc = vcycle_resident(h, d, stop_type);
        h->prof_on = false;
        if (rc) return rc;
        if ((rc = wait_norm(h))) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->prof_n != 2 * L + 3) return fail(h, GMG_ERR_STATE, "unexpected number of leg boundaries");
        auto span = [&](int a, int b) { float ms = 0.f; (void)hipEventElapsedTime(&ms, h->prof_ev[a], h->prof_ev[b]); return (double)ms; };
        for (int k = 0; k < L; ++k) acc[k] += span(k, k + 1) + span(L + 1 + (L - 1 - k), L + 2 + (L - 1 - k));
        acc[L] += span(L, L + 1);
        acc[L + 1] += span(2 * L + 1, 2 * L + 2);
    }
    for (int k = 0; k < L + 2; ++k) ms_out[k] = acc[k] / reps;
    return GMG_OK;
} GMG_CATCH_H

int gmg_fetch_solution(gmg_handle h, double* x) try {
    NEED_DEVICE();
    if (h->loaded_d <= 0) return fail(h, GMG_ERR_STATE, "no problem loaded (gmg_load_problem)");
    if (!x) return fail(h, GMG_ERR_INVALID, "bad arguments");
    return to_host(h, 0, h->lv[0].x, h->loaded_d, x);
} GMG_CATCH_H

int gmg_vcycle(gmg_handle h, const double* b, double* x, int d) try {
    int rc = gmg_load_problem(h, b, x, d);
    if (rc) return rc;
    if ((rc = gmg_run_cycles(h, 1, -1, nullptr))) return rc;
    return gmg_fetch_solution(h, x);
} GMG_CATCH_H

// The solve loop.  Where the problem comes from and where the last iterate goes is the caller's: load() makes b and x of level 0 resident (and
// h->loaded_d = d), fetch() delivers x and returns once it is there -- host arrays (gmg_solve, gmg_solve_x0_rhs) or the caller's device memory
// (gmg_solve_device).  bad_args: what is wrong with the caller's arguments (no device needed to tell), or nullptr.
extern "C++" {
template <class Load, class Fetch>
static int solve_common(gmg_handle h, const char* bad_args, int d, double tol, int stop_type, int max_iter, int* iters_out, double* residue_out, double* conv,
                        Load&& load, Fetch&& fetch) {
    NEED_DEVICE();
    int rc;
    if (bad_args) return fail(h, GMG_ERR_INVALID, bad_args);
    if ((rc = check_whole_system(h))) return rc;
    if ((rc = check_norm_type(h, stop_type))) return rc;
    auto t_all = clk::now();
    HelperScope helper_scope(h, d);
    if ((rc = load())) return rc;
    // gmg_config::nullspace = 1: b <- b - (1^T b / n) 1, the orthogonal projection onto range(A); everything behind this line -- the three
    // loops, their residual checks -- sees the projected right-hand side (the fp32 inner cycle's first defect is formed again from it)
    const int nullspace = h->cfg.nullspace;
    if (nullspace) {
        if ((rc = ensure_nullspace(h))) return rc;
        launch_nullspace_project(h, d, h->lv[0].b, nullptr, 0);
        if (h->cfg.inner_precision && (rc = launch_residual_to_f32(h, d, -1))) return rc;
    }
    h->timing["solve_load"] = ms_since(t_all);
    h->timing["coarse_host_ms"] = 0.0;
    auto t0 = clk::now();
    // gmg_config::accelerate = m > 0: every cycle's step is recombined with the last m - 1 (truncated GCR, the cycle as the preconditioner:
    // launch_accel_step) so that the weighted residual the loop tests is minimal.  The residue then comes out of a recurrence (r -= alpha q); one that
    // would end the loop is CONFIRMED by the ordinary check on the new iterate -- that value is the one reported and tested (the recurrence can
    // drop below the accuracy floor of b - A x) -- and the loop goes on from the recomputed residual where it does not hold.  No speculated head:
    // the host decides.
    const int accel = h->cfg.accelerate;
    int confirmations = 0;
    Level& l0 = h->lv[0];
    auto accel_step = [&](SolveRule& rule, double& residue, int&) -> int {
        if ((rc = vcycle_resident(h, d, -1))) return rc;
        launch_spmv<double>(h, l0, d, 1, l0.b, l0.x, l0.r);                  // r~ = b - A x~ (q = r - r~ = A z: no product of its own)
        if ((rc = launch_accel_step(h, d, stop_type, rule.cycles))) return rc;
        if ((rc = wait_norm(h))) return rc;
        residue = norm_from_sums(h->h_norm, d, stop_type);
        if (rule_goes_on(rule_after(rule, residue))) return GMG_OK;
        const double recurrence = residue;
        if ((rc = launch_norm(h, d, stop_type))) return rc;                   // it would end the loop: the check on the iterate itself decides
        if ((rc = wait_norm(h))) return rc;
        residue = norm_from_sums(h->h_norm, d, stop_type);
        ++confirmations;
        // (a recurrence that ran on below the accuracy floor is not what the verdict measures this residue against: solve_rule.hpp)
        rule = rule_confirmed(rule, recurrence, residue, rule_floor(h->h_norm, d, stop_type));
        // (confirmed, above the tolerance and the loop will go on: the recurrence restarts from the residual of the iterate, the directions stay)
        if (rule_goes_on(rule_after(rule, residue))) launch_spmv<double>(h, l0, d, 1, l0.b, l0.x, h->accel.r);
        return GMG_OK;
    };
    // gmg_config::pcg = 1: conjugate gradients with the cycle as the preconditioner (launch_pcg_step).  The cycle runs on the CG
    // residual from a zero guess, so for the duration of the loop level 0's x / b are z / r and the CG iterate and the true right-hand side live in
    // the PCG state (pcg_exchange); the confirming check -- as in the accelerated branch -- and the caller's fetch() see them exchanged back.
    // gmg_config::precond_precision = 1: z = (double) cycle32(fl32(r)).  The fp32 cycle reads level 0's b32 and leaves z in x32; it does not touch
    // level 0's fp64 x / b, so the CG iterate and the true right-hand side stay where they are -- nothing is exchanged -- and r lives in the PCG
    // state (pcg.b).  (Level 0 is never the coarsest level, whose fp32 solve converts through its fp64 vectors: gmg_set_system refuses a hierarchy
    // without a transfer level.)  fl32(r) reaches b32 from pcg_update; the fresh residuals (the first, and after a confirmation that did not hold) through launch_cvt.
    const int pcg = h->cfg.pcg;
    const bool pcg32 = pcg && h->cfg.precond_precision;
    const size_t l0_count = (size_t)l0.n_pad * d;
    int pcg_confirmations = 0;
    bool pcg_first = true, pcg_fresh = false;
    struct PcgRestore { gmg_handle h; ~PcgRestore() { if (h->pcg.exchanged) pcg_exchange(h); } } pcg_restore{h};        // (every way out, errors included)
    auto pcg_step = [&](SolveRule& rule, double& residue, int&) -> int {
        // z = cycle(rhs = r, x = 0); with gmg_config::zero_guess_step the cycle knows that its guess is zero and nobody writes the zeros
        if ((rc = pcg32 ? vcycle_legs<float>(h, d, -1, kPcgGraphSalt32, 0, nullptr, /*zero_guess*/ true, /*precond*/ true)
                        : vcycle_legs<double>(h, d, -1, kPcgGraphSalt, 0, nullptr, /*zero_guess*/ true))) return rc;
        if ((rc = launch_pcg_step(h, d, stop_type, pcg_first, pcg_fresh))) return rc;
        pcg_first = pcg_fresh = false;
        if ((rc = wait_norm(h))) return rc;
        residue = norm_from_sums(h->h_norm, d, stop_type);
        if (rule_goes_on(rule_after(rule, residue))) return GMG_OK;
        const double recurrence = residue;
        if (!pcg32) pcg_exchange(h);                                              // level 0 holds the iterate and the true right-hand side
        if ((rc = launch_norm(h, d, stop_type))) return rc;                       // it would end the loop: the check on the iterate itself decides
        if ((rc = wait_norm(h))) return rc;
        residue = norm_from_sums(h->h_norm, d, stop_type);
        ++pcg_confirmations;
        rule = rule_confirmed(rule, recurrence, residue, rule_floor(h->h_norm, d, stop_type));
        // (confirmed, above the tolerance and the loop will go on: r is recomputed from the iterate, the next step starts a new recurrence)
        if (rule_goes_on(rule_after(rule, residue))) {
            launch_spmv<double>(h, l0, d, 1, l0.b, l0.x, h->pcg.b);
            if (pcg32) launch_cvt(h, h->pcg.b.get(), l0.b32.get(), l0_count);
            else pcg_exchange(h);
            pcg_fresh = true;
        }
        return GMG_OK;
    };
    // Head of the next cycle (gmg_config::speculate_head): the check's reduction takes the loop's decision on the device too (same sums, same
    // functions: gmgk::reduce_partials / SolveWatch, solve_rule.hpp) and the first colour launch of the next cycle is enqueued behind it at
    // once -- it returns without touching x when the iteration has stopped.  The ~6 us the host needs to see the norm and to get a launch to
    // the device are hidden behind that launch.  The loop follows the device's word.
    const bool heads = loop_enqueues_heads(h, d, accel == 0 && pcg == 0);
    CycleWatch watch{1, tol, stop_type, 0};
    // gmg_config::fold_head: the check computes the head's values too and the launch enqueued behind it is the second colour launch, which
    // commits them (engine_cycle.hip.hpp::fold_eligible) -- a stopped iteration still returns at once, x the iterate that was checked.
    int head_done = HEAD_NONE;       // the coming cycle's first colour launch is in the stream (HEAD_FOLDED: its first two) and found the word set
    auto plain_step = [&](const SolveRule& rule, double& residue, int& device_go) -> int {
        watch.cycles_done = rule.cycles + 1;
        const bool head = heads && rule.cycles + 2 <= rule.max_iter;          // (a cycle after this one is allowed)
        watch.fold = head && fold_eligible(h, d);                             // (asked anew every iteration)
        if ((rc = vcycle_resident(h, d, stop_type, head_done, heads ? &watch : nullptr))) return rc;
        head_done = head ? enqueue_head(h, d, watch.fold) : HEAD_NONE;
        if ((rc = wait_norm(h))) return rc;
        residue = norm_from_sums(h->h_norm, d, stop_type);
        if (head) device_go = __atomic_load_n(h->h_flag + 1, __ATOMIC_ACQUIRE) != 0;
        if (device_go == 0) head_done = HEAD_NONE;              // that launch found the word cleared and returned
        return GMG_OK;
    };
    int verdict;
    if (accel > 0) {
        if ((rc = ensure_accel(h))) return rc;
        HIPCHK(hipMemsetAsync(h->accel.scal, 0, sizeof(double) * ((size_t)9 * h->accel.d + 1), h->stream));      // nothing stored (s_j = 0), no guarded step, <b, b> not known
        HIPCHK(hipMemcpyAsync(h->accel.xk, l0.x, sizeof(double) * (size_t)l0.n_pad * d, hipMemcpyDeviceToDevice, h->stream));
        launch_spmv<double>(h, l0, d, 1, l0.b, l0.x, h->accel.r);
        verdict = solve_loop(h, tol, max_iter, t0, conv, h->cfg.verbose, iters_out, residue_out, accel_step);
    } else if (pcg) {
        if ((rc = ensure_pcg(h))) return rc;
        HIPCHK(hipMemsetAsync(h->pcg.scal, 0, sizeof(double) * ((size_t)4 * h->pcg.d + 2), h->stream));
        launch_spmv<double>(h, l0, d, 1, l0.b, l0.x, h->pcg.b);                  // r = b - A x0
        // the first cycle's zero guess (later ones: pcg_direction) -- unless the cycle starts from zero by itself (level0_zero_guess)
        if (pcg32) {
            launch_cvt(h, h->pcg.b.get(), l0.b32.get(), l0_count);               // fl32(r): the first cycle's right-hand side (later ones: pcg_update)
            if (!level0_zero_guess(h)) HIPCHK(hipMemsetAsync(l0.x32, 0, sizeof(float) * l0_count, h->stream));
        } else {
            if (!level0_zero_guess(h)) HIPCHK(hipMemsetAsync(h->pcg.x, 0, sizeof(double) * l0_count, h->stream));
            pcg_exchange(h);
        }
        verdict = solve_loop(h, tol, max_iter, t0, conv, h->cfg.verbose, iters_out, residue_out, pcg_step);
    } else
        verdict = solve_loop(h, tol, max_iter, t0, conv, h->cfg.verbose, iters_out, residue_out, plain_step);
    if (verdict < 0) return verdict;
    if (h->pcg.exchanged) return fail(h, GMG_ERR_STATE, "the preconditioned CG loop ended without its confirming check");      // (cannot happen: solve_loop ends where the step confirmed)
    h->timing["pcg"] = pcg;
    if (pcg32) h->timing["precond_precision"] = 1;
    h->timing["pcg_confirmations"] = pcg_confirmations;
    double pcg_counts[2] = {0.0, 0.0};
    if (pcg) {
        HIPCHK(hipMemcpyAsync(pcg_counts, h->pcg.scal + (size_t)4 * h->pcg.d, sizeof(pcg_counts), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    h->timing["pcg_guard_steps"] = pcg_counts[0];
    h->timing["pcg_restarts"] = pcg_counts[1];
    h->timing["accelerate"] = accel;
    h->timing["accel_confirmations"] = confirmations;
    double guard_steps = 0.0;
    if (accel > 0) {
        HIPCHK(hipMemcpyAsync(&guard_steps, h->accel.scal + (size_t)8 * h->accel.d, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    h->timing["accel_guard_steps"] = guard_steps;
    if (nullspace) {
        // x <- x - (m^T x / m^T 1) 1: the solution of zero mass-weighted mean (unit weights without a mass); A 1 = 0 leaves the residue as reported
        launch_nullspace_project(h, d, l0.x, h->d_mass ? h->d_mass.get() : nullptr, 1);
        std::vector<double> sums((size_t)6 * h->nullsp.d, 0.0);
        HIPCHK(hipMemcpyAsync(sums.data(), h->nullsp.scal, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        // max over the columns of |1^T b| / (sqrt(n) |b|_2) before the projection (a zero column counts 0)
        double defect = 0.0;
        const int DA = h->nullsp.d;
        for (int c = 0; c < d; ++c) {
            const double s1 = sums[(size_t)DA + c], s2 = sums[(size_t)2 * DA + c];
            if (s2 > 0.0) defect = std::max(defect, std::fabs(s1) / (std::sqrt((double)l0.n) * std::sqrt(s2)));
        }
        h->timing["nullspace_rhs_defect"] = defect;
    }
    auto t_f = clk::now();
    if ((rc = fetch())) return rc;
    h->timing["solve_fetch"] = ms_since(t_f);
    h->timing["solve_call"] = ms_since(t_all);
    h->timing["solver_total"] = h->timing["setup_total"] + h->timing["solve_call"];
    return verdict;
}
}  // extern "C++"

// x0: the initial guess (may be rhs itself: then it is copied on the device, not uploaded); x: receives the last iterate
static int solve_host(gmg_handle h, const double* rhs, const double* x0, double* x, int d, double tol, int stop_type, int max_iter, int* iters_out,
                      double* residue_out, double* conv) {
    return solve_common(h, rhs && x0 && x ? nullptr : "bad arguments", d, tol, stop_type, max_iter, iters_out, residue_out, conv,
                        [&] { return gmg_load_problem(h, rhs, x0, d); }, [&] { return gmg_fetch_solution(h, x); });
}

int gmg_solve(gmg_handle h, const double* rhs, double* x, int d, double tol, int stop_type, int max_iter, int* iters_out,
              double* residue_out, double* conv) try {
    return solve_host(h, rhs, x, x, d, tol, stop_type, max_iter, iters_out, residue_out, conv);
} GMG_CATCH_H

// The reference's binding always starts from x0 = rhs (gravomg_bindings/src/cpp/core.cpp:69): this entry point says so, and the
// caller neither fills x with a copy of rhs nor pays for the comparison gmg_solve makes to find that out.  x is output only.
int gmg_solve_x0_rhs(gmg_handle h, const double* rhs, double* x, int d, double tol, int stop_type, int max_iter, int* iters_out,
                     double* residue_out, double* conv) try {
    return solve_host(h, rhs, rhs, x, d, tol, stop_type, max_iter, iters_out, residue_out, conv);
} GMG_CATCH_H

// The load step on the caller's device memory: what gmg_load_problem leaves behind -- b and x of level 0 in device numbering, padding rows
// zero, with inner_precision = 1 the defect of the initial guess as the fp32 right-hand side -- from one gather kernel on the handle's stream.
// Every check comes before the first enqueue.
static int load_problem_device(gmg_handle h, const gmg_device_vectors& v, int d) {
    int rc = check_level(h, 0, false);
    if (rc) return rc;
    Level& l = h->lv[0];
    if (const char* why = device_vectors_fault(&v, l.n, d)) return fail(h, GMG_ERR_INVALID, why);      // (the extents, which need n)
    if ((rc = check_device_vectors(h, v, l.n, d))) return rc;
    if ((rc = ensure_vectors(h, d))) return rc;
    launch_permute_in2_strided(h, l, v, d);
    if (h->cfg.inner_precision && (rc = launch_residual_to_f32(h, d, -1))) return rc;    // defect of the initial guess -> b32
    h->loaded_d = d;
    return GMG_OK;
}

int gmg_solve_device(gmg_handle h, const gmg_device_vectors* v, int d, double tol, int stop_type, int max_iter, int* iters_out,
                     double* residue_out, double* conv) try {
    return solve_common(h, device_vectors_fault(v, 1, d), d, tol, stop_type, max_iter, iters_out, residue_out, conv,
                        [&] { return load_problem_device(h, *v, d); },
                        [&] {
                            launch_permute_out_strided(h, h->lv[0], *v, d);
                            HIPCHK(hipStreamSynchronize(h->stream));
                            return (int)GMG_OK;
                        });
} GMG_CATCH_H

// gmg_set_system's values-only refresh with the values already on the device (include/gravomg_hip.h)
int gmg_set_system_values_device(gmg_handle h, const double* d_val, int64_t nnz) try {
    NEED_DEVICE();
    int rc;
    if (h->live != LiveSystem::system) return fail(h, GMG_ERR_STATE, h->live == LiveSystem::placeholder ? "no system set: the handle holds the prepared structure only (call gmg_set_system first)" : "no system set (call gmg_set_system first)");
    if ((rc = check_whole_system(h))) return rc;
    if (!h->live_key_valid || !h->refill_ready || (int)h->lv.size() != h->L + 1 || !refresh_possible(h) || h->live_from_copy)
        return fail(h, GMG_ERR_STATE, "the live system cannot be refreshed in place (set up by the host planner, or from arrays that were not in canonical storage): use gmg_set_system");
    Level& l0 = h->lv[0];
    if (nnz != l0.nnz) return fail(h, GMG_ERR_STATE, "nnz = " + std::to_string(nnz) + " but the live system stores " + std::to_string(l0.nnz) + " entries");
    if (!d_val) return fail(h, GMG_ERR_INVALID, "d_val is NULL");
    if ((rc = check_device_block(h, d_val, nnz - 1, "d_val"))) return rc;
    auto t_all = clk::now();
    HIPCHK(hipSetDevice(h->cfg.device));
    if (l0.ord.blocked && h->cfg.block_from_level >= 1) {
        // a level 0 that gmg_config::block_fine blocked stays blocked only while the new values pass its sign test (values_only does the same on the host)
        DevBuf<int> d_bad;
        if ((rc = dev_alloc(h, d_bad, 1))) return rc;
        int bad = 0;
        HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(int), h->stream));
        hipLaunchKernelGGL(gmgk::stieltjes_signs_flag, dim3((l0.n + 255) / 256), dim3(256), 0, h->stream, l0.n, l0.dA.ptr.get(), l0.dA.idx.get(), d_val, d_bad.get());
        HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (bad) return fail(h, GMG_ERR_STATE, "these values fail the sign test of the blocked level 0 (gmg_config::block_fine: positive diagonal, no positive off-diagonal entry): this system needs a full set-up through gmg_set_system");
    }
    HIPCHK(hipMemcpyAsync(l0.dA.val, d_val, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, h->stream));
    rc = refresh_system_values(h, l0.n, nullptr, t_all, /*values_uploaded=*/true);
    if (rc == GMG_OK) {
        h->timing["setup_structure_prepared"] = 0.0;
        h->timing["t_verdict"] = h->timing["setup_total"] = ms_since(t_all);
        h->timing["upload"] = h->timing["setup_total"] - h->timing["reduction"];
        return GMG_OK;
    }
    lose_live_system(h); h->refill_ready = false;       // half-refreshed values: no solves on them
    return rc == 1 ? fail(h, GMG_ERR_STATE, "value refresh could not run in place") : rc;
} GMG_CATCH_H

// ---- multi-GPU: one process per GPU, level 0 row-partitioned per colour, levels >= 1 replicated ---------------
// The caller (gravo_mg_amd/dist.py) owns the level-0 vectors and performs the exchanges (RCCL all-gather of the
// colour segment of x after every colour); these entry points only launch this rank's share of the work.

int gmg_set_stream(gmg_handle h, void* hip_stream) try {
    NEED_DEVICE();
    HIPCHK(hipStreamSynchronize(h->stream));
    drop_graphs(h);
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return GMG_OK;
} GMG_CATCH_H

int gmg_dist_partition(gmg_handle h, int rank, int world) try {
    if (!h) return GMG_ERR_INVALID;
    PoolScope pool_scope_(&h->pool);
    if (world < 1 || rank < 0 || rank >= world) return fail(h, GMG_ERR_INVALID, "bad rank / world size");
    if (world > 1 && h->cfg.accelerate > 0) return fail(h, GMG_ERR_UNSUPPORTED, "gmg_config::accelerate runs on one device only (create the handle with accelerate = 0)");
    if (world > 1 && h->cfg.nullspace) return fail(h, GMG_ERR_UNSUPPORTED, "gmg_config::nullspace runs on one device only (create the handle with nullspace = 0)");
    if (world > 1 && h->cfg.row_align % (64 * world)) return fail(h, GMG_ERR_STATE, "create the handle with row_align = 64 * world (colour classes are cut into `world` pieces of whole slices)");
    if (rank == h->part_rank && world == h->part_world) return GMG_OK;
    if (h->has_device && h->live != LiveSystem::none) { drop_system(h); h->live_key_valid = false; }      // laid out for another partition
    h->part_rank = rank; h->part_world = world;
    h->plan.reset();
    return GMG_OK;
} GMG_CATCH_H

int gmg_dist_setup(gmg_handle h, int rank, int world) try {
    NEED_DEVICE();
    int rc = check_level(h, 0, false);
    if (rc) return rc;
    if (world < 1 || rank < 0 || rank >= world) return fail(h, GMG_ERR_INVALID, "bad rank / world size");
    if (world > 1 && h->cfg.accelerate > 0) return fail(h, GMG_ERR_UNSUPPORTED, "gmg_config::accelerate runs on one device only (create the handle with accelerate = 0)");
    if (world > 1 && h->cfg.nullspace) return fail(h, GMG_ERR_UNSUPPORTED, "gmg_config::nullspace runs on one device only (create the handle with nullspace = 0)");
    if (h->partitioned && (rank != h->part_rank || world != h->part_world)) return fail(h, GMG_ERR_STATE, "the system was laid out for another rank / world size (gmg_dist_partition)");
    const LevelOrdering& o = h->lv[0].ord;
    if (h->cfg.smoother != GMG_SMOOTHER_MULTICOLOR_GS) return fail(h, GMG_ERR_STATE, std::string("the distributed path needs the multicolour / block-hybrid smoothers (gmg_config::smoother), this handle runs ") + smoother_name(h->cfg));
    // a blocked level 0 (gmg_config::block_fine: kNN operators) is ONE class of rows cut into `world` runs of whole 64-row blocks
    if (o.blocked && (h->cfg.block_rows != 64 || !h->lv[0].use_ep)) return fail(h, GMG_ERR_STATE, "a blocked level 0 is partitioned only as 64-row blocks of the entry-parallel sweep (block_rows = 64, block_ep = 1, one lane per row): set block_fine = 0 or block_lanes = 1");
    for (int c = 0; c < dist_classes(o); ++c)
        if ((o.color_begin[c + 1] - o.color_begin[c]) % (64 * world)) return fail(h, GMG_ERR_STATE, "colour classes are not aligned to 64*world rows: create the handle with row_align = 64*world");
    h->rank = rank; h->world = world; h->dist_ready = true;
    return GMG_OK;
} GMG_CATCH_H

int gmg_dist_bind(gmg_handle h, double* x0, double* b0, double* r0, int d) try {
    NEED_DEVICE();
    if (!h->dist_ready) return fail(h, GMG_ERR_STATE, "call gmg_dist_setup first");
    if (!x0 || !b0 || !r0 || d <= 0) return fail(h, GMG_ERR_INVALID, "bad arguments");
    int rc = ensure_vectors(h, d);
    if (rc) return rc;
    drop_graphs(h);
    Level& l = h->lv[0];
    if (!l.x.borrowed()) { h->own_x0 = std::move(l.x); h->own_b0 = std::move(l.b); h->own_r0 = std::move(l.r); }      // the engine's vectors are parked ...
    l.x.borrow(x0); l.b.borrow(b0); l.r.borrow(r0);                                                                        // ... the caller's stay the caller's
    h->bound = true;
    h->loaded_d = d;
    return GMG_OK;
} GMG_CATCH_H

namespace {
inline void own_range(gmg_handle h, int c, int& sb, int& se) {
    const LevelOrdering& o = h->lv[0].ord;
    if (h->dist_all_rows) { sb = o.color_begin[c] / 64; se = o.color_begin[c + 1] / 64; return; }     // the *_all entry points
    const int chunk = (o.color_begin[c + 1] - o.color_begin[c]) / 64 / h->world;
    sb = o.color_begin[c] / 64 + h->rank * chunk;
    se = sb + chunk;
}
int dist_ready(gmg_handle h) {
    if (!h->dist_ready || !h->bound || h->loaded_d <= 0) return fail(h, GMG_ERR_STATE, "distributed state not set (gmg_dist_setup + gmg_dist_bind)");
    return GMG_OK;
}
}  // namespace

// One colour of one Gauss-Seidel sweep on this rank's rows of level 0.  plain_rows (hybrid smoother, engine_dist.hip.hpp::p2p_smooth): one 64-bit word per
// slice, bit set = the row takes omega = 1.
static int dist_smooth_color_impl(gmg_handle h, int c, const unsigned long long* plain_rows) {
    NEED_DEVICE();
    int rc = dist_ready(h);
    if (rc) return rc;
    Level& l = h->lv[0];
    if (c < 0 || c >= dist_classes(l.ord)) return fail(h, GMG_ERR_INVALID, "colour out of range");
    if (l.ord.blocked) return fail(h, GMG_ERR_STATE, "level 0 is blocked: its sweep is a block sweep (gmg_p2p_cycles), not a colour sweep");
    int sb, se;
    own_range(h, c, sb, se);
    // (c16_sel: a rank whose share of the fine operators fits its memory-side cache reads them with ordinary loads)
    if (se > sb) for_col_chunks(h->loaded_d, [&](int c0, int dc) { launch_gs_color<double>(h, l, c0, dc, sb, se, h->cfg.gs_omega, plain_rows); });
    return GMG_OK;
}
int gmg_dist_smooth_color(gmg_handle h, int c) try { return dist_smooth_color_impl(h, c, nullptr); } GMG_CATCH_H

// r0[own rows] = b0 - A x0
int gmg_dist_residual_own(gmg_handle h) try {
    NEED_DEVICE();
    int rc = dist_ready(h);
    if (rc) return rc;
    Level& l = h->lv[0];
    for (int c = 0; c < dist_classes(l.ord); ++c) {
        int sb, se;
        own_range(h, c, sb, se);
        if (se > sb) launch_spmv_lpr<double, 1>(h, l, h->loaded_d, 1, l.b, l.x, l.r, sb, se);
    }
    return GMG_OK;
} GMG_CATCH_H

// Replicated coarse part: b1 = U0^T r0 (needs the complete r0), levels 1..L-1 down, coarsest solve, back up to level 1.
// _enqueue leaves the host half of the coarsest solve pending (coarse_host_serve) so that the caller can queue more work first.
static int dist_coarse_cycle_enqueue(gmg_handle h) {
    int rc = dist_ready(h);
    if (rc) return rc;
    const int d = h->loaded_d;
    const bool first_done = restrict_into<double>(h, 0, d, false);          // (+ level 1's first sweep where the layouts allow it)
    enqueue_down<double>(h, d, 1, first_done);
    if (h->coarse_device) enqueue_coarse_device<double>(h, d);
    else if ((rc = coarse_host_begin<double>(h, d))) return rc;
    enqueue_up<double>(h, d, 1);
    return GMG_OK;
}
int gmg_dist_coarse_cycle(gmg_handle h) try {
    NEED_DEVICE();
    int rc = dist_coarse_cycle_enqueue(h);
    const int served = coarse_host_serve(h);
    return rc ? rc : served;
} GMG_CATCH_H

// x0[own rows] += U0 x1
int gmg_dist_prolong_own(gmg_handle h) try {
    NEED_DEVICE();
    int rc = dist_ready(h);
    if (rc) return rc;
    Level& l = h->lv[0];
    Level& cl = h->lv[1];
    for (int c = 0; c < dist_classes(l.ord); ++c) {
        int sb, se;
        own_range(h, c, sb, se);
        // (quirk kept: C16 = 0 -- the 32-bit columns -- whatever l.P.c16_mode is)
        if (se > sb) launch_prolong_add<double>(h, l, cl, h->loaded_d, cl.x, l.x, false, sb, se, 0);
    }
    return GMG_OK;
} GMG_CATCH_H

// this rank's share of sum w r^2 / sum w b^2 per column -> h->d_norm[2 * d] (on the stream; no synchronisation)
static int dist_norm_launch(gmg_handle h, int type) {
    int rc = dist_ready(h);
    if (rc) return rc;
    if ((rc = check_norm_type(h, type))) return rc;
    Level& l = h->lv[0];
    const int d = h->loaded_d;
    const double* w = type == 1 ? h->d_minv : (type == 2 ? h->d_mass : nullptr);
    const int nc = dist_classes(l.ord);
    const int nblk = std::max(1, kNormBlocks / std::max(nc, 1));
    for_col_chunks(d, [&](int c0, int dc) {
        for (int c = 0; c < nc; ++c) {
            int sb, se;
            own_range(h, c, sb, se);
            DISPATCH_D(dc, hipLaunchKernelGGL(gmgk::residual_norm_partials<D>, dim3(nblk), dim3(gmgk::kBlock), 0, h->stream, l.Aoff.slice_ptr, l.Aoff.col,
                                              l.Aoff.val, l.diag, l.b + (size_t)c0 * l.n_pad, l.x + (size_t)c0 * l.n_pad, w, l.n_pad, sb, se,
                                              h->d_partials + (size_t)c * nblk * 2 * dc));
        }
        hipLaunchKernelGGL(gmgk::reduce_partials, dim3(1), dim3(gmgk::kReduceBlock), 0, h->stream, h->d_partials, nblk * nc, 2 * dc, h->d_norm + 2 * c0,
                           (unsigned long long*)nullptr, 0ull, 0);
    });
    return GMG_OK;
}

// sums[2*c] / sums[2*c+1] = this rank's share of sum w r^2 / sum w b^2 for column c (host output; synchronises).
int gmg_dist_norm_partial(gmg_handle h, int type, double* sums) try {
    NEED_DEVICE();
    if (!sums) return fail(h, GMG_ERR_INVALID, "bad arguments");
    int rc = dist_norm_launch(h, type);
    if (rc) return rc;
    const int d = h->loaded_d;
    HIPCHK(hipMemcpyAsync(h->h_norm, h->d_norm, sizeof(double) * 2 * d, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::memcpy(sums, h->h_norm, sizeof(double) * 2 * d);
    return GMG_OK;
} GMG_CATCH_H

// The same steps over ALL rows of level 0: after the exchange that follows every colour sweep each rank holds the complete x, so residual,
// prolongation-add and the norm sums can be computed redundantly instead of being exchanged (16 collectives per V-cycle, one per colour
// sweep, instead of 24 + an all-reduce; the sums are then identical on all ranks).  on != 0: gmg_dist_residual_own / gmg_dist_prolong_own /
// gmg_dist_norm_partial cover every row until it is switched off again.
int gmg_dist_all_rows(gmg_handle h, int on) try {
    if (!h) return GMG_ERR_INVALID;
    if (on && h->partitioned) return fail(h, GMG_ERR_STATE, "this handle holds one rank's rows only (gmg_dist_partition)");
    h->dist_all_rows = on != 0;
    return GMG_OK;
} GMG_CATCH_H

int gmg_dist_gather(gmg_handle h, const double* src, const int64_t* idx, int64_t n, double* dst) try {
    NEED_DEVICE();
    if (n < 0 || (n > 0 && (!src || !idx || !dst))) return fail(h, GMG_ERR_INVALID, "bad arguments");
    if (n) hipLaunchKernelGGL(gmgk::gather_entries, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, src, idx, n, dst);
    return GMG_OK;
} GMG_CATCH_H
int gmg_dist_scatter(gmg_handle h, const double* src, const int64_t* pos, const int64_t* idx, int64_t n, double* dst) try {
    NEED_DEVICE();
    if (n < 0 || (n > 0 && (!src || !pos || !idx || !dst))) return fail(h, GMG_ERR_INVALID, "bad arguments");
    if (n) hipLaunchKernelGGL(gmgk::scatter_entries, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, src, pos, idx, n, dst);
    return GMG_OK;
} GMG_CATCH_H

// ---- measurement --------------------------------------------------------------------------------------------

int gmg_algorithmic_bytes(gmg_handle h, int kind, int k, int d, double* bytes_out) try {
    if (!h || !bytes_out) return GMG_ERR_INVALID;
    int rc = check_level(h, k, false);
    if (rc) return rc;
    const Level& l = h->lv[k];
    const double s = 8.0, n = l.n, z = (double)l.nnz, u = (double)h->U[k].nnz(), nc = h->lv[k + 1].n;
    // matrix stream (value + int32 index) + row pointer + the dense vectors, each touched once
    const double sweep = z * (s + 4) + 4 * (n + 1) + 3 * n * d * s;
    switch (kind) {
        case 0: case 1: *bytes_out = sweep; break;
        case 2: *bytes_out = u * (s + 4) + 4 * (nc + 1) + n * d * s + nc * d * s; break;
        case 3: *bytes_out = u * (s + 4) + 4 * (n + 1) + nc * d * s + 2 * n * d * s; break;
        case 4: *bytes_out = sweep - n * d * s + n * s; break;       // reads x, b, M; writes nothing
        default: return fail(h, GMG_ERR_INVALID, "unknown kernel kind");
    }
    return GMG_OK;
} GMG_CATCH_H

int gmg_bench_kernel(gmg_handle h, int kind, int k, int d, int reps, double* ms_avg, int* launches_out) try {
    NEED_DEVICE();
    int rc = check_level(h, k, false);
    if (rc) return rc;
    if ((rc = check_whole_system(h))) return rc;
    if (!ms_avg || reps <= 0 || d <= 0) return fail(h, GMG_ERR_INVALID, "bad arguments");
    if ((rc = ensure_vectors(h, d))) return rc;
    Level& l = h->lv[k];
    int launches = 1;
    const bool il = k == 0 && d > 1 && d <= 4 && l.Aoff.lpr == 1;
    const bool il_p = il && h->L >= 2 && h->lv[1].ord.blocked && h->lv[1].use_ep && h->cfg.post_iters > 0 && !pointwise_smoother(h->cfg);
    auto body = [&]() {
        switch (kind) {
            case 0: launch_smooth<double>(h, l, d, 2); launches = (pointwise_smoother(h->cfg) || l.ord.blocked) ? 1 : l.ord.n_colors; break;
            // (level 0 with 2 .. 4 right-hand sides: the variants the cycle runs -- residual written / gathered as an interleaved multi-vector,
            // prolongation from the interleaved copy of level 1's x: engine_cycle.hip.hpp::enqueue_down / enqueue_up)
            case 1: launch_spmv<double>(h, l, d, 1, l.b, l.x, l.r, -1, il); break;
            case 2: launch_restrict<double>(h, l, h->lv[k + 1], d, l.r, h->lv[k + 1].b, il); break;
            case 3: launch_prolong_add<double>(h, l, h->lv[k + 1], d, il_p ? h->lv[k + 1].r : h->lv[k + 1].x, l.x, il_p); break;
            case 4: (void)launch_norm(h, d, 0); launches = 2; break;
            default: break;
        }
    };
    if (kind < 0 || kind > 4) return fail(h, GMG_ERR_INVALID, "unknown kernel kind");
    if (kind == 4 && k != 0) return fail(h, GMG_ERR_INVALID, "the norm kernel runs on level 0");
    for (int i = 0; i < 3; ++i) body();
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    for (int i = 0; i < reps; ++i) body();
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *ms_avg = (double)ms / reps / (kind == 0 ? 2 : 1);     // kind 0 enqueues two sweeps per repetition (ping-pong buffers)
    if (launches_out) *launches_out = launches;
    h->loaded_d = 0;
    return GMG_OK;
} GMG_CATCH_H

// ---- host-only: hierarchy -----------------------------------------------------------------------------------

int gmg_hierarchy_options_default(gmg_hierarchy_options* o) try {
    if (!o) return GMG_ERR_INVALID;
    o->ratio = 8.0; o->lower_bound = 1000; o->check_voronoi = 1; o->nested = 0; o->sampling = 0; o->weighting = 0; o->debug = 0; o->full_clustering = 0; o->use_device = 1;
    return GMG_OK;
} GMG_CATCH_0

// Device stage of the hierarchy builder (HierarchyOptions::device_select): uploads one level's selection inputs, runs
// gmgh::select_parents, downloads the per-point records.  A hierarchy is built before any handle exists, so the stage keeps its
// own stream and two pinned bounce buffers (process-wide, created on first use, one build at a time): the big arrays -- positions
// in, 38 bytes per point out -- cross PCIe in 16 MB pieces with worker threads copying the neighbouring piece between pageable
// memory and the bounce buffer (threaded first touch of the 110 MB result included).  Returns false (the host loop does the level)
// on any HIP failure.
namespace {
struct HierarchyXfer {
    std::mutex m;
    hipStream_t st = nullptr;
    void* buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool ok = false, tried = false;
    int device = -1;                  // the stream's device: the calling thread's current device at first use
    // dev: the device the caller's allocations and launches go to; a process that later builds on another device keeps the host loop
    bool ready(int dev) {
        if (tried) return ok && dev == device;
        tried = true;
        device = dev;
        ok = hipSetDevice(dev) == hipSuccess && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
        for (int i = 0; i < 2 && ok; ++i)
            ok = hipHostMalloc(&buf[i], kBounceBytes, hipHostMallocDefault) == hipSuccess && hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        return ok;
    }
    bool up(void* dst, const void* src, size_t bytes, int threads) {
        int f = 0;
        for (size_t off = 0; off < bytes; off += kBounceBytes, f ^= 1) {
            const size_t len = std::min(kBounceBytes, bytes - off);
            if (hipEventSynchronize(ev[f]) != hipSuccess) return false;
            threaded_copy_bytes(buf[f], (const char*)src + off, len, threads);
            if (hipMemcpyAsync((char*)dst + off, buf[f], len, hipMemcpyHostToDevice, st) != hipSuccess || hipEventRecord(ev[f], st) != hipSuccess) return false;
        }
        return true;
    }
    bool down(void* dst, const void* src, size_t bytes, int threads) {
        const size_t nchunk = (bytes + kBounceBytes - 1) / kBounceBytes;
        auto issue = [&](size_t c) {
            const int f = (int)(c & 1);
            const size_t off = c * kBounceBytes, len = std::min(kBounceBytes, bytes - off);
            return hipMemcpyAsync(buf[f], (const char*)src + off, len, hipMemcpyDeviceToHost, st) == hipSuccess && hipEventRecord(ev[f], st) == hipSuccess;
        };
        if (hipEventSynchronize(ev[0]) != hipSuccess || hipEventSynchronize(ev[1]) != hipSuccess) return false;
        if (nchunk && !issue(0)) return false;
        for (size_t c = 0; c < nchunk; ++c) {
            if (c + 1 < nchunk && !issue(c + 1)) return false;
            const int f = (int)(c & 1);
            const size_t off = c * kBounceBytes, len = std::min(kBounceBytes, bytes - off);
            if (hipEventSynchronize(ev[f]) != hipSuccess) return false;
            threaded_copy_bytes((char*)dst + off, buf[f], len, threads);
        }
        return true;
    }
};
HierarchyXfer& hierarchy_xfer() { static HierarchyXfer* x = new HierarchyXfer(); return *x; }      // (leaked: no destruction order problems at exit)
}  // namespace

static bool hierarchy_select_on_device(const HierarchyOptions::SelectJob& j) {
    HierarchyXfer& X = hierarchy_xfer();
    std::lock_guard<std::mutex> lock(X.m);
    // (the builder runs this stage on a task thread: the device to use travels in the job)
    int dev = j.device;
    if ((dev < 0 && hipGetDevice(&dev) != hipSuccess) || hipSetDevice(dev) != hipSuccess || !X.ready(dev)) { (void)hipGetLastError(); return false; }
    const int threads = std::min(hw_threads(), 16);
    // one device allocation for the whole job, carved into 256-byte aligned pieces
    const size_t nf = (size_t)j.nf, nc = (size_t)j.nc;
    const size_t sizes[14] = {sizeof(double) * 3 * nf, sizeof(double) * 3 * nc, sizeof(int) * nf, j.nested ? sizeof(int) * nc : 0, sizeof(int) * (nc + 1),
                              sizeof(int) * (size_t)j.cadj_ptr[nc], sizeof(int) * 3 * (size_t)j.ntri, sizeof(int) * (nc + 1), sizeof(int) * (size_t)j.tof_ptr[nc],
                              sizeof(int) * nc * (size_t)j.Kc, nf, nf, sizeof(int) * 3 * nf, sizeof(double) * 3 * nf};
    size_t offs[15] = {0};
    for (int i = 0; i < 14; ++i) offs[i + 1] = offs[i] + (sizes[i] + 255) / 256 * 256;
    char* arena = nullptr;
    if (hipMalloc((void**)&arena, std::max<size_t>(offs[14], 256)) != hipSuccess) { (void)hipGetLastError(); return false; }
    const void* srcs[10] = {j.P, j.Pc, j.nearest, j.sample, j.cadj_ptr, j.cadj, j.tris, j.tof_ptr, j.tof, j.NBc};
    bool ok = true;
    for (int i = 0; i < 10 && ok; ++i) ok = sizes[i] == 0 || X.up(arena + offs[i], srcs[i], sizes[i], threads);
    if (ok) {
        hipLaunchKernelGGL(gmgh::select_parents, dim3((unsigned)((nf + 127) / 128)), dim3(128), 0, X.st, j.nf, j.Kc, j.weighting, j.nested,
                           (const double*)(arena + offs[0]), (const double*)(arena + offs[1]), (const int*)(arena + offs[2]), (const int*)(arena + offs[3]),
                           (const int*)(arena + offs[4]), (const int*)(arena + offs[5]), (const int*)(arena + offs[6]), (const int*)(arena + offs[7]),
                           (const int*)(arena + offs[8]), (const int*)(arena + offs[9]), (unsigned char*)(arena + offs[10]), (unsigned char*)(arena + offs[11]),
                           (int*)(arena + offs[12]), (double*)(arena + offs[13]));
        ok = hipGetLastError() == hipSuccess && X.down(j.cnt, arena + offs[10], nf, threads) && X.down(j.kind, arena + offs[11], nf, threads) &&
             X.down(j.col, arena + offs[12], sizeof(int) * 3 * nf, threads) && X.down(j.w, arena + offs[13], sizeof(double) * 3 * nf, threads);
    }
    (void)hipStreamSynchronize(X.st);          // nothing of this job may still be in flight when its buffers go
    (void)sync_hipFree(arena);
    if (!ok) (void)hipGetLastError();
    return ok;
}

int gmg_hierarchy_build(const double* pos, int n, const int* neigh, int K, const gmg_hierarchy_options* opt, gmg_hierarchy* out) try {
    if (!pos || !neigh || n <= 0 || K <= 0 || !out) return GMG_ERR_INVALID;
    gmg_hierarchy_options o;
    if (opt) o = *opt; else gmg_hierarchy_options_default(&o);
    if (o.sampling != 0) return GMG_ERR_UNSUPPORTED;      // only Sampling::FASTDISK (the default) is in scope
    if (o.weighting < 0 || o.weighting > 2 || !(o.ratio > 0)) return GMG_ERR_INVALID;
    for (size_t i = 0; i < (size_t)n * K; ++i) if (neigh[i] >= n) return GMG_ERR_INVALID;
    HierarchyOptions ho;
    ho.ratio = o.ratio; ho.lower_bound = o.lower_bound; ho.check_voronoi = o.check_voronoi != 0; ho.nested = o.nested != 0; ho.weighting = o.weighting; ho.keep_triangles = o.debug != 0; ho.full_clustering = o.full_clustering != 0;
    // the per-point selection stage runs on the GPU when there is one (same bits as the host loop; gmg_hierarchy_options::use_device = 0: host only)
    {
        int ndev = 0;
        if (o.use_device == 2) ho.device_select_min_points = 0;      // test setting: every level on the device, whatever its size
        if (o.use_device != 0 && n >= ho.device_select_min_points && hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) ho.device_select = hierarchy_select_on_device;
        else (void)hipGetLastError();
    }
    // first use in a process: runtime start-up, code object load and the pinned buffers (~80 ms) happen beside the sequential
    // sampling / clustering sweeps of the first level instead of in front of the device stage
    std::future<void> device_warm;
    int caller_device = 0;
    if (ho.device_select && hipGetDevice(&caller_device) != hipSuccess) { (void)hipGetLastError(); ho.device_select = nullptr; }
    ho.device = caller_device;
    if (ho.device_select)
        device_warm = std::async(std::launch::async, [caller_device] {
            HierarchyXfer& X = hierarchy_xfer();
            std::lock_guard<std::mutex> lock(X.m);
            if (hipSetDevice(caller_device) != hipSuccess || !X.ready(caller_device)) { (void)hipGetLastError(); return; }
            hipLaunchKernelGGL(gmgh::select_parents, dim3(1), dim3(128), 0, X.st, 0, 0, 0, 0, (const double*)nullptr, (const double*)nullptr, (const int*)nullptr,
                               (const int*)nullptr, (const int*)nullptr, (const int*)nullptr, (const int*)nullptr, (const int*)nullptr,
                               (const int*)nullptr, (const int*)nullptr, (unsigned char*)nullptr, (unsigned char*)nullptr, (int*)nullptr, (double*)nullptr);
            (void)hipStreamSynchronize(X.st);
            (void)hipGetLastError();
        });
    gmg_hierarchy hh = new gmg_hierarchy_s();
    // A breadth-first order of the points over `neigh`, for inputs whose numbering has no locality (randomly ordered scans, point
    // clouds): one of the two base orders gmg_set_system may give the finest level (choose_base_order).  A sequential sweep of the
    // whole graph (~60 ms at 3 M points) on its own thread, beside the construction.
    std::future<std::vector<int>> fine_order;
    if (n > 65536 && mean_index_distance_table(neigh, n, K) > std::max(32768.0, n / 32.0))
        fine_order = std::async(std::launch::async, [neigh, n, K] { return bfs_point_order(neigh, n, K); });
    // ... and the point graph as a canonical sparsity pattern: what gmg_use_hierarchy gives the engine to prepare its structure for
    std::future<std::shared_ptr<const FineGraph>> graph = std::async(std::launch::async, [neigh, n, K] {
        auto g = std::make_shared<FineGraph>();
        g->n = n;
        neigh_pattern(neigh, n, K, g->ptr, g->idx);
        return std::shared_ptr<const FineGraph>(g);
    });
    struct JoinGraph { std::future<std::shared_ptr<const FineGraph>>& f; ~JoinGraph() { if (f.valid()) f.wait(); } } join_graph{graph};      // (reads the caller's table: never outlives the call)
    hh->res = HierarchyBuilder::build(pos, n, neigh, K, ho);
    if (fine_order.valid()) hh->fine_order = fine_order.get();
    hh->graph = graph.get();
    if (device_warm.valid()) device_warm.get();
    *out = hh;
    return GMG_OK;
} GMG_CATCH_0

void gmg_hierarchy_destroy(gmg_hierarchy hh) { delete hh; }

int gmg_hierarchy_num_levels(gmg_hierarchy hh) { return hh ? (int)hh->res.U.size() : GMG_ERR_INVALID; }

int gmg_hierarchy_level_shape(gmg_hierarchy hh, int k, int* n_fine, int* n_coarse, int* nnz) try {
    if (!hh || k < 0 || k >= (int)hh->res.U.size()) return GMG_ERR_INVALID;
    const Compressed& u = hh->res.U[k];
    if (n_fine) *n_fine = u.n_inner;
    if (n_coarse) *n_coarse = u.n_outer;
    if (nnz) *nnz = u.nnz();
    return GMG_OK;
} GMG_CATCH_0

int gmg_hierarchy_get_prolongation(gmg_hierarchy hh, int k, int* colptr, int* rowidx, double* val) try {
    if (!hh || k < 0 || k >= (int)hh->res.U.size()) return GMG_ERR_INVALID;
    const Compressed& u = hh->res.U[k];
    // (threaded: the destinations are usually fresh arrays -- 108 MB of first touches at 3 M vertices)
    if (colptr) threaded_copy_bytes(colptr, u.ptr.data(), sizeof(int) * (size_t)(u.n_outer + 1), hw_threads());
    if (rowidx) threaded_copy_bytes(rowidx, u.idx.data(), sizeof(int) * (size_t)u.nnz(), hw_threads());
    if (val) threaded_copy_bytes(val, u.val.data(), sizeof(double) * (size_t)u.nnz(), hw_threads());
    return GMG_OK;
} GMG_CATCH_0

int gmg_hierarchy_get_timing(gmg_hierarchy hh, const char* key, double* out) try {
    if (!hh || !key || !out) return GMG_ERR_INVALID;
    auto it = hh->res.timing.find(key);
    if (it == hh->res.timing.end()) return GMG_ERR_INVALID;
    *out = it->second;
    return GMG_OK;
} GMG_CATCH_0

int gmg_hierarchy_get_samples(gmg_hierarchy hh, int k, int* out) try {
    if (!hh || !out || k < 0 || k >= (int)hh->res.samples.size()) return GMG_ERR_INVALID;
    std::memcpy(out, hh->res.samples[k].data(), sizeof(int) * hh->res.samples[k].size());
    return GMG_OK;
} GMG_CATCH_0

int gmg_hierarchy_get_nearest(gmg_hierarchy hh, int k, int* out) try {
    if (!hh || !out || k < 0 || k >= (int)hh->res.nearest.size()) return GMG_ERR_INVALID;
    threaded_copy_bytes(out, hh->res.nearest[k].data(), sizeof(int) * hh->res.nearest[k].size(), hw_threads());
    return GMG_OK;
} GMG_CATCH_0

int gmg_hierarchy_get_points(gmg_hierarchy hh, int k, double* out_xyz) try {
    if (!hh || !out_xyz || k < 0 || k >= (int)hh->res.points.size()) return GMG_ERR_INVALID;
    std::memcpy(out_xyz, hh->res.points[k].data(), sizeof(double) * hh->res.points[k].size());
    return GMG_OK;
} GMG_CATCH_0

int gmg_hierarchy_get_triangles(gmg_hierarchy hh, int k, int* out, int* count) try {
    if (!hh || !count || k < 0 || k >= (int)hh->res.U.size()) return GMG_ERR_INVALID;
    if (k >= (int)hh->res.triangles.size()) { *count = 0; return GMG_OK; }
    const auto& t = hh->res.triangles[k];
    *count = (int)t.size();
    if (out && !t.empty()) std::memcpy(out, t.data(), sizeof(int) * 3 * t.size());
    return GMG_OK;
} GMG_CATCH_0

int gmg_hierarchy_get_fine_order(gmg_hierarchy hh, int* out, int* count) try {
    if (!hh || !count) return GMG_ERR_INVALID;
    *count = (int)hh->fine_order.size();
    if (out && !hh->fine_order.empty()) std::memcpy(out, hh->fine_order.data(), sizeof(int) * hh->fine_order.size());
    return GMG_OK;
} GMG_CATCH_0

int gmg_hierarchy_debug_row_kinds(gmg_hierarchy hh, int k, int* out) try {
    if (!hh || !out || k < 0 || k >= (int)hh->res.row_kinds.size()) return GMG_ERR_INVALID;
    for (int z = 0; z < 4; ++z) out[z] = hh->res.row_kinds[k][z];
    return GMG_OK;
} GMG_CATCH_0

// Test access to the per-point parent selection of one level (gravomg_hip_internal.h): the host routine, the device stage through
// hierarchy_select_on_device -- the builder's own upload / launch / download -- or the builder's combination of the two.
int gmg_debug_select_parents(int nf, int nc, int Kc, int ntri, int weighting, int nested, const double* P, const double* Pc, const int* nearest,
                             const int* sample, const int* cadj_ptr, const int* cadj, const int* tris, const int* tof_ptr, const int* tof,
                             const int* NBc, int mode, unsigned char* cnt, unsigned char* kind, int* col, double* w) try {
    if (nf <= 0 || nc <= 0 || Kc <= 0 || ntri < 0 || weighting < 0 || weighting > 2 || mode < 0 || mode > 2) return GMG_ERR_INVALID;
    if (!P || !Pc || !nearest || !sample || !cadj_ptr || !cadj || !tris || !tof_ptr || !tof || !NBc || !cnt || !kind || !col || !w) return GMG_ERR_INVALID;
    // every index the selection follows, checked once: the device stage reads without bounds
    if (cadj_ptr[0] != 0 || tof_ptr[0] != 0) return GMG_ERR_INVALID;
    for (int c = 0; c < nc; ++c) if (cadj_ptr[c + 1] < cadj_ptr[c] || tof_ptr[c + 1] < tof_ptr[c]) return GMG_ERR_INVALID;
    for (int f = 0; f < nf; ++f) if (nearest[f] < 0 || nearest[f] >= nc) return GMG_ERR_INVALID;
    for (int q = 0; q < cadj_ptr[nc]; ++q) if (cadj[q] < 0 || cadj[q] >= nc) return GMG_ERR_INVALID;
    for (size_t q = 0; q < 3 * (size_t)ntri; ++q) if (tris[q] < 0 || tris[q] >= nc) return GMG_ERR_INVALID;
    for (size_t q = 0; q < (size_t)nc * Kc; ++q) if (NBc[q] >= nc) return GMG_ERR_INVALID;
    for (int c = 0; c < nc; ++c)
        for (int q = tof_ptr[c]; q < tof_ptr[c + 1]; ++q) {        // (the rotation to c only ends when c is a corner)
            if (tof[q] < 0 || tof[q] >= ntri) return GMG_ERR_INVALID;
            const int* t = tris + 3 * (size_t)tof[q];
            if (t[0] != c && t[1] != c && t[2] != c) return GMG_ERR_INVALID;
        }
    HierarchyOptions::SelectJob j;
    j.nf = nf; j.nc = nc; j.Kc = Kc; j.ntri = ntri; j.weighting = weighting; j.nested = nested ? 1 : 0;
    j.P = P; j.Pc = Pc; j.nearest = nearest; j.sample = sample; j.cadj_ptr = cadj_ptr; j.cadj = cadj; j.tris = tris;
    j.tof_ptr = tof_ptr; j.tof = tof; j.NBc = NBc; j.cnt = cnt; j.kind = kind; j.col = col; j.w = w;
    if (mode == 0) { HierarchyBuilder::select_job_on_host(j, false); return GMG_OK; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return GMG_ERR_NO_DEVICE; }
    if (!hierarchy_select_on_device(j)) return GMG_ERR_HIP;      // the stage declined: no silent host rows here
    if (mode == 2) HierarchyBuilder::select_job_on_host(j, true);
    return GMG_OK;
} GMG_CATCH_0

int gmg_set_fine_order(gmg_handle h, int n, const int* order) try {
    if (!h || n < 0 || (n > 0 && !order)) return GMG_ERR_INVALID;
    if (n > 0) {
        if (h->L <= 0 || !h->U_set[0] || h->U[0].n_inner != n) return fail(h, GMG_ERR_STATE, "set the prolongations first: the order must have one entry per level-0 point");
        std::vector<unsigned char> seen((size_t)n, 0);
        for (int i = 0; i < n; ++i) {
            if (order[i] < 0 || order[i] >= n || seen[order[i]]) return fail(h, GMG_ERR_INVALID, "the fine order is not a permutation of the level-0 points");
            seen[order[i]] = 1;
        }
    }
    PoolScope pool_scope_(&h->pool);
    h->bfs_order.assign(order, order + n);
    h->d_bfs_order = {}; h->d_bfs_inv = {};
    h->ord_cache_valid = false;        // cached orderings were built on another base order
    return GMG_OK;
} GMG_CATCH_H

int gmg_set_fine_graph(gmg_handle h, int n, int K, const int* neigh) try {
    if (!h || n < 0 || (n > 0 && (K <= 0 || !neigh))) return GMG_ERR_INVALID;
    if (n == 0) { h->fine_graph.reset(); return GMG_OK; }
    if (h->L <= 0 || !h->U_set[0] || h->U[0].n_inner != n) return fail(h, GMG_ERR_STATE, "set the prolongations first: the graph must have one row per level-0 point");
    {
        std::atomic<bool> bad{false};
        parallel_ranges(n, h->cfg.host_threads, [&](int lo, int hi, int) { for (size_t i = (size_t)lo * K; i < (size_t)hi * K; ++i) if (neigh[i] >= n) { bad = true; return; } }, 1 << 14);
        if (bad) return fail(h, GMG_ERR_INVALID, "neighbour index out of range");
    }
    auto g = std::make_shared<FineGraph>();
    g->n = n;
    neigh_pattern(neigh, n, K, g->ptr, g->idx);
    h->fine_graph = g;
    return GMG_OK;
} GMG_CATCH_H

int gmg_use_hierarchy(gmg_handle h, gmg_hierarchy hh) try {
    if (!h || !hh) return GMG_ERR_INVALID;
    int rc = gmg_set_num_levels(h, (int)hh->res.U.size());
    if (rc) return rc;
    for (int k = 0; k < (int)hh->res.U.size(); ++k) {
        const Compressed& u = hh->res.U[k];
        if ((rc = gmg_set_prolongation(h, k, u.n_inner, u.n_outer, u.ptr.data(), u.idx.data(), u.val.data()))) return rc;
    }
    if (!hh->res.U.empty() && (rc = gmg_set_fine_order(h, (int)hh->fine_order.size(), hh->fine_order.data()))) return rc;
    if (!hh->res.U.empty() && hh->graph && hh->graph->n == hh->res.U[0].n_inner) h->fine_graph = hh->graph;      // (shared, read-only: no copy)
    return gmg_finalize_hierarchy(h);
} GMG_CATCH_H

int gmg_finalize_hierarchy(gmg_handle h) try {
    if (!h) return GMG_ERR_INVALID;
    if (h->L <= 0) return fail(h, GMG_ERR_STATE, "no hierarchy set");
    for (int k = 0; k < h->L; ++k) if (!h->U_set[k]) return fail(h, GMG_ERR_STATE, "prolongation matrix missing for level " + std::to_string(k));
    if (!h->has_device) return GMG_OK;
    PoolScope pool_scope_(&h->pool);      // (everything below allocates and releases through the handle's pool: its byte counts are what gmg_p2p_stat reports)
    // data that belongs to the hierarchy, not to a system (gmg_set_system would make it on its first call otherwise):
    // the compact patches of the blocked levels, the device copies of U_k
    // (the patches are host work on helper threads, the transfers device work driven from this thread: side by side)
    std::future<void> patches;
    if (!h->patches_ready) patches = std::async(std::launch::async, [h] { build_patches(h); });
    int rc = GMG_OK;
    if (h->cfg.device_setup) {
        rc = hipSetDevice(h->cfg.device) == hipSuccess ? ensure_device_transfers(h) : fail(h, GMG_ERR_HIP, "hipSetDevice failed");
    }
    if (patches.valid()) patches.get();
    // with the point graph at hand: everything structural for the systems to come, on placeholder values (prepare_structure)
    if (rc == GMG_OK && h->cfg.prepare_structure && h->cfg.device_setup && h->cfg.device_rap && h->fine_graph && h->fine_graph->n == h->U[0].n_inner &&
        h->live == LiveSystem::none) {
        // (an optional preparation: should it fail -- device memory, a graph the device builders cannot take -- the handle is left as a handle
        // without a system and the first gmg_set_system pays for its structure; the reason stays readable through "structure_prepare_failed")
        const int prc = prepare_structure(h);
        h->timing["structure_prepare_failed"] = prc == GMG_OK ? 0.0 : 1.0;
        if (prc != GMG_OK) { drop_system(h); h->live_key_valid = false; }
        h->fine_graph.reset();      // the digest of the prepared pattern is all that is needed from here on
    }
    return rc;
} GMG_CATCH_H

int gmg_host_galerkin(int n, const int* a_colptr, const int* a_rowidx, const double* a_val, int n_coarse, const int* u_colptr,
                      const int* u_rowidx, const double* u_val, int* c_colptr, int* c_rowidx, double* c_val) try {
    if (n <= 0 || n_coarse <= 0 || !a_colptr || !a_rowidx || !a_val || !u_colptr || !u_rowidx || !u_val || !c_colptr) return GMG_ERR_INVALID;
    Compressed A, U;
    A.assign(n, n, a_colptr, a_rowidx, a_val);
    U.assign(n_coarse, n, u_colptr, u_rowidx, u_val);
    Compressed C = galerkin_rap(A, U, hw_threads());
    std::memcpy(c_colptr, C.ptr.data(), sizeof(int) * (n_coarse + 1));
    if (c_rowidx) std::memcpy(c_rowidx, C.idx.data(), sizeof(int) * C.nnz());
    if (c_val) std::memcpy(c_val, C.val.data(), sizeof(double) * C.nnz());
    return GMG_OK;
} GMG_CATCH_0

// Test access to the device Galerkin product (gravomg_hip_internal.h): the set-up's own upload_csr_raw / build_ell3 / device_rap on local
// DevCsr / DevEll3 objects.  Nothing is launched from here, and of the handle only the stream, the pool and the bounce buffers are used.
int gmg_debug_device_galerkin(gmg_handle h, int n, const int* a_colptr, const int* a_rowidx, const double* a_val, const double* a_val2, int n_coarse,
                              const int* u_colptr, const int* u_rowidx, const double* u_val, int64_t cap, int* c_colptr, int* c_rowidx, double* c_val,
                              double* c_val2, int* status) try {
    NEED_DEVICE();
    if (n <= 0 || n_coarse <= 0 || cap < 0 || !a_colptr || !a_rowidx || !a_val || !u_colptr || !u_rowidx || !u_val || !c_colptr || !c_rowidx || !c_val || !status ||
        (a_val2 && !c_val2)) return fail(h, GMG_ERR_INVALID, "bad arguments");
    // every index the kernels follow, checked once: they read without bounds
    if (a_colptr[0] != 0 || u_colptr[0] != 0) return fail(h, GMG_ERR_INVALID, "column pointers must start at 0");
    for (int i = 0; i < n; ++i) if (a_colptr[i + 1] < a_colptr[i]) return fail(h, GMG_ERR_INVALID, "column pointers of A decrease");
    for (int c = 0; c < n_coarse; ++c) if (u_colptr[c + 1] < u_colptr[c]) return fail(h, GMG_ERR_INVALID, "column pointers of U decrease");
    for (int q = 0; q < a_colptr[n]; ++q) if (a_rowidx[q] < 0 || a_rowidx[q] >= n) return fail(h, GMG_ERR_INVALID, "row index of A out of range");
    for (int q = 0; q < u_colptr[n_coarse]; ++q) if (u_rowidx[q] < 0 || u_rowidx[q] >= n) return fail(h, GMG_ERR_INVALID, "row index of U out of range");
    if (hipSetDevice(h->cfg.device) != hipSuccess) return fail(h, GMG_ERR_HIP, "hipSetDevice failed");
    DevCsr dA, dU, dC;
    DevEll3 e3;
    DevBuf<int> d_err;
    Compressed C;
    int rc, herr = 0;
    if ((rc = dev_alloc(h, d_err, 1))) return rc;
    HIPCHK(hipMemsetAsync(d_err, 0, sizeof(int), h->stream));
    if ((rc = upload_csr_raw(h, dA, n, a_colptr, a_rowidx, a_val)) || (rc = upload_csr_raw(h, dU, n_coarse, u_colptr, u_rowidx, u_val)) ||
        (rc = build_ell3(h, e3, dU, n, d_err))) { (void)hipStreamSynchronize(h->stream); return rc; }
    HIPCHK(hipMemcpyAsync(&herr, d_err, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));      // the caller's arrays have been consumed
    *status = 0;
    if (herr) { *status = 1; return GMG_OK; }     // a U row with more than 3 entries (ensure_device_transfers: dU_flagged): rap_rows is not launched
    int64_t nnz = 0;
    rc = device_rap(h, dA, dU, e3, dC, C, true, true, &nnz, d_err);
    if (rc == 1) { *status = 1; return GMG_OK; }  // a coarse row overflows the hash set: the set-up goes on with the host product
    if (rc) return rc;
    std::memcpy(c_colptr, C.ptr.data(), sizeof(int) * ((size_t)n_coarse + 1));
    if (nnz > cap) return fail(h, GMG_ERR_INVALID, "the product has " + std::to_string(nnz) + " entries: more than the caller's capacity (c_colptr is filled)");
    if (nnz) { std::memcpy(c_rowidx, C.idx.data(), sizeof(int) * (size_t)nnz); std::memcpy(c_val, C.val.data(), sizeof(double) * (size_t)nnz); }
    if (a_val2) {
        // the values-only refresh: new values into the resident A, the numeric pass alone on the pattern at hand (refresh_system_values)
        Compressed C2;
        if ((rc = h2d(h, dA.val, a_val2, sizeof(double) * (size_t)a_colptr[n]))) { (void)hipStreamSynchronize(h->stream); return rc; }
        rc = device_rap(h, dA, dU, e3, dC, C2, false, true, &nnz, d_err, true);
        HIPCHK(hipStreamSynchronize(h->stream));
        if (rc) return rc < 0 ? rc : fail(h, GMG_ERR_STATE, "the numeric pass declined a pattern the product was made on");
        if ((int64_t)C2.val.size() != nnz) return fail(h, GMG_ERR_STATE, "the numeric pass returned another number of entries");
        if (nnz) std::memcpy(c_val2, C2.val.data(), sizeof(double) * (size_t)nnz);
    }
    return GMG_OK;
} GMG_CATCH_H

// Test access to the colouring of gmg_config::device_coloring (gravomg_hip_internal.h): the specification on the host, and the set-up's own
// device_jp_coloring on a pattern of the caller's.  Of the handle only the stream, the pool and the bounce buffers are used.
static bool jp_pattern_ok(int n, const int* colptr, const int* rowidx) {
    if (n <= 0 || !colptr || !rowidx || colptr[0] != 0) return false;
    for (int i = 0; i < n; ++i) if (colptr[i + 1] < colptr[i]) return false;
    for (int q = 0; q < colptr[n]; ++q) if (rowidx[q] < 0 || rowidx[q] >= n) return false;      // every index the kernels and the host loop follow
    return true;
}
int gmg_jp_coloring_host(int n, const int* colptr, const int* rowidx, unsigned char* colours, int* n_colors, int* rounds) try {
    if (!colours || !n_colors || !rounds || !jp_pattern_ok(n, colptr, rowidx)) return GMG_ERR_INVALID;
    RawVec<unsigned char> c8;
    *n_colors = jp_coloring_host(PatternView{n, colptr, rowidx}, c8, rounds);
    if (*n_colors >= 0) std::memcpy(colours, c8.data(), (size_t)n);
    return GMG_OK;
} GMG_CATCH_0

int gmg_jp_coloring_device(gmg_handle h, int n, const int* colptr, const int* rowidx, unsigned char* colours, int* n_colors, int* rounds) try {
    NEED_DEVICE();
    if (!colours || !n_colors || !rounds || !jp_pattern_ok(n, colptr, rowidx)) return fail(h, GMG_ERR_INVALID, "bad arguments");
    if (hipSetDevice(h->cfg.device) != hipSuccess) return fail(h, GMG_ERR_HIP, "hipSetDevice failed");
    DevBuf<int> d_ptr, d_idx;
    DevBuf<unsigned char> d_c8;
    const size_t nnz = (size_t)colptr[n];
    int rc;
    if ((rc = dev_alloc(h, d_ptr, (size_t)n + 1)) || (rc = dev_alloc(h, d_idx, nnz)) || (rc = h2d(h, d_ptr, colptr, sizeof(int) * ((size_t)n + 1))) ||
        (nnz && (rc = h2d(h, d_idx, rowidx, sizeof(int) * nnz))) || (rc = device_jp_coloring(h, d_ptr, d_idx, n, d_c8, n_colors, rounds))) {
        (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    if (*n_colors >= 0 && (rc = d2h(h, colours, d_c8, (size_t)n))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return GMG_OK;
} GMG_CATCH_H

// Test access to the device-built coarse inverse (gravomg_hip_internal.h): the set-up's own factorisation, export and coarse_inverse_core on a
// caller's matrix, into local DevBufs.  Of the handle only the stream, the pool, the bounce buffers and the scratch events are used.
int gmg_debug_coarse_inverse(gmg_handle h, int n, const int* colptr, const int* rowidx, const double* val, int width, int mode, double* out, int64_t out_cap,
                             int64_t* info, int* perm, int* q_col0, int* q_w, int* q_rptr, int* rows, double* vals, double* tri, double* dinv, int* lev_ptr,
                             int* lev_q, int* lev_big, int* tile_ptr, int* tile_q) try {
    if (n <= 0 || !colptr || !rowidx || !val || !info || mode < 0 || mode > 4 || (width != 0 && width != 16 && width != 32 && width != 64) || out_cap < 0)
        return fail(h, GMG_ERR_INVALID, "bad arguments");
    if (mode != 0) {
        if (!h) return GMG_ERR_INVALID;
        if (!h->has_device) return fail(h, GMG_ERR_NO_DEVICE, "no usable HIP device (libgravomg_hip has no CPU fallback)");
    }
    if (colptr[0] != 0) return fail(h, GMG_ERR_INVALID, "column pointers must start at 0");
    for (int i = 0; i < n; ++i) if (colptr[i + 1] < colptr[i]) return fail(h, GMG_ERR_INVALID, "column pointers decrease");
    for (int q = 0; q < colptr[n]; ++q) if (rowidx[q] < 0 || rowidx[q] >= n) return fail(h, GMG_ERR_INVALID, "row index out of range");
    Compressed A;
    A.assign(n, n, colptr, rowidx, val);
    SupernodalLDLT f;
    if (!f.factor(A)) return fail(h, GMG_ERR_NUMERIC, "the matrix is not positive definite");
    SupernodalLDLT::DeviceFactor E;
    f.export_device_factor(E);
    const int w = width ? width : coarse_inverse_width(n);
    std::vector<int> tile_ptr_h, tile_q_h;
    E.tile_paths(w, tile_ptr_h, tile_q_h);
    const std::vector<int> lev_big_h = E.big_per_level(gmgs::kInvBigRows);
    const int lda = (n + 7) / 8 * 8, nb = tri_blocks(n);
    long long shape[10];
    E.shape_info(w, gmgs::kInvBigRows, shape);
    for (int k = 0; k < 10; ++k) info[k] = shape[k];
    info[10] = (int64_t)E.rows.size();
    info[11] = (int64_t)tile_q_h.size();
    info[12] = mode == 4 ? (int64_t)tri_block_count(nb) * kTriBlockDoubles : (mode == 2 || mode == 3) ? (int64_t)n * lda : (int64_t)n * n;
    info[13] = (mode == 2 || mode == 3) ? lda : (mode == 4 ? 64 : n);
    info[14] = gmgs::kInvBigRows;
    info[15] = gmgs::kInvWaves;
    auto give = [](auto* dst, const auto& src) { if (dst && !src.empty()) std::memcpy(dst, src.data(), sizeof(src[0]) * src.size()); };
    give(perm, E.perm); give(q_col0, E.q_col0); give(q_w, E.q_w); give(q_rptr, E.q_rptr); give(rows, E.rows); give(vals, E.vals); give(tri, E.tri);
    give(dinv, E.dinv); give(lev_ptr, E.lev_ptr); give(lev_q, E.lev_q); give(lev_big, lev_big_h); give(tile_ptr, tile_ptr_h); give(tile_q, tile_q_h);
    if (!out) return GMG_OK;                                 // the sizing call
    if (out_cap < info[12]) return fail(h, GMG_ERR_INVALID, "the output needs " + std::to_string(info[12]) + " doubles");
    if (mode == 0) {
        // the host's restatement of the kernel's schedule, every column: rows j >= c of column c, the other triangle left zero
        std::vector<double> col((size_t)n);
        std::fill(out, out + (size_t)n * n, 0.0);
        for (int c = 0; c < n; ++c) {
            SupernodalLDLT::emulate_device_column(E, c, col.data());
            for (int j = c; j < n; ++j) out[(size_t)j * n + c] = col[(size_t)j];
        }
        return GMG_OK;
    }
    PoolScope pool_scope_(&h->pool);
    if (hipSetDevice(h->cfg.device) != hipSuccess) return fail(h, GMG_ERR_HIP, "hipSetDevice failed");
    DevBuf<double> X, dst;
    CoarseInverseRun run;
    int rc;
    const int follow = mode == 1 ? kInvFollowMirror : mode == 2 ? kInvFollowPermute : mode == 3 ? kInvFollowScatter : kInvFollowTriangle;
    if (mode == 2 && n > kInvPermuteLdsMax) return fail(h, GMG_ERR_INVALID, "rows of this length do not fit the LDS: mode 3");
    // (as in the set-up the destination is not cleared: columns n .. lda - 1 of the full inverse are never written and mean nothing)
    if (mode != 1 && (rc = dev_alloc(h, dst, (size_t)info[12]))) return rc;
    if ((rc = coarse_inverse_core(h, E, w, follow, X, dst.get(), lda, run))) { (void)hipStreamSynchronize(h->stream); return rc; }
    return d2h(h, out, mode == 1 ? X.get() : dst.get(), sizeof(double) * (size_t)info[12]);
} GMG_CATCH_H

int gmg_host_plan_level(int n, const int* colptr, const int* rowidx, const double* val, int mode, int block_rows, int sigma, int64_t* info,
                        int* new2old, int* color_begin, int* blk_begin, unsigned char* row_color) try {
    if (n <= 0 || !colptr || !rowidx || !val || mode < 0 || mode > 4) return GMG_ERR_INVALID;
    if (mode == 1 && (block_rows <= 0 || block_rows > gmgk::kBlockRows || block_rows % 64)) return GMG_ERR_INVALID;
    if (sigma < 0 || sigma % 64) return GMG_ERR_INVALID;
    if (mode == 4) {
        // the colouring that a cold gmg_set_system starts ahead of its inspection, on the caller's arrays as they are (greedy_coloring_ahead): -2 is reported
        // as GMG_ERR_INVALID (arrays that would take a reader out of bounds), a result goes through make_ordering like the one made after the inspection
        PreColoring pre;
        std::atomic<int> stop{0};
        pre.n_colors = greedy_coloring_ahead(n, colptr, rowidx, (int64_t)colptr[n], pre.c8, stop);
        if (pre.n_colors == -2) return GMG_ERR_INVALID;
        if (info) info[5] = pre.n_colors >= 0 ? 1 : 0;
        LevelOrdering o = make_ordering(PatternView{n, colptr, rowidx}, true, (block_rows > 0 && block_rows % 64 == 0) ? block_rows : 64, sigma, 0, nullptr, true, &pre);
        if (o.n_colors > kMaxColors) return GMG_ERR_UNSUPPORTED;
        if (info) { info[0] = o.n_pad; info[1] = o.n_colors; info[2] = 0; info[3] = 0; info[4] = 0; }
        if (new2old) std::memcpy(new2old, o.new2old.data(), sizeof(int) * o.n_pad);
        if (color_begin) std::memcpy(color_begin, o.color_begin.data(), sizeof(int) * (o.n_colors + 1));
        return GMG_OK;
    }
    Compressed A;
    A.assign(n, n, colptr, rowidx, val);
    // (mode 2: colour-major with the locality reordering forced -- the colouring then walks a visit ORDER; mode 3: colour-major, row indices declared ascending)
    LevelOrdering o = mode == 1 ? make_block_ordering(A, block_rows)
                                : make_ordering(A, true, (block_rows > 0 && block_rows % 64 == 0) ? block_rows : 64, sigma, mode == 2 ? 1 : 0, nullptr, mode == 3);
    if (o.n_colors > kMaxColors) return GMG_ERR_UNSUPPORTED;
    SellHost sa; std::vector<double> dg; std::string e;
    if (!build_operator_sell(A, o, 0, sa, dg, e)) return GMG_ERR_NUMERIC;
    if (info) { info[0] = o.n_pad; info[1] = o.n_colors; info[2] = o.n_blocks(); info[3] = sa.stored(); info[4] = sa.nnz_real; info[5] = 0; }
    if (new2old) std::memcpy(new2old, o.new2old.data(), sizeof(int) * o.n_pad);
    if (color_begin && !o.blocked) std::memcpy(color_begin, o.color_begin.data(), sizeof(int) * (o.n_colors + 1));
    if (blk_begin && o.blocked) std::memcpy(blk_begin, o.blk_begin.data(), sizeof(int) * o.blk_begin.size());
    if (row_color && o.blocked) std::memcpy(row_color, o.row_color.data(), o.row_color.size());
    return GMG_OK;
} GMG_CATCH_0

// set-up fault injection for the tests (gravomg_hip_internal.h)
int gmg_debug_set(gmg_handle h, const char* key, double value) try {
    if (!h || !key) return GMG_ERR_INVALID;
    if (std::string(key) == "col16_uncovered") { h->dbg_col16_uncovered = (int)value; return GMG_OK; }
    if (std::string(key) == "cheby_ratio") {
        if (value != 0.0 && !cheby_ratio_usable(value)) return fail(h, GMG_ERR_INVALID, "cheby_ratio must be > 1 (0: the process-wide ratio)");
        h->dbg_cheby_ratio = value;
        if (h->has_device) drop_graphs(h);                                         // (the coefficients are arguments of the captured launches)
        if (h->timing.count("cheby_ratio")) h->timing["cheby_ratio"] = cheby_ratio(h);
        return GMG_OK;
    }
    return fail(h, GMG_ERR_INVALID, std::string("unknown debug key: ") + key);
} GMG_CATCH_H

int gmg_host_fine_block_rule(int n, const int* colptr, const int* rowidx, const double* val, int* blocked, int* reason) try {
    if (n <= 0 || !colptr || !rowidx || !val || !blocked) return GMG_ERR_INVALID;
    int why = 0;
    if ((double)colptr[n] < kFineBlockMinRow * (double)n) why = 1;
    else if (!stieltjes_signs(n, colptr, rowidx, val, hw_threads())) why = 2;
    *blocked = why == 0 ? 1 : 0;
    if (reason) *reason = why;
    return GMG_OK;
} GMG_CATCH_0

int gmg_host_ldlt_solve(int n, const int* colptr, const int* rowidx, const double* val, const double* b, int d, double* x, int64_t* factor_nnz) try {
    if (n <= 0 || !colptr || !rowidx || !val || !b || !x || d <= 0) return GMG_ERR_INVALID;
    Compressed A;
    A.assign(n, n, colptr, rowidx, val);
    // the engine's coarsest-level solver (supernodal), cross-checked here against the simplicial implementation it replaced
    SupernodalLDLT f;
    if (!f.factor(A)) return GMG_ERR_NUMERIC;
    std::vector<double> w((size_t)n * d);
    f.solve_multi(b, (size_t)n, x, (size_t)n, d, w.data());
    if (factor_nnz) *factor_nnz = f.factor_nnz();
    return GMG_OK;
} GMG_CATCH_0

// Host-only views of gmg_config::nullspace = 1 (gravomg_hip_internal.h): the set-up's row-sum rule, and the pinned factor between two mean removals
static int csc_fault(int n, const int* colptr, const int* rowidx) {
    if (colptr[0] != 0) return 1;
    for (int i = 0; i < n; ++i) if (colptr[i + 1] < colptr[i]) return 1;
    for (int q = 0; q < colptr[n]; ++q) if (rowidx[q] < 0 || rowidx[q] >= n) return 1;
    return 0;
}
int gmg_host_nullspace_rowsum(int n, const int* colptr, const int* rowidx, const double* val, int coarsest, double* rowsum) try {
    if (n <= 0 || !colptr || !rowidx || !val || csc_fault(n, colptr, rowidx)) return GMG_ERR_INVALID;
    Compressed A;
    A.assign(n, n, colptr, rowidx, val);
    const double worst = nullspace_rowsum(A);
    if (rowsum) *rowsum = worst;
    if (worst <= kNullspaceRowsumMax) return GMG_OK;
    return coarsest ? GMG_ERR_NUMERIC : GMG_ERR_INVALID;
} GMG_CATCH_0

int gmg_host_pinv_solve(int n, const int* colptr, const int* rowidx, const double* val, const double* b, int d, double* x, double* info) try {
    if (n <= 0 || !colptr || !rowidx || !val || !b || !x || d <= 0 || csc_fault(n, colptr, rowidx)) return GMG_ERR_INVALID;
    Compressed A;
    A.assign(n, n, colptr, rowidx, val);
    const double worst = nullspace_rowsum(A);
    if (info) { info[0] = worst; info[1] = 0.0; }
    if (!(worst <= kNullspaceRowsumMax)) return GMG_ERR_NUMERIC;
    SupernodalLDLT f;
    f.pin_last = true;
    if (!f.factor(A)) return GMG_ERR_NUMERIC;
    if (info) info[1] = f.pinned_pivot;
    std::vector<double> rhs(b, b + (size_t)n * d), w((size_t)n * d);
    remove_means(rhs.data(), (size_t)n, n, d);
    f.solve_multi(rhs.data(), (size_t)n, x, (size_t)n, d, w.data());
    remove_means(x, (size_t)n, n, d);
    return GMG_OK;
} GMG_CATCH_0

// Measurement / cross-check aid of the coarsest-level solver (gravomg_hip_internal.h; tests/test_host.py, scripts/ldlt_bench.py): factorises A,
// times the back-substitution on 1 .. 8 threads (`reps` solves per batch, best of 20 batches) and the numeric re-factorisation, compares the
// team solves with the one-thread solve bit for bit and the supernodal factor with the simplicial one, and writes the report (text lines) into
// `report` (cap bytes, NUL-terminated, truncated if need be).
int gmg_host_ldlt_probe(int n, const int* colptr, const int* rowidx, const double* val, const double* b, int reps, char* report, int cap) try {
    if (n <= 0 || !colptr || !rowidx || !val || !b || !report || cap <= 0) return GMG_ERR_INVALID;
    reps = std::max(1, reps);
    Compressed A;
    A.assign(n, n, colptr, rowidx, val);
    SupernodalLDLT f;
    if (!f.factor(A)) return GMG_ERR_NUMERIC;
    std::vector<double> w((size_t)n * 3), x((size_t)n);
    f.solve_multi(b, (size_t)n, x.data(), (size_t)n, 1, w.data());
    std::string text;
    auto say = [&](const char* fmt, auto... args) { char line[1024]; std::snprintf(line, sizeof(line), fmt, args...); text += line; };
    {
        std::vector<double> xb((size_t)n);
        double best = 1e30;
        for (int batch = 0; batch < 20; ++batch) {                     // minimum over batches: the host may be shared
            auto t0 = clk::now();
            for (int i = 0; i < reps; ++i) f.solve_multi(b, (size_t)n, xb.data(), (size_t)n, 1, w.data());
            best = std::min(best, 1e3 * ms_since(t0) / reps);
        }
        say("factorisation: ordering %.2f ms, symbolic %.2f ms, numeric %.2f ms\n", f.phase_ms[0], f.phase_ms[1], f.phase_ms[2]);
        {   // numeric re-factorisation (a system with the same sparsity pattern: the demos' new tau per frame), best and median of 15
            std::vector<double> ts;
            for (int i = 0; i < 15; ++i) { if (!f.factor(A, true)) return GMG_ERR_NUMERIC; ts.push_back(f.phase_ms[2]); }
            std::sort(ts.begin(), ts.end());
            say("numeric re-factorisation on %d thread(s): best %.2f ms, median %.2f ms\n", SupernodalLDLT::numeric_threads(), ts.front(), ts[ts.size() / 2]);
        }
        {   // the factor as the device reads it (export_device_factor) and the device kernel's schedule, on the host: some columns of the inverse by the
            // chunk algorithm against the back-substitution of the same unit vectors
            SupernodalLDLT::DeviceFactor E;
            f.export_device_factor(E);
            std::vector<double> col((size_t)n), e((size_t)n, 0.0), ref((size_t)n), wk((size_t)n);
            double worst = 0.0, scale = 0.0;
            const int picks = std::min(n, 24);
            for (int t = 0; t < picks; ++t) {
                const int c = (int)((long)t * (n - 1) / std::max(picks - 1, 1));          // factor numbering, spread from the first leaf to the root
                SupernodalLDLT::emulate_device_column(E, c, col.data());
                e[(size_t)f.perm[(size_t)c]] = 1.0;
                f.solve(e.data(), ref.data(), wk.data());
                e[(size_t)f.perm[(size_t)c]] = 0.0;
                for (int j = c; j < n; ++j) { worst = std::max(worst, std::fabs(col[(size_t)j] - ref[(size_t)f.perm[(size_t)j]])); scale = std::max(scale, std::fabs(ref[(size_t)f.perm[(size_t)j]])); }
            }
            say("device factor layout: %d chunks of <= %d columns in %d levels; %d columns of the inverse by the chunk algorithm vs back-substitution: max |difference| %.3e of max |entry| %.3e\n",
                E.nq, SupernodalLDLT::kChunk, E.nlev, picks, worst, scale);
        }
        long part[3];
        f.split_report(part);
        say("n=%d nnz(L)=%ld: %.2f us per single-column solve on one thread (best of 20 batches of %d); %d parts of the elimination "
                     "tree, panel entries in the lightest / heaviest part / above them: %ld / %ld / %ld\n", n, f.factor_nnz(), best, reps, f.parts(), part[0], part[1], part[2]);
        for (int threads = 2; threads <= std::min(8, f.parts()); threads += threads < 4 ? 1 : 2) {
            double best2 = 1e30, diff = 0.0;
            SpinTeam team(threads - 1);
            team.arm();
            std::vector<double> x2((size_t)n);
            for (int batch = 0; batch < 20; ++batch) {
                auto t0 = clk::now();
                for (int i = 0; i < reps; ++i) f.solve_multi(b, (size_t)n, x2.data(), (size_t)n, 1, w.data(), &team);
                best2 = std::min(best2, 1e3 * ms_since(t0) / reps);
            }
            team.disarm();
            for (int i = 0; i < n; ++i) diff = std::max(diff, std::fabs(x2[i] - xb[i]));
            double ph[6];
            team.arm();
            f.profile(b, w.data(), &team, reps, ph);
            team.disarm();
            say("%d threads: %.2f us per solve; max |difference| to the one-thread solve %.1e  (phases: parts down %.1f, top down %.1f, top up %.1f, "
                         "parts up %.1f us; %d top supernodes in %d chains)\n", threads, best2, diff, ph[0], ph[1], ph[2], ph[3], (int)ph[4], (int)ph[5]);
        }
        {   // three right-hand sides (the demos' n x 3 call) on the team of a V-cycle solve, against three single-column solves
            const int threads = std::min(8, std::max(2, std::min(f.parts() * 3, hw_threads() - 1)));
            SpinTeam team(threads - 1);
            team.arm();
            std::vector<double> b3((size_t)n * 3), x3((size_t)n * 3), w3((size_t)n * 3), x1((size_t)n);
            for (int c = 0; c < 3; ++c) for (int i = 0; i < n; ++i) b3[(size_t)c * n + i] = b[i] * (c + 1);
            double best3 = 1e30, diff3 = 0.0;
            for (int batch = 0; batch < 20; ++batch) {
                auto t0 = clk::now();
                for (int i = 0; i < reps; ++i) f.solve_multi(b3.data(), (size_t)n, x3.data(), (size_t)n, 3, w3.data(), &team);
                best3 = std::min(best3, 1e3 * ms_since(t0) / reps);
            }
            team.disarm();
            for (int c = 0; c < 3; ++c) {
                f.solve_multi(b3.data() + (size_t)c * n, (size_t)n, x1.data(), (size_t)n, 1, w3.data());
                for (int i = 0; i < n; ++i) diff3 = std::max(diff3, std::fabs(x1[i] - x3[(size_t)c * n + i]));
            }
            say("3 columns on %d threads: %.2f us per solve; max |difference| to single-column solves %.1e\n", threads, best3, diff3);
        }
        { double ph[6]; f.profile(b, w.data(), nullptr, reps, ph);
          say("1 thread phases: parts down %.1f, top down %.1f, top up %.1f, parts up %.1f us\n", ph[0], ph[1], ph[2], ph[3]); }
    }
    {   // the supernodal factorisation against the simplicial one it replaced
        SparseLDLT g;
        if (!g.factor(A)) return GMG_ERR_NUMERIC;
        std::vector<double> xr(n);
        for (int c = 0; c < 1; ++c) {
            g.solve(b + (size_t)c * n, xr.data(), w.data());
            double e2 = 0, n2 = 0;
            for (int i = 0; i < n; ++i) { const double dd = xr[i] - x[(size_t)c * n + i]; e2 += dd * dd; n2 += xr[i] * xr[i]; }
            say("column %d: supernodal vs simplicial relative difference %.3e (nnz(L) %ld vs %ld)\n", c, std::sqrt(e2 / std::max(n2, 1e-300)),
                         f.factor_nnz(), g.factor_nnz());
        }
    }
    std::snprintf(report, (size_t)cap, "%s", text.c_str());
    return GMG_OK;
} GMG_CATCH_0

}  // extern "C"

#include "engine_dist.hip.hpp"
