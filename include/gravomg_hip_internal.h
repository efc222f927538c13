/*
 * gravomg_hip_internal.h -- test and measurement hooks of libgravomg_hip.so.  NOT part of the drop-in boundary (include/gravomg_hip.h):
 * nothing a reference maintainer would bind.  tests/ and scripts/ reach the host-side building blocks (Galerkin product, layout planner,
 * LDL^T probe), the device-resident layouts and two fault-injection knobs of the set-up through these symbols.
 */
#ifndef GRAVOMG_HIP_INTERNAL_H
#define GRAVOMG_HIP_INTERNAL_H

#include "gravomg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test access to the device-resident SELL layouts of level k: which = 0 A (off-diagonal part), 1 A_in, 2 A_out,
 * 3 P (U_k), 4 R (U_k^T).  info[0..3] = n_slices, lanes per row, stored entries, has row_of.  Copy-out pointers may be
 * NULL; col receives 32-bit columns also for the 16-bit A_in; diag (which = 0 only) the level's diagonal. */
int gmg_debug_sell_info(gmg_handle h, int k, int which, int64_t* info);
int gmg_debug_sell_copy(gmg_handle h, int k, int which, int64_t* slice_ptr, int* col, double* val, int* row_of, double* diag);
/* The 16-bit column codes of a level-0 layout (which = 0, 3 or 4 as above; csrc/setup_kernels.hip.hpp::compress_cols) as the kernels read them.
 * info[0..4] = windows per slice (0 no codes, 8 or 32), mode (0 none, 1 codes from slice info[2] on, 2 uncovered slices flagged), c16_from,
 * uniform slice width (0: widths differ), stored words (= the layout's stored entries: of every slice's region the first half is used, the rest
 * was never written).  Copy-out pointers may be NULL: call once for info, then with col16 of info[4] words and win_base of n_slices * info[0]
 * entries.  Plain copies of arrays the handle owns; nothing is launched and the set-up is not touched. */
int gmg_debug_col16_copy(gmg_handle h, int which, int64_t* info, unsigned* col16, int* win_base);

/* Set-up fault injection for the tests, per handle, effective from the next gmg_set_system.  Keys:
 *   "col16_uncovered" = N > 0: every N-th level-0 slice is treated as not covered by its column windows (flagged one by one, c16 mode 2);
 *                       N < 0: the first -N slices (a prefix, c16 mode 1); 0: off.  Results must not change (tests/test_gpu_setup.py).
 *   "cheby_ratio" = R > 1: this handle's Chebyshev smoother runs over [lambda / R, lambda] instead of the process-wide ratio (GMG_CHEBY_RATIO /
 *                       the compiled default), effective from the next smoothing step; 0: off.  Measurement only (scripts/cheby_cycles.py). */
int gmg_debug_set(gmg_handle h, const char* key, double value);

/* The per-point parent selection of ONE hierarchy level (multigrid_solver.cpp:291-452) on job arrays the caller builds by hand, in the layout of
 * HierarchyOptions::SelectJob (csrc/host_hierarchy.hpp): P nf x 3, Pc nc x 3, nearest nf, sample nc, cadj_ptr nc + 1 / cadj (sorted neighbour cells),
 * tris ntri x 3, tof_ptr nc + 1 / tof (triangles of every cell, ascending), NBc nc x Kc (-1 padded).  Out, one record per point: cnt[nf] entries of
 * the row, kind[nf] (0 triangle, 1 edge, 2 closest three, 3 single / one neighbour, 4 nested sample), col[3 nf], w[3 nf]; entries beyond cnt are
 * not written.  mode 0: the host routine (HierarchyBuilder::select_point, triangle normals as the builder makes them) for every point;
 * mode 1: the device stage as the builder calls it (same upload / launch / download code), raw records, cnt = 255 for a point it hands back;
 * mode 2: what the builder makes of them -- device records, the points at cnt = 255 redone by the host routine.  Modes 1 and 2 return
 * GMG_ERR_NO_DEVICE / GMG_ERR_HIP when the stage does not run (no host rows instead).  Indices are checked (GMG_ERR_INVALID). */
int gmg_debug_select_parents(int nf, int nc, int Kc, int ntri, int weighting, int nested, const double* P, const double* Pc, const int* nearest,
                             const int* sample, const int* cadj_ptr, const int* cadj, const int* tris, const int* tof_ptr, const int* tof,
                             const int* NBc, int mode, unsigned char* cnt, unsigned char* kind, int* col, double* w);
/* Rows of U_k by kind, as the builder counted them (host and device levels alike): out[0..3] = containing triangle, edge, closest three,
 * single / one neighbour.  Lets an end-to-end test say which branches of the selection its input reached. */
int gmg_hierarchy_debug_row_kinds(gmg_hierarchy hh, int k, int* out);

/* One operator of the fp32 inner V-cycle (gmg_config::inner_precision = 1; GMG_ERR_STATE on any other handle) through the cycle's own launch
 * code: host fp64 arrays (natural numbering, column-major n x d) go into the level's fp64 vectors, are converted to its fp32 vectors (exact for
 * fp32-representable values), the launch_*<float> / enqueue_*<float> functions of the way down and the way up run, and the results are
 * widened and copied back.  No kernel runs that a cycle does not run.  op (k = level; in1 / out1 / out2 may be NULL where not listed):
 *   SMOOTH           in0 b, in1 x                 -> out0 x after `iters` sweeps of the handle's smoother
 *   SMOOTH_RESIDUAL  in0 b, in1 x, flag from_zero -> out0 x, out1 b - A x as the way down forms it behind the sweeps (from_zero: in1 is not
 *                                                    read; timing key residual_from_sweep = 1 where it came from the sweep's explicit part)
 *   RESIDUAL / SPMV  in0 b, in1 x / in0 x         -> out0 b - A x / A x
 *   RESTRICT         in0 r_k                      -> out0 U_k^T r_k (n_{k+1} rows)
 *   RESTRICT_SWEEPS  in0 r_k, k + 1 < levels      -> out0 U_k^T r_k, out1 level k + 1's iterate after `iters` >= 1 pre-sweeps from zero, out2 its
 *                                                    residual: what the way down does between two levels, fused into one launch where
 *                                                    gmg_config::fuse_restrict_sweep engages (timing key restrict_sweeps_fused counts); on
 *                                                    level 0 with d = 2 .. 4 the restriction reads the interleaved residual, as in a cycle
 *   PROLONG_ADD      in0 e_{k+1}, in1 x_k         -> out0 x_k + U_k e
 *   COARSE           in0 rc (k ignored)           -> out0 the fp64 coarsest solve of float(rc), rounded to fp32
 *   DEFECT           k = 0, in0 b, in1 x (fp64), flag norm type 0..3 -> out0 float(b - A x) widened, out1[0] the norm of b - A x
 *   CORRECT          k = 0, in0 e (fp32 values), in1 x (fp64)        -> out0 x + e, added in fp64 */
enum { GMG_F32_SMOOTH = 0, GMG_F32_SMOOTH_RESIDUAL = 1, GMG_F32_RESIDUAL = 2, GMG_F32_SPMV = 3, GMG_F32_RESTRICT = 4, GMG_F32_RESTRICT_SWEEPS = 5,
       GMG_F32_PROLONG_ADD = 6, GMG_F32_COARSE = 7, GMG_F32_DEFECT = 8, GMG_F32_CORRECT = 9 };
int gmg_debug_f32_op(gmg_handle h, int op, int k, int d, int iters, int flag, const double* in0, const double* in1, double* out0, double* out1,
                     double* out2);

/* Host-only Galerkin product Ac = U^T A U (CSC in / CSC out, caller sizes the output with the first call:
 * pass colptr_out only to get nnz in colptr_out[n_coarse]).  Exposed for the RAP parity tests. */
int gmg_host_galerkin(int n, const int* a_colptr, const int* a_rowidx, const double* a_val,
                      int n_coarse, const int* u_colptr, const int* u_rowidx, const double* u_val,
                      int* c_colptr, int* c_rowidx, double* c_val);

/* The DEVICE Galerkin product Ac = U^T A U (csrc/setup_kernels.hip.hpp::rap_rows) on arrays the caller builds by hand, through the code the
 * set-up runs -- upload of A and U, the by-row regrouping of U, count pass / prefix sum / fill pass -- on objects of its own: the handle lends
 * its stream and its pool and is otherwise left alone (hierarchy, system and timing keys untouched; no kernel launch that the set-up does not
 * make).  A: n x n, CSC as stored (unsorted columns and stored zeros are taken as they are), symmetric pattern; U: n x n_coarse, CSC.
 * Every index is checked (GMG_ERR_INVALID).  Out: *status = 0 and the product (c_colptr n_coarse + 1, c_rowidx / c_val of `cap` entries;
 * GMG_ERR_INVALID with c_colptr filled when the product has more), or *status = 1 when the device declines as it does in the set-up: a coarse
 * row with more distinct columns than the kernel's hash set holds, or a row of U with more than 3 entries (the product kernel is then not
 * launched at all).  a_val2 (optional): a second value array on the pattern of A.  After the product it is written over the resident values
 * and the numeric pass alone runs on the pattern at hand (what a values-only gmg_set_system does); its values go to c_val2 (cap entries).
 * GMG_ERR_NO_DEVICE without a HIP device. */
int gmg_debug_device_galerkin(gmg_handle h, int n, const int* a_colptr, const int* a_rowidx, const double* a_val, const double* a_val2, int n_coarse,
                              const int* u_colptr, const int* u_rowidx, const double* u_val, int64_t cap, int* c_colptr, int* c_rowidx, double* c_val,
                              double* c_val2, int* status);

/* The DEVICE-BUILT dense inverse of a coarsest operator (csrc/setup_kernels.hip.hpp::coarse_inverse_tiles and its follow-up kernels) on a matrix
 * the caller builds by hand, through the code the set-up runs -- factorisation, export of the factor in the device's chunk layout, upload, the
 * tiles launch, mirror / permutation / packing (csrc/engine_system.hip.hpp::coarse_inverse_core) -- into buffers of its own: the handle lends its
 * stream and its pool and is otherwise left alone (hierarchy, system, d_ainv, d_tri and timing keys untouched; no kernel launch that the set-up
 * does not make).  A: n x n symmetric positive definite, CSC as stored, every index checked (GMG_ERR_INVALID; GMG_ERR_NUMERIC when the
 * factorisation fails).  width: 0 = the set-up's rule (16 up to n = 8 192, 32 up to 16 384, 64 beyond), or 16 / 32 / 64 to force that
 * instantiation.  mode:
 *   0  host only (h may be NULL): SupernodalLDLT::emulate_device_column for every column of the same export; out n x n row-major, factor's
 *      numbering, entry [j][c] for j >= c, the other triangle zero
 *   1  device: X in the factor's numbering after mirror_lower_to_upper, n x n row-major
 *   2  device: the full inverse in the level's numbering through permute_symmetric, n rows of info[13] doubles (columns >= n mean nothing);
 *      GMG_ERR_INVALID for n > 8 192
 *   3  as 2 through permute_symmetric_scatter, whatever n is
 *   4  device: the packed triangle of pack_lower_blocks (csrc/coarse_triangle.hpp), info[12] doubles
 * Modes 1 .. 4 return GMG_ERR_NO_DEVICE without a HIP device.  info[0..15]: chunks, levels, tiles, width used, chunks with at least kInvBigRows
 * rows below them (worked off by all waves), most other chunks in one level, most rows below one chunk, most rows below one chunk of the other
 * kind, chunks narrower than 8 columns, chunks of level 0 (roots), row entries of all chunks, entries of tile_q, doubles of `out` for this mode,
 * its leading dimension, kInvBigRows, kInvWaves.  out == NULL: info and the optional arrays only (the sizing call).  The exported factor as the
 * kernel reads it, each array optional: perm n (factor -> level), q_col0 / q_w / lev_q `chunks`, q_rptr chunks + 1, rows info[10], vals
 * 8 info[10], tri 64 chunks, dinv n, lev_ptr levels + 1, lev_big levels (at kInvBigRows), tile_ptr tiles + 1 and tile_q info[11] for the width used. */
int gmg_debug_coarse_inverse(gmg_handle h, int n, const int* colptr, const int* rowidx, const double* val, int width, int mode, double* out, int64_t out_cap,
                             int64_t* info, int* perm, int* q_col0, int* q_w, int* q_rptr, int* rows, double* vals, double* tri, double* dinv, int* lev_ptr,
                             int* lev_q, int* lev_big, int* tile_ptr, int* tile_q);

/* Host-only view of the device layout planner (colouring / block growing / SELL-64), for CPU tests of the
 * host logic.  mode 0: colour-major ordering (exact multicolour Gauss-Seidel), mode 1: block ordering
 * (block-hybrid Gauss-Seidel, `block_rows` rows per block), mode 2: mode 0 with the locality reordering forced (rows of a colour in breadth-first
 * patch order), mode 3: mode 0 for a matrix whose row indices are ascending (the short-cut of the colouring loop), mode 4: mode 3 with the colouring that a cold
 * gmg_set_system starts ahead of its inspection -- on the arrays as given, every index checked (GMG_ERR_INVALID for arrays that would take a reader out of bounds;
 * info[5] = 1 when that colouring was used, 0 when it gave up at 64 colours; no SELL statistics).  In modes 0 / 2 / 3 / 4 `block_rows` is the colour-class
 * alignment (the config's row_align; 0 = 64).  info[0..5] = n_pad, n_colors, n_blocks,
 * stored SELL entries (off-diagonal), real off-diagonal entries, 0.  Output pointers may be NULL: call once
 * with NULL outputs for the sizes, then with new2old / row_color of n_pad entries, color_begin of
 * n_colors + 1 and blk_begin of n_blocks + 1 entries. */
int gmg_host_plan_level(int n, const int* colptr, const int* rowidx, const double* val, int mode, int block_rows, int sigma,
                        int64_t* info, int* new2old, int* color_begin, int* blk_begin, unsigned char* row_color);

/* Host-only view of the rule behind gmg_config::block_fine (engine_setup.hip.hpp::fine_level_blocked), for CPU tests: would level 0 of this
 * system run the block-hybrid sweep under the DEFAULT configuration, given a hierarchy?  *blocked = 1: at least 9 stored entries per row on
 * average, every diagonal entry positive, no positive off-diagonal entry (a Stieltjes matrix, for the symmetric positive definite systems
 * the solver takes: the block sweep is a regular splitting).  reason (optional): 0 chosen, 1 rows too short, 2 signs. */
int gmg_host_fine_block_rule(int n, const int* colptr, const int* rowidx, const double* val, int* blocked, int* reason);

/* The colouring behind gmg_config::device_coloring on a caller's symmetric pattern (n >= 1; CSC or CSR, the same thing; self-loops ignored):
 * Jones-Plassmann in synchronous rounds with first-fit colours (csrc/host_plan.hpp::jp_coloring_host, the specification) and the device kernels
 * that must give the same bytes (csrc/setup_kernels.hip.hpp::jp_round; the handle lends its stream and pool; the pattern is uploaded, the bytes
 * copied back).  colours: n bytes; *n_colors: colours used, or -1 when 254 do not suffice (colours then mean nothing, *rounds = 0); *rounds:
 * rounds until no vertex was left.  GMG_ERR_INVALID for arrays that would take a reader out of bounds; the host entry needs no device. */
int gmg_jp_coloring_host(int n, const int* colptr, const int* rowidx, unsigned char* colours, int* n_colors, int* rounds);
int gmg_jp_coloring_device(gmg_handle h, int n, const int* colptr, const int* rowidx, unsigned char* colours, int* n_colors, int* rounds);

/* ---- measurement ---------------------------------------------------------------------------- */
/* Average duration (ms) of one unit of level-k work, measured with HIP events on the engine stream:
 * kind 0 = full smoothing sweep (all colours), 1 = residual r=b-Ax, 2 = restrict, 3 = prolong_add,
 * 4 = residual-norm kernels.  The repetitions are enqueued back to back between two events (the way the
 * V-cycle issues them); launches_out = kernel launches per repetition (colours for the sweep). */
int gmg_bench_kernel(gmg_handle h, int kind, int k, int d, int reps, double* ms_avg, int* launches_out);
/* Leg-by-leg time of a V-cycle + residual check on the resident problem (HIP events at the leg boundaries, average over `reps` cycles):
 * ms_out[k], k < levels: level k's share (multigrid_solver.cpp:1063-1069 on the way down, :1082-1085 on the way up); ms_out[levels]: the
 * coarsest solve (:1075) with its host round trip; ms_out[levels + 1]: the residual check (:1228-1277).  n_out >= levels + 2. */
int gmg_profile_cycle(gmg_handle h, int stop_type, int reps, double* ms_out, int n_out);
/* Algorithmic (compulsory) bytes of the same unit of work, SURVEY.md 8(d). */
int gmg_algorithmic_bytes(gmg_handle h, int kind, int k, int d, double* bytes_out);

/* average duration (ms) of one exchange of the cycle, `reps` back to back (collective; measurement): "color<k>", "halo_all", "rows0" (every rank's level-0 rows: what a cycle with level 1
 * replicated moves once), and with level 1 partitioned "x1_halo" (after every level-1 sweep), "rows1" (r1 to all, once per
 * cycle), "r0_halo" (before the restriction, once per cycle).  Overwrites halo entries: gmg_p2p_load afterwards. */
int gmg_p2p_bench_kind(gmg_handle h, const char* kind, int reps, double* ms_avg);

/* Collective backend (gmg_config::dist_exchange != 0), after gmg_p2p_load: one exchange of every rank's level-0 rows of x (pack -> all-gather ->
 * unpack), then this rank's slot of the gathered buffer against what it packed.  max_abs_diff must be 0; doubles = values compared.  With
 * dist_exchange = 1 this is ncclAllGather's delivery seen from the host -- also on ONE rank (RCCL takes a one-rank communicator). */
int gmg_p2p_debug_collective_roundtrip(gmg_handle h, double* max_abs_diff, long long* doubles);

/* Host-only probe of the coarsest-level solver (csrc/host_ldlt.hpp): factorises A, times the back-substitution on 1 .. 8 threads (`reps` solves
 * per batch, best of 20) and the numeric re-factorisation, compares the team solves with the one-thread solve bit for bit and the supernodal
 * factor with the simplicial one.  The report (text lines) goes to `report` (cap bytes, NUL-terminated). */
int gmg_host_ldlt_probe(int n, const int* colptr, const int* rowidx, const double* val, const double* b, int reps, char* report, int cap);

/* Host-only views of gmg_config::nullspace = 1, for CPU tests.
 * gmg_host_nullspace_rowsum: the set-up's rule on a caller's matrix -- *rowsum = max_i |sum_j a_ij| / sum_j |a_ij| (an empty or all-zero row
 * counts 0); above 1e-9 the return value is the one gmg_set_system gives: GMG_ERR_INVALID with coarsest = 0 (level 0: "A 1 != 0"),
 * GMG_ERR_NUMERIC with coarsest != 0 ("the prolongations do not preserve constants").
 * gmg_host_pinv_solve: x = P G P b with the coarsest solver's factor in its "pin the last pivot" mode (csrc/host_ldlt.hpp: the last pivot in
 * elimination order accepted whatever it is, 1 / D = 0 in its place; G = [[A11^-1, 0], [0, 0]]) and P = I - 1 1^T / n, the means removed as
 * GMG_COARSE_HOST_LDLT removes them -- A^+ b for a symmetric positive semi-definite A with null space span{1}.  b / x column-major n x d.
 * The row-sum rule is applied first (GMG_ERR_NUMERIC above the bound); GMG_ERR_NUMERIC also for a zero pivot before the last one (a graph of
 * two components).  info (optional, 2 doubles): the row-sum figure, the replaced pivot over the largest pivot. */
int gmg_host_nullspace_rowsum(int n, const int* colptr, const int* rowidx, const double* val, int coarsest, double* rowsum);
int gmg_host_pinv_solve(int n, const int* colptr, const int* rowidx, const double* val, const double* b, int d, double* x, double* info);

#ifdef __cplusplus
}
#endif
#endif /* GRAVOMG_HIP_INTERNAL_H */
