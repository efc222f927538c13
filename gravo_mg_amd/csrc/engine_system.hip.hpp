// engine_system.hip.hpp -- the set-up of a system (gmg_set_system) and of the placeholder structure of a finalized hierarchy (prepare_structure).
// set_system_impl runs: enter_system (inspection + pattern digest beside the first uploads), values_only (the live pattern: refresh_system_values),
// FullSetup (orderings, Galerkin chain, layouts, coarsest factor), finish_system (the epilogue of both).  Part of engine.hip's translation unit.
namespace {

// The order in which the numeric Galerkin pass of level 1 can follow the upload of A_0's values (enter_system): coarse row p needs the rows of
// A_0 its children are (U_0's column p, ascending), so the coarse rows are bucketed by their largest child (64 fine rows per bucket, counting
// sort) -- in a locally numbered mesh a tenth of them becomes computable with every tenth of the upload.
void drop_rap_order(gmg_handle h) {
    h->rap_need.clear(); h->rap_need2.clear();
    if (h->d_rap_order) { (void)sync_hipFree(h->d_rap_order); h->d_rap_order = nullptr; }
    if (h->d_rap_order2) { (void)sync_hipFree(h->d_rap_order2); h->d_rap_order2 = nullptr; }
}
bool ensure_rap_order(gmg_handle h) {
    if (!h->rap_need.empty() && h->d_rap_order) return true;
    drop_rap_order(h);
    const Compressed& U0 = h->U[0];
    const int nc = U0.n_outer, nf = U0.n_inner;
    if (nc <= 0 || nf <= 0) return false;
    const int nb = (nf + 63) / 64 + 1;                    // (bucket 0: coarse rows without children)
    std::vector<int> start((size_t)nb + 1, 0), order((size_t)nc), bucket((size_t)nc);
    // (the largest child: the maximum over the column -- a caller of the raw C-ABI may hand over columns whose row indices are not ascending)
    for (int p = 0; p < nc; ++p) {
        int big = -1;
        for (int e = U0.ptr[p]; e < U0.ptr[p + 1]; ++e) big = std::max(big, U0.idx[e]);
        bucket[p] = big >= 0 ? (big >> 6) + 1 : 0;
        ++start[(size_t)bucket[p] + 1];
    }
    for (int b = 0; b < nb; ++b) start[b + 1] += start[b];
    h->rap_need.resize((size_t)nc);
    for (int p = 0; p < nc; ++p) { const int at = start[bucket[p]]++; order[at] = p; h->rap_need[at] = bucket[p] > 0 ? (bucket[p] - 1) * 64 + 63 : -1; }
    if (hipMalloc((void**)&h->d_rap_order, sizeof(int) * (size_t)nc) != hipSuccess) { (void)hipGetLastError(); h->d_rap_order = nullptr; h->rap_need.clear(); return false; }
    if (hipMemcpy(h->d_rap_order, order.data(), sizeof(int) * (size_t)nc, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); drop_rap_order(h); return false; }
    // level 2 (optional: without it the level's pass simply runs after level 1's): need of row q = the largest need among its children on level 1
    if (h->L >= 3 && h->U[1].n_inner == nc && h->U[1].n_outer > 0) {
        const Compressed& U1 = h->U[1];
        const int nc2 = U1.n_outer;
        std::vector<int> need1((size_t)nc);                     // by level-1 row (natural numbering)
        for (int at = 0; at < nc; ++at) need1[order[at]] = h->rap_need[at];
        std::vector<std::pair<int, int>> rows((size_t)nc2);
        for (int q = 0; q < nc2; ++q) {
            int m = -1;
            for (int e = U1.ptr[q]; e < U1.ptr[q + 1]; ++e) m = std::max(m, need1[U1.idx[e]]);
            rows[q] = {m, q};
        }
        std::sort(rows.begin(), rows.end());
        std::vector<int> order2((size_t)nc2);
        h->rap_need2.resize((size_t)nc2);
        for (int i = 0; i < nc2; ++i) { h->rap_need2[i] = rows[i].first; order2[i] = rows[i].second; }
        if (hipMalloc((void**)&h->d_rap_order2, sizeof(int) * (size_t)nc2) != hipSuccess || hipMemcpy(h->d_rap_order2, order2.data(), sizeof(int) * (size_t)nc2, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            if (h->d_rap_order2) { (void)sync_hipFree(h->d_rap_order2); h->d_rap_order2 = nullptr; }
            h->rap_need2.clear();
        }
    }
    return true;
}

// Can the numeric Galerkin pass of level k (1 or 2) follow the chunks of a values upload on aux_stream?  Level 2 only behind level 1.
bool rap_pipeline(gmg_handle h, int k) {
    const int j = k - 1;
    const bool level_ok = h->L >= k + 1 && h->dU_ready && (int)h->dU.size() == h->L && h->dU[j].ptr && h->dE3[j].cnt && h->lv[k].dA.ptr && h->lv[k].dA.idx &&
                          h->lv[k].dA.val && h->lv[k].dA.n_outer == h->U[j].n_outer;
    if (k == 1) return level_ok && h->aux_stream && h->aux_ev && h->d_aux_err && !h->dU_flagged && ensure_rap_order(h);
    return level_ok && !h->rap_need2.empty() && h->d_rap_order2 && (int)h->rap_need2.size() == h->U[1].n_outer;
}

// rows [first, end) of level k's numeric Galerkin pass, in the order of d_rap_order (level 1) / d_rap_order2 (level 2), on aux_stream
void rap_rows_behind(gmg_handle h, int k, int first, int end) {
    const DevCsr &dA = h->lv[k - 1].dA, &dU = h->dU[k - 1], &dC = h->lv[k].dA;
    const DevEll3& e3 = h->dE3[k - 1];
    hipLaunchKernelGGL(gmgs::rap_rows<2>, dim3(end - first), dim3(64), 0, h->aux_stream, dA.ptr, dA.idx, dA.val, dU.ptr, dU.idx, dU.val, e3.cnt, e3.col, e3.val, end,
                       (const int*)dC.ptr, (int*)nullptr, dC.idx, dC.val, h->d_aux_err, first, (const int*)(k == 1 ? h->d_rap_order : h->d_rap_order2));
}

// h->mass (natural numbering) -> device numbering of level 0 (d_mass, d_minv); needs a system (the ordering)
int upload_mass(gmg_handle h) {
    const int n = (int)h->mass.size();
    // device numbering (padding rows get weight 1: they carry r = b = 0)
    Level& l = h->lv[0];
    if (l.n != n) return fail(h, GMG_ERR_INVALID, "mass size does not match the system");
    int rc = ensure_stage(h, (size_t)n);
    if (rc) return rc;
    for (DevBuf<double>* p : {&h->d_mass, &h->d_minv}) if (!*p && (rc = dev_alloc(h, *p, l.n_pad))) return rc;
    if ((rc = h2d(h, h->d_stage, h->mass.data(), sizeof(double) * (size_t)n))) return rc;
    hipLaunchKernelGGL(gmgk::permute_mass, dim3((l.n_pad + 255) / 256), dim3(256), 0, h->stream, h->d_stage, l.d_new2old, l.n_pad, h->d_mass, h->d_minv);
    HIPCHK(hipStreamSynchronize(h->stream));
    return GMG_OK;
}

// fp32 twins of the value arrays (mixed precision); `alloc`: (re)allocate them, otherwise they exist with the right sizes
int refresh_fp32_twins(gmg_handle h, bool alloc) {
    // dst = (float)src[0 .. count); dst gets `cap` floats first when asked to or missing
    auto twin = [&](const double* src, DevBuf<float>& dst, int64_t count, int64_t cap) -> int {
        int rc = (alloc || !dst) ? dev_alloc(h, dst, (size_t)cap) : GMG_OK;
        if (rc == GMG_OK) launch_cvt(h, src, dst.get(), (size_t)count);
        return rc;
    };
    for (int k = 0; k < h->L; ++k) {
        Level& l = h->lv[k];
        int rc;
        for (DevSell* m : {&l.Aoff, &l.Ain, &l.Aout, &l.P, &l.R})
            if (m->val && m->stored > 0 && (rc = twin(m->val, m->val32, m->stored, m->stored))) return rc;
        if (l.use_bcsr && (rc = twin(l.bc_val, l.bc_val32, l.bc_nnz, std::max<int64_t>(l.bc_nnz, 1)))) return rc;
        if (l.use_ep && ((rc = twin(l.ep_val, l.ep_val32, l.ep_nnz, std::max<int64_t>(l.ep_nnz, 1))) || (rc = twin(l.ee_val, l.ee_val32, l.ee_nnz, std::max<int64_t>(l.ee_nnz, 1))))) return rc;
        if ((rc = twin(l.diag, l.diag32, l.n_pad, l.n_pad))) return rc;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return GMG_OK;
}

// Where the coarsest solve of this system runs (gmg_config::coarse_mode): GMG_COARSE_AUTO puts it on the device while the dense inverse is small
// enough to be read once per cycle for less than the host round trip costs (n_L <= kCoarseDeviceMax: 512 MB, ~0.1 ms; the reference's
// lower_bound = 1000 / ratio = 8 keep n_L below 8 000).
constexpr int kCoarseDeviceMax = 8192;
bool want_coarse_device(gmg_handle h, int n_coarse) {
    if (h->cfg.coarse_mode == GMG_COARSE_DEVICE_INVERSE || h->cfg.coarse_mode == GMG_COARSE_DEVICE_TRIANGLE) return true;
    return h->cfg.coarse_mode == GMG_COARSE_AUTO && n_coarse <= kCoarseDeviceMax;
}
// ... and from which matrix it is applied there: GMG_COARSE_DEVICE_TRIANGLE keeps the packed lower triangle only (coarse_triangle.hpp)
bool want_coarse_triangle(gmg_handle h) { return h->cfg.coarse_mode == GMG_COARSE_DEVICE_TRIANGLE; }

// Dense inverse of the coarsest operator, built ON THE DEVICE from the host's sparse factor (setup_kernels.hip.hpp::coarse_inverse_tiles): the factor
// goes up in the device's chunk layout (a few MB), one launch carries every tile of the identity (16, 32 or 64 columns: coarse_inverse_width) through it, a second one mirrors the
// lower triangle, a third one moves it from the factor's numbering into the level's.  (Until round 6 the host solved n_L right-hand sides one by
// one: 188 - 226 ms of set-up at n_L = 6 005.)
// GMG_COARSE_DEVICE_TRIANGLE stops after the tiles: one launch packs the triangle they computed into 64 x 64 blocks, still in the factor's numbering
// (setup_kernels.hip.hpp::pack_lower_blocks); the full matrix is not made, the permutation stays on the device for the product, and the product's
// scratch is allocated here.
// The core: one exported factor, one tile width (16 / 32 / 64), one choice of follow-up kernels, destinations the caller owns.  X (n x n, the
// inverse in the factor's numbering) is allocated here and handed back; dst: the full inverse in the level's numbering (leading dimension
// ldo) for kInvFollowPermute / kInvFollowScatter, the packed triangle for kInvFollowTriangle, unused for kInvFollowMirror (X with both triangles
// is the result).  Of the handle only the stream, the pool, the bounce buffers and the two scratch events are used: gmg_debug_coarse_inverse
// runs this on a caller's matrix.
enum { kInvFollowPermute = 0, kInvFollowScatter = 1, kInvFollowTriangle = 2, kInvFollowMirror = 3 };
struct CoarseInverseRun { double upload_ms = 0.0; float tiles_ms = 0.f; bool timed = false; };
// center (gmg_config::nullspace = 1, a factor with its last pivot pinned): the triangle the tiles computed is double-centred before the follow-up
// kernels run (gmgs::inverse_col_sums, gmgs::inverse_center): what they mirror, permute or pack is then the pseudo-inverse.
int coarse_inverse_core(gmg_handle h, const SupernodalLDLT::DeviceFactor& E, int width, int follow, DevBuf<double>& X, double* dst, int ldo, CoarseInverseRun& run, bool center = false) {
    auto t0 = clk::now();
    const int nl = E.n;
    std::vector<int> tile_ptr_h, tile_q_h;
    E.tile_paths(width, tile_ptr_h, tile_q_h);
    const std::vector<int> lev_big_h = E.big_per_level(gmgs::kInvBigRows);
    // chunk records in the kernel's two orders (setup_kernels.hip.hpp::InvFactor)
    auto record = [&](int q) { return make_int4(E.q_col0[(size_t)q] | (E.q_w[(size_t)q] << 24), E.q_rptr[(size_t)q], E.q_rptr[(size_t)q + 1], q); };
    std::vector<int4> lev_meta_h(E.lev_q.size()), tile_meta_h(tile_q_h.size());
    for (size_t k = 0; k < E.lev_q.size(); ++k) lev_meta_h[k] = record(E.lev_q[k]);
    for (size_t t = 0; t < tile_q_h.size(); ++t) tile_meta_h[t] = record(tile_q_h[t]);
    DevBuf<int4> lev_meta, tile_meta;
    DevBuf<int> rows, lev_ptr, lev_big, tile_ptr;
    DevBuf<double> vals, tri, dinv;
    int rc;
    if ((rc = upload(h, lev_meta, lev_meta_h)) || (rc = upload(h, tile_meta, tile_meta_h)) || (rc = upload(h, rows, E.rows)) || (rc = upload(h, lev_ptr, E.lev_ptr)) || (rc = upload(h, lev_big, lev_big_h)) ||
        (rc = upload(h, tile_ptr, tile_ptr_h)) || (rc = upload(h, vals, E.vals)) || (rc = upload(h, tri, E.tri)) || (rc = upload(h, dinv, E.dinv)))
        return rc;
    const bool permuted = follow == kInvFollowPermute || follow == kInvFollowScatter;
    std::vector<int> inv_h((size_t)nl);
    for (int i = 0; i < nl; ++i) inv_h[(size_t)E.perm[(size_t)i]] = i;
    DevBuf<int> perm_d, inv_d;
    if (permuted && ((rc = upload(h, perm_d, E.perm)) || (rc = upload(h, inv_d, inv_h)))) return rc;
    const size_t bytes = sizeof(double) * (size_t)nl * nl;
    if ((rc = dev_alloc(h, X, (size_t)nl * nl))) return rc;
    DevBuf<double> col_sums;
    if (center && nl > 0 && (rc = dev_alloc(h, col_sums, (size_t)nl))) return rc;
    HIPCHK(hipMemsetAsync(X, 0, bytes, h->stream));
    gmgs::InvFactor F;
    F.n = nl; F.nq = E.nq; F.nlev = E.nlev;
    F.lev_meta = lev_meta; F.tile_meta = tile_meta; F.rows = rows; F.lev_ptr = lev_ptr; F.lev_big = lev_big; F.tile_ptr = tile_ptr;
    F.vals = vals; F.tri = tri; F.dinv = dinv;
    static_assert(gmgs::kInvChunk == SupernodalLDLT::kChunk, "chunk width of the exported factor");
    const int nt = (nl + width - 1) / width, nm = (nl + 63) / 64;
    const int nb = tri_blocks(nl);
    run.upload_ms = ms_since(t0);
    if (nl > 0) {
        (void)hipEventRecord(h->ev0, h->stream);
        const dim3 block(64 * gmgs::kInvWaves);
        if (width == 16) hipLaunchKernelGGL(gmgs::coarse_inverse_tiles<16>, dim3(nt), block, 0, h->stream, F, X.get());
        else if (width == 32) hipLaunchKernelGGL(gmgs::coarse_inverse_tiles<32>, dim3(nt), block, 0, h->stream, F, X.get());
        else hipLaunchKernelGGL(gmgs::coarse_inverse_tiles<64>, dim3(nt), block, 0, h->stream, F, X.get());
        (void)hipEventRecord(h->ev1, h->stream);
        if (center) {
            hipLaunchKernelGGL(gmgs::inverse_col_sums, dim3(nm), dim3(gmgs::kCenterBlock), 0, h->stream, (const double*)X, nl, col_sums.get());
            hipLaunchKernelGGL(gmgs::inverse_center, dim3(nm, nm), dim3(gmgs::kCenterBlock), 0, h->stream, X.get(), nl, (const double*)col_sums);
        }
        if (follow == kInvFollowTriangle) {
            hipLaunchKernelGGL(gmgs::pack_lower_blocks, dim3(nb, nb), dim3(256), 0, h->stream, (const double*)X, nl, dst);
        } else {
            hipLaunchKernelGGL(gmgs::mirror_lower_to_upper, dim3(nm, nm), dim3(256), 0, h->stream, X.get(), nl);
            // ... and into the level's numbering: the product kernel then reads its vectors contiguously
            if (follow == kInvFollowPermute) hipLaunchKernelGGL(gmgs::permute_symmetric, dim3(nl), dim3(256), sizeof(double) * (size_t)nl, h->stream, (const double*)X, (const int*)perm_d, (const int*)inv_d, nl, dst, ldo);
            else if (follow == kInvFollowScatter) hipLaunchKernelGGL(gmgs::permute_symmetric_scatter, dim3(nl), dim3(256), 0, h->stream, (const double*)X, (const int*)perm_d, nl, dst, ldo);
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));        // (the temporaries above go back to the pool)
    run.timed = nl > 0 && hipEventElapsedTime(&run.tiles_ms, h->ev0, h->ev1) == hipSuccess;
    return GMG_OK;
}

// tile width: enough workgroups for the chip's compute units (121 tiles of 16 columns at n_L = 1 929, 376 at 6 005: two 1024-thread
// workgroups per compute unit are resident), wider tiles only where there would be more tiles than that
inline int coarse_inverse_width(int nl) { return nl <= 8192 ? 16 : (nl <= 16384 ? 32 : 64); }
// rows of the inverse that fit the LDS go through permute_symmetric, longer ones through permute_symmetric_scatter
constexpr int kInvPermuteLdsMax = 8192;

// The set-up's wrapper: the handle's own factor, the width rule, the handle's d_ainv or d_tri as destination, the timing keys.
int build_coarse_inverse_device(gmg_handle h) {
    auto t0 = clk::now();
    const int nl = h->coarse.n;
    const bool tri_mode = want_coarse_triangle(h);
    h->coarse_triangle = tri_mode;
    SupernodalLDLT::DeviceFactor E;
    h->coarse.export_device_factor(E);
    h->timing["coarse_inverse_export_ms"] = ms_since(t0);
    const int width = coarse_inverse_width(nl);
    int rc;
    const int lda = (nl + 7) / 8 * 8;
    const int nb = tri_blocks(nl);
    if (tri_mode) {
        if (h->d_ainv) { h->d_ainv = {}; h->ainv_n = 0; }
        if (h->tri_n != nl) {
            free_coarse_triangle(h);
            if ((rc = dev_alloc(h, h->d_tri, (size_t)tri_block_count(nb) * kTriBlockDoubles)) || (rc = dev_alloc(h, h->d_tri_row, (size_t)tri_row_scratch_doubles(nb))) ||
                (rc = dev_alloc(h, h->d_tri_col, (size_t)tri_col_scratch_doubles(nb))) || (rc = dev_alloc(h, h->d_tri_perm, (size_t)nl))) return rc;
            h->tri_n = nl;
        }
        if (nl > 0 && (rc = h2d(h, h->d_tri_perm, E.perm.data(), sizeof(int) * (size_t)nl))) return rc;
        h->timing["coarse_inverse_bytes"] = (double)(sizeof(double) * (size_t)tri_block_count(nb) * kTriBlockDoubles);
    } else {
        free_coarse_triangle(h);
        if ((!h->d_ainv || h->ainv_n != nl) && (rc = dev_alloc(h, h->d_ainv, (size_t)nl * lda))) return rc;
        h->ainv_n = nl; h->ainv_ld = lda;
        h->timing["coarse_inverse_bytes"] = (double)(sizeof(double) * (size_t)nl * lda);
    }
    DevBuf<double> X;                                       // the inverse in the factor's numbering
    CoarseInverseRun run;
    const int follow = tri_mode ? kInvFollowTriangle : (nl <= kInvPermuteLdsMax ? kInvFollowPermute : kInvFollowScatter);
    const double before = ms_since(t0);
    if ((rc = coarse_inverse_core(h, E, width, follow, X, tri_mode ? h->d_tri.get() : h->d_ainv.get(), lda, run, h->cfg.nullspace != 0))) return rc;
    h->timing["coarse_inverse_upload_ms"] = before + run.upload_ms - h->timing["coarse_inverse_export_ms"];
    if (run.timed) h->timing["coarse_inverse_tiles_ms"] = run.tiles_ms;
    h->timing["coarse_inverse_ms"] = ms_since(t0);
    h->timing["coarse_inverse_levels"] = E.nlev;
    h->timing["coarse_inverse_chunks"] = E.nq;
    long long shape[10];
    E.shape_info(width, gmgs::kInvBigRows, shape);
    h->timing["coarse_inverse_width"] = (double)shape[3];
    h->timing["coarse_inverse_big_chunks"] = (double)shape[4];
    h->timing["coarse_inverse_max_level_chunks"] = (double)shape[5];
    return GMG_OK;
}

// setup timeline: t_<what> = ms since the entry of gmg_set_system
void mark_at(gmg_handle h, clk::time_point t_all, const std::string& what) { h->timing["t_" + what] = ms_since(t_all); }

// numeric LDL^T of the coarsest operator, in the background (same_pattern: the symbolic factorisation of the last one stands)
std::future<bool> spawn_coarse_factor(gmg_handle h, bool same_pattern, double* ms) {
    return std::async(std::launch::async, [h, same_pattern, ms] {
        auto t = clk::now();
        const bool ok = h->coarse.factor(h->lv[h->L].A, same_pattern);
        h->coarse_warm = false;
        *ms = ms_since(t);
        return ok;
    });
}

// GMG_SMOOTHER_CHEBYSHEV: the Gershgorin bound of D^-1 A_k of every smoothed level from the arrays the smoother reads (gmgs::gershgorin_rows +
// its reduction), one double per level, all of them read back with one copy.  Timing keys "cheby_lambda_l<k>" and "cheby_ratio".  The
// coefficients of the steps are kernel arguments: captured graphs hold the old ones, so a bound that moved drops them.
int compute_cheby_bounds(gmg_handle h) {
    const int L = h->L;
    constexpr int per_block = gmgs::kGershBlock / 64;
    int max_blocks = 1;
    for (int k = 0; k < L; ++k) {
        if (h->lv[k].Aoff.lpr != 1 || !h->lv[k].Aoff.slice_ptr || !h->lv[k].diag) return fail(h, GMG_ERR_STATE, "the Chebyshev smoother needs the one-lane-per-row operator layout of every level");
        max_blocks = std::max(max_blocks, (h->lv[k].Aoff.n_slices + per_block - 1) / per_block);
    }
    DevBuf<double> partials, bounds;
    int rc;
    if ((rc = dev_alloc(h, partials, (size_t)max_blocks)) || (rc = dev_alloc(h, bounds, (size_t)L))) return rc;
    for (int k = 0; k < L; ++k) {
        const Level& l = h->lv[k];
        const int nblk = (l.Aoff.n_slices + per_block - 1) / per_block;
        if (nblk > 0) hipLaunchKernelGGL(gmgs::gershgorin_rows<double>, dim3(nblk), dim3(gmgs::kGershBlock), 0, h->stream, l.Aoff.slice_ptr, (const double*)l.Aoff.val,
                                         (const double*)l.diag, l.Aoff.n_slices, partials.get());
        hipLaunchKernelGGL(gmgs::gershgorin_reduce, dim3(1), dim3(gmgs::kGershBlock), 0, h->stream, (const double*)partials, nblk, bounds + k);
    }
    std::vector<double> host((size_t)L, 0.0);
    HIPCHK(hipMemcpyAsync(host.data(), bounds, sizeof(double) * (size_t)L, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (auto it = h->timing.begin(); it != h->timing.end();) it = it->first.rfind("cheby_lambda_l", 0) == 0 ? h->timing.erase(it) : std::next(it);      // (levels of an earlier hierarchy)
    bool moved = false;
    for (int k = 0; k < L; ++k) {
        if (!(host[k] >= 1.0) || !std::isfinite(host[k])) return fail(h, GMG_ERR_NUMERIC, "the Gershgorin bound of level " + std::to_string(k) + " is not finite");
        moved = moved || host[k] != h->lv[k].cheby_lambda;
        h->lv[k].cheby_lambda = host[k];
        h->timing["cheby_lambda_l" + std::to_string(k)] = host[k];
    }
    h->timing["cheby_ratio"] = cheby_ratio(h);
    if (moved) drop_graphs(h);
    return GMG_OK;
}

// gmg_config::nullspace = 1: the claim is checked on every set-up with real values.  Level 0: max_i |sum_j a_ij| / sum_j |a_ij|
// from the resident layout (gmgs::rowsum_rows + its reduction, one double read back); the coarsest operator: the same figure on the host,
// from the matrix the factorisation read.  Timing keys "nullspace", "nullspace_rowsum_l0", "nullspace_rowsum_coarse", "nullspace_pinned_pivot".
int check_nullspace_claim(gmg_handle h) {
    const int L = h->L;
    const Level& l = h->lv[0];
    if (l.Aoff.lpr != 1 || !l.Aoff.slice_ptr || !l.diag || !l.d_new2old) return fail(h, GMG_ERR_STATE, "gmg_config::nullspace needs the one-lane-per-row operator layout of level 0");
    constexpr int per_block = gmgs::kGershBlock / 64;
    const int nblk = (l.Aoff.n_slices + per_block - 1) / per_block;
    DevBuf<double> partials, worst;
    int rc;
    if ((rc = dev_alloc(h, partials, (size_t)std::max(nblk, 1))) || (rc = dev_alloc(h, worst, 1))) return rc;
    if (nblk > 0) hipLaunchKernelGGL(gmgs::rowsum_rows<double>, dim3(nblk), dim3(gmgs::kGershBlock), 0, h->stream, l.Aoff.slice_ptr, (const double*)l.Aoff.val,
                                     (const double*)l.diag, (const int*)l.d_new2old, l.Aoff.n_slices, partials.get());
    hipLaunchKernelGGL(gmgs::rowsum_reduce, dim3(1), dim3(gmgs::kGershBlock), 0, h->stream, (const double*)partials, nblk, worst.get());
    double rowsum0 = 0.0;
    HIPCHK(hipMemcpyAsync(&rowsum0, worst, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    const double rowsum_c = nullspace_rowsum(h->lv[L].A);          // (beside the device's work)
    HIPCHK(hipStreamSynchronize(h->stream));
    h->timing["nullspace"] = 1.0;
    h->timing["nullspace_rowsum_l0"] = rowsum0;
    h->timing["nullspace_rowsum_coarse"] = rowsum_c;
    h->timing["nullspace_pinned_pivot"] = h->coarse.pinned_pivot;
    if (!(rowsum0 <= kNullspaceRowsumMax)) return fail(h, GMG_ERR_INVALID, "nullspace = 1 but A 1 != 0 (largest |row sum| / sum of |entries| on level 0: " + std::to_string(rowsum0) + ")");
    if (!(rowsum_c <= kNullspaceRowsumMax)) return fail(h, GMG_ERR_NUMERIC, "nullspace = 1 but the prolongations do not preserve constants (largest |row sum| / sum of |entries| of the coarsest operator: " + std::to_string(rowsum_c) + ")");
    return GMG_OK;
}

// The end of every set-up: where the coarsest solve runs (+ its dense inverse unless inverse_ready), the fp32 twins, the mass -- when it
// changed or has no device copy (after the drop_system of a full set-up: always), and not for placeholder values.
int finish_system(gmg_handle h, int n, double ms_factor, bool inverse_ready, bool alloc_twins, bool placeholder) {
    const int L = h->L;
    int rc;
    h->timing["coarsest_solve"] = ms_factor;
    if (h->cfg.nullspace && !placeholder && (rc = check_nullspace_claim(h))) return rc;      // (before anything is built on the claim)
    h->timing["fine_level_reordered"] = h->lv[0].ord.reordered ? 1.0 : 0.0;      // level 0 follows a locality order (reorder_fine; gmg_config::reorder_pointwise)
    h->coarse_device = want_coarse_device(h, h->lv[L].A.n_outer);
    h->timing["coarse_on_device"] = h->coarse_device ? 1.0 : 0.0;
    h->coarse_triangle = h->coarse_device && want_coarse_triangle(h);
    h->timing["coarse_triangle"] = h->coarse_triangle ? 1.0 : 0.0;
    h->timing["coarse_triangle_run_blocks"] = h->coarse_triangle ? (double)kTriRun : 0.0;
    if (!h->coarse_device) h->timing["coarse_inverse_bytes"] = 0.0;
    if (h->coarse_device && !inverse_ready && (rc = build_coarse_inverse_device(h))) return rc;
    if (h->cfg.smoother == GMG_SMOOTHER_CHEBYSHEV && !placeholder && (rc = compute_cheby_bounds(h))) return rc;      // (the real values bring the bounds: no keys before a gmg_set_system)
    if (fp32_cycle_wanted(h->cfg) && (rc = refresh_fp32_twins(h, alloc_twins))) return rc;
    if (!placeholder && !h->mass.empty() && (h->mass_dirty || !h->d_mass)) {
        if ((int)h->mass.size() != n) return fail(h, GMG_ERR_INVALID, "mass size does not match the system");
        if ((rc = upload_mass(h))) return rc;
        h->mass_dirty = false;
    }
    h->timing["coarse_host_ms"] = 0.0;
    return GMG_OK;
}

void stamp_done(gmg_handle h, clk::time_point t_all) {
    mark_at(h, t_all, "mass_done");
    h->timing["upload"] = ms_since(t_all) - h->timing["reduction"];      // everything of the setup that is not the RAP chain
    h->timing["setup_total"] = ms_since(t_all);                          // wall time of this call (the coarsest factorisation overlaps)
}

// what refresh_system_values needs of the live levels (it returns 1 without)
bool refresh_possible(gmg_handle h) {
    const int L = h->L;
    for (int k = 0; k <= L; ++k) if (!h->lv[k].dA.ptr || !h->lv[k].dA.idx || !h->lv[k].dA.val) return false;
    for (int k = 0; k < L; ++k) if (!h->lv[k].d_old2new || !h->lv[k].diag) return false;
    return h->lv[L].hostA_pattern;
}

// gmg_set_system for a matrix with the sparsity pattern of the live system: values only.  Returns 1 when it cannot be
// done in place (nothing has been changed then, except values that the full path overwrites anyway).
// values_uploaded: the caller has already put `val` into the resident A_0 (the speculative upload of enter_system; the device copy of
// gmg_set_system_values_device, which passes val = nullptr)
// l1_rows_done: ... and has queued the numeric Galerkin pass of the first l1_rows_done rows of level 1 behind it (flag: h->d_aux_err)
int refresh_system_values(gmg_handle h, int n, const double* val, clk::time_point t_all, bool values_uploaded = false, int l1_rows_done = 0, int l2_rows_done = 0) {
    const int L = h->L;
    if (!refresh_possible(h)) return 1;
    for (auto it = h->timing.begin(); it != h->timing.end();) it = it->first.rfind("t_", 0) == 0 ? h->timing.erase(it) : std::next(it);
    mark_at(h, t_all, "pattern_key");
    int rc;
    DevBuf<int> d_err;
    if ((rc = dev_alloc(h, d_err, 1))) return rc;
    HIPCHK(hipMemsetAsync(d_err, 0, sizeof(int), h->stream));
    h->loaded_d = 0;
    for (int k = 0; k <= L; ++k) h->lv[k].hostA_values = false;          // host copies (if any) keep their pattern only
    if (!values_uploaded && (rc = h2d(h, h->lv[0].dA.val, val, sizeof(double) * (size_t)h->lv[0].nnz))) return rc;
    mark_at(h, t_all, "upload_A0");
    auto t0 = clk::now();
    for (int k = 1; k <= L; ++k) {
        Level& lk = h->lv[k];
        if ((rc = device_rap(h, h->lv[k - 1].dA, h->dU[k - 1], h->dE3[k - 1], lk.dA, lk.A, false, k == L, &lk.nnz, d_err, true, k == 1 ? l1_rows_done : (k == 2 ? l2_rows_done : 0)))) return rc < 0 ? rc : GMG_ERR_STATE;
        if (k == L) lk.hostA_values = true;
        mark_at(h, t_all, "rap_l" + std::to_string(k));
    }
    h->timing["reduction"] = ms_since(t0);
    double ms_factor = 0;
    std::future<bool> factor_done = spawn_coarse_factor(h, true, &ms_factor);
    auto tl = clk::now();
    for (int k = 0; k < L && rc == GMG_OK; ++k) rc = device_refill_level(h, k, d_err);
    int herr = 0, herr_aux = 0;
    if (rc == GMG_OK) {
        (void)hipMemcpyAsync(&herr, d_err, sizeof(int), hipMemcpyDeviceToHost, h->stream);
        if (l1_rows_done > 0) (void)hipMemcpyAsync(&herr_aux, h->d_aux_err, sizeof(int), hipMemcpyDeviceToHost, h->stream);
        (void)hipStreamSynchronize(h->stream);
        if (herr == 0) herr = herr_aux;
    }
    h->timing["setup_rap_rows_pipelined"] = l1_rows_done;
    h->timing["setup_rap_rows_pipelined_l2"] = l2_rows_done;
    h->timing["setup_device_layout"] = ms_since(tl);
    mark_at(h, t_all, "device_layout");
    const bool factor_ok = factor_done.get();
    mark_at(h, t_all, "factor_joined");
    if (rc != GMG_OK) return rc;
    if (herr == 2) return fail(h, GMG_ERR_NUMERIC, "system matrix has a missing or zero diagonal entry");
    if (herr != 0) { h->refill_ready = false; return fail(h, GMG_ERR_STATE, "value refresh failed on the device"); }
    if (!factor_ok) return fail(h, GMG_ERR_NUMERIC, "coarsest operator is singular (LDL^T hit a zero pivot)");
    if ((rc = finish_system(h, n, ms_factor, false, false, false))) return rc;
    h->timing["setup_ordering_cached"] = 1.0;
    h->timing["setup_values_only"] = 1.0;
    h->timing["rap_device_levels"] = (double)L;      // every level by the numeric pass of rap_rows
    h->timing["setup_ordering"] = 0.0; h->timing["setup_sell"] = 0.0; h->timing["setup_wait_ordering"] = 0.0;
    for (int k = 0; k <= L; ++k) h->timing["setup_ordering_l" + std::to_string(k)] = 0.0;
    stamp_done(h, t_all);
    return GMG_OK;
}

// Colouring ahead of the layout decisions (enter_system): the greedy colouring of level 0 in the caller's order -- 10-13 ms on one core at 3 M
// vertices, what a cold set-up waits for longest -- starts with the inspection's verdict (host_plan.hpp::greedy_coloring_ahead).  Used by the
// level-0 ordering task when the decisions come out that way; stopped and joined otherwise, and always before gmg_set_system returns.
struct AheadColoring {
    std::atomic<int> stop{0};
    PreColoring pre;
    std::future<int> fut;
    const int* ptr = nullptr;         // the caller's colptr it colours
    void cancel() { stop.store(1); }
    ~AheadColoring() { stop.store(1); if (fut.valid()) fut.wait(); }
};

// What enter_system leaves for the rest of the set-up: the verdict on the caller's arrays and what already went to the device.
struct SystemEntry {
    const int *colptr = nullptr, *rowidx = nullptr;       // the caller's arrays, or their canonical copy
    const double* val = nullptr;
    Compressed canon;                 // only filled when the caller's storage is unsorted or has duplicates
    uint64_t pat_key[2] = {0, 0};
    bool have_key = false;
    bool speculative = false;         // the values went up into the live system's A_0 ahead of the verdict ...
    bool spec_done = false;           // ... and the refresh ran behind them, with the result rc_spec
    int rc_spec = 1;
    DevCsr early_A0;                  // A_0 in natural numbering, sent up beside the inspection (a handle without a live system)
    AheadColoring ahead;
};

// A system of the live system's size is most likely the live pattern with new values (the demos' new tau per frame; the first system after
// the structure was prepared): its values go up to the resident A_0 AHEAD of the verdict, while worker threads inspect and digest the pattern
// (3-4 ms at 3 M vertices, as long as the upload), and so does the rest of the refresh: none of it reads the pattern, all of it is
// overwritten by the full set-up should the verdict be "another pattern" (the live system is lost then, which that set-up replaces anyway).
int speculate(gmg_handle h, int n, SystemEntry& e, clk::time_point t_all) {
    const int* colptr = e.colptr;
    std::future<void> keyed = std::async(std::launch::async, [&] { pattern_key(n, colptr, e.rowidx, h->cfg.host_threads, e.pat_key); });
    h->loaded_d = 0;
    // ... and the numeric Galerkin pass of level 1 -- the longest kernel of the refresh -- follows the values chunk by chunk on a second
    // stream, over the coarse rows in the order in which their inputs arrive (ensure_rap_order).  A randomly numbered input needs the
    // last chunk for nearly every row: everything then runs after the upload, as before.
    const bool pipeline = rap_pipeline(h, 1), pipeline2 = pipeline && rap_pipeline(h, 2);
    int l1_rows_done = 0, l2_rows_done = 0;
    const size_t val_bytes = sizeof(double) * (size_t)h->lv[0].nnz;
    std::function<void(size_t, hipEvent_t)> after_chunk = [&](size_t bytes_done, hipEvent_t arrived) {
        const int64_t entries = (int64_t)(bytes_done / sizeof(double));
        // complete rows of A_0 (a colptr that is not ascending -- the inspection is still running -- gives some row count: the rows computed from
        // it are recomputed by the full set-up that follows a failed inspection)
        const int rows = (int)(std::upper_bound(colptr, colptr + n + 1, (int)std::min<int64_t>(entries, colptr[n])) - colptr) - 1;
        const bool last = bytes_done >= val_bytes;
        // coarse rows computable so far: those whose largest needed fine row has arrived
        auto ready = [&](const std::vector<int>& need) { return last ? (int)need.size() : (int)(std::upper_bound(need.begin(), need.end(), rows - 1) - need.begin()); };
        const int p_hi = ready(h->rap_need);
        if (p_hi - l1_rows_done < 32768 && !last) return;
        if (p_hi > l1_rows_done) {
            (void)hipStreamWaitEvent(h->aux_stream, arrived, 0);
            rap_rows_behind(h, 1, l1_rows_done, p_hi);
            l1_rows_done = p_hi;
        }
        // level 2 behind it, on the same stream: the rows whose children on level 1 are all among the rows launched so far (the pieces
        // of level 1 end at a boundary of `need`: every row that needs no more than fine row rows - 1 has been launched)
        if (pipeline2) {
            const int q_hi = ready(h->rap_need2);
            if (q_hi > l2_rows_done && (last || q_hi - l2_rows_done >= 4096)) { rap_rows_behind(h, 2, l2_rows_done, q_hi); l2_rows_done = q_hi; }
        }
    };
    if (pipeline) (void)hipMemsetAsync(h->d_aux_err, 0, sizeof(int), h->aux_stream);
    const int rc_up = h2d(h, h->lv[0].dA.val, e.val, val_bytes, pipeline ? &after_chunk : nullptr);
    if (pipeline) { (void)hipEventRecord(h->aux_ev, h->aux_stream); (void)hipStreamWaitEvent(h->stream, h->aux_ev, 0); }
    e.speculative = true;
    if (rc_up == GMG_OK) { e.rc_spec = refresh_system_values(h, n, e.val, t_all, true, l1_rows_done, l2_rows_done); e.spec_done = true; }
    keyed.get();
    e.have_key = true;
    return rc_up;
}

// The first stage of gmg_set_system: the caller's arrays are inspected (range check, canonical storage?) on worker threads while this thread
// sends values up -- the speculative upload + refresh of a live pattern, or, on a handle WITHOUT a live system, A_0 in natural numbering (the
// cold set-up's first device step, 250 MB at 3 M vertices, into a matrix of its own: the levels are rebuilt later).
int enter_system(gmg_handle h, int n, const int* colptr, const int* rowidx, const double* val, clk::time_point t_all, SystemEntry& e) {
    e.colptr = colptr; e.rowidx = rowidx; e.val = val;
    const bool live = h->live != LiveSystem::none;
    const bool want_ahead = !(live && h->live_key_valid && (int)h->lv.size() == h->L + 1 && h->lv[0].n == n && (int64_t)colptr[n] == h->lv[0].nnz) &&
                            !h->ord_cache_valid && h->cfg.smoother == GMG_SMOOTHER_MULTICOLOR_GS && n >= (1 << 17) && h->cfg.color_ahead &&
                            !(h->cfg.block_rows > 0 && h->cfg.block_from_level <= 0);
    // (by value: should this frame be left by an exception, the colouring task keeps the inspection's state alive)
    std::shared_future<int> inspected = std::async(std::launch::async, [h, n, colptr, rowidx] { return inspect_pattern(n, n, colptr, rowidx, h->cfg.host_threads); }).share();
    if (want_ahead) {
        // (behind the inspection's verdict, which takes a millisecond or two -- not behind the upload this thread makes meanwhile: started at
        // entry, beside the inspection's threads, the loop ran at half its speed)
        const int64_t nnz_claimed = colptr[n];
        AheadColoring& ahead = e.ahead;
        ahead.ptr = colptr;
        ahead.fut = std::async(std::launch::async, [&ahead, inspected, n, colptr, rowidx, nnz_claimed] {
            if (inspected.get() != 0) return -2;
            return greedy_coloring_ahead(n, colptr, rowidx, nnz_claimed, ahead.pre.c8, ahead.stop);
        });
    }
    if (live && h->live_key_valid && h->refill_ready && (int)h->lv.size() == h->L + 1 && h->lv[0].n == n && colptr[0] == 0 && (int64_t)colptr[n] == h->lv[0].nnz &&
        h->lv[0].dA.val) {
        const int rc_up = speculate(h, n, e, t_all);
        if (rc_up != GMG_OK) { (void)inspected.get(); lose_live_system(h); return rc_up; }
    }
    if (!live && h->cfg.device_setup && h->cfg.device_rap && h->cfg.smoother == GMG_SMOOTHER_MULTICOLOR_GS && colptr[0] == 0 && colptr[n] >= n) {
        const int rc_up = upload_csr_raw(h, e.early_A0, n, colptr, rowidx, val);
        if (rc_up != GMG_OK) { (void)inspected.get(); return rc_up; }
    }
    const int what = inspected.get();
    if (what == 2) { if (e.speculative) lose_live_system(h); return fail(h, GMG_ERR_INVALID, "index out of range in LHS"); }
    if (what == 1) {
        e.canon = canonical_copy(n, n, colptr, rowidx, val, h->cfg.host_threads);
        e.colptr = e.canon.ptr.data(); e.rowidx = e.canon.idx.data(); e.val = e.canon.val.data();
        e.have_key = false;
        e.ahead.cancel();                           // (coloured from rows that are not ascending: no result)
        e.early_A0 = {};                            // (it went up in the caller's storage order)
        // (the values went up in the caller's storage order, the resident pattern is canonical: the live system is void, and this
        // matrix takes the full set-up from its canonical copy)
        if (e.speculative) { e.speculative = e.spec_done = false; lose_live_system(h); h->refill_ready = false; }
    }
    return GMG_OK;
}

// Same sparsity pattern as the live system (and the same hierarchy: refill_ready dies with it)?  Then every structure on the device stands and
// only values move: LHS values up, numeric Galerkin passes, value refill of the layouts, numeric LDL^T.  (The demos' usage: lhs = M + tau * S
// with a new tau per frame.)  Returns 1 when the full set-up has to run.
int values_only(gmg_handle h, int n, SystemEntry& e, clk::time_point t_all) {
    if (h->live == LiveSystem::none || !h->live_key_valid || !h->refill_ready || (int)h->lv.size() != h->L + 1 || h->lv[0].n != n) return 1;
    if (!e.have_key) { pattern_key(n, e.colptr, e.rowidx, h->cfg.host_threads, e.pat_key); e.have_key = true; }
    // (a level 0 that gmg_config::block_fine blocked stays blocked only while the new values pass its sign test)
    const bool keeps_fine_blocks = !(h->lv[0].ord.blocked && h->cfg.block_from_level >= 1) || stieltjes_signs(n, e.colptr, e.rowidx, e.val, h->cfg.host_threads);
    if (e.pat_key[0] != h->live_key[0] || e.pat_key[1] != h->live_key[1] || e.colptr[n] != h->lv[0].nnz || !keeps_fine_blocks) return 1;
    const bool from_placeholder = h->live == LiveSystem::placeholder;
    const int rc = e.spec_done ? e.rc_spec : refresh_system_values(h, n, e.val, t_all);
    if (rc == GMG_OK) {
        h->live = LiveSystem::system;
        h->timing["setup_structure_prepared"] = from_placeholder ? 1.0 : 0.0;
        h->timing["t_verdict"] = h->timing["setup_total"] = ms_since(t_all);
        h->timing["upload"] = h->timing["setup_total"] - h->timing["reduction"];
    } else if (rc != 1) {
        lose_live_system(h); h->refill_ready = false;       // half-refreshed values: no solves on them
    }
    return rc;
}

// the orderings of the live system, kept under its pattern digest for a later system with the same pattern (and hierarchy)
void stash_orderings(gmg_handle h) {
    h->ord_cache.resize(h->L + 1);
    for (int k = 0; k <= h->L; ++k) h->ord_cache[k] = std::move(h->lv[k].ord);
    h->ord_cache_key[0] = h->live_key[0]; h->ord_cache_key[1] = h->live_key[1];
    h->ord_cache_valid = true;
}

struct LevelStage {
    SellHost sa, sin, sout, sp, sr;
    BlockCsrHost bc, bin;
    bool use_bcsr = false, use_ep = false;
    std::vector<unsigned short> ep16;
    std::vector<double> dg;
    std::vector<unsigned short> c16;
    std::string err;
    bool ok = true;
    double ms_order = 0, ms_sell = 0;
};

// The full set-up, a small task graph: this thread runs the Galerkin chain A_1 .. A_L (multigrid_solver.cpp:1387-1392) and then builds or
// uploads the layouts; per level k a task orders level k as soon as A_k exists (the host planner: + its SELL layout, and P_k / R_k once levels
// k and k+1 are ordered); one task factors A_L (:1401).  The members are what the tasks share; the destructor joins every task.
class FullSetup {
public:
    FullSetup(gmg_handle h, SystemEntry& e, int n, clk::time_point t_all, bool placeholder)
        : h(h), e(e), n(n), L(h->L), colptr(e.colptr), rowidx(e.rowidx), val(e.val), t_all(t_all), placeholder(placeholder),
          mc(h->cfg.smoother == GMG_SMOOTHER_MULTICOLOR_GS), part(h->part_world > 1), device_setup(h->cfg.device_setup != 0),
          stage(L + 1), ord_done(L + 1), op_done(L), tr_done(L) {}
    ~FullSetup() {
        try { join(); } catch (...) {}
        if (factor_done.valid()) factor_done.wait();
    }
    int run() {
        h->timing["setup_wait_ordering"] = 0.0; h->timing["setup_device_layout"] = 0.0;
        if (part && !(device_setup && h->cfg.device_rap && mc)) return fail(h, GMG_ERR_UNSUPPORTED, std::string("a partitioned set-up needs device_setup = 1, device_rap = 1 and the multicolour smoother (this handle runs ") + smoother_name(h->cfg) + ")");
        h->partitioned = false;
        h->pool.reset_peak();
        int rc;
        if (device_setup) {
            if ((rc = ensure_device_transfers(h))) return rc;      // no-op when gmg_use_hierarchy (or an earlier system) made them
            if (h->dU_flagged) device_setup = false;    // prolongation rows with more than 3 entries: host planner and host RAP
            if (part && !device_setup) return fail(h, GMG_ERR_UNSUPPORTED, "a partitioned set-up has no host fallback (a prolongation row has more than 3 entries)");
        }
        start_tasks();
        if ((rc = renumber_level0())) return rc;
        spawn_level(0);
        if ((rc = galerkin_chain())) return rc;
        h->timing["reduction"] = ms_since(t0);
        factor_done = spawn_coarse_factor(h, ord_hit, &ms_factor).share();
        auto tl = clk::now();
        if (device_setup) { device_layouts(); ms_h2d = ms_since(tl); }
        if (!device_setup) host_uploads();
        join();
        h->timing["t_lhs_copied"] = ms_lhs_copied;
        h->timing["setup_colored_ahead"] = colored_ahead.load();
        mark("tasks_joined");
        const bool factor_ok = factor_done.get();
        mark("factor_joined");
        (void)hipStreamSynchronize(h->stream);
        if (rc_all != GMG_OK) return err_all.empty() ? rc_all : fail(h, rc_all, err_all);
        if (!factor_ok) return fail(h, GMG_ERR_NUMERIC, "coarsest operator is singular (LDL^T hit a zero pivot)");
        h->coarse_work.assign((size_t)h->lv[L].A.n_outer * 4, 0.0);       // grown by coarse_host_roundtrip for more than 4 columns
        h->timing["setup_ordering"] = 0.0; h->timing["setup_sell"] = 0.0;
        for (int k = 0; k <= L; ++k) h->timing["setup_ordering_l" + std::to_string(k)] = stage[k].ms_order;
        for (int k = 0; k <= L; ++k) { h->timing["setup_ordering"] = std::max(h->timing["setup_ordering"], stage[k].ms_order); h->timing["setup_sell"] = std::max(h->timing["setup_sell"], stage[k].ms_sell); }
        h->timing["setup_h2d"] = ms_h2d;
        const int nblk = std::max(kNormBlocks, grid_for((h->lv[0].n_pad + 63) / 64));        // one partial per four level-0 slices
        if (nblk > h->partial_blocks) {
            if ((rc = dev_alloc(h, h->d_partials, (size_t)nblk * 8))) return rc;
            h->partial_blocks = nblk;
        }
        return GMG_OK;
    }
    // The set-up succeeded: the handle holds a system from here on.
    int commit() {
        HIPCHK(hipStreamSynchronize(h->stream));
        h->timing["device_bytes_peak"] = (double)h->pool.peak_live_bytes;
        if (part) {
            // This rank's rows of levels 0 / 1 are laid out; what the set-up needed in full -- A_0, A_1 and U_0 in natural numbering (inputs of the
            // Galerkin chain and of the layout builders) and the column maps of the two levels -- goes back to the pool.  A later system pays for
            // them again (no values-only refresh on a partitioned handle); the orderings and the plan stay cached under the pattern digest.
            const bool s1 = h->plan && h->plan->shard1;
            h->lv[0].dA = {};
            if (s1) h->lv[1].dA = {};
            if (!h->dU.empty()) { h->dU[0] = {}; h->dE3[0] = {}; }
            for (int k = 0; k <= (s1 ? 1 : 0); ++k) { h->lv[k].d_old2new = {}; h->lv[k].d_blk_of_row = {}; }
            h->pool.trim_large((size_t)4 << 20);   // (the big temporaries go back to the device, not to this handle's pool)
            h->partitioned = true;
        }
        h->timing["device_bytes"] = (double)h->pool.live_bytes;
        // only now is there a system: a failure above leaves the handle without one (no solves on a half-built state)
        h->live_key[0] = e.pat_key[0]; h->live_key[1] = e.pat_key[1];
        h->live_key_valid = true;
        h->ord_cache_valid = false;       // (moved into the levels on a hit; refilled from them by the next call)
        h->live = LiveSystem::system;
        h->refill_ready = device_setup && device_rap_ok && h->cfg.device_setup != 0 && !part;
        return GMG_OK;
    }
    double ms_factor = 0;
    bool inverse_built = false;       // the dense coarse inverse was built while level 0's ordering ran

private:
    // the host copy of A_0, the staging for right-hand sides, the pattern digest, the decisions on level 0 and the patches
    void start_tasks() {
        // Host copy of the LHS: only where a host stage needs it (host RAP, host planner, block ordering of level 0); the default path works from
        // the caller's arrays and the device copy, and gmg_get_level_operator fetches on demand.
        const bool need_host_A0 = !device_setup || !h->cfg.device_rap;
        h->lv[0].n = n; h->lv[0].nnz = colptr[n];
        if (need_host_A0) {
            lhs_copied = std::async(std::launch::async, [this] { h->lv[0].A.assign(n, n, colptr, rowidx, val); ms_lhs_copied = ms_since(t_all); }).share();
            h->lv[0].hostA_pattern = h->lv[0].hostA_values = true;      // valid once lhs_copied is ready (every reader waits on it)
        }
        // pinned staging for one right-hand side (the solve's b / x transfers): page-locking costs milliseconds, do it now
        stage_ready = std::async(std::launch::async, [h = h, n = n] { (void)hipSetDevice(h->cfg.device); return ensure_host_stage(h, (size_t)n); });
        if (!e.have_key) pattern_key(n, colptr, rowidx, h->cfg.host_threads, e.pat_key);
        mark("pattern_key");
        // Level 0 as a blocked level (one launch per sweep instead of one per colour): asked for (block_from_level = 0), or chosen here
        // (gmg_config::block_fine) for an operator whose multicolour sweep would be a dozen small launches -- long rows -- and for which the
        // block-hybrid sweep is known to converge: positive diagonal, no positive off-diagonal entry (with the symmetric positive definite
        // system the method presumes, a Stieltjes matrix: D + in-block lower part is a regular splitting).  kNN graph Laplacians qualify;
        // meshes keep the colour-major sweep (4-7 colours, over-relaxed), Bilaplacians fail the sign test.
        blocked0 = fine_level_blocked(h, n, colptr, rowidx, val);
        h->timing["fine_level_blocked"] = blocked0 ? 1.0 : 0.0;
        ord_hit = h->ord_cache_valid && (int)h->ord_cache.size() == L + 1 && e.pat_key[0] == h->ord_cache_key[0] && e.pat_key[1] == h->ord_cache_key[1] &&
                  h->ord_cache[0].blocked == blocked0;
        h->timing["setup_ordering_cached"] = ord_hit ? 1.0 : 0.0;
        if (ord_hit || blocked0 || !mc || e.ahead.ptr != colptr) e.ahead.cancel();
        h->timing["setup_values_only"] = 0.0;
        h->ord_cache_valid = false;       // a hit moves the cached orderings into the levels; the next call moves them back
        // hierarchies set level by level (gmg_set_prolongation): grown now, in the background
        if (!h->patches_ready && !ord_hit) patches_done = std::async(std::launch::async, [h = h] { build_patches(h); }).share();
    }
    // Level 0 of a badly numbered input (random-order scans, point clouds) is renumbered for locality.  With the hierarchy's cluster order at hand
    // the LHS pattern is permuted on the device first, so that the (sequential) greedy colouring runs on a locally ordered graph; that needs the LHS
    // on the device before the ordering task starts.
    int renumber_level0() {
        t0 = clk::now();
        // (gmg_config::reorder_pointwise: a pointwise smoother takes the same decision and the same base order; its level 0 is not coloured)
        reorder0 = locality_reorder_smoother(h->cfg) && !ord_hit && !blocked0 && wants_locality_reorder(PatternView{n, colptr, rowidx}, h->cfg.reorder_fine);
        if (reorder0) e.ahead.cancel();                // (the level is coloured along another visit order: the loop started on the caller's order is of no use)
        if (e.early_A0.ptr && device_setup && h->cfg.device_rap) { h->lv[0].dA = std::move(e.early_A0); e.early_A0 = {}; A0_uploaded = true; }
        { const int rc = color_level0_on_device(); if (rc != GMG_OK) return rc; }
        // (h->cluster_order is only read once the patches are ready: build_patches may still be writing it)
        const bool have_bfs = (int)h->bfs_order.size() == n, have_cluster = h->patches_ready && (int)h->cluster_order.size() == n;
        h->base_order_choice = (reorder0 && h->patches_ready && have_bfs && !have_cluster) ? 1 : 0;
        // (a renumbered pointwise handle writes the three keys of the choice on every route, scored or not)
        if (reorder0 && !mc) { h->timing["base_order_score_cluster"] = h->timing["base_order_score_bfs"] = 0.0; h->timing["base_order_choice"] = h->base_order_choice; }
        if (reorder0 && have_bfs && have_cluster && !(device_setup && h->cfg.device_rap)) {
            // host-planner path: the same decision from the host twin of the device score (choose_base_order)
            unsigned long long sc[2], sb[2];
            order_gather_score_host(PatternView{n, colptr, rowidx}, h->cluster_order, 4096, sc);
            order_gather_score_host(PatternView{n, colptr, rowidx}, h->bfs_order, 4096, sb);
            h->base_order_choice = (sc[1] && sb[1] && (double)sb[0] / (double)sb[1] < (double)sc[0] / (double)sc[1]) ? 1 : 0;
            h->timing["base_order_score_cluster"] = sc[1] ? (double)sc[0] / (double)sc[1] : 0.0;
            h->timing["base_order_score_bfs"] = sb[1] ? (double)sb[0] / (double)sb[1] : 0.0;
            h->timing["base_order_choice"] = h->base_order_choice;
        }
        if (reorder0 && device_setup && h->cfg.device_rap && (have_cluster || (h->patches_ready && have_bfs))) {
            int rc = A0_uploaded ? GMG_OK : upload_csr_raw(h, h->lv[0].dA, n, colptr, rowidx, val);
            if (rc == GMG_OK) { A0_uploaded = true; rc = choose_base_order(h, h->lv[0].dA, n); }
            // (colours from the device depend on no visit order: the pattern need not come back permuted for a host loop to walk it)
            // (... nor for a pointwise smoother, which colours nothing: make_ordering puts its one class in base order)
            if (rc == GMG_OK && !colored_dev && mc) rc = device_permute_pattern(h, h->lv[0].dA, n, colptr[n]);
            if (rc != GMG_OK) return rc;
            permuted0 = !colored_dev && mc;
            if (permuted0) mark("permuted_pattern");
        }
        return GMG_OK;
    }
    // gmg_config::device_coloring: the colour bytes of level 0 from the device (engine_setup.hip.hpp::device_jp_coloring), enqueued as soon as A_0 is
    // there and copied back (n bytes) for make_ordering.  Only where a new colour-major ordering of level 0 is due and the set-up runs on the
    // device; every other case, 254 colours that do not suffice and a failure of the device colouring leave the host's greedy colouring in charge,
    // with the results of device_coloring = 0.  Timing keys "colored_on_device", "device_coloring_ms", "device_coloring_rounds".
    int color_level0_on_device() {
        h->timing["colored_on_device"] = 0.0; h->timing["device_coloring_ms"] = 0.0; h->timing["device_coloring_rounds"] = 0.0;
        const bool colour_major0 = !blocked0 && !(h->cfg.block_rows > 0 && h->cfg.block_from_level <= 0);
        if (!h->cfg.device_coloring || ord_hit || !mc || !colour_major0 || !device_setup || !h->cfg.device_rap) return GMG_OK;
        if (!A0_uploaded) {
            const int rc = upload_csr_raw(h, h->lv[0].dA, n, colptr, rowidx, val);
            if (rc != GMG_OK) return rc;
            A0_uploaded = true;
        }
        auto tc = clk::now();
        DevBuf<unsigned char> d_c8;
        int ncol = -1, rounds = 0;
        int rc = device_jp_coloring(h, h->lv[0].dA.ptr, h->lv[0].dA.idx, n, d_c8, &ncol, &rounds);
        if (rc == GMG_OK && ncol >= 0) {
            dev_pre.c8.resize((size_t)n);
            rc = d2h(h, dev_pre.c8.data(), d_c8, (size_t)n);
        }
        if (rc != GMG_OK) {                  // the host colours: the stream must be usable for the rest of the set-up, or that fails with its own message
            (void)hipStreamSynchronize(h->stream);
            (void)hipGetLastError();
            h->err.clear();
            return GMG_OK;
        }
        h->timing["device_coloring_ms"] = ms_since(tc);
        h->timing["device_coloring_rounds"] = rounds;
        if (ncol < 0) return GMG_OK;
        dev_pre.n_colors = ncol;
        dev_pre.any_order = true;
        colored_dev = true;
        h->timing["colored_on_device"] = 1.0;
        e.ahead.cancel();                    // (the greedy loop started ahead of the inspection colours for nobody)
        mark("colored_on_device");
        return GMG_OK;
    }
    // A_1 .. A_L.  The device keeps A_k (Level::dA) and U_k (h->dU, h->dE3, built once per hierarchy) in natural numbering: inputs of the device
    // RAP and of the device layout builder, and the source of the on-demand host copies.
    int galerkin_chain() {
        int rc;
        if (device_setup) {
            rc = dev_alloc(h, d_rap_err, 1);
            if (rc == GMG_OK) rc = hipMemsetAsync(d_rap_err, 0, sizeof(int), h->stream) == hipSuccess ? GMG_OK : GMG_ERR_HIP;
            if (rc != GMG_OK) return rc;
        }
        device_rap_ok = device_setup && h->cfg.device_rap != 0;
        h->timing["rap_device_levels"] = 0.0;      // levels 1 .. L whose operator rap_rows produced (gravomg_hip.h)
        if (!device_rap_ok) return host_chain(1);
        rc = A0_uploaded ? GMG_OK : upload_csr_raw(h, h->lv[0].dA, n, colptr, rowidx, val);
        mark("upload_A0");
        int k = 1;
        for (; k <= L && rc == GMG_OK; ++k) {
            Level& lk = h->lv[k];
            const bool want_pattern = !ord_hit && k < L, want_values = k == L;
            rc = device_rap(h, h->lv[k - 1].dA, h->dU[k - 1], h->dE3[k - 1], lk.dA, lk.A, want_pattern, want_values, &lk.nnz, d_rap_err);
            if (rc != GMG_OK) break;
            lk.n = lk.dA.n_outer;
            lk.hostA_pattern = want_pattern || want_values; lk.hostA_values = want_values;
            spawn_level(k);
            h->timing["rap_device_levels"] = (double)k;
            mark("rap_l" + std::to_string(k));
        }
        if (rc != 1) return rc;
        // a coarse row with more distinct columns than the device hash set holds (or a U row with > 3 entries): finish the chain with the host
        // implementation
        device_rap_ok = false;
        wait_lhs();
        if ((rc = ensure_host_A(h, k - 1, true))) return rc;
        return host_chain(k);
    }
    // A_k .. A_L by the host's Galerkin products (and the host-planned transfer layouts behind them)
    int host_chain(int k) {
        wait_lhs();
        for (; k <= L; ++k) {
            Level& l = h->lv[k];
            l.A = galerkin_rap(h->lv[k - 1].A, h->U[k - 1], h->cfg.host_threads);
            l.n = l.A.n_outer; l.nnz = l.A.nnz(); l.hostA_pattern = l.hostA_values = true;
            spawn_level(k);
            spawn_transfer(k - 1);
        }
        return GMG_OK;
    }
    // -- layouts built on the device from the raw matrices + orderings (setup_kernels.hip.hpp)
    void device_layouts() {
        DevBuf<int> d_err;
        if ((rc_all = dev_alloc(h, d_err, 1)) != GMG_OK) return;
        (void)hipMemsetAsync(d_err, 0, sizeof(int), h->stream);
        // the coarse levels first: their orderings are short jobs, while level 0's (a sequential greedy colouring of the whole mesh) is the longest
        // host task of the set-up and may still be running
        for (int k = L; k >= 1 && rc_all == GMG_OK; --k) device_ordering(k);
        DevBuf<int> d_mask0, d_mask1;
        bool shard1 = false;
        if (part && rc_all == GMG_OK) plan_partition(d_mask0, d_mask1, &shard1);
        double ms_layout = 0;
        auto tlay = clk::now();
        for (int k = 1; k < L && rc_all == GMG_OK; ++k) rc_all = device_layout_level(h, k, d_err, (k == 1 && shard1) ? d_mask1.get() : nullptr, nullptr);
        if (part && shard1 && rc_all == GMG_OK && !h->lv[1].use_ep) { rc_all = GMG_ERR_UNSUPPORTED; err_all = "level 1 cannot run the entry-parallel block sweep (a block is too large for its LDS buffers): create the handle with dist_shard_levels = 1"; }
        ms_layout += ms_since(tlay);
        early_inverse();
        if (rc_all == GMG_OK && !part) device_ordering(0);
        tlay = clk::now();
        if (rc_all == GMG_OK) rc_all = device_layout_level(h, 0, d_err, part ? d_mask0.get() : nullptr, (part && shard1) ? d_mask1.get() : nullptr);
        ms_layout += ms_since(tlay);
        h->timing["setup_device_layout"] = ms_layout;
        mark("device_layout");
        if (rc_all != GMG_OK) return;
        int herr = 0;
        (void)hipMemcpyAsync(&herr, d_err, sizeof(int), hipMemcpyDeviceToHost, h->stream);
        (void)hipStreamSynchronize(h->stream);
        if (herr == 2) { rc_all = GMG_ERR_NUMERIC; err_all = "system matrix has a missing or zero diagonal entry"; }
        else if (herr != 0 && part) { rc_all = GMG_ERR_UNSUPPORTED; err_all = "rows too long for the device layout builder: a partitioned set-up has no host fallback"; }
        else if (herr != 0) {
            // rows too long for the device builder: redo the layout with the host planner
            device_setup = false;
            wait_lhs();
            for (int k = 0; k < L && rc_all == GMG_OK; ++k) rc_all = ensure_host_A(h, k, true);
            for (int k = 0; k < L && rc_all == GMG_OK; ++k) spawn_level_ops(k);
            for (int k = 0; k < L && rc_all == GMG_OK; ++k) spawn_transfer(k);
        }
    }
    // A partitioned set-up (gmg_dist_partition) lays out this rank's rows of levels 0 / 1 only: it needs the partition plan -- hence both orderings
    // -- before the first layout; everybody else's rows are masked out of the row maps the builders read
    void plan_partition(DevBuf<int>& d_mask0, DevBuf<int>& d_mask1, bool* shard1) {
        device_ordering(0);
        auto tp = clk::now();
        const LevelOrdering& o0 = h->lv[0].ord;
        if (rc_all == GMG_OK && o0.blocked) { rc_all = GMG_ERR_STATE; err_all = "a partitioned set-up needs the colour-major level 0 (block_from_level >= 1)"; }
        for (int c = 0; c < o0.n_colors && rc_all == GMG_OK; ++c)
            if ((o0.color_begin[c + 1] - o0.color_begin[c]) % (64 * h->part_world)) { rc_all = GMG_ERR_STATE; err_all = "colour classes are not aligned to 64*world rows: create the handle with row_align = 64*world"; }
        if (rc_all == GMG_OK) {
            *shard1 = plan_can_shard_level1(h, h->part_world, false);
            const bool reuse = h->plan && h->plan->key[0] == e.pat_key[0] && h->plan->key[1] == e.pat_key[1] && h->plan->rank == h->part_rank &&
                               h->plan->world == h->part_world && h->plan->shard1 == *shard1 && h->plan->n_colors == o0.n_colors;
            if (!reuse) {
                if (*shard1) rc_all = ensure_host_A(h, 1, false);
                auto plan = std::make_shared<DistPlan>();
                if (rc_all == GMG_OK) rc_all = build_dist_plan(h, *plan, h->part_rank, h->part_world, PatternView{n, colptr, rowidx}, *shard1 ? &h->lv[1].A : nullptr, *shard1);
                plan->key[0] = e.pat_key[0]; plan->key[1] = e.pat_key[1];
                if (rc_all == GMG_OK) h->plan = plan;
            }
            h->timing["dist_plan_cached"] = reuse ? 1.0 : 0.0;
        }
        if (rc_all == GMG_OK) rc_all = make_row_masks(h, *h->plan, d_mask0, d_mask1);
        h->timing["dist_plan_ms"] = ms_since(tp);
    }
    // The device has nothing to do until the ordering of level 0 arrives (a sequential colouring on the host): when the coarsest factor is there
    // first, the dense inverse of the coarsest operator is built in that gap instead of at the end of the call
    void early_inverse() {
        if (rc_all != GMG_OK || part || placeholder || !want_coarse_device(h, h->lv[L].A.n_outer)) return;
        while (ord_done[0].wait_for(std::chrono::seconds(0)) != std::future_status::ready &&
               factor_done.wait_for(std::chrono::microseconds(200)) != std::future_status::ready) {}
        if (factor_done.wait_for(std::chrono::seconds(0)) != std::future_status::ready || !factor_done.get()) return;
        h->coarse_device = true;
        rc_all = build_coarse_inverse_device(h);
        inverse_built = rc_all == GMG_OK;
        mark("coarse_inverse_early");
    }
    // -- host-planned layouts: uploads in the order the stages complete (level 0 first: the largest, ready early)
    void host_uploads() {
        // host-planned layouts carry no 16-bit column codes (upload_sell resets them): the keys must not keep what a device layout reported -- the
        // one this call abandoned for rows too long for the device builder, or an earlier system's
        for (const char* key : {"col16_l0", "col16_R_l0", "col16_P_l0"})
            for (const char* sfx : {"", "_failed_slices", "_mode", "_windows", "_uniform_width"}) h->timing[std::string(key) + sfx] = 0.0;
        for (int k = 0; k <= L && rc_all == GMG_OK; ++k) {
            if (!ordering_arrived(k)) break;
            auto tu = clk::now();
            if ((rc_all = upload(h, h->lv[k].d_new2old, h->lv[k].ord.new2old))) break;
            ms_h2d += ms_since(tu);
            if (k == L) break;
            op_done[k].get();
            if (!stage[k].ok) { rc_all = GMG_ERR_NUMERIC; err_all = "level " + std::to_string(k) + ": " + stage[k].err; break; }
            tu = clk::now();
            if ((rc_all = upload_host_layout(k))) break;
            ms_h2d += ms_since(tu);
        }
        for (int k = 0; k < L && rc_all == GMG_OK; ++k) {
            tr_done[k].get();
            auto tu = clk::now();
            if ((rc_all = upload_sell(h, h->lv[k].P, stage[k].sp)) || (rc_all = upload_sell(h, h->lv[k].R, stage[k].sr))) break;
            ms_h2d += ms_since(tu);
        }
    }
    int upload_host_layout(int k) {
        Level& l = h->lv[k];
        const LevelStage& st = stage[k];
        int rc;
        if ((rc = upload_sell(h, l.Aoff, st.sa)) || (rc = upload(h, l.diag, st.dg))) return rc;
        if (!l.ord.blocked) return GMG_OK;
        if (st.use_ep) {
            l.use_ep = true;
            l.ee_nnz = st.bc.ptr[l.n_pad]; l.ep_nnz = st.bin.ptr[l.n_pad];
            l.ep_cap_e = (st.bc.max_block_entries + 63) / 64 * 64; l.ep_cap_l = std::max(st.bin.max_block_entries, 1);
            if ((rc = upload(h, l.ee_ptr, st.bc.ptr)) || (rc = upload(h, l.ee_col, st.bc.col)) || (rc = upload(h, l.ee_val, st.bc.val)) ||
                (rc = upload(h, l.ep_ptr, st.bin.ptr)) || (rc = upload(h, l.ep_col, st.ep16)) || (rc = upload(h, l.ep_val, st.bin.val))) return rc;
        } else {
            if ((rc = upload_sell(h, l.Ain, st.sin)) || (rc = upload_sell(h, l.Aout, st.sout)) || (rc = upload(h, l.ain_col16, st.c16))) return rc;
            if (st.use_bcsr) {
                l.use_bcsr = true;
                l.bc_cap = (st.bc.max_block_entries + 63) / 64 * 64;
                l.bc_nnz = st.bc.ptr[l.n_pad];
                if ((rc = upload(h, l.bc_ptr, st.bc.ptr)) || (rc = upload(h, l.bc_mid, st.bc.mid)) || (rc = upload(h, l.bc_col, st.bc.col)) || (rc = upload(h, l.bc_val, st.bc.val))) return rc;
            }
        }
        if ((rc = upload(h, l.d_blk_begin, l.ord.blk_begin)) || (rc = upload(h, l.d_blk_ncolors, l.ord.blk_ncolors)) || (rc = upload(h, l.d_row_color, l.ord.row_color))) return rc;
        return GMG_OK;
    }
    void spawn_level(int k) {
        ord_done[k] = std::async(std::launch::async, [this, k] { order_level(k); }).share();
        if (k < L && !device_setup) spawn_level_ops(k);
    }
    void spawn_level_ops(int k) { op_done[k] = std::async(std::launch::async, [this, k] { lay_out_level(k); }); }
    void spawn_transfer(int k) { if (!device_setup) tr_done[k] = std::async(std::launch::async, [this, k] { build_transfer(k); }); }
    void order_level(int k) {
        auto t = clk::now();
        Level& lk = h->lv[k];
        const bool blocked = mc && k < L && h->cfg.block_rows > 0 && (k >= h->cfg.block_from_level || (k == 0 && blocked0));
        if (ord_hit) lk.ord = std::move(h->ord_cache[k]);          // same pattern + same hierarchy => same orderings
        else if (k == L) lk.ord = identity_ordering(lk.n);
        else if (blocked) {
            if (patches_done.valid()) patches_done.wait();
            // level 0: blocks = runs of block_rows points of the hierarchy's cluster order (level0_patches), coloured from the caller's arrays
            // (row_align = 64 P: the block count is padded to a multiple of P, so that P ranks own whole blocks -- engine_dist.hip.hpp::p2p_smooth)
            if (k == 0) lk.ord = make_block_ordering(PatternView{n, colptr, rowidx}, h->cfg.block_rows, level0_patches(h, n), std::max(1, h->cfg.row_align / 64));
            else lk.ord = make_block_ordering(lk.A, h->cfg.block_rows, k < (int)h->patches.size() ? &h->patches[k] : nullptr);
        }
        else if (k == 0) {
            if (reorder0 && patches_done.valid()) patches_done.wait();
            const std::vector<int>* base = reorder0 && (int)base_order(h).size() == n ? &base_order(h) : nullptr;
            if (permuted0 && base) {
                // colour the LHS pattern in cluster order (made on the device, see device_permute_pattern), then map back
                LevelOrdering c = make_ordering(PatternView{n, h->reo_ptr.data(), h->reo_idx.data()}, mc, h->cfg.row_align, h->cfg.sigma, 0);
                const int T = std::min(h->cfg.host_threads, 32);
                parallel_ranges(c.n_pad, T, [&](int lo, int hi, int) { for (int r = lo; r < hi; ++r) if (c.new2old[r] >= 0) c.new2old[r] = (*base)[c.new2old[r]]; });
                parallel_ranges(c.n_pad, T, [&](int lo, int hi, int) { for (int r = lo; r < hi; ++r) if (c.new2old[r] >= 0) c.old2new[c.new2old[r]] = r; });
                c.reordered = true;
                lk.ord = std::move(c);
            } else {
                AheadColoring& ahead = e.ahead;
                PreColoring* pre = nullptr;
                if (colored_dev) { ahead.cancel(); pre = &dev_pre; }      // the device's colours (color_level0_on_device): good for any visit order
                else if (!reorder0 && !base && mc && ahead.fut.valid() && ahead.ptr == colptr && !ahead.stop.load()) {
                    ahead.pre.n_colors = ahead.fut.get();
                    if (ahead.pre.n_colors >= 0) pre = &ahead.pre;
                } else ahead.cancel();
                colored_ahead.store(pre && !colored_dev ? 1 : 0);
                lk.ord = make_ordering(PatternView{n, colptr, rowidx}, mc, h->cfg.row_align, h->cfg.sigma, reorder0 ? 1 : 0, base, /*idx_sorted=*/true, pre);   // the caller's arrays (canonical: checked / canonicalised at entry)
            }
        }
        else lk.ord = make_ordering(lk.A, mc, h->cfg.row_align, h->cfg.sigma);
        lk.n_pad = lk.ord.n_pad;
        stage[k].ms_order = ms_since(t);
    }
    void lay_out_level(int k) {
        ord_done[k].wait();
        if (k == 0) wait_lhs();      // level 0 is ordered from the caller's arrays, but laid out from the host copy: that copy must be complete
        auto t = clk::now();
        Level& lk = h->lv[k];
        LevelStage& st = stage[k];
        // lanes per row on a blocked level: the quad layout pays where the level is latency-bound (few wavefronts);
        // a big level is throughput-bound and keeps one lane per row (single-wave blocks, no cross-wave barriers).
        // Level 0 always keeps one lane per row: the residual-norm kernels read its operator in that layout.
        const int lanes_auto = lk.n < kQuadLevelRows ? 4 : 1;
        const int lpr = (lk.ord.blocked && k > 0) ? (h->cfg.block_lanes ? h->cfg.block_lanes : lanes_auto) : 1;
        if (lk.ord.n_colors > kMaxColors) { st.ok = false; st.err = "more than " + std::to_string(kMaxColors) + " colours"; return; }
        if (!build_operator_sell(lk.A, lk.ord, lpr, st.sa, st.dg, st.err)) { st.ok = false; return; }
        if (lk.ord.blocked && wants_block_ep(h, lpr)) {
            build_operator_blockcsr(lk.A, lk.ord, st.bc, 3);       // "explicit" part
            build_operator_blockcsr(lk.A, lk.ord, st.bin, 4);      // "lower" part
            st.use_ep = st.bc.max_block_entries <= kEpMaxBlockEntries && st.bin.max_block_entries <= kEpMaxBlockLower;
            if (st.use_ep) {
                st.ep16.resize(st.bin.col.size());
                for (size_t i = 0; i < st.ep16.size(); ++i) st.ep16[i] = (unsigned short)st.bin.col[i];
            }
        }
        if (lk.ord.blocked && !st.use_ep && wants_block_csr(h, lpr)) {
            build_operator_blockcsr(lk.A, lk.ord, st.bc);
            st.use_bcsr = st.bc.max_block_entries <= kBcsrMaxBlockEntries;
        }
        if (lk.ord.blocked && !st.use_ep) {
            build_operator_sell_split(lk.A, lk.ord, st.sin, st.sout, lpr);
            st.c16.resize(st.sin.col.size());
            parallel_ranges((int)st.sin.col.size(), h->cfg.host_threads, [&](int lo, int hi, int) { for (int i = lo; i < hi; ++i) st.c16[i] = (unsigned short)st.sin.col[i]; });
        }
        st.ms_sell += ms_since(t);
    }
    void build_transfer(int k) {
        ord_done[k].wait();
        ord_done[k + 1].wait();
        auto t = clk::now();
        Level& lk = h->lv[k];
        Compressed Urows = transpose_parallel(h->U[k]);                            // outer = fine rows
        stage[k].sp = build_transfer_sell(Urows, lk.ord, h->lv[k + 1].ord, 0);
        stage[k].sr = build_transfer_sell(h->U[k], h->lv[k + 1].ord, lk.ord, h->cfg.restrict_sigma > 0 ? h->cfg.restrict_sigma : 0,
                                          h->cfg.block_lanes == 1 ? 1 : 4);       // outer = coarse rows (~18 entries each)
        stage[k].ms_sell += ms_since(t);
    }
    // the ordering of level k, awaited: a failure of its task becomes an error that names the level
    bool ordering_arrived(int k) {
        try { ord_done[k].get(); } catch (const std::exception& x) { rc_all = GMG_ERR_STATE; err_all = std::string("ordering of level ") + std::to_string(k) + ": " + x.what(); return false; }
        return true;
    }
    void device_ordering(int k) {
        auto tw = clk::now();
        if (!ordering_arrived(k)) return;
        h->timing["setup_wait_ordering"] += ms_since(tw);
        mark("ordering_ready_l" + std::to_string(k));
        if (h->lv[k].ord.n_colors > kMaxColors) { rc_all = GMG_ERR_UNSUPPORTED; err_all = "more than " + std::to_string(kMaxColors) + " colours on level " + std::to_string(k); return; }
        rc_all = upload(h, h->lv[k].d_new2old, h->lv[k].ord.new2old);
    }
    void wait_lhs() { if (lhs_copied.valid()) lhs_copied.wait(); }
    void mark(const std::string& what) { mark_at(h, t_all, what); }
    void join() {
        wait_lhs();
        if (patches_done.valid()) patches_done.wait();
        if (stage_ready.valid()) (void)stage_ready.get();
        for (int j = 0; j <= L; ++j) if (ord_done[j].valid()) ord_done[j].wait();
        for (int j = 0; j < L; ++j) { if (op_done[j].valid()) op_done[j].wait(); if (tr_done[j].valid()) tr_done[j].wait(); }
    }

    gmg_handle h;
    SystemEntry& e;
    const int n, L;
    const int *colptr, *rowidx;
    const double* val;
    const clk::time_point t_all;
    const bool placeholder;           // prepare_structure's placeholder values: no dense coarse inverse (the refresh with the real ones builds it)
    const bool mc, part;              // part: gmg_dist_partition -- lay out and keep this rank's rows of levels 0 / 1 only
    bool device_setup;                // layouts built on the device (false: the host planner; also the fallback for rows too long for the device)
    bool device_rap_ok = false;       // A_1 .. A_L by the device's Galerkin chain
    bool ord_hit = false, blocked0 = false;
    bool reorder0 = false, permuted0 = false;      // level-0 locality renumbering (decided before level 0 is spawned)
    bool A0_uploaded = false;
    bool colored_dev = false;         // level 0's colours came from the device (gmg_config::device_coloring), in dev_pre: set before level 0 is spawned
    PreColoring dev_pre;
    std::vector<LevelStage> stage;
    std::vector<std::shared_future<void>> ord_done;
    std::vector<std::future<void>> op_done, tr_done;
    std::shared_future<void> lhs_copied, patches_done;
    std::future<int> stage_ready;
    std::shared_future<bool> factor_done;
    std::atomic<int> colored_ahead{0};             // the level-0 ordering took the colouring made ahead of the verdict (AheadColoring)
    double ms_lhs_copied = 0, ms_h2d = 0;
    clk::time_point t0;
    DevBuf<int> d_rap_err;
    int rc_all = GMG_OK;
    std::string err_all;
};

// placeholder: the set-up of prepare_structure (no dense coarse inverse, no mass: the refresh with the real values brings both)
int set_system_impl(gmg_handle h, int n, const int* colptr, const int* rowidx, const double* val, bool placeholder = false) {
    NEED_DEVICE();
    if (h->L <= 0) return fail(h, GMG_ERR_STATE, "hierarchy has no transfer levels (U is empty)");
    for (int k = 0; k < h->L; ++k) if (!h->U_set[k]) return fail(h, GMG_ERR_STATE, "prolongation matrix missing for level " + std::to_string(k));
    if (n <= 0 || !colptr || !rowidx || !val) return fail(h, GMG_ERR_INVALID, "bad system arguments");
    if (h->U[0].n_inner != n) return fail(h, GMG_ERR_INVALID, "system size does not match U[0]");
    for (int k = 0; k + 1 < h->L; ++k)
        if (h->U[k].n_outer != h->U[k + 1].n_inner) return fail(h, GMG_ERR_INVALID, "U[k] / U[k+1] shapes do not chain");
    auto t_all = clk::now();
    HIPCHK(hipSetDevice(h->cfg.device));
    SystemEntry e;
    int rc = enter_system(h, n, colptr, rowidx, val, t_all, e);
    if (rc != GMG_OK) return rc;
    const bool live = h->live != LiveSystem::none;
    if ((rc = values_only(h, n, e, t_all)) != 1) { if (rc == GMG_OK) h->live_from_copy = false; return rc; }
    // (the resident values were overwritten ahead of the verdict and the pattern turned out to be another one: the live system is gone -- the
    // full set-up drops it anyway; a failure on the way must not leave a system that solves with foreign values)
    if (e.speculative) {
        lose_live_system(h);
        if (e.spec_done && e.rc_spec != GMG_OK) h->err.clear();      // (the refresh ran on a matrix of another pattern: its complaint is about that combination, not about this call)
    }
    if (live && h->live_key_valid && (int)h->lv.size() == h->L + 1) stash_orderings(h);
    h->live_key_valid = false;
    drop_system(h);
    h->lv.resize(h->L + 1);
    FullSetup s(h, e, n, t_all, placeholder);
    if ((rc = s.run()) || (rc = finish_system(h, n, s.ms_factor, s.inverse_built || placeholder, true, placeholder)) || (rc = s.commit())) return rc;
    stamp_done(h, t_all);
    h->timing["setup_structure_prepared"] = 0.0;
    h->live_from_copy = e.colptr != colptr;
    return GMG_OK;
}

// gmg_finalize_hierarchy with a fine graph (gmg_set_fine_graph / gmg_use_hierarchy): the complete set-up for a PLACEHOLDER matrix with the
// graph's pattern -- diagonally dominant (row i: its entry count on the diagonal, -1 elsewhere: symmetric positive definite, and of the sign
// structure of the graph Laplacians the hierarchy is built for, so that the rules that look at values -- gmg_config::block_fine -- decide as
// they will for the real system; a system that makes them decide otherwise takes the cold path).  Everything structural then stands on the
// device: orderings and colourings of all levels, SELL / block layouts, 16-bit column codes, the patterns of the Galerkin operators, the
// symbolic LDL^T.  The handle holds no system afterwards (solves are refused until gmg_set_system), but a gmg_set_system whose pattern
// digest equals the prepared one is a values-only refresh: values up, numeric Galerkin passes, layout refill, numeric LDL^T -- the part of
// the reference's solve() preamble (multigrid_solver.cpp:1387-1401) that depends on the matrix, and nothing else.
int prepare_structure(gmg_handle h) {
    const FineGraph& g = *h->fine_graph;
    const int n = g.n;
    auto t0 = clk::now();
    {   // The systems to come are symmetric (tau M + S): a point graph that is not (the kNN table of a point cloud: j among i's neighbours, i not among
        // j's) is not their pattern -- its placeholder set-up would be paid here and the first real system would take the cold path all the same
        // (round-5 advice).  One threaded pass, a binary search per entry (the rows are sorted).
        std::atomic<bool> symmetric{true};
        parallel_ranges(n, h->cfg.host_threads, [&](int lo, int hi, int) {
            for (int i = lo; i < hi && symmetric.load(std::memory_order_relaxed); ++i)
                for (int p = g.ptr[i]; p < g.ptr[i + 1]; ++p) {
                    const int j = g.idx[p];
                    if (j == i) continue;
                    if (!std::binary_search(g.idx.data() + g.ptr[j], g.idx.data() + g.ptr[j + 1], i)) { symmetric.store(false, std::memory_order_relaxed); break; }
                }
        }, 1 << 14);
        h->timing["structure_prepare_symmetric_graph"] = symmetric.load() ? 1.0 : 0.0;
        if (!symmetric.load()) { h->timing["structure_prepare_ms"] = ms_since(t0); return GMG_OK; }
    }
    RawVec<double> val;
    val.resize((size_t)g.ptr[n]);
    parallel_ranges(n, h->cfg.host_threads, [&](int lo, int hi, int) {
        for (int i = lo; i < hi; ++i) {
            const double diag = (double)(g.ptr[i + 1] - g.ptr[i]);
            for (int p = g.ptr[i]; p < g.ptr[i + 1]; ++p) val[p] = g.idx[p] == i ? diag : -1.0;
        }
    }, 1 << 14);
    const int rc = set_system_impl(h, n, g.ptr.data(), g.idx.data(), val.data(), /*placeholder=*/true);
    if (rc != GMG_OK) return rc;
    if (h->part_world > 1) {
        // a partitioned handle cannot refresh values in place (it keeps no whole operator): what carries over to the real system is what
        // depends on the pattern alone and lives on the host -- the orderings of all levels and the partition plan, both under the digest
        stash_orderings(h);
        h->live_key_valid = false;
        drop_system(h);
        h->pool.trim_large((size_t)4 << 20);
    }
    // nothing to solve with: the values are placeholders
    h->live = h->refill_ready && h->live_key_valid ? LiveSystem::placeholder : LiveSystem::none;
    // (the level vectors of a one-column problem, so that the first solve does not pay their allocation either; a wider block re-allocates)
    if (h->live == LiveSystem::placeholder) { (void)ensure_vectors(h, 1); (void)ensure_rap_order(h); }
    h->mass_dirty = !h->mass.empty();
    h->timing["structure_prepare_ms"] = ms_since(t0);
    return GMG_OK;
}

}  // namespace
