// sbm_capi_match.inc — part of libsbm_hip.so's host side (included by sbm_capi.hip, one translation unit): the C ABI of include/sbm.h -- contexts, templates, selection, the match entry points (host, device, batch, host batch), pinning, pyramid state.
// ---------------------------------------------------------------------------
extern "C" {

const char* sbm_last_error(void) { return g_err.c_str(); }
int sbm_abi_version(void) { return SBM_ABI_VERSION; }

int sbm_create(const sbm_config* cfg, sbm_ctx** out)
{
    if (!cfg || !out) return fail(SBM_ERR_INVALID, "null argument");
    if (cfg->n_levels < 1 || cfg->n_levels > SBM_MAX_LEVELS) return fail(SBM_ERR_INVALID, "n_levels %d out of range", cfg->n_levels);
    for (int l = 0; l < cfg->n_levels; ++l)
        if (cfg->T[l] < 1 || cfg->T[l] > 64) return fail(SBM_ERR_INVALID, "T[%d]=%d out of range", l, cfg->T[l]);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(SBM_ERR_HIP, "no HIP device available: libsbm_hip has no CPU fallback");
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(SBM_ERR_INVALID, "device_id %d out of range (%d devices)", cfg->device_id, ndev);
    HIP_TRY(hipSetDevice(cfg->device_id));
    sbm_ctx* c = new sbm_ctx();
    c->cfg = *cfg;
    c->L = cfg->n_levels;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device_id) == hipSuccess && prop.multiProcessorCount > 0) c->n_simd = 4 * prop.multiProcessorCount;
        else (void)hipGetLastError();
    }
    c->cand_cap = cfg->max_candidates > 0 ? cfg->max_candidates : (int64_t)1 << 20;
    if (c->cand_cap > INT32_MAX / 2) c->cand_cap = INT32_MAX / 2;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(SBM_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
    }
    if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_call, hipEventDisableTiming) != hipSuccess) {
        sbm_destroy(c);
        return fail(SBM_ERR_HIP, "stream/event creation failed");
    }
    for (int l = 0; l < SBM_MAX_LEVELS; ++l)
        if (hipEventCreateWithFlags(&c->ev_fork[l], hipEventDisableTiming) != hipSuccess) {
            sbm_destroy(c);
            return fail(SBM_ERR_HIP, "event creation failed");
        }
    int rc = 0;
    if ((rc = c->d_cands.ensure((size_t)c->cand_cap * sizeof(Cand))) || (rc = c->d_counters.ensure(CTR_STRIDE * sizeof(int32_t) + 256, true)) ||
        (rc = c->d_out.ensure((size_t)c->cand_cap * sizeof(sbm_match_rec))) || (rc = c->d_outcount.ensure(16, true)) ||
        (rc = c->d_call.ensure(CALL_WORDS * sizeof(uint32_t), true))) {
        sbm_destroy(c);
        return rc;
    }
    // the count of match calls enqueued: host memory one thread per launch reads in place.  Without it every call keeps its copy.
    if (hipHostMalloc((void**)&c->h_enqueued, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
        *c->h_enqueued = 0;
        if (hipHostGetDevicePointer((void**)&c->d_enqueued, c->h_enqueued, 0) != hipSuccess) c->d_enqueued = nullptr;
    } else {
        c->h_enqueued = nullptr;
    }
    (void)hipGetLastError();
    *out = c;
    return 0;
}

void sbm_destroy(sbm_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->cfg.device_id);
    (void)hipDeviceSynchronize();
    if (c->comm && g_rccl_destroy_hook) g_rccl_destroy_hook(c);
    for (auto& pr : c->pinned) (void)hipHostUnregister((void*)pr.p); // the caller never unpinned them: still registered by us
    c->pinned.clear();
    for (int i = 0; i < 8; ++i)
        if (c->ev_band[i]) (void)hipEventDestroy(c->ev_band[i]);
    for (int i = 0; i < 2; ++i) {
        if (c->ev_up[i]) (void)hipEventDestroy(c->ev_up[i]);
        if (c->ev_free[i]) (void)hipEventDestroy(c->ev_free[i]);
    }
    if (c->h_bout) (void)hipHostFree(c->h_bout);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->h_res) (void)hipHostFree(c->h_res);
    if (c->h_res_count) (void)hipHostFree(c->h_res_count);
    if (c->h_nms_counts) (void)hipHostFree(c->h_nms_counts);
    if (c->h_verify_out) (void)hipHostFree(c->h_verify_out);
    if (c->h_train_table) (void)hipHostFree(c->h_train_table);
    if (c->h_enqueued) (void)hipHostFree(c->h_enqueued);
    if (c->ev_train_table) (void)hipEventDestroy(c->ev_train_table);
    c->drop_graphs();
    for (int l = 0; l < SBM_MAX_LEVELS; ++l)
        if (c->ev_fork[l]) (void)hipEventDestroy(c->ev_fork[l]);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev_call) (void)hipEventDestroy(c->ev_call);
    if (c->side) (void)hipStreamDestroy(c->side);
    c->clear_timings();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c; // every device buffer frees itself (DevBuf): nothing reads them after the device-wide wait above
}

int sbm_upload_templates(sbm_ctx* c, int32_t n_templates, const sbm_template_level* levels, const sbm_feature* features,
                         int64_t n_features, const int32_t* class_idx, const int32_t* template_id)
{
    if (!c || n_templates < 0 || (n_templates && !levels) || n_features < 0 || (n_features && !features))
        return fail(SBM_ERR_INVALID, "bad template arguments");
    if (n_features >= (int64_t)INT32_MAX) return fail(SBM_ERR_INVALID, "too many features");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    const int L = c->L;
    std::vector<DevTL> tls((size_t)n_templates * L);
    std::vector<uint32_t> fxy((size_t)n_features, 0);
    std::vector<uint8_t> flabel((size_t)n_features, 0), flevel((size_t)n_features, 0);
    std::vector<uint32_t> fext((size_t)n_templates * L, 0); // largest feature x | largest feature y << 16 per template level
    for (int t = 0; t < n_templates; ++t)
        for (int l = 0; l < L; ++l) {
            const sbm_template_level& s = levels[(size_t)t * L + l];
            if (s.n_features < 0 || s.n_features > SBM_MAX_FEATURES) // CV_Error line2Dup.cpp:1195, :1260
                return fail(SBM_ERR_INVALID, "template %d level %d: feature size too large (%d >= 8192)", t, l, s.n_features);
            if (s.feature_offset < 0 || s.feature_offset + s.n_features > n_features)
                return fail(SBM_ERR_INVALID, "template %d level %d: feature range out of bounds", t, l);
            for (int i = 0; i < s.n_features; ++i) {
                const sbm_feature& f = features[s.feature_offset + i];
                if (!feature_in_bounds(f)) // CV_DbgAssert(f.x >= 0 && f.y >= 0), line2Dup.cpp:788-789
                    return fail(SBM_ERR_INVALID, "template %d level %d feature %d: (%d,%d,label %d) outside the supported range", t, l, i, f.x, f.y, f.label);
                fxy[s.feature_offset + i] = (uint32_t)f.x | ((uint32_t)f.y << 16);
                flabel[s.feature_offset + i] = (uint8_t)f.label;
                flevel[s.feature_offset + i] = (uint8_t)l;
                uint32_t& e = fext[(size_t)t * L + l];
                e = std::max(e & 0xffffu, (uint32_t)f.x) | (std::max(e >> 16, (uint32_t)f.y) << 16);
            }
            DevTL d;
            d.width = s.width;
            d.height = s.height;
            d.nf = s.n_features;
            d.feat_off = (int32_t)s.feature_offset;
            tls[(size_t)t * L + l] = d;
        }
    // class-sorted copies for the refinement pass on the strip-interleaved plane (accumulate_rows16_q): inside a
    // template level the features are ordered by (x / T) & 15 (stable), fcls holds the 17 class offsets.  A sum does not
    // care about the order of its terms; every other kernel keeps the caller's order.
    std::vector<uint32_t> fxy_s(fxy);
    std::vector<uint8_t> flabel_s(flabel);
    std::vector<uint16_t> fcls((size_t)n_templates * L * 17, 0);
    for (int t = 0; t < n_templates; ++t)
        for (int l = 0; l < L; ++l) {
            const DevTL& d = tls[(size_t)t * L + l];
            const int T = c->cfg.T[l];
            const int log2t = T == 4 ? 2 : (T == 8 ? 3 : -1);
            uint16_t* cl = &fcls[((size_t)t * L + l) * 17];
            if (log2t < 0) { // never read (the strip plane exists for T = 4 and 8 only)
                for (int k = 1; k <= 16; ++k) cl[k] = (uint16_t)d.nf;
                continue;
            }
            int cnt[17] = {0};
            for (int i = 0; i < d.nf; ++i) ++cnt[(((fxy[d.feat_off + i] & 0xffff) >> log2t) & 15) + 1];
            for (int k = 0; k < 16; ++k) cnt[k + 1] += cnt[k];
            for (int k = 0; k <= 16; ++k) cl[k] = (uint16_t)cnt[k];
            int pos[16];
            for (int k = 0; k < 16; ++k) pos[k] = cnt[k];
            for (int i = 0; i < d.nf; ++i) {
                const int k = ((fxy[d.feat_off + i] & 0xffff) >> log2t) & 15;
                fxy_s[d.feat_off + pos[k]] = fxy[d.feat_off + i];
                flabel_s[d.feat_off + pos[k]] = flabel[d.feat_off + i];
                ++pos[k];
            }
        }
    std::vector<int32_t> cls(n_templates), tid(n_templates);
    for (int t = 0; t < n_templates; ++t) {
        cls[t] = class_idx ? class_idx[t] : 0;
        tid[t] = template_id ? template_id[t] : t;
    }
    HIP_TRY(hipDeviceSynchronize()); // the buffers below may be re-allocated while frames are in flight
    int rc = 0;
    if ((rc = c->d_tls.ensure(tls.size() * sizeof(DevTL))) || (rc = c->d_fxy.ensure(fxy.size() * 4)) ||
        (rc = c->d_flabel.ensure(flabel.size())) || (rc = c->d_flevel.ensure(flevel.size())) ||
        (rc = c->d_foff.ensure(fxy.size() * 4)) || (rc = c->d_class.ensure(cls.size() * 4)) ||
        (rc = c->d_tid.ensure(tid.size() * 4)) || (rc = c->d_fxy_s.ensure(fxy_s.size() * 4)) ||
        (rc = c->d_flabel_s.ensure(flabel_s.size())) || (rc = c->d_fcls.ensure(std::max<size_t>(fcls.size(), 1) * 2)) ||
        (rc = c->d_fext.ensure(std::max<size_t>(fext.size(), 1) * 4)))
        return rc;
    HIP_TRY(hipDeviceSynchronize()); // frames still in flight on the caller's streams read the old tables
    if (!tls.empty()) HIP_TRY(hipMemcpy(c->d_tls.p, tls.data(), tls.size() * sizeof(DevTL), hipMemcpyHostToDevice));
    if (!fxy.empty()) {
        HIP_TRY(hipMemcpy(c->d_fxy.p, fxy.data(), fxy.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_flabel.p, flabel.data(), flabel.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_flevel.p, flevel.data(), flevel.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_fxy_s.p, fxy_s.data(), fxy_s.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_flabel_s.p, flabel_s.data(), flabel_s.size(), hipMemcpyHostToDevice));
    }
    if (!fcls.empty()) HIP_TRY(hipMemcpy(c->d_fcls.p, fcls.data(), fcls.size() * 2, hipMemcpyHostToDevice));
    if (!fext.empty()) HIP_TRY(hipMemcpy(c->d_fext.p, fext.data(), fext.size() * 4, hipMemcpyHostToDevice));
    if (n_templates) {
        HIP_TRY(hipMemcpy(c->d_class.p, cls.data(), cls.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_tid.p, tid.data(), tid.size() * 4, hipMemcpyHostToDevice));
    }
    TemplateCommit k;
    k.n_templates = n_templates;
    k.n_features = n_features;
    k.tls.swap(tls);
    k.fxy.swap(fxy);
    k.cls.swap(cls);
    k.tid.swap(tid);
    return commit_templates(c, k); // (sbm_capi_ctx.inc: the step shared with sbm_upload_templates_device)
}

static int set_active(sbm_ctx* c, std::vector<int32_t>& act)
{
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    HIP_TRY(hipDeviceSynchronize()); // frames in flight read the current selection
    if (int e = c->d_active.ensure(std::max<size_t>(act.size(), 1) * 4)) return e;
    if (!act.empty()) HIP_TRY(hipMemcpy(c->d_active.p, act.data(), act.size() * 4, hipMemcpyHostToDevice));
    c->h_active.swap(act);
    c->citems_dirty = true;
    c->drop_graphs(); // grid sizes depend on the active set
    return 0;
}

int sbm_select_classes(sbm_ctx* c, const int32_t* class_idx, int32_t n)
{
    if (!c || n < 0 || (n && !class_idx)) return fail(SBM_ERR_INVALID, "bad class selection");
    std::vector<int32_t> act;
    select_classes_list(c->h_class.data(), c->n_templates, class_idx, n, act); // (sbm_frame_plan.h: a frame plan builds its lists with it too)
    return set_active(c, act);
}

int sbm_select_range(sbm_ctx* c, int32_t first, int32_t count)
{
    if (!c || first < 0 || count < 0 || first + count > c->n_templates) return fail(SBM_ERR_INVALID, "bad template range");
    std::vector<int32_t> act(count);
    for (int i = 0; i < count; ++i) act[i] = first + i;
    return set_active(c, act);
}

int sbm_select_templates(sbm_ctx* c, const int32_t* idx, int32_t n)
{
    if (!c || n < 0 || (n && !idx)) return fail(SBM_ERR_INVALID, "bad template list");
    std::vector<int32_t> act(idx, idx + n);
    for (int32_t t : act)
        if (t < 0 || t >= c->n_templates) return fail(SBM_ERR_INVALID, "template index %d out of range", t);
    return set_active(c, act);
}

int sbm_partition_templates(sbm_ctx* c, int32_t rows, int32_t cols, const int32_t* idx, int32_t n, int32_t n_shards, int32_t* first,
                            int32_t* count)
{
    if (!c || n_shards < 1 || !first || !count || n < 0 || rows <= 0 || cols <= 0) return fail(SBM_ERR_INVALID, "bad partition arguments");
    // the template list to divide: idx[0..n) if given, else every uploaded template in upload order
    std::vector<int32_t> list;
    if (idx) list.assign(idx, idx + n);
    else {
        list.resize(c->n_templates);
        for (int t = 0; t < c->n_templates; ++t) list[t] = t;
    }
    const int L = c->L, lc = L - 1, T = c->cfg.T[lc];
    const int rl = rows >> lc, cl = cols >> lc, W = cl / T, H = rl / T;
    if (int e = ensure_host_fxy(c)) return e; // (a device install leaves the features on the device)
    // work of a template = byte-adds of its coarse pass (in-bounds features x template_positions, line2Dup.cpp:818-837);
    // at least 1 so that templates without work still spread out
    std::vector<double> cum(list.size() + 1, 0.0);
    for (size_t i = 0; i < list.size(); ++i) {
        const int32_t t = list[i];
        if (t < 0 || t >= c->n_templates) return fail(SBM_ERR_INVALID, "template index %d out of range", t);
        const DevTL& tl = c->h_tls[(size_t)t * L + lc];
        const int npos = host_template_npos(tl, T, W, H);
        const int64_t inb = npos > 0 ? features_in_bounds(c, tl, rl, cl) : 0;
        cum[i + 1] = cum[i] + std::max<double>(1.0, (double)inb * std::max(npos, 0));
    }
    int prev = 0;
    for (int sh = 0; sh < n_shards; ++sh) {
        int end = (int)list.size();
        if (sh + 1 < n_shards) {
            const double target = cum.back() * (sh + 1) / n_shards;
            end = (int)(std::lower_bound(cum.begin(), cum.end(), target) - cum.begin());
            end = std::min(std::max(end, prev), (int)list.size());
        }
        first[sh] = prev;
        count[sh] = end - prev;
        prev = end;
    }
    return 0;
}

int sbm_match_device(sbm_ctx* c, const void* d_img, int32_t rows, int32_t cols, int32_t stride, int32_t channels,
                     const void* d_mask, float threshold, void* d_out, int64_t cap, void* d_count, void* stream)
{
    const MatchCall m{strided_frames(d_img, stride, channels, 1, 0), strided_masks(d_mask, 0), rows, cols, threshold, (sbm_match_rec*)d_out, cap, (int32_t*)d_count};
    if (int e = check_match_call(c, m)) return e;
    hipStream_t s;
    if (int e = begin_match(c, stream, m, &s)) return e;
    return match_or_replay(c, s, m, 0);
}

int sbm_match_batch_device(sbm_ctx* c, const void* d_imgs, int64_t frame_stride, int32_t n_frames, int32_t rows, int32_t cols,
                           int32_t stride, int32_t channels, const void* d_mask, float threshold, void* d_out, int64_t cap,
                           void* d_counts, void* stream)
{
    const MatchCall m{strided_frames(d_imgs, stride, channels, n_frames, frame_stride), strided_masks(d_mask, 0), rows, cols, threshold,
                      (sbm_match_rec*)d_out, cap, (int32_t*)d_counts};
    if (int e = check_match_call(c, m)) return e;
    hipStream_t s;
    if (int e = begin_match(c, stream, m, &s)) return e;
    return match_or_replay(c, s, m, n_frames);
}

int sbm_match_batch_device_masked(sbm_ctx* c, const void* d_imgs, int64_t frame_stride, int32_t n_frames, int32_t rows, int32_t cols,
                                  int32_t stride, int32_t channels, const void* d_masks, int64_t mask_stride, float threshold, void* d_out,
                                  int64_t cap, void* d_counts, void* stream)
{
    if (!d_masks) return fail(SBM_ERR_INVALID, "null masks (sbm_match_batch_device matches without one)");
    const MatchCall m{strided_frames(d_imgs, stride, channels, n_frames, frame_stride), strided_masks(d_masks, mask_stride), rows, cols, threshold,
                      (sbm_match_rec*)d_out, cap, (int32_t*)d_counts};
    if (int e = check_match_call(c, m)) return e;
    hipStream_t s;
    if (int e = begin_match(c, stream, m, &s)) return e;
    return match_or_replay(c, s, m, n_frames);
}

// The frames (and masks) are named by device arrays of addresses that only the level-0 gradient launch reads, on the stream
// (launch_quantize: the table forms of its kernels).  The call travels as every batch call does, its frames a FrameSource of kind
// FRAMES_TABLE that holds the table's address and the flags, its masks a MaskSource of kind MASK_TABLE (sbm_frame_source.h): those
// records are also part of the key of its captured graph, and the tables' contents are no part of it.
int sbm_match_batch_device_ptrs(sbm_ctx* c, const void* d_frame_ptrs, int32_t n_frames, int32_t rows, int32_t cols, int32_t stride,
                                int32_t channels, const void* d_mask_ptrs, int32_t flags, float threshold, void* d_out, int64_t cap,
                                void* d_counts, void* stream)
{
    if (!c || !d_out || !d_counts) return fail(SBM_ERR_INVALID, "null argument");
    if (const int e = frame_ptrs_check(d_frame_ptrs != nullptr, n_frames, cols, stride, channels, flags)) return fail(SBM_ERR_INVALID, "%s", frame_ptrs_error(e));
    const MatchCall m{table_frames(FRAMES_TABLE, d_frame_ptrs, stride, channels, n_frames, flags), table_masks(d_mask_ptrs), rows, cols, threshold,
                      (sbm_match_rec*)d_out, cap, (int32_t*)d_counts};
    hipStream_t s;
    if (int e = begin_match(c, stream, m, &s)) return e;
    return match_or_replay(c, s, m, n_frames);
}

// Planar frames: the table holds three plane addresses per frame and only the level-0 gradient launch reads it (launch_quantize: the
// plane forms of its kernels).  The call travels as a table call does, its frames a FrameSource of kind FRAMES_PLANES with three
// channels (sbm_frame_source.h) -- the kind is part of the key of its captured graph, so a _ptrs graph at the same table address is
// another graph; the masks, if any, are a table of mask addresses as a _ptrs call's are.
int sbm_match_batch_device_planes(sbm_ctx* c, const void* d_plane_ptrs, int32_t n_frames, int32_t rows, int32_t cols, int32_t stride,
                                  const void* d_mask_ptrs, int32_t flags, float threshold, void* d_out, int64_t cap, void* d_counts,
                                  void* stream)
{
    if (!c || !d_out || !d_counts) return fail(SBM_ERR_INVALID, "null argument");
    if (const int e = frame_planes_check(d_plane_ptrs != nullptr, n_frames, cols, stride, flags)) return fail(SBM_ERR_INVALID, "%s", frame_planes_error(e));
    const MatchCall m{table_frames(FRAMES_PLANES, d_plane_ptrs, stride, FPL_CHANNELS, n_frames, flags), table_masks(d_mask_ptrs), rows, cols, threshold,
                      (sbm_match_rec*)d_out, cap, (int32_t*)d_counts};
    hipStream_t s;
    if (int e = begin_match(c, stream, m, &s)) return e;
    return match_or_replay(c, s, m, n_frames);
}

int sbm_match_templates_device(sbm_ctx* c, float threshold, void* d_out, int64_t cap, void* d_count, void* stream)
{
    if (!c || !d_out || !d_count) return fail(SBM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    hipStream_t s = launch_stream(c, stream);
    if (templates_dirty(c, threshold)) HIP_TRY(hipDeviceSynchronize());
    if (c->profiling && !c->profiling_keep) c->clear_timings();
    // no image: the pyramid is the resident one
    const MatchCall m{FrameSource{}, MaskSource{}, c->rows[0], c->cols[0], threshold, (sbm_match_rec*)d_out, cap, (int32_t*)d_count};
    return match_or_replay(c, s, m, -1);
}

int sbm_set_quantize_mode(sbm_ctx* c, int32_t mode, int32_t rows_per_wave)
{
    if (!c || mode < 0 || mode > 2 || rows_per_wave < 0 || rows_per_wave > 4096) return fail(SBM_ERR_INVALID, "bad quantize mode");
    c->quantize_mode = mode;
    c->quantize_hs = rows_per_wave;
    c->drop_graphs(); // captured launches hold the old kernel choice
    return 0;
}

int sbm_set_sparse_list_rows(sbm_ctx* c, int32_t rows_per_item)
{
    if (!c || rows_per_item < -1 || rows_per_item > 4096) return fail(SBM_ERR_INVALID, "bad rows per listed work item");
    c->sparse_list_rows = rows_per_item;
    c->drop_graphs(); // captured launches hold the old grid of the lists
    return 0;
}

int sbm_set_coarse_mode(sbm_ctx* c, int32_t mode)
{
    if (!c || mode < 0 || mode > 4) return fail(SBM_ERR_INVALID, "bad coarse mode");
    c->coarse_mode = mode;
    c->drop_graphs(); // captured launches hold the old kernel choice
    return 0;
}

int sbm_set_refine_bits(sbm_ctx* c, int32_t mode)
{
    if (!c || mode < -1 || mode > 1) return fail(SBM_ERR_INVALID, "bad refinement form");
    c->refine_bits = mode;
    c->drop_graphs(); // captured launches hold the old form
    return 0;
}

int sbm_set_refine_order(sbm_ctx* c, int32_t order)
{
    if (!c || (order != -1 && order != 0 && order != 2)) return fail(SBM_ERR_INVALID, "bad refinement order");
    c->local_order = order;
    c->drop_graphs(); // captured launches hold the old grid
    return 0;
}

int sbm_set_pipeline_depth(sbm_ctx* c, int32_t batches_in_flight)
{
    if (!c || batches_in_flight < 1) return fail(SBM_ERR_INVALID, "bad pipeline depth");
    c->pipeline_depth = batches_in_flight;
    c->drop_graphs(); // captured launches hold the old launch geometry
    return 0;
}

int sbm_set_graph_mode(sbm_ctx* c, int32_t enabled)
{
    if (!c || enabled < -1 || enabled > 1) return fail(SBM_ERR_INVALID, "bad graph mode");
    c->graph_pref = enabled;
    c->auto_graph_off = false;
    c->graph_captures_since_hit = 0;
    c->graph_seen.clear();
    if (enabled == 0) {
        (void)hipDeviceSynchronize();
        c->drop_graphs();
    }
    return 0;
}

int sbm_graph_count(sbm_ctx* c, int32_t* n)
{
    if (!c || !n) return fail(SBM_ERR_INVALID, "null argument");
    *n = (int32_t)c->graphs.size();
    return 0;
}

// the copy stream of the host pipelines and the events that order its two input buffers against the kernels' stream
static int ensure_copy_stream(sbm_ctx* c)
{
    if (c->copy_stream) return 0;
    HIP_TRY(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(hipEventCreateWithFlags(&c->ev_up[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_free[i], hipEventDisableTiming));
    }
    return 0;
}

// The result mirror pointed elsewhere for the length of a scope (a host entry point's own pinned block): the caller's
// mirror (sbm_set_result_mirror) is back on every way out
struct MirrorScope {
    sbm_ctx* c;
    sbm_match_rec* const out;
    int32_t* const count;
    explicit MirrorScope(sbm_ctx* c_) : c(c_), out(c_->mirror_out), count(c_->mirror_count) {}
    MirrorScope(const MirrorScope&) = delete;
    void to(sbm_match_rec* o, int32_t* n) { c->mirror_out = o, c->mirror_count = n; }
    ~MirrorScope() { to(out, count); }
};

static int upload_image(sbm_ctx* c, const uint8_t* img, int rows, int cols, int stride, int ch, const uint8_t* mask)
{
    if (!img) return fail(SBM_ERR_INVALID, "null image");
    if (int e = check_stride(stride, cols, ch)) return e;
    if (int e = ensure_geometry(c, rows, cols, ch)) return e;
    // No implicit pinning: whether the copy below is a direct DMA (the frame lies in memory the caller pinned with
    // sbm_pin_host_buffer / hipHostMalloc / hipHostRegister) or a staged pageable copy is decided by the runtime from
    // the pointer's current attributes, never from a cache of addresses seen before.
    HIP_TRY(hipMemcpy2DAsync(c->d_img[0].p, (size_t)cols * ch, img, stride, (size_t)cols * ch, rows, hipMemcpyHostToDevice, c->stream));
    if (mask) HIP_TRY(hipMemcpyAsync(c->d_mask[0].p, mask, (size_t)rows * cols, hipMemcpyHostToDevice, c->stream));
    return 0;
}

} // extern "C"

// sbm_match_batch_host_begin (mask: one for all frames, or NULL) and sbm_match_batch_host_begin_masked (masks: one pointer per
// frame, a NULL entry = no mask for that frame)
static int host_batch_begin(sbm_ctx* c, const uint8_t* const* frames, int32_t n_frames, int32_t rows, int32_t cols, int32_t stride,
                            int32_t channels, const uint8_t* mask, const uint8_t* const* masks, float threshold, int64_t cap, int32_t sub_batch)
{
    if (!c || !frames || n_frames < 1 || cap < 1) return fail(SBM_ERR_INVALID, "bad batch arguments");
    if (c->pending.active) return fail(SBM_ERR_STATE, "a host batch is already in flight (call sbm_match_batch_host_end)");
    if (int e = check_stride(stride, cols, channels)) return e;
    for (int f = 0; f < n_frames; ++f)
        if (!frames[f]) return fail(SBM_ERR_INVALID, "frame %d is null", f);
    int sub = std::max(1, std::min(sub_batch > 0 ? sub_batch : 8, n_frames));
    const size_t frame_bytes = (size_t)rows * cols * channels, mask_bytes = (size_t)rows * cols;
    // one sub-batch: frames from an input buffer of the pipeline, packed; image, results and frame count follow per sub-batch
    // (and its masks, one per frame, from the mask buffer beside that input buffer)
    MatchCall m{packed_frames(nullptr, rows, cols, channels, sub), MaskSource{}, rows, cols, threshold, nullptr, cap, nullptr};
    if (masks) m.mask.kind = MASK_STRIDED, m.mask.stride = (int64_t)mask_bytes; // (base: the sub-batch's, below)
    if (int e = begin_host_match(c, m, c->citems_dirty)) return e;
    // geometries the one-launch linear-memory builder does not take (level widths that are not multiples of 16, other
    // strides) batch through the any-stride builder (k_build_lm_any) up to T = 16; a pyramid with a larger stride goes one
    // frame per "sub-batch" through the generic kernels -- the uploads still overlap the kernels
    if (!all_rows_ok(c) && !any_batch_ok(c)) sub = 1;
    if (int e = ensure_copy_stream(c)) return e;
    for (int i = 0; i < 2; ++i)
        if (int e = c->d_in[i].ensure((size_t)sub * frame_bytes)) return e;
    for (int i = 0; i < 2 && masks; ++i)
        if (int e = c->d_min[i].ensure((size_t)sub * mask_bytes)) return e;
    // results: n_frames blocks of cap records, then n_frames {n_matches, overflow} pairs -- on the device and in pinned memory
    const size_t rec_bytes = (size_t)n_frames * (size_t)cap * sizeof(sbm_match_rec), total = rec_bytes + (size_t)n_frames * 8;
    if (int e = c->d_bout.ensure(total)) return e;
    if (total > c->h_bout_bytes) {
        if (c->h_bout) (void)hipHostFree(c->h_bout);
        c->h_bout = nullptr;
        c->h_bout_bytes = 0;
        HIP_TRY(hipHostMalloc((void**)&c->h_bout, total, hipHostMallocDefault));
        c->h_bout_bytes = total;
    }
    int32_t* h_counts = (int32_t*)(c->h_bout + rec_bytes);
    for (int f = 0; f < n_frames; ++f) h_counts[2 * f] = -1, h_counts[2 * f + 1] = 0;
    if (mask) {
        HIP_TRY(hipMemcpyAsync(c->d_mask[0].p, mask, (size_t)rows * cols, hipMemcpyHostToDevice, c->stream));
        m.mask = strided_masks(c->d_mask[0].p, 0);
    }
    MirrorScope mirror(c);
    int rc = 0;
    for (int f0 = 0, k = 0; f0 < n_frames && !rc; f0 += sub, ++k) {
        const int nf = std::min(sub, n_frames - f0), buf = k & 1;
        // the kernels of sub-batch k-2 must have finished reading this input buffer
        if (k >= 2 && hipStreamWaitEvent(c->copy_stream, c->ev_free[buf], 0) != hipSuccess) rc = fail(SBM_ERR_HIP, "stream wait failed");
        for (int f = 0; f < nf && !rc;) {
            uint8_t* dst = c->d_in[buf].as<uint8_t>() + (size_t)f * frame_bytes;
            // one DMA per frame when the caller's memory is pinned (sbm_pin_host_buffer / hipHostMalloc); staged by the
            // runtime otherwise -- either way the kernels of the previous sub-batch keep the GPU busy meanwhile.  Frames that
            // follow each other in host memory (a capture ring) travel in ONE copy: a runtime call costs a few microseconds.
            int run = 1;
            if (stride == cols * channels)
                while (f + run < nf && frames[f0 + f + run] == frames[f0 + f + run - 1] + frame_bytes) ++run;
            hipError_t he = stride == cols * channels
                                ? hipMemcpyAsync(dst, frames[f0 + f], (size_t)run * frame_bytes, hipMemcpyHostToDevice, c->copy_stream)
                                : hipMemcpy2DAsync(dst, (size_t)cols * channels, frames[f0 + f], stride, (size_t)cols * channels, rows,
                                                   hipMemcpyHostToDevice, c->copy_stream);
            if (he != hipSuccess) rc = fail(SBM_ERR_HIP, "frame upload failed: %s", hipGetErrorString(he));
            f += run;
        }
        // the sub-batch's masks travel with it; a frame without one gets an all-255 mask (quantize() keeps every pixel)
        for (int f = 0; f < nf && !rc && masks; ++f) {
            uint8_t* dst = c->d_min[buf].as<uint8_t>() + (size_t)f * mask_bytes;
            const hipError_t he = masks[f0 + f] ? hipMemcpyAsync(dst, masks[f0 + f], mask_bytes, hipMemcpyHostToDevice, c->copy_stream)
                                                : hipMemsetAsync(dst, 255, mask_bytes, c->copy_stream);
            if (he != hipSuccess) rc = fail(SBM_ERR_HIP, "mask upload failed: %s", hipGetErrorString(he));
        }
        if (rc) break;
        if (hipEventRecord(c->ev_up[buf], c->copy_stream) != hipSuccess || hipStreamWaitEvent(c->stream, c->ev_up[buf], 0) != hipSuccess) {
            rc = fail(SBM_ERR_HIP, "event record / wait failed");
            break;
        }
        m.src.base = c->d_in[buf].p;
        if (masks) m.mask.base = c->d_min[buf].p;
        m.out = c->d_bout.as<sbm_match_rec>() + (size_t)f0 * cap;
        m.counts = (int32_t*)((char*)c->d_bout.p + rec_bytes) + 2 * f0;
        m.src.frames = nf;
        mirror.to((sbm_match_rec*)c->h_bout + (size_t)f0 * cap, h_counts + 2 * f0);
        rc = enqueue_match(c, c->stream, m);
        if (!rc) call_enqueued(c, c->stream);
        if (!rc && hipEventRecord(c->ev_free[buf], c->stream) != hipSuccess) rc = fail(SBM_ERR_HIP, "event record failed");
    }
    if (rc) {
        (void)hipDeviceSynchronize();
        return rc;
    }
    c->pending.active = true;
    c->pending.n_frames = n_frames;
    c->pending.cap = cap;
    return 0;
}

extern "C" {

int sbm_match_batch_host_begin(sbm_ctx* c, const uint8_t* const* frames, int32_t n_frames, int32_t rows, int32_t cols, int32_t stride,
                               int32_t channels, const uint8_t* mask, float threshold, int64_t cap, int32_t sub_batch)
{
    return host_batch_begin(c, frames, n_frames, rows, cols, stride, channels, mask, nullptr, threshold, cap, sub_batch);
}

int sbm_match_batch_host_begin_masked(sbm_ctx* c, const uint8_t* const* frames, int32_t n_frames, int32_t rows, int32_t cols, int32_t stride,
                                      int32_t channels, const uint8_t* const* masks, float threshold, int64_t cap, int32_t sub_batch)
{
    if (!masks) return fail(SBM_ERR_INVALID, "null mask list (sbm_match_batch_host_begin matches without one)");
    return host_batch_begin(c, frames, n_frames, rows, cols, stride, channels, nullptr, masks, threshold, cap, sub_batch);
}

int sbm_match_batch_host_end(sbm_ctx* c, sbm_match_rec* out, int32_t* counts)
{
    if (!c || !out || !counts) return fail(SBM_ERR_INVALID, "null argument");
    if (!c->pending.active) return fail(SBM_ERR_STATE, "no host batch in flight");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    c->pending.active = false;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int n = c->pending.n_frames;
    const int64_t cap = c->pending.cap;
    const int32_t* h_counts = (const int32_t*)(c->h_bout + (size_t)n * (size_t)cap * sizeof(sbm_match_rec));
    int bad = -1;
    for (int f = 0; f < n; ++f) {
        counts[2 * f] = h_counts[2 * f];
        counts[2 * f + 1] = h_counts[2 * f + 1];
        const int64_t k = std::min<int64_t>(std::max(h_counts[2 * f], 0), cap);
        if (k > 0) memcpy(out + (size_t)f * cap, (const sbm_match_rec*)c->h_bout + (size_t)f * cap, (size_t)k * sizeof(sbm_match_rec));
        if ((h_counts[2 * f] < 0 || h_counts[2 * f] > cap || h_counts[2 * f + 1]) && bad < 0) bad = f;
    }
    if (c->profiling) collect_timings(c);
    if (bad >= 0)
        return fail(SBM_ERR_CAPACITY, "frame %d: %d matches (overflow flag %d) exceed the per-frame capacity %lld", bad, h_counts[2 * bad],
                    h_counts[2 * bad + 1], (long long)cap);
    return 0;
}

int sbm_match_batch_host(sbm_ctx* c, const uint8_t* const* frames, int32_t n_frames, int32_t rows, int32_t cols, int32_t stride,
                         int32_t channels, const uint8_t* mask, float threshold, sbm_match_rec* out, int64_t cap, int32_t* counts,
                         int32_t sub_batch)
{
    if (!out || !counts) return fail(SBM_ERR_INVALID, "null argument");
    if (int e = sbm_match_batch_host_begin(c, frames, n_frames, rows, cols, stride, channels, mask, threshold, cap, sub_batch)) return e;
    return sbm_match_batch_host_end(c, out, counts);
}

int sbm_match_batch_host_masked(sbm_ctx* c, const uint8_t* const* frames, int32_t n_frames, int32_t rows, int32_t cols, int32_t stride,
                                int32_t channels, const uint8_t* const* masks, float threshold, sbm_match_rec* out, int64_t cap,
                                int32_t* counts, int32_t sub_batch)
{
    if (!out || !counts) return fail(SBM_ERR_INVALID, "null argument");
    if (int e = sbm_match_batch_host_begin_masked(c, frames, n_frames, rows, cols, stride, channels, masks, threshold, cap, sub_batch)) return e;
    return sbm_match_batch_host_end(c, out, counts);
}

int sbm_pin_host_buffer(sbm_ctx* c, const void* p, int64_t bytes)
{
    if (!c || !p || bytes <= 0) return fail(SBM_ERR_INVALID, "bad buffer");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    for (auto& pr : c->pinned)
        if (pr.p == (const uint8_t*)p) return fail(SBM_ERR_STATE, "buffer %p is already pinned by this context (unpin it first)", p);
    hipError_t e = hipHostRegister((void*)p, (size_t)bytes, hipHostRegisterPortable); // every device of the process may DMA from it
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(SBM_ERR_HIP, "hipHostRegister(%p, %lld) failed: %s", p, (long long)bytes, hipGetErrorString(e));
    }
    c->pinned.push_back({(const uint8_t*)p, (size_t)bytes});
    return 0;
}

int sbm_unpin_host_buffer(sbm_ctx* c, const void* p)
{
    if (!c || !p) return fail(SBM_ERR_INVALID, "bad buffer");
    for (size_t i = 0; i < c->pinned.size(); ++i)
        if (c->pinned[i].p == (const uint8_t*)p) {
            HIP_TRY(hipSetDevice(c->cfg.device_id));
            HIP_TRY(hipStreamSynchronize(c->stream)); // an upload from it may still be in flight
            hipError_t e = hipHostUnregister((void*)p);
            c->pinned.erase(c->pinned.begin() + i);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                return fail(SBM_ERR_HIP, "hipHostUnregister(%p) failed: %s", p, hipGetErrorString(e));
            }
            return 0;
        }
    return fail(SBM_ERR_STATE, "buffer %p was not pinned by this context", p);
}

// The frame's upload in row bands with level 0's gradient launches following band by band (the latency path of sbm_match:
// one Detector::match(cv::Mat) is upload + kernels + one synchronisation, and the upload -- 55 us for a 1024^2 BGR frame --
// used to be serial with the kernels).  The copies go to a copy stream, one event per band; the context's stream waits for
// band j and launches the rows of 16 x 64 tiles whose 5-row halo has arrived (all but the band's last tile row; after the
// last band everything that is left).  A tile reads the source rows it needs and nothing else, so the orientation map and
// the fused cv::pyrDown output are those of the whole-level launch.  Returns 0 with *done = false when the geometry takes
// the plain path (small frames, the row-streaming kernel, SBM_MATCH_BANDS unset).  OFF by default: it was built to take the
// upload off the critical path (VERDICT round 3, item 6) and measured SLOWER on ROCm 7.2 -- each band's hipMemcpy2DAsync +
// event record + cross-stream wait costs 16 - 30 us: 115 us per Detector::match with one copy, 141 / 177 / 247 us with 2 /
// 4 / 8 bands (tools/r04_latency.sh).  Kept behind the knob, with its parity tests, for a runtime where that overhead is gone.
static int upload_image_banded(sbm_ctx* c, const uint8_t* img, int rows, int cols, int stride, int ch, const uint8_t* mask, bool* done)
{
    *done = false;
    const int NB = tuning().match_bands;
    const int n_tile_rows = (rows + QT_R - 1) / QT_R;
    if (NB < 2 || n_tile_rows < 4 * NB || quantize_stream_rows(c, rows, cols, packed_frames(nullptr, rows, cols, ch, 1), MaskSource{}, false) != 0) return 0;
    if (!img) return fail(SBM_ERR_INVALID, "null image");
    if (int e = check_stride(stride, cols, ch)) return e;
    if (int e = ensure_geometry(c, rows, cols, ch)) return e;
    if (int e = ensure_copy_stream(c)) return e;
    for (int j = 0; j < NB; ++j)
        if (!c->ev_band[j]) HIP_TRY(hipEventCreateWithFlags(&c->ev_band[j], hipEventDisableTiming));
    if (mask) HIP_TRY(hipMemcpyAsync(c->d_mask[0].p, mask, (size_t)rows * cols, hipMemcpyHostToDevice, c->stream));
    uint8_t* d = c->d_img[0].as<uint8_t>();
    const size_t row_bytes = (size_t)cols * ch;
    int t_lo = 0;
    for (int j = 0; j < NB; ++j) {
        const int r0 = std::min(rows, n_tile_rows * j / NB * QT_R), r1 = j + 1 == NB ? rows : std::min(rows, n_tile_rows * (j + 1) / NB * QT_R);
        HIP_TRY(hipMemcpy2DAsync(d + (size_t)r0 * row_bytes, row_bytes, img + (size_t)r0 * stride, stride, row_bytes, r1 - r0, hipMemcpyHostToDevice,
                                 c->copy_stream));
        HIP_TRY(hipEventRecord(c->ev_band[j], c->copy_stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_band[j], 0));
        const int t_hi = j + 1 == NB ? n_tile_rows : r1 / QT_R - 1; // the band's last tile row needs the next band's first rows
        if (t_hi > t_lo) {
            QuantizeLaunch q;
            q.src = level_frames(c, 0, 1);
            q.mask = strided_masks(mask ? c->d_mask[0].p : nullptr, 0);
            q.rows = rows, q.cols = cols;
            q.weak = c->cfg.weak_threshold;
            q.out = c->d_quant[0].as<uint8_t>();
            q.pyr = c->L > 1 ? c->d_img[1].as<uint8_t>() : nullptr;
            q.row_lo = t_lo * QT_R, q.row_hi = std::min(rows, t_hi * QT_R);
            q.tile_band = true;
            if (int e = launch_quantize(c, c->stream, q)) return e;
            t_lo = t_hi;
        }
    }
    *done = true;
    return 0;
}

int sbm_match(sbm_ctx* c, const uint8_t* img, int32_t rows, int32_t cols, int32_t stride, int32_t channels,
              const uint8_t* mask, float threshold, sbm_match_rec* out, int64_t cap, int64_t* n_out)
{
    if (!c || (!out && cap > 0) || !n_out) return fail(SBM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    if (int e = order_after_caller_work(c)) return e;
    if (c->profiling && !c->profiling_keep) c->clear_timings();
    bool l0_done = false;
    if (int e = upload_image_banded(c, img, rows, cols, stride, channels, mask, &l0_done)) return e;
    if (!l0_done)
        if (int e = upload_image(c, img, rows, cols, stride, channels, mask)) return e;
    if (int e = prepare_templates(c, threshold, c->cand_cap)) return e;
    // results: the emitting kernel also stores every record and the final {count, overflow} pair into pinned host
    // memory, so one stream synchronisation ends the call; lists longer than the pinned buffer take the copy path
    bool own_mirror = false;
    if (!c->mirror_out) {
        if (!c->h_res) {
            c->h_res_cap = 4096;
            if (hipHostMalloc((void**)&c->h_res, (size_t)c->h_res_cap * sizeof(sbm_match_rec), hipHostMallocDefault) != hipSuccess ||
                hipHostMalloc((void**)&c->h_res_count, 16, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                if (c->h_res) (void)hipHostFree(c->h_res);
                c->h_res = nullptr;
                c->h_res_count = nullptr;
            }
        }
        own_mirror = c->h_res && c->h_res_count;
    }
    // with the pinned mirror the emitting kernel's record capacity is the pinned buffer's (it bounds both copies)
    const int64_t dev_cap = own_mirror ? std::min<int64_t>(c->cand_cap, c->h_res_cap) : c->cand_cap;
    const MatchCall m{level_frames(c, 0, 1), strided_masks(mask ? c->d_mask[0].p : nullptr, 0), rows, cols, threshold,
                      c->d_out.as<sbm_match_rec>(), dev_cap, c->d_outcount.as<int32_t>()};
    {
        MirrorScope mirror(c);
        if (own_mirror) {
            c->h_res_count[0] = -1;
            c->h_res_count[1] = 0;
            mirror.to(c->h_res, c->h_res_count);
        }
        if (int e = enqueue_match(c, c->stream, m, nullptr, l0_done)) return e;
        call_enqueued(c, c->stream);
    }
    if (own_mirror) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        const int n = c->h_res_count[0];
        if (n >= 0 && c->h_res_count[1] == 0 && n <= dev_cap) {
            *n_out = n;
            if (n > cap) return fail(SBM_ERR_CAPACITY, "%d matches exceed the output capacity %lld", n, (long long)cap);
            if (n > 0) memcpy(out, c->h_res, (size_t)n * sizeof(sbm_match_rec));
            if (c->profiling) collect_timings(c);
            return 0;
        }
        // more records than the pinned buffer holds (or a candidate overflow to report): run the template loop again on
        // the resident pyramid with the full device capacity and take the copy path
        if (int e = enqueue_loop(c, c->stream, m.out, c->cand_cap, m.counts, 1, false)) return e;
    }
    const int rc = fetch_results(c, c->stream, out, cap, n_out);
    if (c->profiling) collect_timings(c);
    return rc;
}

static int rec_cmp(const sbm_match_rec& x, const sbm_match_rec& y)
{
    if (x.similarity != y.similarity) return x.similarity > y.similarity ? -1 : 1;
    if (x.template_id != y.template_id) return x.template_id < y.template_id ? -1 : 1;
    if (x.class_idx != y.class_idx) return x.class_idx < y.class_idx ? -1 : 1;
    if (x.y != y.y) return x.y < y.y ? -1 : 1;
    if (x.x != y.x) return x.x < y.x ? -1 : 1;
    return 0;
}

int64_t sbm_canonicalize(sbm_match_rec* recs, int64_t n)
{
    if (!recs || n <= 0) return 0;
    std::sort(recs, recs + n, [](const sbm_match_rec& a, const sbm_match_rec& b) { return rec_cmp(a, b) < 0; });
    int64_t k = 1;
    for (int64_t i = 1; i < n; ++i)
        if (rec_cmp(recs[i], recs[k - 1]) != 0) recs[k++] = recs[i];
    return k;
}

int sbm_build_pyramid(sbm_ctx* c, const uint8_t* img, int32_t rows, int32_t cols, int32_t stride, int32_t channels,
                      const uint8_t* mask)
{
    if (!c) return fail(SBM_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    if (int e = order_after_caller_work(c)) return e;
    if (c->profiling && !c->profiling_keep) c->clear_timings();
    if (int e = upload_image(c, img, rows, cols, stride, channels, mask)) return e;
    if (int e = enqueue_pyramid(c, c->stream, level_frames(c, 0, 1), strided_masks(mask ? c->d_mask[0].p : nullptr, 0))) return e;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->profiling) collect_timings(c);
    return 0;
}

int sbm_set_quantized(sbm_ctx* c, int32_t level, const uint8_t* q, int32_t rows, int32_t cols)
{
    if (!c || !q || level < 0 || level >= c->L) return fail(SBM_ERR_INVALID, "bad level");
    if (level > c->rec.levels_valid) return fail(SBM_ERR_STATE, "levels must be set from 0 upwards");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    if (int e = order_after_caller_work(c)) return e;
    if (int e = ensure_level(c, level, rows, cols)) return e;
    if (c->profiling && !c->profiling_keep && level == 0) c->clear_timings();
    // (a sparse call's other frames stay readable: their maps are completed before frame 0's is replaced)
    if (level == 0)
        if (int e = ensure_level0_map(c, c->stream)) return e;
    HIP_TRY(hipMemcpyAsync(c->d_quant[level].p, q, (size_t)rows * cols, hipMemcpyHostToDevice, c->stream));
    if (int e = launch_build_lm(c, c->stream, level)) return e;
    c->rec.forms[level].set(LM_PLANES8);
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->rec.levels_valid = std::max(c->rec.levels_valid, level + 1);
    if (c->profiling) collect_timings(c);
    return 0;
}

int sbm_get_quantized(sbm_ctx* c, int32_t level, uint8_t* out)
{
    if (!c || !out || level < 0 || level >= c->rec.levels_valid) return fail(SBM_ERR_STATE, "level not resident");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    if (int e = order_after_caller_work(c)) return e;
    if (level == 0)
        if (int e = ensure_level0_map(c, c->stream)) return e;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->d_quant[level].p, (size_t)c->rows[level] * c->cols[level], hipMemcpyDeviceToHost));
    return 0;
}

int sbm_get_quantized_frame(sbm_ctx* c, int32_t level, int32_t frame, uint8_t* out)
{
    if (!c || !out) return fail(SBM_ERR_INVALID, "null argument");
    if (level < 0 || level >= c->rec.levels_valid) return fail(SBM_ERR_STATE, "level not resident");
    if (frame < 0 || frame >= c->rec.last_frames) return fail(SBM_ERR_INVALID, "frame %d outside the last batch (%d frames)", frame, c->rec.last_frames);
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    HIP_TRY(hipDeviceSynchronize()); // the batch may have been built on the caller's stream
    if (level == 0) { // a sparse call left the map in pieces: the whole launch on the retained source, once
        if (int e = ensure_level0_map(c, c->stream)) return e;
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    const size_t n = (size_t)c->rows[level] * c->cols[level];
    HIP_TRY(hipMemcpy(out, c->d_quant[level].as<uint8_t>() + (size_t)frame * n, n, hipMemcpyDeviceToHost));
    return 0;
}

int sbm_get_linear_memories(sbm_ctx* c, int32_t level, uint8_t* out, int64_t cap_bytes, int64_t* lm_stride)
{
    if (!c || level < 0 || level >= c->rec.levels_valid) return fail(SBM_ERR_STATE, "level not resident");
    if (lm_stride) *lm_stride = c->lm_stride[level];
    if (!out) return 0;
    const int64_t need = 8 * c->lm_stride[level];
    if (cap_bytes < need) return fail(SBM_ERR_CAPACITY, "need %lld bytes", (long long)need);
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    HIP_TRY(hipDeviceSynchronize()); // the pyramid may have been built on the caller's stream
    if (int e = ensure_full_lm(c, level, c->stream)) return e;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->d_lm[level].p, (size_t)need, hipMemcpyDeviceToHost));
    return 0;
}

int sbm_get_coarse_bitplanes(sbm_ctx* c, int32_t frame, uint8_t* out, int64_t cap_bytes)
{
    if (!c || !out || frame < 0 || frame >= c->batch) return fail(SBM_ERR_INVALID, "bad argument");
    if (c->rec.levels_valid < c->L) return fail(SBM_ERR_STATE, "pyramid not built");
    const int64_t need = 2 * c->lm_stride[c->L - 1];
    if (cap_bytes < need) return fail(SBM_ERR_CAPACITY, "need %lld bytes", (long long)need);
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    HIP_TRY(hipDeviceSynchronize());
    if (!c->rec.forms[c->L - 1].bit_planes || !c->d_blm.p) return fail(SBM_ERR_STATE, "the last call did not build the coarsest level's bit planes");
    HIP_TRY(hipMemcpy(out, c->d_blm.as<uint8_t>() + (size_t)frame * need, (size_t)need, hipMemcpyDeviceToHost));
    return 0;
}

int sbm_get_coarse_form(sbm_ctx* c, int32_t out[4])
{
    if (!c || !out) return fail(SBM_ERR_INVALID, "null argument");
    memcpy(out, c->rec.coarse_form, sizeof c->rec.coarse_form);
    return 0;
}

int sbm_get_refine_form(sbm_ctx* c, int32_t level, int32_t out[6])
{
    if (!c || !out) return fail(SBM_ERR_INVALID, "null argument");
    if (level < 0 || level >= c->L - 1) return fail(SBM_ERR_INVALID, "level %d is no refinement level", level);
    memcpy(out, c->rec.refine_form[level], sizeof c->rec.refine_form[level]);
    return 0;
}

int sbm_get_source_form(sbm_ctx* c, int32_t* out)
{
    if (!c || !out) return fail(SBM_ERR_INVALID, "null argument");
    *out = c->rec.source_form;
    return 0;
}

int sbm_get_source_retention(sbm_ctx* c, int32_t out[2])
{
    if (!c || !out) return fail(SBM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    HIP_TRY(hipDeviceSynchronize()); // the totals are the device's: every call enqueued has been counted
    uint32_t w[CALL_WORDS];
    HIP_TRY(hipMemcpy(w, c->d_call.p, sizeof w, hipMemcpyDeviceToHost));
    out[0] = (int32_t)w[CALL_RETAINED], out[1] = (int32_t)w[CALL_SKIPPED];
    return 0;
}

int sbm_get_sparse_items(sbm_ctx* c, int32_t out[3])
{
    if (!c || !out) return fail(SBM_ERR_INVALID, "null argument");
    if (c->rec.sparse_items_pending) { // the profiled launch counted on the device: fetch it once
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(&c->rec.sparse_items[1], c->d_sparse_items.p, sizeof(int32_t), hipMemcpyDeviceToHost));
        c->rec.sparse_items_pending = false;
    }
    memcpy(out, c->rec.sparse_items, sizeof c->rec.sparse_items);
    return 0;
}

int sbm_get_sparse_list(sbm_ctx* c, int32_t out[3])
{
    if (!c || !out) return fail(SBM_ERR_INVALID, "null argument");
    memcpy(out, c->rec.sparse_list, sizeof c->rec.sparse_list);
    return 0;
}

int sbm_get_level_build(sbm_ctx* c, int32_t level, int32_t out[6])
{
    if (!c || !out) return fail(SBM_ERR_INVALID, "null argument");
    if (level < 0 || level >= c->L) return fail(SBM_ERR_INVALID, "level %d of %d", level, c->L);
    const LevelForms& f = c->rec.forms[level];
    const LevelBuild& b = c->rec.level_build[level];
    out[0] = (f.planes8 ? 1 : 0) | (f.spread ? 2 : 0) | (f.spread && f.spread_strip ? 4 : 0) | (f.bit_strips ? 8 : 0) | (f.bit_planes ? 16 : 0);
    out[1] = b.form, out[2] = b.builder, out[3] = b.split, out[4] = b.allty, out[5] = b.packed;
    return 0;
}

int sbm_get_level_stored(sbm_ctx* c, int32_t level, int32_t frame, int32_t which, uint8_t* out, int64_t cap_bytes, int64_t* bytes)
{
    if (!c || !bytes) return fail(SBM_ERR_INVALID, "null argument");
    if (level < 0 || level >= c->L || which < 0 || which > 3 || (which == 3 && level != 0))
        return fail(SBM_ERR_INVALID, "no buffer %d at level %d", which, level);
    const DevBuf& buf = which == 0 ? c->d_lm[level] : which == 1 ? c->d_lmc[level] : which == 2 ? c->d_lbits[level] : c->d_tiles;
    if (!buf.p) return fail(SBM_ERR_STATE, "buffer %d of level %d is not allocated", which, level);
    if (frame < 0 || frame >= c->rec.last_frames) return fail(SBM_ERR_INVALID, "frame %d outside the last batch (%d frames)", frame, c->rec.last_frames);
    const int T = c->cfg.T[level];
    const int64_t need = which == 0   ? 8 * c->lm_stride[level]
                         : which == 1 ? c->lm_stride[level]
                         : which == 2 ? lbits_frame_bytes(c, level)
                                      : (int64_t)refine_tile_count(c->cols[0] / T, c->rows[0] / T);
    *bytes = need;
    if (!out) return 0;
    if (cap_bytes < need) return fail(SBM_ERR_CAPACITY, "need %lld bytes", (long long)need);
    if ((int64_t)(frame + 1) * need > (int64_t)buf.cap) return fail(SBM_ERR_STATE, "buffer %d of level %d holds no frame %d", which, level, frame);
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    HIP_TRY(hipDeviceSynchronize()); // the batch may have been built on the caller's stream
    HIP_TRY(hipMemcpy(out, (const uint8_t*)buf.p + (size_t)frame * need, (size_t)need, hipMemcpyDeviceToHost));
    return 0;
}

int sbm_level_dims(sbm_ctx* c, int32_t level, int32_t* rows, int32_t* cols)
{
    if (!c || level < 0 || level >= c->rec.levels_valid) return fail(SBM_ERR_STATE, "level not resident");
    if (rows) *rows = c->rows[level];
    if (cols) *cols = c->cols[level];
    return 0;
}

int sbm_match_templates(sbm_ctx* c, float threshold, sbm_match_rec* out, int64_t cap, int64_t* n_out)
{
    if (!c || (!out && cap > 0) || !n_out) return fail(SBM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    if (int e = order_after_caller_work(c)) return e;
    if (c->profiling && !c->profiling_keep) c->clear_timings();
    if (int e = enqueue_templates(c, c->stream, threshold, c->d_out.as<sbm_match_rec>(), c->cand_cap, c->d_outcount.as<int32_t>())) return e;
    int rc = fetch_results(c, c->stream, out, cap, n_out);
    if (c->profiling) collect_timings(c);
    return rc;
}

