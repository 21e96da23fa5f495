// sbm_capi_verify.inc — part of libsbm_hip.so's host side (included by sbm_capi.hip, one translation unit): the verify
// stage (HCORR of the reference's production driver, test_jabil.cpp:152-207) -- the patch set (sbm_upload_verify_patches),
// the stage over the three kinds of frame source (sbm_verify_batch_device, _ptrs, _planes) and the blocking host sibling
// that runs match, NMS and verify on one upload of the frames (sbm_match_batch_host_verified).
// ---------------------------------------------------------------------------

// The one path of the three entry points: two launches on s, nothing else.  Grows the {score, status} scratch first where
// the call is larger than any before it (synchronises then, as nms_enqueue does for its scratch).
static int verify_enqueue(sbm_ctx* c, hipStream_t s, const FrameSource& src, int rows, int cols, const void* d_recs, const void* d_counts,
                          int64_t cap, const sbm_verify_params* p, void* d_out, void* d_scores, int64_t out_cap, void* d_out_counts)
{
    if (!c || !src.base || !d_recs || !d_counts || !p || !d_out_counts || (out_cap > 0 && (!d_out || !d_scores))) return fail(SBM_ERR_INVALID, "null argument");
    if (cap < 0 || cap > INT32_MAX || out_cap < 0 || src.frames < 1 || src.frames > 65535)
        return fail(SBM_ERR_INVALID, "bad sizes (cap %lld, %d frames, out_cap %lld)", (long long)cap, src.frames, (long long)out_cap);
    if (rows <= 0 || cols <= 0 || (int64_t)rows * cols > INT32_MAX) return fail(SBM_ERR_INVALID, "bad frame size %dx%d", rows, cols);
    if (src.ch != 1 && src.ch != 3) return fail(SBM_ERR_INVALID, "channels must be 1 or 3, got %d", src.ch);
    if (src.stride < cols * (src.kind == FRAMES_PLANES ? 1 : src.ch)) return fail(SBM_ERR_INVALID, "stride %d smaller than a row", src.stride);
    if (src.kind == FRAMES_STRIDED && src.frames > 1 && src.frame_stride < (int64_t)src.stride * rows)
        return fail(SBM_ERR_INVALID, "frame_stride smaller than one frame");
    if (c->n_templates == 0) return fail(SBM_ERR_STATE, "no templates uploaded");
    if (c->verify_gen != c->templates_gen) return fail(SBM_ERR_STATE, "no verify patches uploaded for the current templates (sbm_upload_verify_patches)");
    const size_t want = (size_t)src.frames * (size_t)std::max<int64_t>(cap, 1) * sizeof(VerifySlot);
    if (want > c->d_verify_scratch.cap) {
        HIP_TRY(hipDeviceSynchronize()); // calls in flight may use the old scratch
        if (int e = c->d_verify_scratch.ensure(want)) return e;
    }
    VerifyArgs a;
    a.base = src.base;
    a.kind = (int32_t)src.kind;
    a.ch = src.ch;
    a.rows = rows, a.cols = cols, a.stride = src.stride;
    a.frame_stride = kernel_frame_stride(src);
    a.recs = (const sbm_match_rec*)d_recs;
    a.counts = (const int32_t*)d_counts;
    a.cap = cap;
    a.labels = c->d_verify_labels.as<VerifyLabel>();
    a.n_labels = (int32_t)c->h_verify_labels.size();
    a.patches = c->d_verify_patches.as<uint8_t>();
    a.slots = c->d_verify_scratch.as<VerifySlot>();
    a.min_corr = p->min_corr;
    a.keep_unverified = p->keep_unverified;
    a.out = (sbm_match_rec*)d_out;
    a.scores = (float*)d_scores;
    a.out_cap = out_cap;
    a.out_counts = (int32_t*)d_out_counts;
    if (cap > 0)
        SBM_LAUNCH(c, "k_verify_rois", k_verify_rois, dim3((unsigned)std::min<int64_t>(cap, VERIFY_MAX_SLOTS), (unsigned)src.frames), dim3(VERIFY_ROI_THREADS), 0, s, a);
    SBM_LAUNCH(c, "k_verify_compact", k_verify_compact, dim3((unsigned)src.frames), dim3(VERIFY_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the prologue of the three device entry points
static int verify_begin(sbm_ctx* c, void* stream, hipStream_t* s)
{
    if (!c) return fail(SBM_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    *s = launch_stream(c, stream);
    if (c->profiling && !c->profiling_keep) c->clear_timings();
    return 0;
}

extern "C" {

int sbm_upload_verify_patches(sbm_ctx* c, const sbm_verify_patch* patches, int32_t n)
{
    if (!c || n < 0 || (n && !patches)) return fail(SBM_ERR_INVALID, "bad patch arguments");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    // the labels of the current upload, sorted, with their level-0 sizes
    std::vector<NmsLabel> have((size_t)c->n_templates);
    for (int t = 0; t < c->n_templates; ++t) {
        const DevTL& d = c->h_tls[(size_t)t * c->L];
        have[(size_t)t] = NmsLabel{c->h_class[(size_t)t], c->h_tid[(size_t)t], d.width, d.height};
    }
    auto before = [](const NmsLabel& a, const NmsLabel& b) { return a.cls != b.cls ? a.cls < b.cls : a.tid < b.tid; };
    std::sort(have.begin(), have.end(), before);
    // every patch normalised (rule 2) into one dense store, in the order of the sorted label table
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        const sbm_verify_patch &x = patches[a], &y = patches[b];
        return x.class_idx != y.class_idx ? x.class_idx < y.class_idx : (x.template_id != y.template_id ? x.template_id < y.template_id : a < b);
    });
    std::vector<VerifyLabel> labels((size_t)n);
    int64_t total = 0;
    for (int k = 0; k < n; ++k) {
        const int i = order[(size_t)k];
        const sbm_verify_patch& q = patches[i];
        if (!q.gray) return fail(SBM_ERR_INVALID, "patch %d: null image", i);
        if (k > 0 && patches[order[(size_t)k - 1]].class_idx == q.class_idx && patches[order[(size_t)k - 1]].template_id == q.template_id)
            return fail(SBM_ERR_INVALID, "patch %d: label (%d, %d) is given twice (also by patch %d)", i, q.class_idx, q.template_id, order[(size_t)k - 1]);
        const NmsLabel key{q.class_idx, q.template_id, 0, 0};
        const auto it = std::lower_bound(have.begin(), have.end(), key, before);
        if (it == have.end() || it->cls != q.class_idx || it->tid != q.template_id)
            return fail(SBM_ERR_INVALID, "patch %d: no uploaded template is labelled (%d, %d)", i, q.class_idx, q.template_id);
        if (q.width != it->w || q.height != it->h)
            return fail(SBM_ERR_INVALID, "patch %d: %dx%d is not the level-0 size %dx%d of template (%d, %d)", i, q.width, q.height, it->w, it->h,
                        q.class_idx, q.template_id);
        if (q.stride < q.width) return fail(SBM_ERR_INVALID, "patch %d: stride %d < width %d", i, q.stride, q.width);
        labels[(size_t)k] = VerifyLabel{q.class_idx, q.template_id, q.width, q.height, total, 0};
        total += (int64_t)std::max(q.width, 0) * std::max(q.height, 0);
    }
    std::vector<uint8_t> bytes((size_t)total + VERIFY_PATCH_PAD, 0); // (the kernels read a patch in quads)
    for (int k = 0; k < n; ++k) {
        const sbm_verify_patch& q = patches[order[(size_t)k]];
        VerifyLabel& l = labels[(size_t)k];
        if (l.w > 0 && l.h > 0) l.sbb = verify_normalise_image(q.gray, l.w, l.h, q.stride, bytes.data() + l.off);
    }
    // the new set in buffers of its own, in place of the old one only once it is whole
    DevBuf d_labels, d_bytes;
    if (int e = d_labels.ensure(std::max<size_t>(labels.size(), 1) * sizeof(VerifyLabel))) return e;
    if (int e = d_bytes.ensure(std::max<size_t>(bytes.size(), 1))) return e;
    if (!labels.empty()) HIP_TRY(hipMemcpy(d_labels.p, labels.data(), labels.size() * sizeof(VerifyLabel), hipMemcpyHostToDevice));
    if (!bytes.empty()) HIP_TRY(hipMemcpy(d_bytes.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize()); // calls in flight read the old set, which is freed below
    c->d_verify_labels.swap(d_labels);
    c->d_verify_patches.swap(d_bytes);
    c->h_verify_labels.swap(labels);
    c->verify_patch_bytes = total;
    c->verify_gen = c->templates_gen;
    return 0;
}

int sbm_get_verify_patch(sbm_ctx* c, int32_t class_idx, int32_t template_id, uint8_t* out_host, int64_t cap_bytes, uint64_t* sbb)
{
    if (!c || (cap_bytes > 0 && !out_host) || cap_bytes < 0) return fail(SBM_ERR_INVALID, "bad arguments");
    if (c->verify_gen != c->templates_gen) return fail(SBM_ERR_STATE, "no verify patches uploaded for the current templates");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    for (size_t i = 0; i < c->h_verify_labels.size(); ++i) {
        const VerifyLabel& l = c->h_verify_labels[i];
        if (l.cls != class_idx || l.tid != template_id) continue;
        const int64_t bytes = (int64_t)l.w * l.h;
        if (bytes > cap_bytes) return fail(SBM_ERR_CAPACITY, "patch of %lld bytes exceeds cap_bytes %lld", (long long)bytes, (long long)cap_bytes);
        // (the stored copy the kernels read, label record included)
        VerifyLabel d;
        HIP_TRY(hipMemcpy(&d, c->d_verify_labels.as<VerifyLabel>() + i, sizeof d, hipMemcpyDeviceToHost));
        if (bytes > 0) HIP_TRY(hipMemcpy(out_host, c->d_verify_patches.as<uint8_t>() + d.off, (size_t)bytes, hipMemcpyDeviceToHost));
        if (sbb) *sbb = d.sbb;
        return 0;
    }
    return fail(SBM_ERR_INVALID, "label (%d, %d) has no patch", class_idx, template_id);
}

int sbm_verify_batch_device(sbm_ctx* c, const void* d_imgs, int64_t frame_stride, int32_t n_frames, int32_t rows, int32_t cols, int32_t stride,
                            int32_t channels, const void* d_recs, const void* d_counts, int64_t cap, const sbm_verify_params* p, void* d_out,
                            void* d_scores, int64_t out_cap, void* d_out_counts, void* stream)
{
    hipStream_t s;
    if (int e = verify_begin(c, stream, &s)) return e;
    return verify_enqueue(c, s, strided_frames(d_imgs, stride, channels, n_frames, frame_stride), rows, cols, d_recs, d_counts, cap, p, d_out, d_scores,
                          out_cap, d_out_counts);
}

int sbm_verify_batch_device_ptrs(sbm_ctx* c, const void* d_frame_ptrs, int32_t n_frames, int32_t rows, int32_t cols, int32_t stride, int32_t channels,
                                 const void* d_recs, const void* d_counts, int64_t cap, const sbm_verify_params* p, void* d_out, void* d_scores,
                                 int64_t out_cap, void* d_out_counts, void* stream)
{
    hipStream_t s;
    if (int e = verify_begin(c, stream, &s)) return e;
    if (const int e = frame_ptrs_check(d_frame_ptrs != nullptr, n_frames, cols, stride, channels, 0)) return fail(SBM_ERR_INVALID, "%s", frame_ptrs_error(e));
    return verify_enqueue(c, s, table_frames(FRAMES_TABLE, d_frame_ptrs, stride, channels, n_frames, 0), rows, cols, d_recs, d_counts, cap, p, d_out,
                          d_scores, out_cap, d_out_counts);
}

int sbm_verify_batch_device_planes(sbm_ctx* c, const void* d_plane_ptrs, int32_t n_frames, int32_t rows, int32_t cols, int32_t stride,
                                   const void* d_recs, const void* d_counts, int64_t cap, const sbm_verify_params* p, void* d_out, void* d_scores,
                                   int64_t out_cap, void* d_out_counts, void* stream)
{
    hipStream_t s;
    if (int e = verify_begin(c, stream, &s)) return e;
    if (const int e = frame_planes_check(d_plane_ptrs != nullptr, n_frames, cols, stride, 0)) return fail(SBM_ERR_INVALID, "%s", frame_planes_error(e));
    return verify_enqueue(c, s, table_frames(FRAMES_PLANES, d_plane_ptrs, stride, FPL_CHANNELS, n_frames, 0), rows, cols, d_recs, d_counts, cap, p,
                          d_out, d_scores, out_cap, d_out_counts);
}

int sbm_match_batch_host_verified(sbm_ctx* c, const uint8_t* const* frames, int32_t n_frames, int32_t rows, int32_t cols, int32_t stride,
                                  int32_t channels, float threshold, int64_t cap, const sbm_nms_params* nms, const sbm_verify_params* verify,
                                  sbm_match_rec* out, float* scores, int64_t out_cap, int32_t* counts)
{
    if (!c || !frames || !nms || !verify || !counts || (out_cap > 0 && (!out || !scores))) return fail(SBM_ERR_INVALID, "null argument");
    if (n_frames < 1 || cap < 1 || out_cap < 0) return fail(SBM_ERR_INVALID, "bad batch arguments");
    if (c->pending.active) return fail(SBM_ERR_STATE, "a host batch is in flight (call sbm_match_batch_host_end)");
    if (int e = check_stride(stride, cols, channels)) return e;
    for (int f = 0; f < n_frames; ++f)
        if (!frames[f]) return fail(SBM_ERR_INVALID, "frame %d is null", f);
    if (c->n_templates && c->verify_gen != c->templates_gen)
        return fail(SBM_ERR_STATE, "no verify patches uploaded for the current templates (sbm_upload_verify_patches)");
    const size_t row_bytes = (size_t)cols * channels, frame_bytes = (size_t)rows * row_bytes;
    // the frames, packed, in one block of the context's: all three stages read them there
    MatchCall m{packed_frames(nullptr, rows, cols, channels, n_frames), MaskSource{}, rows, cols, threshold, nullptr, cap, nullptr};
    if (int e = begin_host_match(c, m, c->citems_dirty)) return e;
    const size_t n = (size_t)n_frames, oc = (size_t)std::max<int64_t>(out_cap, 1);
    const size_t raw_bytes = n * (size_t)cap * sizeof(sbm_match_rec), kept_bytes = n * oc * sizeof(sbm_match_rec), score_bytes = n * oc * sizeof(float);
    // raw lists, raw pairs, NMS lists (cap records a frame: the NMS stage cannot run out of room), NMS pairs, kept lists, scores, pairs
    const size_t o_rawc = raw_bytes, o_nms = o_rawc + n * 8, o_nmsc = o_nms + raw_bytes, o_out = o_nmsc + n * 8, o_sc = o_out + kept_bytes,
                 o_outc = o_sc + score_bytes, total = o_outc + n * 8;
    if (int e = c->d_verify_in.ensure(n * frame_bytes)) return e;
    if (int e = c->d_verify_lists.ensure(total)) return e;
    if (n * 8 > c->h_verify_out_bytes) {
        if (c->h_verify_out) (void)hipHostFree(c->h_verify_out);
        c->h_verify_out = nullptr;
        c->h_verify_out_bytes = 0;
        HIP_TRY(hipHostMalloc((void**)&c->h_verify_out, n * 8, hipHostMallocDefault));
        c->h_verify_out_bytes = n * 8;
    }
    char* const d = (char*)c->d_verify_lists.p;
    int rc = 0;
    for (int f = 0; f < n_frames && !rc; ++f) {
        uint8_t* dst = c->d_verify_in.as<uint8_t>() + (size_t)f * frame_bytes;
        const hipError_t he = (size_t)stride == row_bytes ? hipMemcpyAsync(dst, frames[f], frame_bytes, hipMemcpyHostToDevice, c->stream)
                                                          : hipMemcpy2DAsync(dst, row_bytes, frames[f], stride, row_bytes, rows, hipMemcpyHostToDevice, c->stream);
        if (he != hipSuccess) rc = fail(SBM_ERR_HIP, "frame upload failed: %s", hipGetErrorString(he));
    }
    m.src.base = c->d_verify_in.p;
    m.out = (sbm_match_rec*)d;
    m.counts = (int32_t*)(d + o_rawc);
    {
        MirrorScope mirror(c); // the caller's result mirror is none of this call's
        mirror.to(nullptr, nullptr);
        if (!rc) rc = match_or_replay(c, c->stream, m, n_frames);
    }
    if (!rc) rc = nms_enqueue(c, c->stream, d, d + o_rawc, cap, n_frames, 1, 0, nms, d + o_nms, cap, d + o_nmsc);
    if (!rc) rc = verify_enqueue(c, c->stream, m.src, rows, cols, d + o_nms, d + o_nmsc, cap, verify, d + o_out, d + o_sc, out_cap, d + o_outc);
    if (!rc && hipMemcpyAsync(c->h_verify_out, d + o_outc, n * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = fail(SBM_ERR_HIP, "count copy failed");
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail(SBM_ERR_HIP, "hipStreamSynchronize failed");
    if (rc) return rc;
    const int32_t* h = (const int32_t*)c->h_verify_out;
    int bad = -1;
    for (int f = 0; f < n_frames; ++f) {
        counts[2 * f] = h[2 * f];
        counts[2 * f + 1] = h[2 * f + 1];
        const int64_t k = std::min<int64_t>(h[2 * f], out_cap);
        if (k > 0) {
            HIP_TRY(hipMemcpy(out + (size_t)f * out_cap, d + o_out + (size_t)f * oc * sizeof(sbm_match_rec), (size_t)k * sizeof(sbm_match_rec), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(scores + (size_t)f * out_cap, d + o_sc + (size_t)f * oc * sizeof(float), (size_t)k * sizeof(float), hipMemcpyDeviceToHost));
        }
        if ((h[2 * f + 1] & 3) && bad < 0) bad = f;
    }
    if (c->profiling) collect_timings(c);
    if (bad >= 0)
        return fail(SBM_ERR_CAPACITY, "frame %d: flags %d (1: the raw list exceeded the capacity %lld, 2: %d kept records exceed out_cap %lld)", bad,
                    counts[2 * bad + 1], (long long)cap, counts[2 * bad], (long long)out_cap);
    return 0;
}

} // extern "C"
