// sbm_capi_nms.inc — part of libsbm_hip.so's host side (included by sbm_capi.hip, one translation unit): the match
// epilogue + NMS on the device (sbm_nms_batch_device) and its host-batch sibling (sbm_match_batch_host_end_nms).
// ---------------------------------------------------------------------------

// The (class_idx, template_id) -> level-0 (width, height) table of the current upload, built on the first call after an
// upload (synchronises then; never afterwards).  Labels that are not unique within the upload make every call fail.
static int nms_ensure_labels(sbm_ctx* c)
{
    if (c->nms_labels_gen == c->templates_gen) return c->nms_labels_unique ? 0 : fail(SBM_ERR_INVALID, "template labels (class_idx, template_id) are not unique");
    std::vector<NmsLabel> tab((size_t)c->n_templates);
    for (int t = 0; t < c->n_templates; ++t) {
        const DevTL& d = c->h_tls[(size_t)t * c->L];
        tab[(size_t)t] = NmsLabel{c->h_class[(size_t)t], c->h_tid[(size_t)t], d.width, d.height};
    }
    std::sort(tab.begin(), tab.end(), [](const NmsLabel& a, const NmsLabel& b) { return a.cls != b.cls ? a.cls < b.cls : a.tid < b.tid; });
    bool unique = true;
    for (size_t i = 1; i < tab.size(); ++i)
        if (tab[i].cls == tab[i - 1].cls && tab[i].tid == tab[i - 1].tid) unique = false;
    HIP_TRY(hipDeviceSynchronize()); // calls in flight may read the old table
    if (int e = c->d_nms_labels.ensure(std::max<size_t>(tab.size(), 1) * sizeof(NmsLabel))) return e;
    if (!tab.empty()) HIP_TRY(hipMemcpy(c->d_nms_labels.p, tab.data(), tab.size() * sizeof(NmsLabel), hipMemcpyHostToDevice));
    c->nms_n_labels = (int)tab.size();
    c->nms_labels_unique = unique;
    c->nms_labels_gen = c->templates_gen;
    return unique ? 0 : fail(SBM_ERR_INVALID, "template labels (class_idx, template_id) are not unique");
}

static int nms_enqueue(sbm_ctx* c, hipStream_t s, const void* d_recs, const void* d_counts, int64_t cap, int32_t n_frames, int32_t n_parts,
                       int64_t part_stride, const sbm_nms_params* p, void* d_out, int64_t out_cap, void* d_out_counts)
{
    if (!c || !d_recs || !d_counts || !p || !d_out_counts || (out_cap > 0 && !d_out)) return fail(SBM_ERR_INVALID, "null argument");
    if (cap < 0 || n_frames < 1 || n_parts < 1 || out_cap < 0) return fail(SBM_ERR_INVALID, "bad sizes (cap %lld, %d frames, %d parts, out_cap %lld)",
                                                                             (long long)cap, n_frames, n_parts, (long long)out_cap);
    const int64_t N = (int64_t)n_parts * cap;
    if (N > ((int64_t)1 << 28)) return fail(SBM_ERR_INVALID, "n_parts * cap = %lld records per frame exceeds 2^28", (long long)N);
    if (n_parts > 1 && part_stride < (int64_t)n_frames * cap * (int64_t)sizeof(sbm_match_rec))
        return fail(SBM_ERR_INVALID, "part_stride %lld smaller than one part's records", (long long)part_stride);
    if (c->n_templates == 0) return fail(SBM_ERR_STATE, "no templates uploaded");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    if (int e = nms_ensure_labels(c)) return e;
    int64_t frame_bytes = 0;
    if (N > NMS_LDS_MAX) {
        frame_bytes = NMS_SCRATCH_BYTES(N);
        const size_t want = (size_t)frame_bytes * (size_t)n_frames;
        if (want > c->d_nms_scratch.cap) {
            HIP_TRY(hipDeviceSynchronize()); // calls in flight may use the old scratch
            if (int e = c->d_nms_scratch.ensure(want)) return e;
        }
    }
    NmsArgs a;
    a.recs = (const uint8_t*)d_recs;
    a.counts = (const uint8_t*)d_counts;
    a.cap = cap;
    a.part_stride = part_stride;
    a.n_parts = n_parts;
    a.labels = c->d_nms_labels.as<NmsLabel>();
    a.n_labels = c->nms_n_labels;
    a.score_threshold = p->score_threshold;
    a.nms_threshold = p->nms_threshold;
    a.eta = p->eta;
    a.top_k = p->top_k;
    a.out = (sbm_match_rec*)d_out;
    a.out_cap = out_cap;
    a.out_counts = (int32_t*)d_out_counts;
    a.scratch = frame_bytes ? c->d_nms_scratch.as<uint8_t>() : nullptr;
    a.scratch_frame_bytes = frame_bytes;
    SBM_LAUNCH(c, "k_nms_frames", k_nms_frames, dim3((unsigned)n_frames), dim3(NMS_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" {

int sbm_nms_batch_device(sbm_ctx* c, const void* d_recs, const void* d_counts, int64_t cap, int32_t n_frames, int32_t n_parts,
                         int64_t part_stride, const sbm_nms_params* p, void* d_out, int64_t out_cap, void* d_out_counts, void* stream)
{
    if (!c) return fail(SBM_ERR_INVALID, "null context");
    if (c->profiling && !c->profiling_keep) c->clear_timings();
    return nms_enqueue(c, stream ? (hipStream_t)stream : c->stream, d_recs, d_counts, cap, n_frames, n_parts, part_stride, p, d_out, out_cap,
                       d_out_counts);
}

int sbm_match_batch_host_end_nms(sbm_ctx* c, const sbm_nms_params* p, sbm_match_rec* out, int64_t out_cap, int32_t* counts)
{
    if (!c || !p || !counts || (out_cap > 0 && !out)) return fail(SBM_ERR_INVALID, "null argument");
    if (!c->pending.active) return fail(SBM_ERR_STATE, "no host batch in flight");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    c->pending.active = false;
    const int n = c->pending.n_frames;
    const int64_t cap = c->pending.cap;
    const size_t rec_bytes = (size_t)n * (size_t)cap * sizeof(sbm_match_rec);
    int rc = 0;
    if (n > c->h_nms_counts_frames) {
        HIP_TRY(hipStreamSynchronize(c->stream)); // the old pinned block may still be written
        if (c->h_nms_counts) (void)hipHostFree(c->h_nms_counts);
        c->h_nms_counts = nullptr;
        c->h_nms_counts_frames = 0;
        HIP_TRY(hipHostMalloc((void**)&c->h_nms_counts, (size_t)n * 8, hipHostMallocDefault));
        c->h_nms_counts_frames = n;
    }
    if ((rc = c->d_nms_out.ensure((size_t)n * (size_t)std::max<int64_t>(out_cap, 1) * sizeof(sbm_match_rec) + (size_t)n * 8))) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    int32_t* d_cnt = (int32_t*)((char*)c->d_nms_out.p + (size_t)n * (size_t)std::max<int64_t>(out_cap, 1) * sizeof(sbm_match_rec));
    // the batch's lists: n frames of cap records, then the {n_matches, overflow} pairs (sbm_match_batch_host_begin)
    rc = nms_enqueue(c, c->stream, c->d_bout.p, (const char*)c->d_bout.p + rec_bytes, cap, n, 1, 0, p, c->d_nms_out.p, out_cap, d_cnt);
    if (!rc && hipMemcpyAsync(c->h_nms_counts, d_cnt, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = fail(SBM_ERR_HIP, "count copy failed");
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail(SBM_ERR_HIP, "hipStreamSynchronize failed");
    if (rc) return rc;
    int bad = -1;
    for (int f = 0; f < n; ++f) {
        const int32_t k = c->h_nms_counts[2 * f], flags = c->h_nms_counts[2 * f + 1];
        counts[2 * f] = k;
        counts[2 * f + 1] = flags;
        const int64_t m = std::min<int64_t>(k, out_cap);
        if (m > 0)
            HIP_TRY(hipMemcpy(out + (size_t)f * out_cap, c->d_nms_out.as<sbm_match_rec>() + (size_t)f * std::max<int64_t>(out_cap, 1),
                              (size_t)m * sizeof(sbm_match_rec), hipMemcpyDeviceToHost));
        if ((flags & 3) && bad < 0) bad = f;
    }
    if (c->profiling) collect_timings(c);
    if (bad >= 0)
        return fail(SBM_ERR_CAPACITY, "frame %d: flags %d (1: a raw list exceeded the batch capacity %lld, 2: %d kept records exceed out_cap %lld)",
                    bad, counts[2 * bad + 1], (long long)cap, counts[2 * bad], (long long)out_cap);
    return 0;
}

} // extern "C"
