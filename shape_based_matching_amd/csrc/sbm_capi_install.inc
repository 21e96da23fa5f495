// sbm_capi_install.inc — part of libsbm_hip.so's host side (included by sbm_capi.hip, one translation unit): trained pyramids in
// device memory as the context's template set (sbm_upload_templates_device), and the accessors that read a set back
// (sbm_get_templates, sbm_get_template_table).  The rules are sbm_install_plan.h's, the kernels sbm_install_kernels.h's.

namespace {

const char* install_fault_text(int fault)
{
    return fault == INSTALL_LEVEL_COUNT ? "n_features outside 0 .. 8191 (feature size too large)" : "its features leave the pyramid's block [0, feat_cap)";
}

// the header as the kernels left it, after everything enqueued on the stream so far
int install_read_header(sbm_ctx* c, hipStream_t s, InstallHeader* h)
{
    HIP_TRY(hipMemcpyAsync(h, c->d_install.p, sizeof *h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

} // namespace

extern "C" {

int sbm_upload_templates_device(sbm_ctx* c, const sbm_template_source* sources, int32_t n_sources, int32_t* template_index_out, void* stream)
{
    if (!c || !sources) return fail(SBM_ERR_INVALID, "null argument");
    const int L = c->L;
    const InstallPlan p = install_plan(sources, n_sources, L);
    if (p.error) {
        if (p.error_source < 0) return fail(SBM_ERR_INVALID, "%d sources: %s", n_sources, install_error(p.error));
        return fail(SBM_ERR_INVALID, "source %d: %s", p.error_source, install_error(p.error));
    }
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    hipStream_t s = launch_stream(c, stream);
    const int64_t P = p.n_pyramids, S = n_sources;
    sbm_ctx::TemplateTables& st = c->staged;
    int rc = 0;
    // the scratch and the staged tables belong to this call alone (it ends with a device-wide wait); what the scan writes is
    // sized for every pyramid kept
    if ((rc = c->d_install.ensure((size_t)p.total)) || (rc = st.tls.ensure((size_t)std::max<int64_t>(P * L, 1) * sizeof(DevTL))) ||
        (rc = st.cls.ensure((size_t)std::max<int64_t>(P, 1) * 4)) || (rc = st.tid.ensure((size_t)std::max<int64_t>(P, 1) * 4)))
        return rc;
    uint8_t* d = c->d_install.as<uint8_t>();
    std::vector<uint8_t> head((size_t)p.o_index, 0); // the header, the table of sources, the zeroed per-source counts
    InstallHeader h{};
    h.level_verdict = INSTALL_NO_LEVEL_FAULT;
    h.feature_verdict = INSTALL_NO_FEATURE_FAULT;
    memcpy(head.data() + p.o_header, &h, sizeof h);
    memcpy(head.data() + p.o_table, p.table.data(), (size_t)S * sizeof(InstallSource));
    HIP_TRY(hipMemcpyAsync(d, head.data(), head.size(), hipMemcpyHostToDevice, s));
    if (c->profiling && !c->profiling_keep) c->clear_timings();
    InstallHeader* d_hdr = (InstallHeader*)(d + p.o_header);
    const InstallItem* d_items = (const InstallItem*)(d + p.o_items);
    SBM_LAUNCH(c, "k_install_scan", k_install_scan, dim3(1), dim3(INSTALL_CHUNK), 0, s, (const InstallSource*)(d + p.o_table), (int)S, (int)P, L, d_hdr,
               (int32_t*)(d + p.o_index), (InstallItem*)(d + p.o_items), (int32_t*)(d + p.o_src_t0), (int32_t*)(d + p.o_src_kept),
               (int32_t*)(d + p.o_src_base), st.tls.as<DevTL>(), st.cls.as<int32_t>(), st.tid.as<int32_t>());
    HIP_TRY(hipGetLastError());
    if ((rc = install_read_header(c, s, &h))) return rc; // (the host block above has left by now too)
    if (h.level_verdict != INSTALL_NO_LEVEL_FAULT) {
        const InstallWhere w = install_where_level(p, h.level_verdict);
        return fail(SBM_ERR_INVALID, "source %d pyramid %d level %d: %s", w.source, w.pyramid, w.level, install_fault_text(w.fault));
    }
    if (h.total_features >= (int64_t)INT32_MAX) return fail(SBM_ERR_INVALID, "too many features (%lld)", (long long)h.total_features);
    const int32_t K = h.n_kept;
    const int64_t NF = h.total_features;
    // what the host plans with: the kept flags and the kept pyramids' level records -- O(pyramids), never a feature
    std::vector<int32_t> index((size_t)P);
    TemplateCommit k;
    k.tls.resize((size_t)K * L);
    if (P) HIP_TRY(hipMemcpy(index.data(), d + p.o_index, (size_t)P * 4, hipMemcpyDeviceToHost));
    if (K) HIP_TRY(hipMemcpy(k.tls.data(), st.tls.p, k.tls.size() * sizeof(DevTL), hipMemcpyDeviceToHost));
    if ((rc = st.fxy.ensure((size_t)std::max<int64_t>(NF, 1) * 4)) || (rc = st.flabel.ensure((size_t)std::max<int64_t>(NF, 1))) ||
        (rc = st.flevel.ensure((size_t)std::max<int64_t>(NF, 1))) || (rc = st.fxy_s.ensure((size_t)std::max<int64_t>(NF, 1) * 4)) ||
        (rc = st.flabel_s.ensure((size_t)std::max<int64_t>(NF, 1))) ||
        (rc = st.fcls.ensure((size_t)std::max<int64_t>((int64_t)K * L * (INSTALL_CLASSES + 1), 1) * 2)) ||
        (rc = st.fext.ensure((size_t)std::max<int64_t>((int64_t)K * L, 1) * 4)))
        return rc;
    if (K) {
        InstallGeo geo{};
        for (int l = 0; l < L; ++l) geo.log2t[l] = install_log2t(c->cfg.T[l]);
        SBM_LAUNCH(c, "k_install_features", k_install_features, dim3((unsigned)((int64_t)K * L)), dim3(INSTALL_CHUNK), 0, s, d_items,
                   (const DevTL*)st.tls.p, L, geo, d_hdr, st.fxy.as<uint32_t>(), st.flabel.as<uint8_t>(), st.flevel.as<uint8_t>(), st.fxy_s.as<uint32_t>(),
                   st.flabel_s.as<uint8_t>(), st.fcls.as<uint16_t>(), st.fext.as<uint32_t>());
        HIP_TRY(hipGetLastError());
    }
    if ((rc = install_read_header(c, s, &h))) return rc;
    std::vector<int32_t> kept_pyramid((size_t)K); // template -> flat pyramid
    std::vector<uint8_t> kept((size_t)P);
    for (int64_t j = 0; j < P; ++j) {
        kept[(size_t)j] = index[(size_t)j] >= 0;
        if (index[(size_t)j] >= 0 && index[(size_t)j] < K) kept_pyramid[(size_t)index[(size_t)j]] = (int32_t)j;
    }
    if (K && h.feature_verdict != INSTALL_NO_FEATURE_FAULT) {
        int32_t feature = 0;
        const int64_t rec = install_where_feature(&k.tls[0].feat_off, 4,(int64_t)K * L, h.feature_verdict, &feature);
        const int32_t j = kept_pyramid[(size_t)(rec / L)];
        const int src = install_source_of(p.table.data(), (int)S, j);
        return fail(SBM_ERR_INVALID, "source %d pyramid %d level %d feature %d: outside the supported range (x, y in 0 .. 65535, label 0 .. 7)", src,
                    j - p.table[(size_t)src].pyr_first, (int)(rec % L), feature);
    }
    // class and id of the kept pyramids, by the rule the scan kernel follows (sbm_install_math.h)
    std::vector<int32_t> cls_of((size_t)P);
    for (int64_t sidx = 0; sidx < S; ++sidx)
        for (int32_t i = 0; i < p.table[(size_t)sidx].n_pyramids; ++i) cls_of[(size_t)(p.table[(size_t)sidx].pyr_first + i)] = p.table[(size_t)sidx].class_idx;
    k.cls.resize((size_t)K);
    k.tid.resize((size_t)K);
    if (install_number(kept.data(), cls_of.data(), P, nullptr, k.cls.data(), k.tid.data()) != K) return fail(SBM_ERR_STATE, "kept flags and count disagree");
    HIP_TRY(hipDeviceSynchronize()); // frames still in flight on other streams read the live tables
    c->caller_work = false;
    if ((rc = c->d_foff.ensure((size_t)std::max<int64_t>(NF, 0) * 4))) return rc;
    k.n_templates = K;
    k.n_features = NF;
    k.fxy_valid = false;
    k.staged = true;
    if ((rc = commit_templates(c, k))) return rc;
    if (template_index_out)
        for (int64_t j = 0; j < P; ++j) template_index_out[j] = index[(size_t)j];
    return 0;
}

int sbm_get_templates(sbm_ctx* c, sbm_template_level* levels_out, sbm_feature* feats_out, int64_t feat_cap, int32_t* class_idx_out,
                      int32_t* template_id_out, int32_t* n_templates, int64_t* n_features)
{
    if (!c || !n_templates || !n_features) return fail(SBM_ERR_INVALID, "null argument");
    *n_templates = c->n_templates;
    *n_features = c->n_features;
    const int L = c->L;
    if (levels_out)
        for (size_t r = 0; r < (size_t)c->n_templates * L; ++r) {
            const DevTL& d = c->h_tls[r];
            sbm_template_level v{};
            v.width = d.width;
            v.height = d.height;
            v.pyramid_level = (int32_t)(r % (size_t)L);
            v.n_features = d.nf;
            v.feature_offset = d.feat_off;
            levels_out[r] = v;
        }
    for (int t = 0; t < c->n_templates; ++t) {
        if (class_idx_out) class_idx_out[t] = c->h_class[(size_t)t];
        if (template_id_out) template_id_out[t] = c->h_tid[(size_t)t];
    }
    if (!feats_out || c->n_features == 0) return 0;
    if (feat_cap < c->n_features) return fail(SBM_ERR_CAPACITY, "feats_out holds %lld records, the set has %lld", (long long)feat_cap, (long long)c->n_features);
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint32_t> xy((size_t)c->n_features);
    std::vector<uint8_t> label((size_t)c->n_features);
    HIP_TRY(hipMemcpy(xy.data(), c->d_fxy.p, xy.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(label.data(), c->d_flabel.p, label.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < xy.size(); ++i) feats_out[i] = sbm_feature{(int32_t)(xy[i] & 0xffffu), (int32_t)(xy[i] >> 16), (int32_t)label[i]};
    return 0;
}

int sbm_get_template_table(sbm_ctx* c, int32_t which, void* out, int64_t cap_bytes, int64_t* bytes)
{
    if (!c || !bytes) return fail(SBM_ERR_INVALID, "null argument");
    const int64_t n = install_table_bytes(which, c->n_templates, c->L, c->n_features);
    if (n < 0) return fail(SBM_ERR_INVALID, "no template table %d", which);
    *bytes = n;
    if (!out) return 0;
    if (cap_bytes < n) return fail(SBM_ERR_CAPACITY, "table %d has %lld bytes, the buffer %lld", which, (long long)n, (long long)cap_bytes);
    const DevBuf* const tables[INSTALL_TABLES] = {&c->d_tls, &c->d_fxy, &c->d_flabel, &c->d_flevel, &c->d_fxy_s, &c->d_flabel_s, &c->d_fcls, &c->d_fext,
                                                  &c->d_class, &c->d_tid};
    if (n == 0) return 0;
    if (!tables[which]->p || tables[which]->cap < (size_t)n) return fail(SBM_ERR_STATE, "template table %d is not allocated", which);
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, tables[which]->p, (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

} // extern "C"
