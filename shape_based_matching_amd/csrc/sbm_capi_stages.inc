// sbm_capi_stages.inc — part of libsbm_hip.so's host side (included by sbm_capi.hip, one translation unit): the single-function stage entry points (one HIP kernel each, host arrays in and out), profiling and statistics.
// ---- stage entry points -----------------------------------------------------
int sbm_quantized_orientations(sbm_ctx* c, const uint8_t* img, int32_t rows, int32_t cols, int32_t stride, int32_t ch,
                               float weak, float* magnitude, uint8_t* angle, float* angle_ori)
{
    if (!c || !img || !angle || rows < 3 || cols < 3) return fail(SBM_ERR_INVALID, "bad argument");
    if (ch != 1 && ch != 3) return fail(SBM_ERR_INVALID, "channels must be 1 or 3");
    if (stride < cols * ch) return fail(SBM_ERR_INVALID, "stride too small");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    const size_t npx = (size_t)rows * cols;
    DevBuf d_in, d_q, d_mag, d_ori;
    int rc = 0;
    if ((rc = d_in.ensure(npx * ch)) || (rc = d_q.ensure(npx)) || (magnitude && (rc = d_mag.ensure(npx * 4))) ||
        (angle_ori && (rc = d_ori.ensure(npx * 4))))
        return rc;
    if (hipMemcpy2D(d_in.p, (size_t)cols * ch, img, stride, (size_t)cols * ch, rows, hipMemcpyHostToDevice) != hipSuccess)
        return fail(SBM_ERR_HIP, "image upload failed");
    QuantizeLaunch q;
    q.src = packed_frames(d_in.p, rows, cols, ch, 1);
    q.rows = rows, q.cols = cols;
    q.weak = weak;
    q.out = d_q.as<uint8_t>();
    q.mag = magnitude ? d_mag.as<float>() : nullptr;
    q.ori = angle_ori ? d_ori.as<float>() : nullptr;
    if ((rc = launch_quantize(c, c->stream, q))) return rc;
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(angle, d_q.p, npx, hipMemcpyDeviceToHost) != hipSuccess ||
        (magnitude && hipMemcpy(magnitude, d_mag.p, npx * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
        (angle_ori && hipMemcpy(angle_ori, d_ori.p, npx * 4, hipMemcpyDeviceToHost) != hipSuccess))
        return fail(SBM_ERR_HIP, "quantize kernel or download failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

int sbm_extract_local_maxima(sbm_ctx* c, const float* magnitude, const uint8_t* mask, int32_t rows, int32_t cols, float strong_threshold,
                             int32_t* xy, int64_t cap, int64_t* n_out)
{
    if (!c || !magnitude || !n_out || (!xy && cap > 0) || rows < 1 || cols < 1 || rows > 32767 || cols > 32767) return fail(SBM_ERR_INVALID, "bad argument");
    *n_out = 0;
    if (rows < 5 || cols < 5) return 0; // the scanned region [2, rows-2) x [2, cols-2) is empty
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    const size_t npx = (size_t)rows * cols;
    DevBuf d_mag, d_mask, d_xy, d_cnt;
    std::vector<int32_t> pts;
    int rc = 0;
    int64_t dev_cap = std::max<int64_t>(4096, std::min<int64_t>((int64_t)npx / 8, 1 << 22));
    if ((rc = d_mag.ensure(npx * 4)) || (mask && (rc = d_mask.ensure(npx))) || (rc = d_cnt.ensure(16))) return rc;
    if (hipMemcpy(d_mag.p, magnitude, npx * 4, hipMemcpyHostToDevice) != hipSuccess ||
        (mask && hipMemcpy(d_mask.p, mask, npx, hipMemcpyHostToDevice) != hipSuccess))
        return fail(SBM_ERR_HIP, "upload failed");
    for (;;) {
        int32_t n = 0;
        if ((rc = d_xy.ensure((size_t)dev_cap * 4))) return rc;
        if (hipMemsetAsync(d_cnt.p, 0, 16, c->stream) != hipSuccess) return fail(SBM_ERR_HIP, "memset failed");
        hipLaunchKernelGGL(k_local_maxima5, dim3((unsigned)std::min<size_t>((npx + 255) / 256, 8192)), dim3(256), 0, c->stream, d_mag.as<float>(),
                           mask ? d_mask.as<uint8_t>() : nullptr, rows, cols, strong_threshold * strong_threshold, d_xy.as<int32_t>(),
                           d_cnt.as<int32_t>(), (int)dev_cap);
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(&n, d_cnt.p, 4, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(SBM_ERR_HIP, "k_local_maxima5 failed: %s", hipGetErrorString(hipGetLastError()));
        if (n > dev_cap) { // more maxima than the buffer holds: once more with room for all of them
            dev_cap = n;
            continue;
        }
        pts.resize((size_t)n);
        if (n && hipMemcpy(pts.data(), d_xy.p, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(SBM_ERR_HIP, "download failed");
        break;
    }
    // row-major order, then the reference's invalidation among equal-score neighbours: a maximum is dropped when an
    // earlier kept one lies within its 5x5 window (sbm_train_kernels.h).  y << 16 | x sorts row-major as an integer.
    std::sort(pts.begin(), pts.end());
    std::vector<int32_t> kept;
    size_t lo = 0; // first kept point that can still be within two rows of the current one
    for (int32_t p : pts) {
        const int y = p >> 16, x = p & 0xffff;
        while (lo < kept.size() && (kept[lo] >> 16) < y - 2) ++lo;
        bool ok = true;
        for (size_t i = lo; i < kept.size() && ok; ++i) ok = std::abs((kept[i] & 0xffff) - x) > 2;
        if (ok) kept.push_back(p);
    }
    *n_out = (int64_t)kept.size();
    if ((int64_t)kept.size() > cap) return fail(SBM_ERR_CAPACITY, "%zu local maxima exceed the capacity %lld", kept.size(), (long long)cap);
    for (size_t i = 0; i < kept.size(); ++i) xy[i] = kept[i];
    return 0;
}

int sbm_orientation_bins(sbm_ctx* c, const int16_t* gx, const int16_t* gy, int64_t n, uint8_t* q16)
{
    if (!c || !gx || !gy || !q16 || n < 0) return fail(SBM_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    DevBuf a, b, o;
    int rc = 0;
    if ((rc = a.ensure((size_t)n * 2)) || (rc = b.ensure((size_t)n * 2)) || (rc = o.ensure((size_t)n))) return rc;
    if (hipMemcpy(a.p, gx, (size_t)n * 2, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(b.p, gy, (size_t)n * 2, hipMemcpyHostToDevice) != hipSuccess)
        return fail(SBM_ERR_HIP, "upload failed");
    hipLaunchKernelGGL(k_orientation_bins, dim3((unsigned)std::min<int64_t>((n + 255) / 256 + 1, 8192)), dim3(256), 0, c->stream,
                       a.as<int16_t>(), b.as<int16_t>(), n, o.as<uint8_t>());
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(q16, o.p, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(SBM_ERR_HIP, "orientation_bins failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

int sbm_pyrdown(sbm_ctx* c, const uint8_t* img, int32_t rows, int32_t cols, int32_t stride, int32_t ch, uint8_t* out)
{
    if (!c || !img || !out || rows < 2 || cols < 2 || ch < 1 || ch > 4) return fail(SBM_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    DevBuf d_in, d_out;
    int rc = 0;
    const size_t nout = (size_t)(rows / 2) * (cols / 2) * ch;
    if ((rc = d_in.ensure((size_t)rows * cols * ch)) || (rc = d_out.ensure(nout))) return rc;
    if (hipMemcpy2D(d_in.p, (size_t)cols * ch, img, stride, (size_t)cols * ch, rows, hipMemcpyHostToDevice) != hipSuccess)
        return fail(SBM_ERR_HIP, "upload failed");
    hipLaunchKernelGGL(k_pyrdown, dim3((unsigned)std::min<size_t>((nout / ch + 255) / 256, 4096)), dim3(256), 0, c->stream,
                       d_in.as<uint8_t>(), rows, cols, ch, cols * ch, d_out.as<uint8_t>());
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(out, d_out.p, nout, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(SBM_ERR_HIP, "pyrdown failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

int sbm_resize_linear(sbm_ctx* c, const uint8_t* img, int32_t rows, int32_t cols, int32_t stride, int32_t ch, double fx, double fy,
                      uint8_t* out, int64_t cap_bytes, int32_t* out_rows, int32_t* out_cols)
{
    if (!c || !img || rows < 1 || cols < 1 || ch < 1 || ch > 4 || !(fx > 0) || !(fy > 0)) return fail(SBM_ERR_INVALID, "bad argument");
    if (stride < cols * ch) return fail(SBM_ERR_INVALID, "stride too small");
    int dr, dc;
    resize_linear_dims(rows, cols, fx, fy, &dr, &dc);
    if (out_rows) *out_rows = dr;
    if (out_cols) *out_cols = dc;
    if (!out) return 0; // size query
    if (dr < 1 || dc < 1) return fail(SBM_ERR_INVALID, "resize to an empty image");
    const size_t nout = (size_t)dr * dc * ch;
    if ((int64_t)nout > cap_bytes) return fail(SBM_ERR_CAPACITY, "need %zu bytes", nout);
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    std::vector<int32_t> xi, yi;
    std::vector<int16_t> xa, ya;
    resize_linear_table(dc, cols, 1.0 / fx, xi, xa);
    resize_linear_table(dr, rows, 1.0 / fy, yi, ya);
    DevBuf d_in, d_out, d_xi, d_xa, d_yi, d_ya;
    int rc = 0;
    if ((rc = d_in.ensure((size_t)rows * cols * ch)) || (rc = d_out.ensure(nout)) || (rc = d_xi.ensure(xi.size() * 4)) ||
        (rc = d_xa.ensure(xa.size() * 2)) || (rc = d_yi.ensure(yi.size() * 4)) || (rc = d_ya.ensure(ya.size() * 2)))
        return rc;
    if (hipMemcpy2D(d_in.p, (size_t)cols * ch, img, stride, (size_t)cols * ch, rows, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_xi.p, xi.data(), xi.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_xa.p, xa.data(), xa.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_yi.p, yi.data(), yi.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_ya.p, ya.data(), ya.size() * 2, hipMemcpyHostToDevice) != hipSuccess)
        return fail(SBM_ERR_HIP, "upload failed");
    hipLaunchKernelGGL(k_resize_linear_u8, dim3((unsigned)std::min<size_t>((nout + 255) / 256, 4096)), dim3(256), 0, c->stream,
                       d_in.as<uint8_t>(), rows, cols, ch, cols * ch, d_xi.as<int32_t>(), d_xa.as<int16_t>(), d_yi.as<int32_t>(),
                       d_ya.as<int16_t>(), d_out.as<uint8_t>(), dr, dc);
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(out, d_out.p, nout, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(SBM_ERR_HIP, "resize failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

int sbm_spread(sbm_ctx* c, const uint8_t* src, int32_t rows, int32_t cols, int32_t T, uint8_t* dst)
{
    if (!c || !src || !dst || rows < 1 || cols < 1 || T < 1) return fail(SBM_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    const size_t n = (size_t)rows * cols;
    DevBuf a, b;
    int rc = 0;
    if ((rc = a.ensure(n)) || (rc = b.ensure(n))) return rc;
    if (hipMemcpy(a.p, src, n, hipMemcpyHostToDevice) != hipSuccess)
        return fail(SBM_ERR_HIP, "upload failed");
    hipLaunchKernelGGL(k_spread, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, c->stream,
                       a.as<uint8_t>(), rows, cols, T, b.as<uint8_t>());
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(dst, b.p, n, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(SBM_ERR_HIP, "spread failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

int sbm_compute_response_maps(sbm_ctx* c, const uint8_t* spread, int32_t rows, int32_t cols, uint8_t* maps)
{
    if (!c || !spread || !maps || rows < 1 || cols < 1) return fail(SBM_ERR_INVALID, "bad argument");
    if (((int64_t)rows * cols) % 16) return fail(SBM_ERR_INVALID, "rows*cols %% 16 != 0 (line2Dup.cpp:639)");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    const size_t n = (size_t)rows * cols;
    DevBuf a, b;
    int rc = 0;
    if ((rc = a.ensure(n)) || (rc = b.ensure(8 * n))) return rc;
    if (hipMemcpy(a.p, spread, n, hipMemcpyHostToDevice) != hipSuccess)
        return fail(SBM_ERR_HIP, "upload failed");
    hipLaunchKernelGGL(k_response, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, c->stream,
                       a.as<uint8_t>(), (int64_t)n, b.as<uint8_t>());
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(maps, b.p, 8 * n, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(SBM_ERR_HIP, "response failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

int sbm_linearize(sbm_ctx* c, const uint8_t* map, int32_t rows, int32_t cols, int32_t T, uint8_t* lm)
{
    if (!c || !map || !lm || rows < 1 || cols < 1 || T < 1) return fail(SBM_ERR_INVALID, "bad argument");
    if (rows % T || cols % T) return fail(SBM_ERR_INVALID, "rows/cols not a multiple of T (line2Dup.cpp:751-752)");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    const size_t n = (size_t)rows * cols;
    DevBuf a, b;
    int rc = 0;
    if ((rc = a.ensure(n)) || (rc = b.ensure(n))) return rc;
    if (hipMemcpy(a.p, map, n, hipMemcpyHostToDevice) != hipSuccess)
        return fail(SBM_ERR_HIP, "upload failed");
    hipLaunchKernelGGL(k_linearize, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, c->stream,
                       a.as<uint8_t>(), rows, cols, T, b.as<uint8_t>());
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(lm, b.p, n, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(SBM_ERR_HIP, "linearize failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

int sbm_similarity(sbm_ctx* c, int32_t t, uint16_t* dst)
{
    if (!c || !dst || t < 0 || t >= c->n_templates) return fail(SBM_ERR_INVALID, "bad template index");
    if (c->rec.levels_valid < c->L) return fail(SBM_ERR_STATE, "pyramid not built");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    if (int e = ensure_foff(c, c->stream)) return e;
    const int lc = c->L - 1, T = c->cfg.T[lc], W = c->cols[lc] / T, H = c->rows[lc] / T;
    HIP_TRY(hipDeviceSynchronize());
    if (int e = ensure_full_lm(c, lc, c->stream)) return e;
    DevBuf d;
    if (int e = d.ensure((size_t)W * H * 2)) return e;
    hipLaunchKernelGGL(k_similarity_map, dim3((W * H + SIM_POS_PER_BLOCK - 1) / SIM_POS_PER_BLOCK), dim3(256), 0, c->stream,
                       c->d_lm[lc].as<uint8_t>(), c->lm_stride[lc], c->rows[lc], c->cols[lc], T, W, H, c->h_tls[(size_t)t * c->L + lc],
                       c->d_fxy.as<uint32_t>(), c->d_foff.as<int32_t>(), d.as<uint16_t>());
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(dst, d.p, (size_t)W * H * 2, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(SBM_ERR_HIP, "similarity failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

int sbm_similarity_local(sbm_ctx* c, int32_t level, int32_t t, int32_t cx, int32_t cy, uint16_t* dst)
{
    if (!c || !dst || t < 0 || t >= c->n_templates || level < 0 || level >= c->L) return fail(SBM_ERR_INVALID, "bad argument");
    if (c->rec.levels_valid <= level) return fail(SBM_ERR_STATE, "level not resident");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    if (int e = ensure_foff(c, c->stream)) return e;
    HIP_TRY(hipDeviceSynchronize());
    if (int e = ensure_full_lm(c, level, c->stream)) return e;
    const int T = c->cfg.T[level], W = c->cols[level] / T, H = c->rows[level] / T;
    DevBuf d;
    if (int e = d.ensure(512)) return e;
    hipLaunchKernelGGL(k_similarity_local_patch, dim3(1), dim3(64 * LOCAL_WAVES), 0, c->stream, c->d_lm[level].as<uint8_t>(),
                       c->lm_stride[level], c->rows[level], c->cols[level], T, W, H, c->h_tls[(size_t)t * c->L + level], c->d_fxy.as<uint32_t>(),
                       c->d_foff.as<int32_t>(), cx, cy, d.as<uint16_t>());
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(dst, d.p, 512, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(SBM_ERR_HIP, "similarity_local failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

int sbm_set_profiling(sbm_ctx* c, int32_t enabled)
{
    if (!c) return fail(SBM_ERR_INVALID, "null context");
    c->profiling = enabled != 0;
    c->profiling_keep = enabled == 2;
    c->clear_timings();
    return 0;
}

int sbm_get_timings(sbm_ctx* c, const char** names, float* ms, int32_t cap, int32_t* n)
{
    if (!c || !n) return fail(SBM_ERR_INVALID, "null argument");
    if (c->timing_ms.size() != c->timings.size()) collect_timings(c);
    *n = (int32_t)c->timings.size();
    for (int i = 0; i < *n && i < cap; ++i) {
        if (names) names[i] = c->timings[i].name;
        if (ms) ms[i] = c->timing_ms[i];
    }
    if (c->profiling_keep && cap >= *n && *n > 0) c->clear_timings(); // read out: start the next accumulation
    return 0;
}

int sbm_get_stats(sbm_ctx* c, int64_t* n_candidates, int64_t* refine_bytes)
{
    if (!c) return fail(SBM_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    HIP_TRY(hipDeviceSynchronize());
    int32_t h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpy(h, c->d_counters.p, sizeof h, hipMemcpyDeviceToHost));
    if (n_candidates) *n_candidates = h[0];
    if (refine_bytes) {
        uint64_t b;
        memcpy(&b, &h[2], sizeof b);
        *refine_bytes = (int64_t)b;
    }
    return 0;
}

int sbm_set_result_mirror(sbm_ctx* c, void* mirror_out, void* mirror_count)
{
    if (!c || ((mirror_out == nullptr) != (mirror_count == nullptr))) return fail(SBM_ERR_INVALID, "both mirror pointers or neither");
    c->mirror_out = (sbm_match_rec*)mirror_out;
    c->mirror_count = (int32_t*)mirror_count;
    return 0;
}

} // extern "C" (reopened below)
