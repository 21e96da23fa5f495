// sbm_capi_train.inc — part of libsbm_hip.so's host side (included by sbm_capi.hip, one translation unit): batched
// template training, Detector::addTemplate (line2Dup.cpp:1299-1353) for a batch of images of one geometry with no host
// round trip (sbm_train_batch_device) and its host-array sibling (sbm_train_batch).
// ---------------------------------------------------------------------------

namespace {

size_t train_align(size_t v) { return (v + 255) / 256 * 256; }

// The gradient stage per image and level with the launch helpers as they are (the float outputs of k_quantize are not
// offset by the frame, so one launch per image), then the five training kernels, each once for the batch.
int train_enqueue(sbm_ctx* c, hipStream_t s, const uint8_t* d_imgs, int64_t img_stride, int n, int rows, int cols, int stride, int ch,
                  const uint8_t* d_masks, int64_t mask_stride, float strong, int num_features, sbm_template_level* d_levels,
                  sbm_train_feature* d_feats, int64_t feat_cap, int32_t* d_status)
{
    const int L = c->L;
    TrainPlan p;
    memset(&p, 0, sizeof p);
    p.L = L;
    p.n_images = n;
    p.thr_sq = strong * strong;
    int lr[SBM_MAX_LEVELS], lc[SBM_MAX_LEVELS];
    size_t img_fs[SBM_MAX_LEVELS] = {}, img_off[SBM_MAX_LEVELS] = {}, mask_off[SBM_MAX_LEVELS] = {};
    const int mask_frames = d_masks ? (mask_stride ? n : 1) : 0;
    size_t bytes = 0;
    for (int l = 0; l < L; ++l) {
        lr[l] = l ? lr[l - 1] / 2 : rows;
        lc[l] = l ? lc[l - 1] / 2 : cols;
        TrainLevel& v = p.lv[l];
        v.rows = lr[l];
        v.cols = lc[l];
        v.cand_cap = (int32_t)train_cand_bound(lr[l], lc[l]);
        v.nf = (uint32_t)train_level_features((size_t)num_features, l);
        v.pix_off = p.pix_stride;
        v.cand_off = p.cand_stride;
        v.sort_off = p.sort_stride;
        int64_t pow2 = 1;
        while (pow2 < v.cand_cap) pow2 <<= 1;
        p.pix_stride += (int64_t)train_align((size_t)lr[l] * lc[l]);
        p.cand_stride += (int64_t)train_align((size_t)v.cand_cap);
        p.sort_stride += (int64_t)train_align((size_t)pow2);
        if (l > 0) { // the level's images (k_pyrdown) and masks (k_resize_mask)
            img_fs[l] = train_align((size_t)lr[l] * lc[l] * ch + 64);
            img_off[l] = bytes;
            bytes += img_fs[l] * n;
            mask_off[l] = bytes;
            bytes += train_align((size_t)lr[l] * lc[l]) * mask_frames;
        }
    }
    const size_t N = (size_t)n;
    const size_t o_mag = bytes, o_ori = o_mag + train_align(N * p.pix_stride * 4), o_quant = o_ori + train_align(N * p.pix_stride * 4),
                 o_flags = o_quant + train_align(N * p.pix_stride), o_cand = o_flags + train_align(N * p.pix_stride),
                 o_keys = o_cand + train_align(N * p.cand_stride * sizeof(TrainCand)), o_sel = o_keys + train_align(N * p.sort_stride * 8),
                 o_kept = o_sel + train_align(N * p.cand_stride * 4), o_counts = o_kept + train_align(N * p.cand_stride * 4),
                 total = o_counts + train_align(N * L * 2 * 4);
    if (total > c->d_train.cap) {
        HIP_TRY(hipDeviceSynchronize()); // calls in flight may use the old scratch
        if (int e = c->d_train.ensure(total)) return e;
    }
    uint8_t* base = c->d_train.as<uint8_t>();
    p.mag = (const float*)(base + o_mag);
    p.ori = (const float*)(base + o_ori);
    p.quant = base + o_quant;
    p.flags = base + o_flags;
    p.cand = (TrainCand*)(base + o_cand);
    p.keys = (uint64_t*)(base + o_keys);
    p.sel = (int32_t*)(base + o_sel);
    p.kept_xy = (uint32_t*)(base + o_kept);
    p.counts = (int32_t*)(base + o_counts);

    for (int l = 0; l < L; ++l) {
        TrainLevel& v = p.lv[l];
        const size_t npx = (size_t)lr[l] * lc[l];
        if (l == 0) {
            v.mask = d_masks;
            v.mask_fs = d_masks ? mask_stride : 0;
        } else {
            const int gx = (int)std::min<size_t>((npx + 255) / 256, 4096);
            for (int i = 0; i < n; ++i) {
                const uint8_t* src = l == 1 ? d_imgs + (int64_t)i * img_stride : base + img_off[l - 1] + img_fs[l - 1] * i;
                SBM_LAUNCH(c, "k_pyrdown", k_pyrdown, dim3(gx), dim3(256), 0, s, src, lr[l - 1], lc[l - 1], ch, l == 1 ? stride : lc[l - 1] * ch,
                           base + img_off[l] + img_fs[l] * i);
            }
            if (d_masks) { // level l's masks from level l-1's, nearest neighbour, image by image (:439)
                const TrainLevel& u = p.lv[l - 1];
                v.mask = base + mask_off[l];
                v.mask_fs = mask_stride ? (int64_t)train_align(npx) : 0;
                SBM_LAUNCH(c, "k_resize_mask", k_resize_mask, dim3(gx, mask_frames), dim3(256), 0, s, u.mask, lr[l - 1], lc[l - 1], (uint8_t*)v.mask, lr[l],
                           lc[l], u.mask_fs, v.mask_fs);
            }
            HIP_TRY(hipGetLastError());
        }
        for (int i = 0; i < n; ++i) {
            const uint8_t* img = l == 0 ? d_imgs + (int64_t)i * img_stride : base + img_off[l] + img_fs[l] * i;
            const size_t px = (size_t)i * p.pix_stride + v.pix_off;
            // the training side quantises without the mask (ColorGradientPyramid::update); the mask enters with the erosion
            QuantizeLaunch q;
            q.src = l == 0 ? strided_frames(img, stride, ch, 1, 0) : packed_frames(img, lr[l], lc[l], ch, 1);
            q.rows = lr[l], q.cols = lc[l];
            q.weak = c->cfg.weak_threshold;
            q.out = (uint8_t*)p.quant + px;
            q.mag = (float*)p.mag + px;
            q.ori = (float*)p.ori + px;
            if (int e = launch_quantize(c, s, q)) return e;
        }
    }
    const int gx0 = (int)std::min<size_t>(((size_t)rows * cols + 255) / 256, 4096);
    SBM_LAUNCH(c, "k_train_maxima", k_train_maxima, dim3(gx0, L, n), dim3(256), 0, s, p);
    SBM_LAUNCH(c, "k_train_resolve", k_train_resolve, dim3(L, n), dim3(64), 0, s, p);
    SBM_LAUNCH(c, "k_train_sort", k_train_sort, dim3(L, n), dim3(256), 0, s, p);
    SBM_LAUNCH(c, "k_train_select", k_train_select, dim3(L, n), dim3(64), 0, s, p);
    SBM_LAUNCH(c, "k_train_crop", k_train_crop, dim3(n), dim3(256), 0, s, p, d_levels, d_feats, feat_cap, d_status);
    HIP_TRY(hipGetLastError());
    return 0;
}

int train_check_args(const sbm_ctx* c, int n, int rows, int cols, int stride, int ch, bool masks, int64_t mask_stride, int num_features, int64_t feat_cap)
{
    if (n < 1 || n > 65535) return fail(SBM_ERR_INVALID, "batch of %d images out of range", n);
    if (ch != 1 && ch != 3) return fail(SBM_ERR_INVALID, "channels must be 1 or 3, got %d", ch);
    if (rows < 1 || cols < 1 || rows > 32767 || cols > 32767) return fail(SBM_ERR_INVALID, "image of %d x %d out of range (positions are 15-bit)", rows, cols);
    if ((rows >> (c->L - 1)) < 3 || (cols >> (c->L - 1)) < 3) return fail(SBM_ERR_INVALID, "image of %d x %d too small for %d pyramid levels", rows, cols, c->L);
    if (stride < cols * ch) return fail(SBM_ERR_INVALID, "stride too small");
    if (masks && (mask_stride < 0 || (mask_stride > 0 && mask_stride < (int64_t)rows * cols)))
        return fail(SBM_ERR_INVALID, "mask stride %lld below rows * cols", (long long)mask_stride);
    if (num_features < 1 || train_level_features((size_t)num_features, c->L - 1) < 1)
        return fail(SBM_ERR_INVALID, "num_features %d leaves no feature for the last of %d levels", num_features, c->L);
    if (feat_cap < 0) return fail(SBM_ERR_INVALID, "negative feature capacity");
    return 0;
}

} // namespace

extern "C" {

int sbm_train_batch_device(sbm_ctx* c, const void* d_imgs, int64_t img_stride, int32_t n_images, int32_t rows, int32_t cols, int32_t stride,
                           int32_t channels, const void* d_masks, int64_t mask_stride, float strong_threshold, int32_t num_features,
                           void* d_levels, void* d_feats, int64_t feat_cap, void* d_status, void* stream)
{
    if (!c || !d_imgs || !d_levels || !d_status || (!d_feats && feat_cap > 0)) return fail(SBM_ERR_INVALID, "null argument");
    if (int e = train_check_args(c, n_images, rows, cols, stride, channels, d_masks != nullptr, mask_stride, num_features, feat_cap)) return e;
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    hipStream_t s = launch_stream(c, stream);
    if (c->profiling && !c->profiling_keep) c->clear_timings();
    return train_enqueue(c, s, (const uint8_t*)d_imgs, img_stride, n_images, rows, cols, stride, channels, (const uint8_t*)d_masks, mask_stride,
                         strong_threshold, num_features, (sbm_template_level*)d_levels, (sbm_train_feature*)d_feats, feat_cap, (int32_t*)d_status);
}

int sbm_train_batch(sbm_ctx* c, const uint8_t* const* imgs, int32_t n_images, int32_t rows, int32_t cols, int32_t stride, int32_t channels,
                    const uint8_t* const* masks, float strong_threshold, int32_t num_features, sbm_template_level* levels,
                    sbm_train_feature* feats, int64_t feat_cap, int32_t* status)
{
    if (!c || !imgs || !levels || !status || (!feats && feat_cap > 0)) return fail(SBM_ERR_INVALID, "null argument");
    if (int e = train_check_args(c, n_images, rows, cols, stride, channels, false, 0, num_features, feat_cap)) return e;
    bool any_mask = false;
    for (int i = 0; i < n_images; ++i) {
        if (!imgs[i]) return fail(SBM_ERR_INVALID, "image %d is null", i);
        any_mask = any_mask || (masks && masks[i]);
    }
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    if (int e = order_after_caller_work(c)) return e;
    const size_t n = (size_t)n_images, row_bytes = (size_t)cols * channels, img_bytes = train_align(row_bytes * rows + 64),
                 npx = (size_t)rows * cols, lv_bytes = n * c->L * sizeof(sbm_template_level), ft_bytes = n * (size_t)feat_cap * sizeof(sbm_train_feature);
    const size_t o_feats = train_align(lv_bytes), o_status = o_feats + train_align(ft_bytes);
    if (img_bytes * n > c->d_train_in.cap || (any_mask && npx * n > c->d_train_mask.cap) || o_status + n * 8 > c->d_train_out.cap)
        HIP_TRY(hipStreamSynchronize(c->stream));
    int rc = 0;
    if ((rc = c->d_train_in.ensure(img_bytes * n)) || (any_mask && (rc = c->d_train_mask.ensure(npx * n))) || (rc = c->d_train_out.ensure(o_status + n * 8)))
        return rc;
    hipStream_t s = c->stream;
    uint8_t* d_in = c->d_train_in.as<uint8_t>();
    uint8_t* d_mask = any_mask ? c->d_train_mask.as<uint8_t>() : nullptr;
    uint8_t* d_out = c->d_train_out.as<uint8_t>();
    for (size_t i = 0; i < n; ++i) {
        HIP_TRY(hipMemcpy2DAsync(d_in + i * img_bytes, row_bytes, imgs[i], (size_t)stride, row_bytes, (size_t)rows, hipMemcpyHostToDevice, s));
        if (!any_mask) continue;
        // an image without a mask among masked ones: all set, which the erosion leaves all set
        if (masks[i]) HIP_TRY(hipMemcpyAsync(d_mask + i * npx, masks[i], npx, hipMemcpyHostToDevice, s));
        else HIP_TRY(hipMemsetAsync(d_mask + i * npx, 255, npx, s));
    }
    HIP_TRY(hipMemsetAsync(d_out, 0, o_status + n * 8, s));
    if (c->profiling && !c->profiling_keep) c->clear_timings();
    if ((rc = train_enqueue(c, s, d_in, (int64_t)img_bytes, n_images, rows, cols, (int)row_bytes, channels, d_mask, (int64_t)npx, strong_threshold,
                            num_features, (sbm_template_level*)d_out, (sbm_train_feature*)(d_out + o_feats), feat_cap, (int32_t*)(d_out + o_status))))
        return rc;
    HIP_TRY(hipMemcpyAsync(levels, d_out, lv_bytes, hipMemcpyDeviceToHost, s));
    if (ft_bytes) HIP_TRY(hipMemcpyAsync(feats, d_out + o_feats, ft_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(status, d_out + o_status, n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

} // extern "C"
