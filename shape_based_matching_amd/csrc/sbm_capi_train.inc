// sbm_capi_train.inc — part of libsbm_hip.so's host side (included by sbm_capi.hip, one translation unit): batched
// template training, Detector::addTemplate (line2Dup.cpp:1299-1353) for a batch of images of one geometry with no host
// round trip (sbm_train_batch_device) and its host-array sibling (sbm_train_batch); the ragged form for images of
// different sizes and feature counts (sbm_train_ragged_device, sbm_train_ragged), whose host rules are
// sbm_train_plan.h's, and the scale sweep of one source on top of it (sbm_train_sweep_device, sbm_train_sweep); at the
// end, Detector::addTemplate_rotate (line2Dup.cpp:1395-1451) for every (base, angle) pair of a call
// (sbm_train_rotate_device, sbm_train_rotate), whose scalar rule is sbm_rotate_math.h's.
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
    SBM_LAUNCH(c, "k_train_maxima", k_train_maxima<false>, dim3(gx0, L, n), dim3(256), 0, s, p);
    SBM_LAUNCH(c, "k_train_resolve", k_train_resolve<false>, dim3(L, n), dim3(64), 0, s, p);
    SBM_LAUNCH(c, "k_train_sort", k_train_sort<false>, dim3(L, n), dim3(256), 0, s, p);
    SBM_LAUNCH(c, "k_train_select", k_train_select<false>, dim3(L, n), dim3(64), 0, s, p);
    SBM_LAUNCH(c, "k_train_crop", k_train_crop<false>, dim3(n), dim3(256), 0, s, p, d_levels, d_feats, feat_cap, d_status);
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

// ---- the ragged form ---------------------------------------------------------------------------------------------------

// The resize launch a sweep puts in front of its ragged call: the source, and the scale, index and coefficient tables as
// one block of host bytes that travels in the same pinned slot as the records.
struct TrainSweepJob {
    const uint8_t* d_img;
    const uint8_t* d_mask;
    int rows, cols, stride;
    int grid_x; // from the largest scaled image
    std::vector<uint8_t> blob; // [TrainSweepScale n][int32 idx][int16 coef], 256-aligned parts
    size_t o_idx, o_coef;
    uint8_t* d_blob;
};

// The pinned slot, `bytes` large and free to be written: the previous call's copies out of it have left.
int train_table_slot(sbm_ctx* c, size_t bytes, uint8_t** slot)
{
    if (!c->ev_train_table) HIP_TRY(hipEventCreateWithFlags(&c->ev_train_table, hipEventDisableTiming));
    if (c->train_table_busy) {
        if (c->train_table_recorded) HIP_TRY(hipEventSynchronize(c->ev_train_table));
        else HIP_TRY(hipStreamSynchronize(c->train_table_stream)); // the last call failed between its copies and its event
        c->train_table_busy = false;
    }
    if (bytes > c->h_train_table_cap) {
        if (c->h_train_table) (void)hipHostFree(c->h_train_table);
        c->h_train_table = nullptr;
        c->h_train_table_cap = 0;
        HIP_TRY(hipHostMalloc(&c->h_train_table, bytes, hipHostMallocDefault));
        c->h_train_table_cap = bytes;
    }
    *slot = (uint8_t*)c->h_train_table;
    return 0;
}

// Everything of a ragged call behind its argument check: the scratch by the plan's running sums, the records (and a
// sweep's tables) through the pinned slot onto the stream, the sweep's resize, then per level the two level steps once
// for the batch and the gradient stage image by image (k_quantize's float outputs are not offset by the frame, and the
// kernel is the match path's: it stays as it is), then the five training kernels in their ragged form.
int train_ragged_enqueue(sbm_ctx* c, hipStream_t s, const sbm_train_image* images, TrainRaggedPlan& plan, float strong, sbm_template_level* d_levels,
                         sbm_train_feature* d_feats, int32_t* d_status, const TrainSweepJob* sweep)
{
    const int L = plan.L, n = plan.n, ch = plan.ch;
    if ((size_t)plan.total > c->d_train.cap) {
        HIP_TRY(hipDeviceSynchronize()); // calls in flight may use the old scratch
        if (int e = c->d_train.ensure((size_t)plan.total)) return e;
    }
    uint8_t* base = c->d_train.as<uint8_t>();
    train_ragged_bind(plan, images, base);
    const size_t table_bytes = plan.table.size() * sizeof(TrainRecord), blob_bytes = sweep ? train_align(sweep->blob.size()) : 0;
    uint8_t* slot = nullptr;
    if (int e = train_table_slot(c, blob_bytes + table_bytes, &slot)) return e;
    if (sweep) memcpy(slot, sweep->blob.data(), sweep->blob.size());
    memcpy(slot + blob_bytes, plan.table.data(), table_bytes);
    const TrainRecord* d_table = (const TrainRecord*)(base + plan.o_table);
    // busy from before the first copy: should a later step fail, the next call still waits for what was enqueued (an
    // event never recorded, or recorded earlier, is complete, and then the stream itself is waited for)
    c->train_table_busy = true;
    c->train_table_stream = s;
    c->train_table_recorded = false;
    if (sweep) HIP_TRY(hipMemcpyAsync(sweep->d_blob, slot, sweep->blob.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync((void*)d_table, slot + blob_bytes, table_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->ev_train_table, s));
    c->train_table_recorded = true;
    if (sweep) {
        SBM_LAUNCH(c, "k_resize_sweep_u8", k_resize_sweep_u8, dim3(sweep->grid_x, n), dim3(256), 0, s, sweep->d_img, sweep->rows, sweep->cols, ch, sweep->stride,
                   sweep->d_mask, (const TrainSweepScale*)sweep->d_blob, (const int32_t*)(sweep->d_blob + sweep->o_idx),
                   (const int16_t*)(sweep->d_blob + sweep->o_coef));
        HIP_TRY(hipGetLastError());
    }

    TrainPlan p;
    memset(&p, 0, sizeof p);
    p.L = L;
    p.n_images = n;
    p.thr_sq = strong * strong;
    p.mag = (const float*)(base + plan.o_mag);
    p.ori = (const float*)(base + plan.o_ori);
    p.quant = base + plan.o_quant;
    p.flags = base + plan.o_flags;
    p.cand = (TrainCand*)(base + plan.o_cand);
    p.keys = (uint64_t*)(base + plan.o_keys);
    p.sel = (int32_t*)(base + plan.o_sel);
    p.kept_xy = (uint32_t*)(base + plan.o_kept);
    p.counts = (int32_t*)(base + plan.o_counts);
    p.table = d_table;
    for (int l = 0; l < L; ++l) {
        if (l > 0 && plan.grid_level[l]) {
            SBM_LAUNCH(c, "k_train_pyrdown", k_train_pyrdown, dim3(plan.grid_level[l], n), dim3(256), 0, s, d_table, L, l, ch);
            if (plan.any_mask) SBM_LAUNCH(c, "k_train_resize_mask", k_train_resize_mask, dim3(plan.grid_level[l], n), dim3(256), 0, s, d_table, L, l);
            HIP_TRY(hipGetLastError());
        }
        for (int i = 0; i < n; ++i) {
            const TrainRecord& v = plan.table[(size_t)i * L + l];
            if (v.rows == 0) continue;
            // the training side quantises without the mask (ColorGradientPyramid::update); the mask enters with the erosion
            QuantizeLaunch q;
            q.src = l == 0 ? strided_frames(v.img, v.stride, ch, 1, 0) : packed_frames(v.img, v.rows, v.cols, ch, 1);
            q.rows = v.rows, q.cols = v.cols;
            q.weak = c->cfg.weak_threshold;
            q.out = (uint8_t*)p.quant + v.pix_off;
            q.mag = (float*)p.mag + v.pix_off;
            q.ori = (float*)p.ori + v.pix_off;
            if (int e = launch_quantize(c, s, q)) return e;
        }
    }
    SBM_LAUNCH(c, "k_train_maxima", k_train_maxima<true>, dim3(plan.grid_maxima, L, n), dim3(256), 0, s, p);
    SBM_LAUNCH(c, "k_train_resolve", k_train_resolve<true>, dim3(L, n), dim3(64), 0, s, p);
    SBM_LAUNCH(c, "k_train_sort", k_train_sort<true>, dim3(L, n), dim3(256), 0, s, p);
    SBM_LAUNCH(c, "k_train_select", k_train_select<true>, dim3(L, n), dim3(64), 0, s, p);
    SBM_LAUNCH(c, "k_train_crop", k_train_crop<true>, dim3(n), dim3(256), 0, s, p, d_levels, d_feats, (int64_t)0, d_status);
    HIP_TRY(hipGetLastError());
    return 0;
}

int train_ragged_verdict(const TrainRaggedPlan& plan)
{
    if (plan.error == TRP_OK) return 0;
    if (plan.error_image < 0) return fail(SBM_ERR_INVALID, "%s", train_ragged_error(plan.error));
    return fail(SBM_ERR_INVALID, "image %d: %s", plan.error_image, train_ragged_error(plan.error));
}

// the end of the feature array the blocks lie in, in records
int64_t train_feats_end(const sbm_train_image* images, int n)
{
    int64_t end = 0;
    for (int i = 0; i < n; ++i) end = std::max(end, images[i].feat_first + images[i].feat_cap);
    return end;
}

int train_sweep_source_check(int rows, int cols, int stride, int ch)
{
    if (ch != 1 && ch != 3) return fail(SBM_ERR_INVALID, "%s", train_ragged_error(TRP_CHANNELS));
    if (rows < 1 || cols < 1 || rows > 32767 || cols > 32767) return fail(SBM_ERR_INVALID, "source: %s", train_ragged_error(TRP_GEOMETRY));
    if (stride < cols * ch) return fail(SBM_ERR_INVALID, "source: %s", train_ragged_error(TRP_STRIDE));
    return 0;
}

// The images of a sweep: sizes by resize_linear_dims, the scaled images and masks behind each other in the context's
// sweep buffer, the tables of sbm_resize_table.h concatenated.  `imgs` come out as the ragged call's descriptors.
int train_sweep_prepare(sbm_ctx* c, const uint8_t* d_img, int rows, int cols, int stride, int ch, const uint8_t* d_mask, const sbm_train_scale* scales, int n,
                        std::vector<sbm_train_image>& imgs, TrainSweepJob& job)
{
    if (n < 1 || n > 65535 || !scales) return fail(SBM_ERR_INVALID, "%s", train_ragged_error(TRP_COUNT));
    if (int e = train_sweep_source_check(rows, cols, stride, ch)) return e;
    imgs.assign((size_t)n, sbm_train_image{});
    std::vector<TrainSweepScale> sc((size_t)n);
    std::vector<int32_t> idx, xi;
    std::vector<int16_t> coef, xa;
    std::vector<size_t> o_img((size_t)n), o_mask((size_t)n);
    size_t bytes = 0;
    int64_t max_samples = 1;
    for (int k = 0; k < n; ++k) {
        if (!(scales[k].fx > 0) || !(scales[k].fy > 0)) return fail(SBM_ERR_INVALID, "scale %d: factors must be positive", k);
        int dr, dc;
        resize_linear_dims(rows, cols, scales[k].fx, scales[k].fy, &dr, &dc);
        if (dr < 1 || dc < 1) return fail(SBM_ERR_INVALID, "scale %d resizes to an empty image", k);
        if (dr > 32767 || dc > 32767) return fail(SBM_ERR_INVALID, "scale %d: %s", k, train_ragged_error(TRP_GEOMETRY));
        sc[(size_t)k].rows = dr, sc[(size_t)k].cols = dc;
        for (int axis = 0; axis < 2; ++axis) { // x, then y
            resize_linear_table(axis ? dr : dc, axis ? rows : cols, 1.0 / (axis ? scales[k].fy : scales[k].fx), xi, xa);
            (axis ? sc[(size_t)k].y_off : sc[(size_t)k].x_off) = (int64_t)idx.size();
            idx.insert(idx.end(), xi.begin(), xi.end());
            coef.insert(coef.end(), xa.begin(), xa.end());
        }
        const size_t npx = (size_t)dr * dc;
        o_img[(size_t)k] = bytes;
        bytes += train_align(npx * ch + 64);
        o_mask[(size_t)k] = bytes;
        if (d_mask) bytes += train_align(npx);
        max_samples = std::max<int64_t>(max_samples, (int64_t)npx * (ch + (d_mask ? 1 : 0)));
        sbm_train_image& im = imgs[(size_t)k];
        im.rows = dr, im.cols = dc, im.stride = dc * ch;
        im.num_features = scales[k].num_features;
        im.feat_first = scales[k].feat_first, im.feat_cap = scales[k].feat_cap;
    }
    const size_t o_idx = train_align(sc.size() * sizeof(TrainSweepScale)), o_coef = o_idx + train_align(idx.size() * 4),
                 blob_bytes = o_coef + train_align(coef.size() * 2);
    if (bytes + blob_bytes > c->d_train_sweep.cap) {
        HIP_TRY(hipDeviceSynchronize()); // a call in flight may read the old buffer
        if (int e = c->d_train_sweep.ensure(bytes + blob_bytes)) return e;
    }
    uint8_t* d = c->d_train_sweep.as<uint8_t>();
    for (int k = 0; k < n; ++k) {
        sc[(size_t)k].img = d + o_img[(size_t)k];
        sc[(size_t)k].mask = d_mask ? d + o_mask[(size_t)k] : nullptr;
        imgs[(size_t)k].img = sc[(size_t)k].img;
        imgs[(size_t)k].mask = sc[(size_t)k].mask;
    }
    job.d_img = d_img, job.d_mask = d_mask;
    job.rows = rows, job.cols = cols, job.stride = stride;
    job.grid_x = (int)std::min<int64_t>((max_samples + 255) / 256, 4096);
    job.blob.assign(blob_bytes, 0);
    memcpy(job.blob.data(), sc.data(), sc.size() * sizeof(TrainSweepScale));
    memcpy(job.blob.data() + o_idx, idx.data(), idx.size() * 4);
    memcpy(job.blob.data() + o_coef, coef.data(), coef.size() * 2);
    job.o_idx = o_idx, job.o_coef = o_coef;
    job.d_blob = d + bytes;
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

int sbm_train_ragged_device(sbm_ctx* c, const sbm_train_image* images, int32_t n_images, int32_t channels, float strong_threshold, void* d_levels,
                            void* d_feats, void* d_status, void* stream)
{
    if (!c || !d_levels || !d_status) return fail(SBM_ERR_INVALID, "null argument");
    TrainRaggedPlan plan = train_ragged_plan(images, n_images, channels, c->L);
    if (int e = train_ragged_verdict(plan)) return e;
    if (!d_feats && train_feats_end(images, n_images) > 0) return fail(SBM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    hipStream_t s = launch_stream(c, stream);
    if (c->profiling && !c->profiling_keep) c->clear_timings();
    return train_ragged_enqueue(c, s, images, plan, strong_threshold, (sbm_template_level*)d_levels, (sbm_train_feature*)d_feats, (int32_t*)d_status, nullptr);
}

} // extern "C"

namespace {

// the results of a ragged call on the context's stream, from the context's output buffer into the caller's arrays
struct TrainOut {
    size_t lv_bytes, ft_bytes, o_feats, o_status, total;
};
int train_out_ensure(sbm_ctx* c, int n, int64_t feats_end, TrainOut& o)
{
    o.lv_bytes = (size_t)n * c->L * sizeof(sbm_template_level);
    o.ft_bytes = (size_t)feats_end * sizeof(sbm_train_feature);
    o.o_feats = train_align(o.lv_bytes);
    o.o_status = o.o_feats + train_align(o.ft_bytes);
    o.total = o.o_status + (size_t)n * 8;
    if (o.total > c->d_train_out.cap) HIP_TRY(hipStreamSynchronize(c->stream));
    return c->d_train_out.ensure(o.total);
}
// Of the feature array only the records the call made reach the caller's: an image that is ok gets its features, and
// what lies between the blocks, or in the block of an image that is not ok, stays as the caller left it.
int train_out_download(sbm_ctx* c, const sbm_train_image* images, int n, const TrainOut& o, sbm_template_level* levels, sbm_train_feature* feats,
                       int32_t* status)
{
    const uint8_t* d_out = c->d_train_out.as<uint8_t>();
    std::vector<sbm_train_feature> made(o.ft_bytes / sizeof(sbm_train_feature));
    HIP_TRY(hipMemcpyAsync(levels, d_out, o.lv_bytes, hipMemcpyDeviceToHost, c->stream));
    if (o.ft_bytes) HIP_TRY(hipMemcpyAsync(made.data(), d_out + o.o_feats, o.ft_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(status, d_out + o.o_status, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; ++i)
        if (status[2 * i] == 0 && status[2 * i + 1] > 0)
            memcpy(feats + images[i].feat_first, made.data() + images[i].feat_first, (size_t)status[2 * i + 1] * sizeof(sbm_train_feature));
    return 0;
}

} // namespace

extern "C" {

int sbm_train_ragged(sbm_ctx* c, const sbm_train_image* images, int32_t n_images, int32_t channels, float strong_threshold, sbm_template_level* levels,
                     sbm_train_feature* feats, int32_t* status)
{
    if (!c || !levels || !status) return fail(SBM_ERR_INVALID, "null argument");
    TrainRaggedPlan plan = train_ragged_plan(images, n_images, channels, c->L);
    if (int e = train_ragged_verdict(plan)) return e;
    const int64_t feats_end = train_feats_end(images, n_images);
    if (!feats && feats_end > 0) return fail(SBM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    if (int e = order_after_caller_work(c)) return e;
    const size_t n = (size_t)n_images;
    std::vector<size_t> o_img(n), o_mask(n);
    size_t in_bytes = 0, mask_bytes = 0;
    for (size_t i = 0; i < n; ++i) {
        o_img[i] = in_bytes;
        in_bytes += train_align((size_t)images[i].cols * channels * images[i].rows + 64);
        o_mask[i] = mask_bytes;
        if (images[i].mask) mask_bytes += train_align((size_t)images[i].rows * images[i].cols);
    }
    TrainOut o;
    if (in_bytes > c->d_train_in.cap || mask_bytes > c->d_train_mask.cap) HIP_TRY(hipStreamSynchronize(c->stream));
    int rc = 0;
    if ((rc = c->d_train_in.ensure(in_bytes)) || (mask_bytes && (rc = c->d_train_mask.ensure(mask_bytes))) || (rc = train_out_ensure(c, n_images, feats_end, o)))
        return rc;
    hipStream_t s = c->stream;
    uint8_t* d_in = c->d_train_in.as<uint8_t>();
    uint8_t* d_mask = c->d_train_mask.as<uint8_t>();
    uint8_t* d_out = c->d_train_out.as<uint8_t>();
    std::vector<sbm_train_image> dev(images, images + n);
    for (size_t i = 0; i < n; ++i) {
        const size_t row_bytes = (size_t)images[i].cols * channels;
        HIP_TRY(hipMemcpy2DAsync(d_in + o_img[i], row_bytes, images[i].img, (size_t)images[i].stride, row_bytes, (size_t)images[i].rows, hipMemcpyHostToDevice, s));
        dev[i].img = d_in + o_img[i];
        dev[i].stride = (int32_t)row_bytes;
        if (images[i].mask) {
            HIP_TRY(hipMemcpyAsync(d_mask + o_mask[i], images[i].mask, (size_t)images[i].rows * images[i].cols, hipMemcpyHostToDevice, s));
            dev[i].mask = d_mask + o_mask[i];
        }
    }
    HIP_TRY(hipMemsetAsync(d_out, 0, o.total, s));
    if (c->profiling && !c->profiling_keep) c->clear_timings();
    plan = train_ragged_plan(dev.data(), n_images, channels, c->L); // the device copies' strides
    if ((rc = train_ragged_enqueue(c, s, dev.data(), plan, strong_threshold, (sbm_template_level*)d_out, (sbm_train_feature*)(d_out + o.o_feats),
                                   (int32_t*)(d_out + o.o_status), nullptr)))
        return rc;
    return train_out_download(c, images, n_images, o, levels, feats, status);
}

int sbm_train_sweep_device(sbm_ctx* c, const void* d_img, int32_t rows, int32_t cols, int32_t stride, int32_t channels, const void* d_mask,
                           const sbm_train_scale* scales, int32_t n_scales, float strong_threshold, void* d_levels, void* d_feats, void* d_status,
                           void* stream)
{
    if (!c || !d_img || !d_levels || !d_status) return fail(SBM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    std::vector<sbm_train_image> imgs;
    TrainSweepJob job;
    if (int e = train_sweep_prepare(c, (const uint8_t*)d_img, rows, cols, stride, channels, (const uint8_t*)d_mask, scales, n_scales, imgs, job)) return e;
    TrainRaggedPlan plan = train_ragged_plan(imgs.data(), n_scales, channels, c->L);
    if (int e = train_ragged_verdict(plan)) return e;
    if (!d_feats && train_feats_end(imgs.data(), n_scales) > 0) return fail(SBM_ERR_INVALID, "null argument");
    hipStream_t s = launch_stream(c, stream);
    if (c->profiling && !c->profiling_keep) c->clear_timings();
    return train_ragged_enqueue(c, s, imgs.data(), plan, strong_threshold, (sbm_template_level*)d_levels, (sbm_train_feature*)d_feats, (int32_t*)d_status, &job);
}

int sbm_train_sweep(sbm_ctx* c, const uint8_t* img, int32_t rows, int32_t cols, int32_t stride, int32_t channels, const uint8_t* mask,
                    const sbm_train_scale* scales, int32_t n_scales, float strong_threshold, sbm_template_level* levels, sbm_train_feature* feats,
                    int32_t* status)
{
    if (!c || !img || !levels || !status) return fail(SBM_ERR_INVALID, "null argument");
    if (int e = train_sweep_source_check(rows, cols, stride, channels)) return e;
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    if (int e = order_after_caller_work(c)) return e;
    const size_t row_bytes = (size_t)cols * channels, in_bytes = train_align(row_bytes * rows + 64), npx = (size_t)rows * cols;
    if (in_bytes > c->d_train_in.cap || (mask && npx > c->d_train_mask.cap)) HIP_TRY(hipStreamSynchronize(c->stream));
    int rc = 0;
    if ((rc = c->d_train_in.ensure(in_bytes)) || (mask && (rc = c->d_train_mask.ensure(npx)))) return rc;
    const uint8_t* d_img = c->d_train_in.as<uint8_t>();
    const uint8_t* d_mask = mask ? c->d_train_mask.as<uint8_t>() : nullptr;
    std::vector<sbm_train_image> imgs;
    TrainSweepJob job;
    if ((rc = train_sweep_prepare(c, d_img, rows, cols, (int)row_bytes, channels, d_mask, scales, n_scales, imgs, job))) return rc;
    TrainRaggedPlan plan = train_ragged_plan(imgs.data(), n_scales, channels, c->L);
    if ((rc = train_ragged_verdict(plan))) return rc;
    const int64_t feats_end = train_feats_end(imgs.data(), n_scales);
    if (!feats && feats_end > 0) return fail(SBM_ERR_INVALID, "null argument");
    TrainOut o;
    if ((rc = train_out_ensure(c, n_scales, feats_end, o))) return rc;
    hipStream_t s = c->stream;
    uint8_t* d_out = c->d_train_out.as<uint8_t>();
    // the source and its mask, once
    HIP_TRY(hipMemcpy2DAsync((void*)d_img, row_bytes, img, (size_t)stride, row_bytes, (size_t)rows, hipMemcpyHostToDevice, s));
    if (mask) HIP_TRY(hipMemcpyAsync((void*)d_mask, mask, npx, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_out, 0, o.total, s));
    if (c->profiling && !c->profiling_keep) c->clear_timings();
    if ((rc = train_ragged_enqueue(c, s, imgs.data(), plan, strong_threshold, (sbm_template_level*)d_out, (sbm_train_feature*)(d_out + o.o_feats),
                                   (int32_t*)(d_out + o.o_status), &job)))
        return rc;
    return train_out_download(c, imgs.data(), n_scales, o, levels, feats, status);
}

} // extern "C"

// ---- rotated template families ---------------------------------------------------------------------------------------------

namespace {

// What the host can judge of a rotate call: the counts, the angles and centres against the domain of sbm_rotate_math.h,
// the output blocks (base b's n_thetas * out_cap records from out_first) against each other.  *feats_end: the end of the
// feature array the blocks lie in, in records.
int train_rotate_check(const sbm_ctx* c, const sbm_rotate_base* bases, int n_bases, const float* thetas, int n_thetas, int64_t* feats_end)
{
    if (n_bases < 1 || n_thetas < 1) return fail(SBM_ERR_INVALID, "%d bases and %d angles: at least one of each", n_bases, n_thetas);
    if ((int64_t)n_bases * n_thetas > ((int64_t)1 << 31) / c->L)
        return fail(SBM_ERR_INVALID, "%d bases x %d angles exceed 2^31 / %d levels", n_bases, n_thetas, c->L);
    for (int k = 0; k < n_thetas; ++k)
        if (!rotate_theta_ok(thetas[k])) return fail(SBM_ERR_INVALID, "angle %d: not finite or beyond +-36000 degrees", k);
    std::vector<std::pair<int64_t, int64_t>> blocks; // [first, end) of the bases that write anything
    int64_t end = 0;
    for (int b = 0; b < n_bases; ++b) {
        const sbm_rotate_base& r = bases[b];
        if (!r.levels || !r.feats) return fail(SBM_ERR_INVALID, "base %d: null levels or features", b);
        if (!rotate_center_ok(r.center_x) || !rotate_center_ok(r.center_y)) return fail(SBM_ERR_INVALID, "base %d: centre not finite or beyond +-65536", b);
        if (r.out_first < 0 || r.out_cap < 0) return fail(SBM_ERR_INVALID, "base %d: negative out_first or out_cap", b);
        if (r.out_cap > (INT64_MAX / (int64_t)sizeof(sbm_train_feature) - r.out_first) / n_thetas) return fail(SBM_ERR_INVALID, "base %d: output block too large", b);
        if (r.out_cap == 0) continue;
        blocks.emplace_back(r.out_first, r.out_first + r.out_cap * n_thetas);
        end = std::max(end, blocks.back().second);
    }
    std::sort(blocks.begin(), blocks.end());
    for (size_t i = 1; i < blocks.size(); ++i)
        if (blocks[i].first < blocks[i - 1].second) return fail(SBM_ERR_INVALID, "the output blocks of two bases overlap");
    *feats_end = end;
    return 0;
}

// The records and the angle table through the pinned slot onto the stream, into the training scratch, then the one launch.
int train_rotate_enqueue(sbm_ctx* c, hipStream_t s, const sbm_rotate_base* bases, int n_bases, const float* thetas, int n_thetas, sbm_template_level* d_levels,
                         sbm_train_feature* d_feats, int32_t* d_status)
{
    const size_t base_bytes = train_align((size_t)n_bases * sizeof(sbm_rotate_base)), total = base_bytes + train_align((size_t)n_thetas * sizeof(RotateAngle));
    if (total > c->d_train.cap) {
        HIP_TRY(hipDeviceSynchronize()); // calls in flight may use the old scratch
        if (int e = c->d_train.ensure(total)) return e;
    }
    uint8_t* d_table = c->d_train.as<uint8_t>();
    uint8_t* slot = nullptr;
    if (int e = train_table_slot(c, total, &slot)) return e;
    memset(slot, 0, total);
    memcpy(slot, bases, (size_t)n_bases * sizeof(sbm_rotate_base));
    RotateAngle* angles = (RotateAngle*)(slot + base_bytes);
    for (int k = 0; k < n_thetas; ++k) angles[k] = rotate_angle(thetas[k]);
    c->train_table_busy = true; // as train_ragged_enqueue: from before the copy
    c->train_table_stream = s;
    c->train_table_recorded = false;
    HIP_TRY(hipMemcpyAsync(d_table, slot, total, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->ev_train_table, s));
    c->train_table_recorded = true;
    SBM_LAUNCH(c, "k_train_rotate", k_train_rotate, dim3(n_thetas, std::min(n_bases, 65535)), dim3(256), 0, s, (const sbm_rotate_base*)d_table,
               (const RotateAngle*)(d_table + base_bytes), c->L, n_bases, d_levels, d_feats, d_status);
    HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace

extern "C" {

int sbm_train_rotate_device(sbm_ctx* c, const sbm_rotate_base* bases, int32_t n_bases, const float* thetas, int32_t n_thetas, void* d_levels, void* d_feats,
                            void* d_status, void* stream)
{
    if (!c || !bases || !thetas || !d_levels || !d_status) return fail(SBM_ERR_INVALID, "null argument");
    int64_t feats_end = 0;
    if (int e = train_rotate_check(c, bases, n_bases, thetas, n_thetas, &feats_end)) return e;
    if (!d_feats && feats_end > 0) return fail(SBM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    hipStream_t s = launch_stream(c, stream);
    if (c->profiling && !c->profiling_keep) c->clear_timings();
    return train_rotate_enqueue(c, s, bases, n_bases, thetas, n_thetas, (sbm_template_level*)d_levels, (sbm_train_feature*)d_feats, (int32_t*)d_status);
}

int sbm_train_rotate(sbm_ctx* c, const sbm_rotate_base* bases, int32_t n_bases, const float* thetas, int32_t n_thetas, sbm_template_level* levels,
                     sbm_train_feature* feats, int32_t* status)
{
    if (!c || !bases || !thetas || !levels || !status) return fail(SBM_ERR_INVALID, "null argument");
    int64_t feats_end = 0;
    if (int e = train_rotate_check(c, bases, n_bases, thetas, n_thetas, &feats_end)) return e;
    if (!feats && feats_end > 0) return fail(SBM_ERR_INVALID, "null argument");
    const int L = c->L;
    const size_t nb = (size_t)n_bases, pairs = nb * (size_t)n_thetas;
    // the bases as one block of host bytes: per base its level records, its status pair, its features up to the end the
    // records give (none of a base that is not ok, or whose counts the kernel refuses: it reads no feature of those)
    std::vector<size_t> o_lv(nb), o_st(nb), o_ft(nb), n_ft(nb, 0);
    size_t in_bytes = 0;
    for (size_t b = 0; b < nb; ++b) {
        const sbm_rotate_base& r = bases[b];
        o_lv[b] = in_bytes;
        in_bytes += train_align((size_t)L * sizeof(sbm_template_level));
        o_st[b] = in_bytes;
        in_bytes += 256;
        o_ft[b] = in_bytes;
        if (rotate_base_verdict(r.status, r.levels, L, INT64_MAX).code != ROTATE_OK) continue;
        int64_t ext = 0;
        for (int l = 0; l < L; ++l) {
            if (r.levels[l].n_features == 0) continue;
            if (r.levels[l].feature_offset < 0) return fail(SBM_ERR_INVALID, "base %zu: negative feature_offset at level %d", b, l);
            ext = std::max(ext, r.levels[l].feature_offset + r.levels[l].n_features);
        }
        n_ft[b] = (size_t)ext;
        in_bytes += train_align(n_ft[b] * sizeof(sbm_train_feature));
    }
    std::vector<uint8_t> in(in_bytes, 0);
    for (size_t b = 0; b < nb; ++b) {
        memcpy(in.data() + o_lv[b], bases[b].levels, (size_t)L * sizeof(sbm_template_level));
        if (bases[b].status) memcpy(in.data() + o_st[b], bases[b].status, 8);
        if (n_ft[b]) memcpy(in.data() + o_ft[b], bases[b].feats, n_ft[b] * sizeof(sbm_train_feature));
    }
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    if (int e = order_after_caller_work(c)) return e;
    const size_t lv_bytes = pairs * (size_t)L * sizeof(sbm_template_level), ft_bytes = (size_t)feats_end * sizeof(sbm_train_feature),
                 o_feats = train_align(lv_bytes), o_status = o_feats + train_align(ft_bytes), out_total = o_status + pairs * 8;
    if (in_bytes > c->d_train_in.cap || out_total > c->d_train_out.cap) HIP_TRY(hipStreamSynchronize(c->stream));
    int rc = 0;
    if ((rc = c->d_train_in.ensure(in_bytes)) || (rc = c->d_train_out.ensure(out_total))) return rc;
    hipStream_t s = c->stream;
    uint8_t* d_in = c->d_train_in.as<uint8_t>();
    uint8_t* d_out = c->d_train_out.as<uint8_t>();
    std::vector<sbm_rotate_base> dev(bases, bases + nb);
    for (size_t b = 0; b < nb; ++b) {
        dev[b].levels = (const sbm_template_level*)(d_in + o_lv[b]);
        dev[b].status = bases[b].status ? (const int32_t*)(d_in + o_st[b]) : nullptr;
        dev[b].feats = (const sbm_train_feature*)(d_in + o_ft[b]);
    }
    HIP_TRY(hipMemcpyAsync(d_in, in.data(), in_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_out, 0, out_total, s));
    if (c->profiling && !c->profiling_keep) c->clear_timings();
    if ((rc = train_rotate_enqueue(c, s, dev.data(), n_bases, thetas, n_thetas, (sbm_template_level*)d_out, (sbm_train_feature*)(d_out + o_feats),
                                   (int32_t*)(d_out + o_status))))
        return rc;
    // of the feature array only the records the call made reach the caller's (train_out_download)
    std::vector<sbm_train_feature> made((size_t)feats_end);
    HIP_TRY(hipMemcpyAsync(levels, d_out, lv_bytes, hipMemcpyDeviceToHost, s));
    if (ft_bytes) HIP_TRY(hipMemcpyAsync(made.data(), d_out + o_feats, ft_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(status, d_out + o_status, pairs * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t b = 0; b < nb; ++b)
        for (size_t k = 0; k < (size_t)n_thetas; ++k) {
            const size_t p = b * (size_t)n_thetas + k;
            const int64_t first = bases[b].out_first + (int64_t)k * bases[b].out_cap;
            if (status[2 * p] == 0 && status[2 * p + 1] > 0) memcpy(feats + first, made.data() + first, (size_t)status[2 * p + 1] * sizeof(sbm_train_feature));
        }
    return 0;
}

} // extern "C"
