// sbm_train_kernels.h — training side of the engine (gfx950): the per-pixel scan of
// ColorGradientPyramid::extractTemplate (line2Dup.cpp:452-539) as a data-parallel kernel.
//
// The reference walks the image in row-major order with a `magnitude_valid` map: a pixel that is still valid and has no
// 5x5 neighbour of strictly larger squared magnitude (:485) is a local maximum, invalidates its 24 neighbours (:494-500)
// and becomes a feature candidate if its score exceeds strong_threshold^2 and it has a quantised orientation (:504).
// That scan is order-dependent only through ties: a maximum q can invalidate a pixel p that would itself have been a
// maximum only if score(p) == score(q) (each is >= the other).  So:
//   1. (this kernel) every pixel of the scanned region [2, rows-2) x [2, cols-2) that passes the eroded mask, scores
//      above strong_threshold^2 and has no strictly larger 5x5 neighbour is emitted -- no order involved;
//   2. (host, sbm_extract_local_maxima) the emitted pixels are sorted row-major and a pixel is dropped when an earlier
//      KEPT pixel lies within its 5x5 window -- the reference's invalidation among equal-score neighbours, exactly.
// Maxima at or below the threshold never influence the result: to invalidate a candidate they would need its score.
// The batched path (sbm_train_batch_device, below) does step 2 and everything after it on the device as well.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sbm.h"
#include "sbm_resize_table.h"
#include "sbm_train_math.h"
#include "sbm_train_plan.h"

namespace sbm {

// out_xy[k] = x | y << 16; *count may exceed cap (the caller retries with a larger buffer)
__global__ __launch_bounds__(256) void k_local_maxima5(const float* __restrict__ mag, const uint8_t* __restrict__ mask, int rows, int cols,
                                                       float thr_sq, int32_t* __restrict__ out_xy, int32_t* __restrict__ count, int cap)
{
    const int iw = cols - 4, ih = rows - 4;
    const int n = iw * ih;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < n; idx += gridDim.x * 256) {
        const int r = 2 + idx / iw, c = 2 + idx % iw;
        const float s = mag[(size_t)r * cols + c];
        if (!(s > thr_sq)) continue;
        if (mask) { // cv::erode(mask, 3x3, BORDER_REPLICATE): every pixel of the 3x3 window (clamped) must be set (:459-463)
            bool keep = true;
            for (int dr = -1; dr <= 1 && keep; ++dr) {
                const int rr = min(max(r + dr, 0), rows - 1);
                for (int dc = -1; dc <= 1; ++dc) keep = keep && mask[(size_t)rr * cols + min(max(c + dc, 0), cols - 1)] != 0;
            }
            if (!keep) continue;
        }
        bool is_max = true;
        for (int dr = -2; dr <= 2 && is_max; ++dr) {
            const float* row = mag + (size_t)(r + dr) * cols + c;
            for (int dc = -2; dc <= 2; ++dc) is_max = is_max && !(s < row[dc]);
        }
        if (!is_max) continue;
        const int k = atomicAdd(count, 1);
        if (k < cap) out_xy[k] = c | (r << 16);
    }
}

// ---- batched training (sbm_train_batch_device): everything after the gradient stage, without a host round trip --------
// Per (image, level): S = the pixels k_local_maxima5 would emit, as a dense flag plane (k_train_maxima); the row-major
// tie resolution on it and the row-major list of candidates (k_train_resolve); their order (k_train_sort); the
// selection of scattered features (k_train_select); per image, cropTemplates and the caller's layout (k_train_crop).
// The scalar rules are those of sbm_train_math.h.  The level is a grid dimension beside the image; the levels of an
// image lie behind each other in one per-image "pixel space" (planes) and "candidate space" (lists).
// TrainCand, TrainLevel and the ragged form's TrainRecord: sbm_train_plan.h, which a CPU compiler takes.
struct TrainPlan {
    int32_t L, n_images;
    float thr_sq;
    int64_t pix_stride, cand_stride, sort_stride; // per image
    const float* mag;     // [n_images][pix_stride]
    const float* ori;
    const uint8_t* quant;
    uint8_t* flags;       // bit 0: in S; bit 1: kept by the tie resolution
    TrainCand* cand;      // [n_images][cand_stride]
    uint64_t* keys;       // [n_images][sort_stride]
    int32_t* sel;         // [n_images][cand_stride]: the selected candidates, as indices into the level's list
    uint32_t* kept_xy;    // [n_images][cand_stride]: their positions beyond what LDS holds
    int32_t* counts;      // [n_images][L][2]: candidates; selected features, -1 = the level failed
    TrainLevel lv[8];
    const TrainRecord* table; // the ragged form: [n_images][L] records of the images' own geometry (lv unused, strides 0)
};

// The record of (image, level).  RAGGED = false: the call's one geometry, p.lv[l], and offsets img * stride + off.
// RAGGED = true: the image's own record of the device table -- absolute offsets under strides of 0, its own mask and
// feature count; indexed by blockIdx only, so the record is wave-uniform and its fields are scalar loads.
template <bool RAGGED>
__device__ __forceinline__ const TrainLevel& train_level(const TrainPlan& p, int img, int l)
{
    if constexpr (RAGGED) return p.table[(int64_t)img * p.L + l];
    else return p.lv[l];
}

enum { TRAIN_KEPT_LDS = 4096 };

template <bool RAGGED>
__global__ __launch_bounds__(256) void k_train_maxima(const TrainPlan p)
{
    const TrainLevel& v = train_level<RAGGED>(p, blockIdx.z, blockIdx.y);
    const int64_t base = (int64_t)blockIdx.z * p.pix_stride + v.pix_off;
    const float* __restrict__ mag = p.mag + base;
    uint8_t* __restrict__ flags = p.flags + base;
    const uint8_t* __restrict__ mask = v.mask ? v.mask + (int64_t)blockIdx.z * v.mask_fs : nullptr;
    const int rows = v.rows, cols = v.cols, n = rows * cols;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < n; idx += gridDim.x * 256) {
        const int r = idx / cols, c = idx % cols;
        bool in = r >= 2 && r < rows - 2 && c >= 2 && c < cols - 2;
        float s = 0.f;
        if (in) {
            s = mag[idx];
            in = s > p.thr_sq;
        }
        if (in && mask) { // cv::erode(mask, 3x3, BORDER_REPLICATE); the window of a scanned pixel lies inside the image
            for (int dr = -1; dr <= 1; ++dr)
                for (int dc = -1; dc <= 1; ++dc) in = in && mask[idx + dr * cols + dc] != 0;
        }
        if (in) {
            for (int dr = -2; dr <= 2; ++dr)
                for (int dc = -2; dc <= 2; ++dc) in = in && !(s < mag[idx + dr * cols + dc]);
        }
        flags[idx] = in ? 1 : 0;
    }
}

// One wave per (image, level) walks the rows.  Lane i owns the columns [i * K, (i + 1) * K): it composes the column
// maps of its segment, the wave composes the segments' maps by a prefix scan, and the lane replays its segment from its
// incoming state.  Kept pixels are marked in the flag plane, where the next two rows find them.
template <bool RAGGED>
__global__ __launch_bounds__(64) void k_train_resolve(const TrainPlan p)
{
    const int l = blockIdx.x, img = blockIdx.y, lane = threadIdx.x;
    const TrainLevel& v = train_level<RAGGED>(p, img, l);
    const int cand_cap = v.cand_cap; // read before the first store: the record stays in scalar registers
    const int64_t base = (int64_t)img * p.pix_stride + v.pix_off;
    uint8_t* flags = p.flags + base;
    const uint8_t* __restrict__ quant = p.quant + base;
    const float* __restrict__ mag = p.mag + base;
    const float* __restrict__ ori = p.ori + base;
    TrainCand* __restrict__ cand = p.cand + (int64_t)img * p.cand_stride + v.cand_off;
    const int rows = v.rows, cols = v.cols;
    const int K = (cols + 63) / 64;
    const int c0 = min(lane * K, cols), c1 = min(c0 + K, cols);
    int total = 0;
    for (int r = 2; r < rows - 2; ++r) {
        uint8_t* f0 = flags + (size_t)r * cols;
        const uint8_t* f1 = f0 - cols;
        const uint8_t* f2 = f1 - cols;
        // a pixel of S has its five columns inside the image
        auto available = [&](int c) {
            if (!(f0[c] & 1)) return false;
            uint32_t above = 0;
            for (int d = -2; d <= 2; ++d) above |= (uint32_t)f1[c + d] | (uint32_t)f2[c + d];
            return (above & 2u) == 0;
        };
        uint32_t f = TRAIN_TIE_IDENTITY;
        for (int c = c0; c < c1; ++c) f = train_tie_compose(f, train_tie_fn(available(c)));
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t g = __shfl_up(f, d);
            if (lane >= d) f = train_tie_compose(g, f);
        }
        const uint32_t before = __shfl_up(f, 1);
        uint32_t state = lane ? train_tie_apply(before, 0) : 0u;
        int cnt = 0;
        for (int c = c0; c < c1; ++c) {
            const bool a = available(c);
            if (train_tie_keeps(a, state)) {
                f0[c] = 3;
                cnt += quant[(size_t)r * cols + c] != 0;
            }
            state = train_tie_apply(train_tie_fn(a), state);
        }
        int incl = cnt;
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        int pos = total + incl - cnt;
        total += __shfl(incl, 63);
        if (cnt) {
            for (int c = c0; c < c1; ++c) {
                const uint32_t a = quant[(size_t)r * cols + c];
                if ((f0[c] & 2) && a) {
                    if (pos < cand_cap) {
                        TrainCand k;
                        k.xy = c | (r << 16);
                        k.label = __ffs(a) - 1;
                        k.score = mag[(size_t)r * cols + c];
                        k.theta = ori[(size_t)r * cols + c];
                        cand[pos] = k;
                    }
                    ++pos;
                }
            }
        }
        __syncthreads(); // the marks of this row, before the next row reads them
    }
    if (lane == 0) p.counts[((int64_t)img * p.L + l) * 2] = min(total, cand_cap);
}

// bitonic sort of the level's keys (train_key), descending, in global scratch by one workgroup
template <bool RAGGED>
__global__ __launch_bounds__(256) void k_train_sort(const TrainPlan p)
{
    const int l = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
    const TrainLevel& v = train_level<RAGGED>(p, img, l);
    const uint32_t nf = v.nf;
    const TrainCand* __restrict__ cand = p.cand + (int64_t)img * p.cand_stride + v.cand_off;
    uint64_t* keys = p.keys + (int64_t)img * p.sort_stride + v.sort_off;
    const int n = p.counts[((int64_t)img * p.L + l) * 2];
    if (train_level_fails((size_t)n, nf)) return;
    int P = 1;
    while (P < n) P <<= 1;
    for (int i = tid; i < P; i += 256) keys[i] = i < n ? train_key(__float_as_uint(cand[i].score), (uint32_t)i) : 0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P / 2; t += 256) {
                const int i = (t / j) * 2 * j + (t % j);
                const uint64_t a = keys[i], b = keys[i + j];
                const bool descending = (i & k) == 0;
                if ((a < b) == descending) {
                    keys[i] = b;
                    keys[i + j] = a;
                }
            }
            __syncthreads();
        }
}

// selectScatteredFeatures by one wave per (image, level): the candidates in sorted order, 64 at a time -- every lane
// tests its candidate against the features kept before the chunk, then the chunk's survivors are taken in order, each
// one striking out the later survivors too close to it.  That is the sequential sweep: a candidate is taken iff it is far
// from every feature taken before it.
template <bool RAGGED>
__global__ __launch_bounds__(64) void k_train_select(const TrainPlan p)
{
    __shared__ uint32_t s_kept[TRAIN_KEPT_LDS];
    const int l = blockIdx.x, img = blockIdx.y, lane = threadIdx.x;
    const TrainLevel& v = train_level<RAGGED>(p, img, l);
    const int cand_cap = v.cand_cap; // read before the first store: the record stays in scalar registers
    const uint32_t nf = v.nf;
    const TrainCand* __restrict__ cand = p.cand + (int64_t)img * p.cand_stride + v.cand_off;
    const uint64_t* __restrict__ keys = p.keys + (int64_t)img * p.sort_stride + v.sort_off;
    int32_t* __restrict__ sel = p.sel + (int64_t)img * p.cand_stride + v.cand_off;
    uint32_t* kept_g = p.kept_xy + (int64_t)img * p.cand_stride + v.cand_off;
    int32_t* counts = p.counts + ((int64_t)img * p.L + l) * 2;
    const int n = counts[0];
    if (train_level_fails((size_t)n, nf)) {
        if (lane == 0) counts[1] = -1;
        return;
    }
    TrainSelect st = train_select_begin((size_t)n, nf);
    int cnt = 0;
    for (;;) {
        const float d2 = st.distance * st.distance;
        for (int first = 0; first < n; first += 64) {
            const int i = first + lane;
            int idx = 0, xy = 0;
            if (i < n) {
                idx = (int)train_key_index(keys[i]);
                xy = cand[idx].xy;
            }
            const int x = xy & 0xffff, y = xy >> 16;
            bool alive = i < n;
            for (int j = 0; j < cnt; ++j) {
                const uint32_t k = j < TRAIN_KEPT_LDS ? s_kept[j] : kept_g[j];
                alive = alive && train_far(x, y, (int)(k & 0xffffu), (int)(k >> 16), d2);
                if ((j & 15) == 15 && !__builtin_amdgcn_ballot_w64(alive)) break;
            }
            uint64_t m = __builtin_amdgcn_ballot_w64(alive);
            while (m) {
                const int k = __ffsll((unsigned long long)m) - 1;
                const int kxy = __shfl(xy, k);
                if (lane == k) {
                    if (cnt < cand_cap) {
                        if (cnt < TRAIN_KEPT_LDS) s_kept[cnt] = (uint32_t)xy;
                        else kept_g[cnt] = (uint32_t)xy;
                        sel[cnt] = idx;
                    }
                    alive = false;
                }
                ++cnt;
                alive = alive && train_far(x, y, kxy & 0xffff, kxy >> 16, d2);
                m = __builtin_amdgcn_ballot_w64(alive);
            }
            __syncthreads(); // the chunk's features, before the next chunk reads them
        }
        const int next = train_select_next(st, (size_t)cnt, nf);
        if (next == TRAIN_PASS_STOP) break;
        if (next == TRAIN_PASS_RESTART) cnt = 0;
    }
    if (lane == 0) counts[1] = min(cnt, cand_cap);
}

// cropTemplates and the caller's layout, one workgroup per image.  status: {0, features} | {1, first failing level} |
// {2, features needed} when they exceed feat_cap; the level records of an image that is not ok are zeroed.  The
// ragged form takes the image's feature block from its record (feat_first, feat_cap) instead of img * feat_cap.
template <bool RAGGED>
__global__ __launch_bounds__(256) void k_train_crop(const TrainPlan p, sbm_template_level* __restrict__ levels, sbm_train_feature* __restrict__ feats,
                                                    int64_t feat_cap, int32_t* __restrict__ status)
{
    __shared__ int s_mm[4];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int32_t* counts = p.counts + (int64_t)img * p.L * 2;
    levels += (int64_t)img * p.L;
    if constexpr (RAGGED) {
        const TrainRecord& rec = p.table[(int64_t)img * p.L];
        feats += rec.feat_first;
        feat_cap = rec.feat_cap;
    } else {
        feats += (int64_t)img * feat_cap;
    }
    int failed = -1;
    int64_t total = 0;
    for (int l = p.L - 1; l >= 0; --l) {
        if (counts[2 * l + 1] < 0) failed = l;
        else total += counts[2 * l + 1];
    }
    if (failed >= 0 || total > feat_cap) {
        if (tid < p.L) {
            sbm_template_level z;
            z.width = z.height = z.tl_x = z.tl_y = z.pyramid_level = z.n_features = 0;
            z.feature_offset = 0;
            levels[tid] = z;
        }
        if (tid == 0) {
            status[2 * img] = failed >= 0 ? 1 : 2;
            status[2 * img + 1] = failed >= 0 ? failed : (int32_t)min(total, (int64_t)INT32_MAX);
        }
        return;
    }
    if (tid == 0) {
        s_mm[0] = s_mm[1] = INT32_MAX;
        s_mm[2] = s_mm[3] = INT32_MIN;
    }
    __syncthreads();
    int mn_x = INT32_MAX, mn_y = INT32_MAX, mx_x = INT32_MIN, mx_y = INT32_MIN;
    for (int l = 0; l < p.L; ++l) {
        const TrainCand* __restrict__ cand = p.cand + (int64_t)img * p.cand_stride + train_level<RAGGED>(p, img, l).cand_off;
        const int32_t* __restrict__ sel = p.sel + (int64_t)img * p.cand_stride + train_level<RAGGED>(p, img, l).cand_off;
        for (int k = tid; k < counts[2 * l + 1]; k += 256) {
            const int xy = cand[sel[k]].xy;
            const int x = (xy & 0xffff) << l, y = (xy >> 16) << l;
            mn_x = min(mn_x, x), mn_y = min(mn_y, y), mx_x = max(mx_x, x), mx_y = max(mx_y, y);
        }
    }
    atomicMin(&s_mm[0], mn_x);
    atomicMin(&s_mm[1], mn_y);
    atomicMax(&s_mm[2], mx_x);
    atomicMax(&s_mm[3], mx_y);
    __syncthreads();
    const int min_x = train_crop_even(s_mm[0]), min_y = train_crop_even(s_mm[1]);
    int64_t off = 0;
    for (int l = 0; l < p.L; ++l) {
        const TrainCand* __restrict__ cand = p.cand + (int64_t)img * p.cand_stride + train_level<RAGGED>(p, img, l).cand_off;
        const int32_t* __restrict__ sel = p.sel + (int64_t)img * p.cand_stride + train_level<RAGGED>(p, img, l).cand_off;
        const int nl = counts[2 * l + 1];
        const TrainBox b = train_crop_level(min_x, min_y, s_mm[2], s_mm[3], l);
        if (tid == 0) {
            sbm_template_level t;
            t.width = b.width;
            t.height = b.height;
            t.tl_x = b.tl_x;
            t.tl_y = b.tl_y;
            t.pyramid_level = l;
            t.n_features = nl;
            t.feature_offset = off;
            levels[l] = t;
        }
        for (int k = tid; k < nl; k += 256) {
            const TrainCand c = cand[sel[k]];
            sbm_train_feature f;
            f.x = (c.xy & 0xffff) - b.tl_x;
            f.y = (c.xy >> 16) - b.tl_y;
            f.label = c.label;
            f.theta = c.theta;
            feats[off + k] = f;
        }
        off += nl;
    }
    if (tid == 0) {
        status[2 * img] = 0;
        status[2 * img + 1] = (int32_t)total;
    }
}

// ---- the level steps of the ragged form: one launch per level, image = blockIdx.y --------------------------------------
// Level l's image from level l-1's (cv::pyrDown, line2Dup.cpp:431-433) and level l's mask from level l-1's (nearest
// neighbour, :439), both geometries and all four addresses from the image's records; the samples are k_pyrdown's and
// k_resize_mask's.  The grid's x is sized for the batch's largest level l; a level that is not built has no pixel.
__global__ __launch_bounds__(256) void k_train_pyrdown(const TrainRecord* __restrict__ table, int L, int l, int ch)
{
    const TrainRecord& s = table[(int64_t)blockIdx.y * L + l - 1];
    const TrainRecord& d = table[(int64_t)blockIdx.y * L + l];
    const uint8_t* __restrict__ src = s.img;
    uint8_t* __restrict__ dst = const_cast<uint8_t*>(d.img);
    const int rows = s.rows, cols = s.cols, stride = s.stride, dc = d.cols;
    const int n = d.rows * dc;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < n; idx += gridDim.x * 256) pyrdown_pixel(src, rows, cols, ch, stride, dst, idx, dc);
}

__global__ __launch_bounds__(256) void k_train_resize_mask(const TrainRecord* __restrict__ table, int L, int l)
{
    const TrainRecord& s = table[(int64_t)blockIdx.y * L + l - 1];
    const TrainRecord& d = table[(int64_t)blockIdx.y * L + l];
    const uint8_t* __restrict__ src = s.mask;
    uint8_t* __restrict__ dst = const_cast<uint8_t*>(d.mask);
    const int rows = s.rows, cols = s.cols, drows = d.rows, dcols = d.cols;
    const int n = dst ? drows * dcols : 0; // an image without a mask, or a level that is not built
    if (n == 0) return;
    const double fx = (double)cols / dcols, fy = (double)rows / drows;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < n; idx += gridDim.x * 256) dst[idx] = resize_mask_sample(src, rows, cols, fx, fy, idx, dcols);
}

// ---- the scale sweep (sbm_train_sweep_device): every scaled image and mask of one source in one launch -----------------
// cv::resize(src, dst, Size(), fx, fy) of shapeInfo_producer::transform (line2Dup.h:379-405), scale = blockIdx.y.  The
// coefficient tables of sbm_resize_table.h, one pair per scale, lie behind each other in one index and one coefficient
// array; one thread makes one destination sample (resize_linear_sample).  The samples behind the image's are the mask's,
// resized with the same tables as a one-channel plane and thresholded as mask_of does (`> 0`, :455-457).
__global__ __launch_bounds__(256) void k_resize_sweep_u8(const uint8_t* __restrict__ src, int rows, int cols, int ch, int stride,
                                                         const uint8_t* __restrict__ mask, const TrainSweepScale* __restrict__ scales,
                                                         const int32_t* __restrict__ tab_idx, const int16_t* __restrict__ tab_coef)
{
    const TrainSweepScale& sc = scales[blockIdx.y];
    const int drows = sc.rows, dcols = sc.cols;
    const int32_t* __restrict__ xi = tab_idx + sc.x_off;
    const int32_t* __restrict__ yi = tab_idx + sc.y_off;
    const int16_t* __restrict__ xa = tab_coef + 2 * sc.x_off;
    const int16_t* __restrict__ ya = tab_coef + 2 * sc.y_off;
    uint8_t* __restrict__ dst = sc.img;
    uint8_t* __restrict__ dmask = sc.mask;
    const int64_t npx = (int64_t)drows * dcols, n_img = npx * ch, n = n_img + (mask ? npx : 0);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const bool m = i >= n_img;
        const int64_t j = m ? i - n_img : i;
        const int c = m ? 1 : ch, k = (int)(j % c);
        const int64_t px = j / c;
        const int x = (int)(px % dcols), y = (int)(px / dcols);
        const int x0 = xi[x], x1 = x0 + 1 < cols ? x0 + 1 : cols - 1;
        const int y0 = yi[y], y1 = y0 + 1 < rows ? y0 + 1 : rows - 1;
        const int64_t st = m ? cols : stride;
        const uint8_t* r0 = (m ? mask : src) + y0 * st;
        const uint8_t* r1 = (m ? mask : src) + y1 * st;
        const uint8_t v = resize_linear_sample(r0[x0 * c + k], r0[x1 * c + k], r1[x0 * c + k], r1[x1 * c + k], xa[2 * x], xa[2 * x + 1], ya[2 * y], ya[2 * y + 1]);
        if (m) dmask[j] = v > 0 ? 255 : 0;
        else dst[j] = v;
    }
}

} // namespace sbm
