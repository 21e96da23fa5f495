// TEST INFRASTRUCTURE: the two reduced forms of the row-streaming gradient kernel (sbm_quantize_stream.h: QS_SOURCE, QS_SPARSE)
// compiled for the CPU against wave_emu.h, the footprint arithmetic they share with the host (sbm_refine_tiles.h) and the
// plan input that selects them (sbm_level_forms.h), behind a C interface.  Compiled by tests/test_sparse_gradient.py into its
// temporary directory; never loaded by the product.
#define SBM_WAVE_EMU 1
#define SBM_WAVE_HEADER "wave_emu.h"
#include <climits>
#include <cmath>
#include <vector>

#include "sbm_level_forms.h"
#include "sbm_quantize_stream.h"

using namespace sbm;

static QSArgs batch_args(const uint8_t* img, int frames, int rows, int cols, int ch, float weak, int hs, int pack)
{
    QSArgs a{};
    a.img = img;
    a.img_fs = (int64_t)rows * cols * ch;
    a.out_fs = (int64_t)rows * cols;
    a.pyr_fs = (int64_t)(rows / 2) * (cols / 2) * ch;
    a.rows = rows;
    a.cols = cols;
    a.stride = cols * ch;
    const float thr_sq = weak * weak;
    a.thr_i = thr_sq < 2147483000.f ? (int)floorf(thr_sq) : INT_MAX;
    a.hs = hs;
    a.row_lo = 0;
    a.row_hi = rows;
    a.n_strips = (cols + QS_USEFUL - 1) / QS_USEFUL;
    a.n_rblocks = (rows + hs - 1) / hs;
    a.frames = frames;
    a.pack_lanes = pack ? quantize_stream_pack_lanes(rows, cols, ch, frames) : 0;
    a.pack_groups = a.pack_lanes ? (frames + 64 / a.pack_lanes - 1) / (64 / a.pack_lanes) : 0;
    return a;
}

static bool bad_geometry(int frames, int rows, int cols, int ch, int hs)
{
    return (ch != 1 && ch != 3) || cols < 4 || (cols & 3) || rows < 2 || (rows & 1) || hs < 2 || (hs & 1) || frames < 1;
}

// the whole row loop, as the engine launches it today: what the two forms together must reproduce
extern "C" int sbm_emu_whole_pass(const uint8_t* img, int frames, int rows, int cols, int ch, float weak, int hs, int pack, uint8_t* out, uint8_t* pyr)
{
    if (bad_geometry(frames, rows, cols, ch, hs)) return -1;
    QSArgs a = batch_args(img, frames, rows, cols, ch, weak, hs, pack);
    a.out = out;
    a.pyr = pyr;
    for (int item = 0; item < quantize_stream_items(a); ++item) {
        if (ch == 3) quantize_stream_item<3>(a, item);
        else quantize_stream_item<1>(a, item);
    }
    return a.pack_lanes;
}

// the source pass over `frames` frames in the caller's layout (rows of `stride` bytes, frames `img_fs` bytes apart):
// pyr = the next level's images, keep = the retained copy, both packed
extern "C" int sbm_emu_source_pass(const uint8_t* img, int frames, int rows, int cols, int ch, int hs, int pack, int stride, int64_t img_fs,
                                   uint8_t* pyr, uint8_t* keep)
{
    if (bad_geometry(frames, rows, cols, ch, hs) || stride < cols * ch || img_fs < (int64_t)rows * stride) return -1;
    QSArgs a = batch_args(img, frames, rows, cols, ch, 0.f, hs, pack);
    a.stride = stride;
    a.img_fs = img_fs;
    a.pyr = pyr;
    a.keep = keep;
    a.keep_fs = (int64_t)rows * cols * ch;
    for (int item = 0; item < quantize_stream_items(a); ++item) {
        if (ch == 3) quantize_stream_item<3, QS_SOURCE>(a, item);
        else quantize_stream_item<1, QS_SOURCE>(a, item);
    }
    return a.pack_lanes;
}

// the sparse gradient pass over the retained copy.  flags: frames x n_tiles bytes of the (T, W, H) strip level, or null.
extern "C" int sbm_emu_sparse_pass(const uint8_t* keep, int frames, int rows, int cols, int ch, float weak, int hs, int pack, const uint8_t* flags,
                                   int T, int W, int H, uint8_t* out)
{
    if (bad_geometry(frames, rows, cols, ch, hs)) return -1;
    QSArgs a = batch_args(keep, frames, rows, cols, ch, weak, hs, pack);
    a.out = out;
    a.tile_flags = flags;
    a.n_tiles = refine_tile_count(W, H);
    a.grid_t = T;
    a.grid_w = W;
    a.grid_h = H;
    for (int item = 0; item < quantize_stream_items(a); ++item) {
        if (ch == 3) quantize_stream_item<3, QS_SPARSE>(a, item);
        else quantize_stream_item<1, QS_SPARSE>(a, item);
    }
    return a.pack_lanes;
}

// One flagged tile (tx, ty) of the T = 4 level of a rows x cols frame, hs rows per gradient work item.  The loads of the tile's
// strip builder are enumerated thread by thread as build_lm_strip4_allty<true> (sbm_lm_kernels.h) issues them -- thread t:
// row = t / 8, kk = t % 8, grid row gy = ty * 32 + row, cells k = tx * 8 + kk, active when gy < H and k * 4 < W; pixel rows
// gy * 4 + d, d < 7, below `rows`; a 16-byte load at column c0 = k * 16 and, when c0 + 16 < cols, a 4-byte load behind it --
// and every loaded pixel must lie in the output rectangle of a work item that gradient_item_needed keeps (the rectangle by the
// kernel's rule, restated here: rows [rb * hs, +hs), the last block moved up to end at the last row; 240 columns per strip).
// Returns the number of loaded pixels no kept item writes, or -1 on bad arguments; *kept = kept items, *loaded = pixels loaded.
extern "C" int64_t sbm_emu_footprint(int rows, int cols, int hs, int tx, int ty, int32_t* kept, int64_t* loaded)
{
    const int T = 4, W = cols / T, H = rows / T;
    const int n_cb = refine_tile_cols(W), n_rb = refine_tile_rows(H);
    if (tx < 0 || tx >= n_cb || ty < 0 || ty >= n_rb || hs < 2 || (hs & 1)) return -1;
    std::vector<uint8_t> flags((size_t)n_cb * n_rb, 0);
    flags[(size_t)ty * n_cb + tx] = 1;
    const int n_strips = (cols + 239) / 240, n_rblocks = (rows + hs - 1) / hs;
    std::vector<uint8_t> cov((size_t)n_strips * rows, 0); // cov[strip][y]: a kept item of that strip writes row y
    *kept = 0;
    for (int s = 0; s < n_strips; ++s)
        for (int rb = 0; rb < n_rblocks; ++rb) {
            if (!gradient_item_needed(flags.data(), s, rb, hs, 240, rows, cols, T, W, H)) continue;
            ++*kept;
            int r0 = rb * hs;
            if (r0 + hs > rows) r0 = rows > hs ? rows - hs : 0;
            for (int y = r0; y < r0 + hs && y < rows; ++y) cov[(size_t)s * rows + y] = 1;
        }
    int64_t missing = 0;
    *loaded = 0;
    for (int t = 0; t < 256; ++t) {
        const int row = t / 8, kk = t % 8, gy = ty * 32 + row, k = tx * 8 + kk;
        if (!(gy < H && k * 4 < W)) continue;
        const int c0 = k * 16;
        for (int d = 0; d < 7; ++d) {
            const int y = gy * T + d;
            if (y >= rows) continue;
            const int c1 = c0 + 16 < cols ? c0 + 20 : c0 + 16;
            for (int x = c0; x < c1; ++x) {
                ++*loaded;
                if (!cov[(size_t)(x / 240) * rows + y]) ++missing;
            }
        }
    }
    return missing;
}

// BuildPlan::sparse_gradient for a pyramid (geo: L, then T, rows, cols of L levels; every buffer allocated, threshold 90) and
// the inputs given; *form0 = the plan's form of level 0
extern "C" int sbm_emu_sparse_gradient_plan(const int32_t* geo, int sparse_strips, int sparse_gradient, int l0_stream, int l0_mask, int banded,
                                            int one_launch, int match_entry, int32_t* form0)
{
    PlanInputs p;
    p.L = geo[0];
    for (int l = 0; l < p.L; ++l) {
        p.T[l] = geo[1 + l], p.rows[l] = geo[1 + p.L + l], p.cols[l] = geo[1 + 2 * p.L + l];
        p.has_spread[l] = true;
        p.has_bit_strips[l] = l < p.L - 1 && p.T[l] == 4;
    }
    p.has_bit_planes = true;
    p.have_thr = true;
    p.thr = 90.f;
    p.sparse_strips = sparse_strips != 0;
    p.sparse_gradient = sparse_gradient != 0;
    p.l0_stream = l0_stream != 0;
    p.l0_mask = l0_mask != 0;
    p.banded = banded != 0;
    const BuildPlan b = plan_build(p, one_launch != 0, match_entry != 0);
    *form0 = b.form[0];
    return b.sparse_gradient ? 1 : 0;
}
