// TEST INFRASTRUCTURE: the record of need rectangles (sbm_refine_tiles.h: refine_need, gradient_rect_item_needed) and the sparse
// form of the row-streaming gradient kernel that takes its work items from it (sbm_quantize_stream.h, QS_SPARSE with
// QSArgs::need_rects), compiled for the CPU against wave_emu.h behind a C interface.  Compiled by tests/test_sparse_rects.py into
// its temporary directory; never loaded by the product.
#define SBM_WAVE_EMU 1
#define SBM_WAVE_HEADER "wave_emu.h"
#include <climits>
#include <cmath>
#include <vector>

#include "sbm_quantize_stream.h"

using namespace sbm;

// What k_mark_refine_tiles leaves for one frame: cand = n x (cx, cy, declared width, declared height, feature extent x, feature
// extent y) -- the clamps use the declared box, the footprint the features' own.  flags: n_tiles bytes, zeroed here;
// rects: refine_band_count(rows) {xmin, xmax} pairs, emptied here.  origin (may be null): n x (x, y, ox, oy).
// Returns the number of tile marks that fell outside the grid (0 is right).
extern "C" int sbm_emu_mark(int64_t n, const int32_t* cand, int rows, int cols, int T, int W, int H, uint8_t* flags, int32_t* rects, int32_t* origin)
{
    const int n_tiles = refine_tile_count(W, H), n_bands = refine_band_count(rows);
    for (int i = 0; i < n_tiles; ++i) flags[i] = 0;
    for (int b = 0; b < n_bands; ++b) rects[2 * b] = INT_MAX, rects[2 * b + 1] = 0;
    int outside = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t* c = cand + 6 * i;
        const RefineOrigin o = refine_origin(c[0], c[1], c[2], c[3], rows, cols, T);
        if (origin) origin[4 * i] = o.x, origin[4 * i + 1] = o.y, origin[4 * i + 2] = o.ox, origin[4 * i + 3] = o.oy;
        refine_tiles_for_each(refine_tiles(o, c[4], c[5], rows, cols, T, W, H), W, H, [&](int tile) {
            if (tile < 0 || tile >= n_tiles) ++outside;
            else flags[tile] = 1;
        });
        const RefineNeed need = refine_need(o, c[4], c[5], rows, cols, T, W, H);
        for (int q = 0; q < 2; ++q)
            for (int b = need.r[q].b0; b <= need.r[q].b1; ++b) {
                if (b < 0 || b >= n_bands) {
                    ++outside;
                    continue;
                }
                if (need.r[q].x0 < rects[2 * b]) rects[2 * b] = need.r[q].x0;
                if (need.r[q].x1 > rects[2 * b + 1]) rects[2 * b + 1] = need.r[q].x1;
            }
    }
    return outside;
}

// The work items of one frame's sparse launch with hs rows per item.  items (may be null): per (row block, k) the strip's first
// column where the item works, else -1, ceil(cols / 240) entries per row block; rects null: the tile-driven items of the fixed grid.
// Returns the number of working items.
extern "C" int sbm_emu_items(const int32_t* rects, const uint8_t* flags, int rows, int cols, int hs, int T, int W, int H, int32_t* items)
{
    const int n_strips = (cols + QS_USEFUL - 1) / QS_USEFUL, n_rblocks = (rows + hs - 1) / hs;
    int n = 0;
    for (int rb = 0; rb < n_rblocks; ++rb)
        for (int k = 0; k < n_strips; ++k) {
            int x0 = k * QS_USEFUL;
            const bool need = rects ? gradient_rect_item_needed(rects, flags, k, rb, hs, QS_USEFUL, rows, cols, T, W, H, &x0)
                                    : gradient_item_needed(flags, k, rb, hs, QS_USEFUL, rows, cols, T, W, H);
            if (items) items[rb * n_strips + k] = need ? x0 : -1;
            n += need;
        }
    return n;
}

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

// the whole row loop over the packed frames: the map every form must reproduce where it writes
extern "C" int sbm_emu_whole_map(const uint8_t* img, int frames, int rows, int cols, int ch, float weak, int hs, uint8_t* out)
{
    if (bad_geometry(frames, rows, cols, ch, hs)) return -1;
    QSArgs a = batch_args(img, frames, rows, cols, ch, weak, hs, 1);
    a.out = out;
    for (int item = 0; item < quantize_stream_items(a); ++item) {
        if (ch == 3) quantize_stream_item<3>(a, item);
        else quantize_stream_item<1>(a, item);
    }
    return 0;
}

// The sparse pass as the host launches it (a narrow last strip packed, several frames per wave).  flags: frames x n_tiles;
// rects: frames x n_bands pairs, or null = the tile-driven launch.  `out` lies inside a larger buffer of the caller's, whose guard bytes it checks itself.
// Returns the working items (counted as under profiling), or -1.
extern "C" int sbm_emu_sparse_rect_pass(const uint8_t* keep, int frames, int rows, int cols, int ch, float weak, int hs, const uint8_t* flags,
                                        const int32_t* rects, int T, int W, int H, uint8_t* out)
{
    if (bad_geometry(frames, rows, cols, ch, hs)) return -1;
    QSArgs a = batch_args(keep, frames, rows, cols, ch, weak, hs, 1);
    a.out = out;
    a.tile_flags = flags;
    a.n_tiles = refine_tile_count(W, H);
    a.grid_t = T;
    a.grid_w = W;
    a.grid_h = H;
    a.need_rects = rects;
    a.n_bands = refine_band_count(rows);
    int32_t count = 0;
    a.item_count = &count;
    for (int item = 0; item < quantize_stream_items(a); ++item) {
        if (ch == 3) quantize_stream_item<3, QS_SPARSE>(a, item);
        else quantize_stream_item<1, QS_SPARSE>(a, item);
    }
    return count;
}
