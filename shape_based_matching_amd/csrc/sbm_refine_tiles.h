// sbm_refine_tiles.h — which tiles of a T = 4 level's bit strips (sbm_local_bits.h) the refinement of one coarse candidate
// reads.  A match call whose plan holds level 0 as LM_BIT_STRIPS_SPARSE (sbm_level_forms.h) builds the strips only in the
// tiles that k_mark_refine_tiles flags by this arithmetic.  Plain integer code, no HIP types: the kernels use it on the
// device, tests/test_refine_tiles.py compiles it for the CPU suite.
// Further down: which pixels of the level's orientation map a tile's strip builder loads, and which work items of the streaming
// gradient kernel write them (gradient_item_needed: the sparse gradient pass of sbm_quantize_stream.h, tests/test_sparse_gradient.py).
// Last: the finer record of what the refinement reads -- per band of pixel rows the hull of the needed map columns (refine_need) --
// and the work items of the sparse gradient pass placed by it (gradient_rect_item_needed, tests/test_sparse_rects.py), listed per
// frame for the launch to run from (gradient_rect_list, tests/test_sparse_list.py).
//
// A TILE is one workgroup of build_lm_strip4_allty<true> (sbm_lm_kernels.h): RT_STRIPS strips of 16 cells x RT_ROWS grid
// rows, for all 128 (sub-plane, orientation) planes; tile (tx, ty) of a W x H grid has index ty * ((W + 31) / 32) + tx, the
// workgroup's block number inside its level.
//
// What local_best_bits loads for a feature at pixel (x, y), cell (gx0, gy0) = (x / 4, y / 4), strip s = gx0 / 16:
//     dwords  lm_bits_offset(plane, s, gy0) + r  and  ... + r + H,   r = 0 .. 15
// i.e. rows gy0 .. gy0 + 15 of strips s and s + 1.  The index is flat: a row past H - 1 is row (gy0 + r - H) of the NEXT strip
// (strips s + 1 and s + 2), and a strip past the last one is strip 0, 1, ... of the next plane -- the same tile column as
// that strip of any plane, since a tile holds all planes.  Behind the last plane lies the zero tail, which needs no tile.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBM_RT_HD __host__ __device__ __forceinline__
#else
#define SBM_RT_HD inline
#endif

namespace sbm {

constexpr int RT_STRIPS = 2; // strips of 16 cells per tile
constexpr int RT_ROWS = 32;  // grid rows per tile

SBM_RT_HD int refine_tile_cols(int W) { return (W + 16 * RT_STRIPS - 1) / (16 * RT_STRIPS); }
SBM_RT_HD int refine_tile_rows(int H) { return (H + RT_ROWS - 1) / RT_ROWS; }
SBM_RT_HD int refine_tile_count(int W, int H) { return refine_tile_cols(W) * refine_tile_rows(H); }

// Where the refinement of a candidate looks (similarityLocal's caller, line2Dup.cpp:1234-1262): the candidate's position one
// level down, clamped so that the template and the 16 x 16 search window stay inside the level, and the window's origin.
// cx, cy: Match::x, ::y at the level above; width, height: the template's box at this level.
struct RefineOrigin {
    int x, y;   // the clamped position
    int ox, oy; // pixel offset added to every feature: the window's first cell
};
SBM_RT_HD RefineOrigin refine_origin(int cx, int cy, int width, int height, int rows, int cols, int T)
{
    const int border = 8 * T;
    int x = cx * 2 + 1, y = cy * 2 + 1;
    const int max_x = cols - width - border, max_y = rows - height - border;
    x = x < border ? border : x;
    y = y < border ? border : y;
    x = x > max_x ? max_x : x;
    y = y > max_y ? max_y : y;
    return RefineOrigin{x, y, (x / T - 8) * T, (y / T - 8) * T};
}

// The strips and rows a candidate's patches cover, before wrapping (refine_tiles_for_each wraps):
//   strips s0 .. s1, rows r0 .. r1   the patch rows below H of every in-bounds feature, strips s and s + 1
//   strips s0 + 1 .. s1 + 1, rows 0 .. over   the flat overrun of patches that pass row H - 1 (over < 0: none)
struct RefineTiles {
    int s0, s1, r0, r1, over;
    bool any; // false: no feature of the box can lie inside the level
};
SBM_RT_HD RefineTiles refine_tiles(const RefineOrigin& o, int width, int height, int rows, int cols, int T, int W, int H)
{
    RefineTiles t{0, 0, 0, 0, -1, false};
    // in-bounds features (fx < width, fy < height) land on pixels [ox, ox + width) x [oy, oy + height), cut to the level
    const int x_lo = o.ox > 0 ? o.ox : 0, x_hi = o.ox + width - 1 < cols - 1 ? o.ox + width - 1 : cols - 1;
    const int y_lo = o.oy > 0 ? o.oy : 0, y_hi = o.oy + height - 1 < rows - 1 ? o.oy + height - 1 : rows - 1;
    if (x_lo > x_hi || y_lo > y_hi) return t;
    t.any = true;
    if (H < 16) { // a patch is longer than a strip: everything
        t.s1 = (W >> 4) - 1;
        t.r1 = H - 1;
        return t;
    }
    const int gy_hi = y_hi / T + 15;
    t.s0 = (x_lo / T) >> 4;
    t.s1 = ((x_hi / T) >> 4) + 1;
    t.r0 = y_lo / T;
    t.r1 = gy_hi < H - 1 ? gy_hi : H - 1;
    t.over = gy_hi >= H ? gy_hi - H : -1;
    return t;
}

// mark(tile index) for every tile of the footprint; a tile may be named more than once
template <class F>
SBM_RT_HD void refine_tiles_for_each(const RefineTiles& t, int W, int H, F mark)
{
    if (!t.any) return;
    (void)H;
    const int ns = W >> 4, n_cb = refine_tile_cols(W);
    for (int s = t.s0; s <= t.s1; ++s)
        for (int ty = t.r0 / RT_ROWS; ty <= t.r1 / RT_ROWS; ++ty) mark(ty * n_cb + (s % ns) / RT_STRIPS);
    if (t.over >= 0)
        for (int s = t.s0 + 1; s <= t.s1 + 1; ++s)
            for (int ty = 0; ty <= t.over / RT_ROWS; ++ty) mark(ty * n_cb + (s % ns) / RT_STRIPS);
}

// ---- which pixels of the level's orientation map a tile's strip builder loads, and which gradient work items make them ----
// The workgroup of tile (tx, ty) of build_lm_strip4_allty<true> (T = 4, W a multiple of 16): thread (row, kk) owns the 4 cells
// k = tx * 8 + kk of grid row gy = ty * RT_ROWS + row (gy < H) and loads, of the map, pixel rows gy * T .. gy * T + 2T - 2 that lie
// below `rows`, columns k * 4T .. k * 4T + 4T - 1 and -- short of the last column -- the T pixels to their right (the spread's
// reach).  Over the workgroup that is one rectangle [x0, x1) x [y0, y1):
struct PixelRect {
    int x0, y0, x1, y1;
};
SBM_RT_HD PixelRect refine_tile_pixels(int tx, int ty, int rows, int cols, int T, int W, int H)
{
    const int cells = 16 * RT_STRIPS;
    const int gx1 = (tx + 1) * cells < W ? (tx + 1) * cells : W, gy1 = (ty + 1) * RT_ROWS < H ? (ty + 1) * RT_ROWS : H;
    const int x1 = gx1 * T + T, y1 = gy1 * T + T - 1; // right halo; the last grid row's window of 2T - 1 rows
    return PixelRect{tx * cells * T, ty * RT_ROWS * T, x1 < cols ? x1 : cols, y1 < rows ? y1 : rows};
}

// some flagged tile's builder loads a pixel of [x0, x1) x [y0, y1).  flags: one byte per tile of one frame.
SBM_RT_HD bool refine_rect_needed(const uint8_t* flags, int x0, int y0, int x1, int y1, int rows, int cols, int T, int W, int H)
{
    const int n_cb = refine_tile_cols(W), n_rb = refine_tile_rows(H), tw = 16 * RT_STRIPS * T, th = RT_ROWS * T;
    if (x0 >= x1 || y0 >= y1) return false;
    // the first tile column / row whose rectangle can reach x0 / y0 (it ends T, T - 1 pixels past the tile), the last that starts before x1 / y1
    const int tx_lo = x0 >= T ? (x0 - T) / tw : 0, ty_lo = y0 >= T - 1 ? (y0 - (T - 1)) / th : 0;
    const int tx_hi = (x1 - 1) / tw < n_cb - 1 ? (x1 - 1) / tw : n_cb - 1, ty_hi = (y1 - 1) / th < n_rb - 1 ? (y1 - 1) / th : n_rb - 1;
    for (int ty = ty_lo; ty <= ty_hi; ++ty)
        for (int tx = tx_lo; tx <= tx_hi; ++tx) {
            if (!flags[ty * n_cb + tx]) continue;
            const PixelRect r = refine_tile_pixels(tx, ty, rows, cols, T, W, H);
            if (r.x0 < x1 && x0 < r.x1 && r.y0 < y1 && y0 < r.y1) return true;
        }
    return false;
}

// Output rows [*r0, *r1) of row block rb of a whole-level launch of the streaming gradient kernel with hs rows per work item
// (sbm_quantize_stream.h: the last block is moved up to end at the last row)
SBM_RT_HD void gradient_item_rows(int rb, int hs, int rows, int* r0, int* r1)
{
    int a = rb * hs;
    if (a + hs > rows) a = rows > hs ? rows - hs : 0;
    *r0 = a;
    *r1 = a + hs < rows ? a + hs : rows;
}

// The gradient work item (strip, rb) -- `useful` output columns per strip, hs rows per item -- writes a pixel that the strip
// builder of a flagged tile loads.  The kernel and tests/test_sparse_gradient.py share this function.
SBM_RT_HD bool gradient_item_needed(const uint8_t* flags, int strip, int rb, int hs, int useful, int rows, int cols, int T, int W, int H)
{
    int r0, r1;
    gradient_item_rows(rb, hs, rows, &r0, &r1);
    const int x0 = strip * useful, x1 = x0 + useful < cols ? x0 + useful : cols;
    return refine_rect_needed(flags, x0, r0, x1, r1, rows, cols, T, W, H);
}

// ---- the finer record: per band of RT_BAND pixel rows, the hull of the map columns some candidate's refinement depends on ----
// Of the two dwords local_best_bits loads per patch row, a response is formed from the 16 cells gx0 .. gx0 + 15 only (the pair is
// shifted right by gx0 & 15 and cut to 16 bits), in grid rows gy0 .. gy0 + 15: the other cells of strips s and s + 1 are loaded and
// dropped.  Over a candidate's in-bounds features that is the CELL rectangle [x_lo / T, x_hi / T + 15] x [y_lo / T, y_hi / T + 15],
// where refine_tiles works at strip precision.  Cell (gx, gy) -- all T * T sub-planes of it -- is spread from the map pixels
// [gx T, gx T + 2T - 2] x [gy T, gy T + 2T - 2] (pixel p of the response plane ORs the pixels p .. p + T - 1).
// The record: int32 pairs {xmin, xmax} per band and frame, columns [xmin, xmax), empty when xmin >= xmax (cleared to
// {INT32_MAX, 0}; a zeroed record is empty too).  The wrap cases of the flat index (a patch that passes row H - 1, a strip index past
// the last strip), H < 16 and a grid of cut strips keep the strip-precise footprint of refine_tiles: a superset is always correct.
constexpr int RT_BAND = 8; // pixel rows per band
SBM_RT_HD int refine_band_count(int rows) { return (rows + RT_BAND - 1) / RT_BAND; }

struct BandRect {
    int b0, b1, x0, x1; // bands b0 .. b1 (none when b1 < b0), columns [x0, x1)
};
// the map pixels the cells [gx0, gx1] x [gy0, gy1] are spread from, as bands and columns
SBM_RT_HD BandRect refine_cells_bands(int gx0, int gx1, int gy0, int gy1, int rows, int cols, int T)
{
    const int x1 = gx1 * T + 2 * T - 1, y1 = gy1 * T + 2 * T - 2;
    return BandRect{gy0 * T / RT_BAND, (y1 < rows - 1 ? y1 : rows - 1) / RT_BAND, gx0 * T, x1 < cols ? x1 : cols};
}
struct RefineNeed {
    BandRect r[2]; // r[1]: the flat overrun of a wrap case, else none
};
SBM_RT_HD RefineNeed refine_need(const RefineOrigin& o, int width, int height, int rows, int cols, int T, int W, int H)
{
    RefineNeed n{{{0, -1, 0, 0}, {0, -1, 0, 0}}};
    const RefineTiles t = refine_tiles(o, width, height, rows, cols, T, W, H);
    if (!t.any) return n;
    const int ns = W >> 4;
    if (H >= 16 && t.over < 0 && t.s1 < ns && (W & 15) == 0) { // no wrap: cell precision
        const int x_lo = o.ox > 0 ? o.ox : 0, x_hi = o.ox + width - 1 < cols - 1 ? o.ox + width - 1 : cols - 1;
        n.r[0] = refine_cells_bands(x_lo / T, x_hi / T + 15, t.r0, t.r1, rows, cols, T);
        return n;
    }
    // strips s0 .. s1, rows r0 .. r1; a strip index that wraps may be any strip of the row: every column
    const bool all0 = t.s1 >= ns || (W & 15) != 0 || H < 16;
    n.r[0] = refine_cells_bands(all0 ? 0 : t.s0 * 16, all0 ? W - 1 : t.s1 * 16 + 15, t.r0, t.r1, rows, cols, T);
    if (all0) n.r[0].x1 = cols;
    if (t.over >= 0) { // strips s0 + 1 .. s1 + 1, rows 0 .. over
        const bool all1 = all0 || t.s1 + 1 >= ns;
        n.r[1] = refine_cells_bands(all1 ? 0 : (t.s0 + 1) * 16, all1 ? W - 1 : (t.s1 + 1) * 16 + 15, 0, t.over, rows, cols, T);
        if (all1) n.r[1].x1 = cols;
    }
    return n;
}

// The hull [*xa, *xb) of the bands that the pixel rows [r0, r1) meet; false: all of them are empty.  iv: one frame's record.
SBM_RT_HD bool refine_rows_hull(const int32_t* iv, int r0, int r1, int* xa, int* xb)
{
    int a = 0x7fffffff, b = 0;
    for (int band = r0 / RT_BAND; band <= (r1 - 1) / RT_BAND; ++band) {
        const int lo = iv[2 * band], hi = iv[2 * band + 1];
        if (lo >= hi) continue;
        a = lo < a ? lo : a;
        b = hi > b ? hi : b;
    }
    *xa = a & ~3; // a lane of the gradient kernel holds 4 pixels: 12 source bytes, dword-aligned only at a multiple of 4
    *xb = b;
    return a < b;
}

// The rect-driven item (k, rb) of the sparse gradient pass: its strip of `useful` columns starts at *x0 = xa + useful * k, xa the
// left end of the hull of its rows, and it works when the strip begins left of the hull's right end AND some flagged tile's
// builder loads a pixel of its rectangle (the tile-driven test on the moved strip: two distant objects in the same rows leave
// the strips between them out, as the tile flags do).  The kernel and tests/test_sparse_rects.py share this function.
SBM_RT_HD bool gradient_rect_item_needed(const int32_t* iv, const uint8_t* flags, int k, int rb, int hs, int useful, int rows, int cols, int T,
                                         int W, int H, int* x0)
{
    int r0, r1, xa, xb;
    gradient_item_rows(rb, hs, rows, &r0, &r1);
    *x0 = 0;
    if (!refine_rows_hull(iv, r0, r1, &xa, &xb)) return false;
    const int s0 = xa + k * useful, s1 = s0 + useful < cols ? s0 + useful : cols;
    *x0 = s0;
    if (s0 >= xb) return false;
    return refine_rect_needed(flags, s0, r0, s1, r1, rows, cols, T, W, H);
}

// ---- the list of working items: what k_mark_refine_tiles leaves for the sparse gradient launch beside flags and hulls ----
// The rect-driven items (k, rb) of one frame that get a wave of their own -- k < n_full strips (a packed last strip is not among
// them), rb < n_rblocks -- tested once, where the hulls and the flags are made, instead of by every wave of the launch.
// One frame's list: RT_LIST_HEAD int32, the first of them the count, then RT_LIST_ENTRY int32 per working item {k, rb, x_first, 0},
// in any order.  Count RT_LIST_NONE: there is no list, every wave tests its own items.
constexpr int RT_LIST_HEAD = 4, RT_LIST_ENTRY = 4; // (entries are 16 bytes, 16-byte aligned: one load each)
constexpr int RT_LIST_NONE = -1;
// entries a frame's list has room for whatever the rows per item (even, >= 2) of the call that fills it
SBM_RT_HD int64_t refine_list_capacity(int rows, int cols, int useful) { return (int64_t)((cols + useful - 1) / useful) * ((rows + 1) / 2); }
SBM_RT_HD int64_t refine_list_stride(int64_t capacity) { return RT_LIST_HEAD + RT_LIST_ENTRY * capacity; }

// Items first, first + step, ... of the n_full * n_rblocks of a frame (item i: strip i % n_full of row block i / n_full):
// append(k, rb, x_first) for each that works.  The kernel runs it with a thread per `first` and an atomic counter behind
// `append`, tests/test_sparse_list.py with first = 0, step = 1.
template <class F>
SBM_RT_HD void gradient_rect_list(const int32_t* iv, const uint8_t* flags, int n_full, int n_rblocks, int hs, int useful, int rows, int cols,
                                  int T, int W, int H, int first, int step, F append)
{
    const int n_items = n_full * n_rblocks;
    for (int i = first; i < n_items; i += step) {
        const int rb = i / n_full, k = i - rb * n_full;
        int x0;
        if (gradient_rect_item_needed(iv, flags, k, rb, hs, useful, rows, cols, T, W, H, &x0)) append(k, rb, x0);
    }
}

} // namespace sbm
