// TEST INFRASTRUCTURE: the two forms of the source pass -- the present one (sbm_quantize_stream.h, QS_SOURCE) and the line-shaped
// one (sbm_source_lines.h) -- compiled for the CPU against wave_emu.h, and the plan header of the second
// (sbm_source_lines_plan.h: the selection rule and a walk of its index arithmetic), behind a C interface.  Compiled by
// tests/test_source_pass.py into its temporary directory; never loaded by the product.
#define SBM_WAVE_EMU 1
#define SBM_WAVE_HEADER "wave_emu.h"
#include "sbm_source_lines.h"

using namespace sbm;

static bool bad_geometry(int frames, int rows, int cols, int ch, int hs, int stride, int64_t img_fs)
{
    return (ch != 1 && ch != 3) || cols < 4 || (cols & 3) || rows < 2 || (rows & 1) || hs < 2 || (hs & 1) || frames < 1 || stride < cols * ch ||
           img_fs < (int64_t)rows * stride;
}

static QSArgs source_args(const uint8_t* img, int frames, int rows, int cols, int ch, int hs, int stride, int64_t img_fs, uint8_t* pyr, uint8_t* keep)
{
    QSArgs a{};
    a.img = img;
    a.img_fs = img_fs;
    a.pyr = pyr;
    a.pyr_fs = (int64_t)(rows / 2) * (cols / 2) * ch;
    a.keep = keep;
    a.keep_fs = (int64_t)rows * cols * ch;
    a.rows = rows;
    a.cols = cols;
    a.stride = stride;
    a.hs = hs;
    a.row_lo = 0;
    a.row_hi = rows;
    a.n_strips = (cols + QS_USEFUL - 1) / QS_USEFUL;
    a.n_rblocks = (rows + hs - 1) / hs;
    a.frames = frames;
    return a;
}

// the present form over `frames` frames in the caller's layout: pyr = the next level's images, keep = the retained copy, packed
extern "C" int sbm_emu_source_present(const uint8_t* img, int frames, int rows, int cols, int ch, int hs, int pack, int stride, int64_t img_fs,
                                      uint8_t* pyr, uint8_t* keep)
{
    if (bad_geometry(frames, rows, cols, ch, hs, stride, img_fs)) return -1;
    QSArgs a = source_args(img, frames, rows, cols, ch, hs, stride, img_fs, pyr, keep);
    a.pack_lanes = pack ? quantize_stream_pack_lanes(rows, cols, ch, frames) : 0;
    a.pack_groups = a.pack_lanes ? (frames + 64 / a.pack_lanes - 1) / (64 / a.pack_lanes) : 0;
    for (int item = 0; item < quantize_stream_items(a); ++item) {
        if (ch == 3) quantize_stream_item<3, QS_SOURCE>(a, item);
        else quantize_stream_item<1, QS_SOURCE>(a, item);
    }
    return 0;
}

// the line form, where the selection rule admits the layout (-2 where it does not); returns its number of work items.  Four
// items past the last are run too: the last workgroup's idle waves
extern "C" int sbm_emu_source_lines(const uint8_t* img, int frames, int rows, int cols, int ch, int hs, int stride, int64_t img_fs, uint8_t* pyr,
                                    uint8_t* keep)
{
    if (bad_geometry(frames, rows, cols, ch, hs, stride, img_fs)) return -1;
    if (!source_lines_ok((uint64_t)(uintptr_t)img, stride, img_fs, frames, rows, cols, ch)) return -2;
    QSArgs a = source_args(img, frames, rows, cols, ch, hs, stride, img_fs, pyr, keep);
    const int n = sl_items(cols, a.n_rblocks, frames);
    for (int item = 0; item < n + 4; ++item) {
        if (ch == 3) source_lines_item<3>(a, item);
        else source_lines_item<1>(a, item);
    }
    return n;
}

extern "C" int sbm_emu_source_lines_ok(uint64_t base, int64_t stride, int64_t frame_stride, int frames, int rows, int cols, int ch)
{
    return source_lines_ok(base, stride, frame_stride, frames, rows, cols, ch) ? 1 : 0;
}

// A walk of the plan header alone: every work item of a launch (rows [0, rows), hs rows per item), every lane, every owned row.
// copy_cnt (frames x rows x cols x ch) and pyr_cnt (frames x rows/2 x cols/2 x ch) count the writes per byte.  Returns the
// number of violations: a write outside a row's bytes, an offset off a dword boundary, an item whose loaded rows do not cover
// the 5-row window of a cv::pyrDown row it owns, an edge load that leaves the row or does not abut the strip.
extern "C" int64_t sbm_emu_source_lines_walk(int frames, int rows, int cols, int ch, int hs, int32_t* copy_cnt, int32_t* pyr_cnt)
{
    int64_t bad = 0;
    const int n_strips = sl_strips(cols), n_rb = sl_row_blocks(0, rows, hs), n = sl_items(cols, n_rb, frames);
    const int64_t row_bytes = (int64_t)cols * ch, drow_bytes = (int64_t)(cols / 2) * ch;
    const int drows = rows / 2;
    for (int item = 0; item < n; ++item) {
        const SlItem it = sl_item(item, n_strips, frames);
        if (it.strip < 0 || it.strip >= n_strips || it.rb < 0 || it.rb >= n_rb || it.frame < 0 || it.frame >= frames) {
            ++bad;
            continue;
        }
        const SlRows rr = sl_rows(it.rb, hs, 0, rows);
        if (rr.r0 < 0 || rr.r1 > rows || rr.own0 < rr.r0 || rr.own0 >= rr.r1 || (rr.r0 & 1) || (rr.own0 & 1) || rr.r1 - rr.r0 != (hs < rows ? hs : rows)) ++bad;
        const int64_t el = sl_edge_left(it.strip, ch), er = sl_edge_right(it.strip, cols, ch);
        if ((el < 0) != (it.strip == 0) || (er < 0) != (it.strip == n_strips - 1)) ++bad;
        if (el >= 0 && (el + sl_edge_bytes(ch) != (int64_t)it.strip * SL_STRIP * ch || (el & 3))) ++bad;
        if (er >= 0 && (er != (int64_t)(it.strip + 1) * SL_STRIP * ch || er + sl_edge_bytes(ch) > row_bytes || (er & 3))) ++bad;
        for (int lane = 0; lane < 64; ++lane) {
            const int64_t off = sl_row_off(it.strip, lane, cols, ch), poff = sl_pyr_off(it.strip, lane, cols, ch);
            if (off >= 0) {
                if ((off & 3) || off + 4 * ch > row_bytes) {
                    ++bad;
                    continue;
                }
                for (int y = rr.own0; y < rr.r1; ++y)
                    for (int b = 0; b < 4 * ch; ++b) ++copy_cnt[((int64_t)it.frame * rows + y) * row_bytes + off + b];
            }
            if (poff >= 0) {
                if ((poff & 3) || poff + 4 * ch > drow_bytes) {
                    ++bad;
                    continue;
                }
                for (int oy = rr.own0 / 2; oy < rr.r1 / 2 && oy < drows; ++oy) {
                    // the window's rows inside the image must be among the loaded rows r0 - 2 .. r1
                    for (int t = -2; t <= 2; ++t) {
                        const int y = 2 * oy + t;
                        if (y >= 0 && y < rows && (y < rr.r0 - 2 || y > rr.r1)) ++bad;
                    }
                    for (int b = 0; b < 4 * ch; ++b) ++pyr_cnt[((int64_t)it.frame * drows + oy) * drow_bytes + poff + b];
                }
            }
        }
    }
    return bad;
}
