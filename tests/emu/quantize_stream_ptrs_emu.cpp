// quantize_stream_ptrs_emu.cpp — TEST INFRASTRUCTURE: the table forms of the gfx950 gradient kernels
// (shape_based_matching_amd/csrc/sbm_quantize_stream.h and sbm_source_lines.h, PTRS) compiled for the CPU against
// tests/emu/wave_emu.h and launched the way launch_quantize launches a call of sbm_match_batch_device_ptrs: QSArgs::img is an
// array of frame addresses, QSArgs::mask null or an array of mask addresses, the last strip never packed.  Beside them the
// contiguous forms on one block of frames.  Built by tests/test_emu_quantize_stream_ptrs.py
// into a shared object of its own; never loaded by the product.
#define SBM_WAVE_EMU 1
#define SBM_WAVE_HEADER "wave_emu.h"
#include <climits>
#include <cmath>
#include "sbm_source_lines.h"
#include "sbm_frame_ptrs_plan.h"

using namespace sbm;

static bool bad_geometry(int frames, int rows, int cols, int ch, int hs, int stride)
{
    return (ch != 1 && ch != 3) || cols < 4 || (cols & 3) || rows < 1 || hs < 2 || (hs & 1) || frames < 1 || stride < cols * ch;
}

// what both layouts share; img / mask / img_fs / mask_fs / pack_lanes are the caller's
static QSArgs common_args(int frames, int rows, int cols, int ch, int hs, int stride, float weak, uint8_t* out, uint8_t* pyr, uint8_t* keep)
{
    QSArgs a{};
    a.out = out;
    a.pyr = pyr;
    a.keep = keep;
    a.out_fs = (int64_t)rows * cols;
    a.pyr_fs = (int64_t)(rows / 2) * (cols / 2) * ch;
    a.keep_fs = (int64_t)rows * cols * ch;
    a.rows = rows;
    a.cols = cols;
    a.stride = stride;
    const float thr_sq = weak * weak;
    a.thr_i = thr_sq < 2147483000.f ? (int)floorf(thr_sq) : INT_MAX;
    a.hs = hs;
    a.row_lo = 0;
    a.row_hi = rows;
    a.n_strips = (cols + QS_USEFUL - 1) / QS_USEFUL;
    a.n_rblocks = (rows + hs - 1) / hs;
    a.frames = frames;
    return a;
}

template <int STAGE, bool PTRS>
static void run_stream(const QSArgs& a, int ch)
{
    // four items past the last: the idle waves of the last workgroup
    for (int item = 0; item < quantize_stream_items(a) + 4; ++item) {
        if (ch == 3) quantize_stream_item<3, STAGE, PTRS>(a, item);
        else quantize_stream_item<1, STAGE, PTRS>(a, item);
    }
}

// QS_WHOLE through the tables: frame f at frame_ptrs[f], under the mask at mask_ptrs[f] if mask_ptrs is not null
extern "C" int sbm_emu_ptrs_whole(const uint8_t* const* frame_ptrs, const uint8_t* const* mask_ptrs, int frames, int rows, int cols, int stride, int ch,
                                  float weak, uint8_t* out, uint8_t* pyr, int hs)
{
    if (bad_geometry(frames, rows, cols, ch, hs, stride)) return -1;
    QSArgs a = common_args(frames, rows, cols, ch, hs, stride, weak, out, pyr, nullptr);
    a.img = reinterpret_cast<const uint8_t*>(frame_ptrs);
    a.mask = reinterpret_cast<const uint8_t*>(mask_ptrs);
    run_stream<QS_WHOLE, true>(a, ch);
    return 0;
}

// QS_WHOLE on one block of frames (mask_fs = 0: no mask or one shared), the last strip packed where the geometry packs it;
// returns the segment lanes of the packed strip
extern "C" int sbm_emu_block_whole(const uint8_t* img, int64_t img_fs, const uint8_t* masks, int64_t mask_fs, int frames, int rows, int cols, int stride,
                                   int ch, float weak, uint8_t* out, uint8_t* pyr, int hs)
{
    if (bad_geometry(frames, rows, cols, ch, hs, stride)) return -1;
    QSArgs a = common_args(frames, rows, cols, ch, hs, stride, weak, out, pyr, nullptr);
    a.img = img;
    a.img_fs = img_fs;
    a.mask = masks;
    a.mask_fs = masks ? mask_fs : 0;
    a.pack_lanes = quantize_stream_pack_lanes(rows, cols, ch, frames, a.mask_fs);
    a.pack_groups = a.pack_lanes ? (frames + 64 / a.pack_lanes - 1) / (64 / a.pack_lanes) : 0;
    run_stream<QS_WHOLE, false>(a, ch);
    return a.pack_lanes;
}

// the source pass through the table: lines != 0 the line form (-2 where the plan's rule, with the flag set, does not admit the
// layout or a pointer breaks the promise), else the strided form QS_SOURCE
extern "C" int sbm_emu_ptrs_source(const uint8_t* const* frame_ptrs, int frames, int rows, int cols, int stride, int ch, uint8_t* pyr, uint8_t* keep,
                                   int hs, int lines)
{
    if (bad_geometry(frames, rows, cols, ch, hs, stride) || (rows & 1)) return -1;
    QSArgs a = common_args(frames, rows, cols, ch, hs, stride, 0.f, nullptr, pyr, keep);
    a.img = reinterpret_cast<const uint8_t*>(frame_ptrs);
    if (!lines) {
        run_stream<QS_SOURCE, true>(a, ch);
        return 0;
    }
    if (!frame_ptrs_source_lines(FP_ALIGNED4, stride, rows, cols, ch, true)) return -2;
    for (int f = 0; f < frames; ++f)
        if ((uintptr_t)frame_ptrs[f] & 3) return -2;
    const int n = sl_items(cols, a.n_rblocks, frames);
    for (int item = 0; item < n + 4; ++item) {
        if (ch == 3) source_lines_item<3, true>(a, item);
        else source_lines_item<1, true>(a, item);
    }
    return n;
}

// the source pass on one block of frames, strided form (packed where the geometry packs) or line form (-2: not admitted)
extern "C" int sbm_emu_block_source(const uint8_t* img, int64_t img_fs, int frames, int rows, int cols, int stride, int ch, uint8_t* pyr, uint8_t* keep,
                                    int hs, int lines)
{
    if (bad_geometry(frames, rows, cols, ch, hs, stride) || (rows & 1)) return -1;
    QSArgs a = common_args(frames, rows, cols, ch, hs, stride, 0.f, nullptr, pyr, keep);
    a.img = img;
    a.img_fs = img_fs;
    if (!lines) {
        a.pack_lanes = quantize_stream_pack_lanes(rows, cols, ch, frames);
        a.pack_groups = a.pack_lanes ? (frames + 64 / a.pack_lanes - 1) / (64 / a.pack_lanes) : 0;
        run_stream<QS_SOURCE, false>(a, ch);
        return 0;
    }
    if (!source_lines_ok((uint64_t)(uintptr_t)img, stride, img_fs, frames, rows, cols, ch)) return -2;
    const int n = sl_items(cols, a.n_rblocks, frames);
    for (int item = 0; item < n + 4; ++item) {
        if (ch == 3) source_lines_item<3>(a, item);
        else source_lines_item<1>(a, item);
    }
    return n;
}
