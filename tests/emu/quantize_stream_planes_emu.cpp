// quantize_stream_planes_emu.cpp — TEST INFRASTRUCTURE: the plane forms of the gfx950 gradient kernel
// (shape_based_matching_amd/csrc/sbm_quantize_stream.h, PLANES) compiled for the CPU against tests/emu/wave_emu.h and launched
// the way launch_quantize launches a call of sbm_match_batch_device_planes: QSArgs::img is an array of three plane addresses per
// frame, QSArgs::mask null or an array of mask addresses, the last strip never packed, `stride` the row of a plane.  Beside them
// the interleaved table forms they must agree with.  Built by tests/test_emu_quantize_stream_planes.py into a shared object of its
// own; never loaded by the product.
#define SBM_WAVE_EMU 1
#define SBM_WAVE_HEADER "wave_emu.h"
#include <climits>
#include <cmath>
#include "sbm_quantize_stream.h"
#include "sbm_frame_planes_plan.h"

using namespace sbm;

// stride: bytes per source row (of a plane, or of an interleaved frame)
static bool bad_geometry(int frames, int rows, int cols, int hs, int stride, int row_bytes)
{
    return cols < 4 || (cols & 3) || rows < 1 || hs < 2 || (hs & 1) || frames < 1 || stride < row_bytes;
}

static QSArgs common_args(int frames, int rows, int cols, int hs, int stride, float weak, uint8_t* out, uint8_t* pyr, uint8_t* keep)
{
    constexpr int ch = FPL_CHANNELS;
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

template <int STAGE, bool PLANES>
static void run_stream(const QSArgs& a)
{
    // four items past the last: the idle waves of the last workgroup
    for (int item = 0; item < quantize_stream_items(a) + 4; ++item) quantize_stream_item<3, STAGE, true, PLANES>(a, item);
}

// QS_WHOLE through the plane table: channel c of frame f at plane_ptrs[3 f + c], under the mask at mask_ptrs[f] if mask_ptrs is not null
extern "C" int sbm_emu_planes_whole(const uint8_t* const* plane_ptrs, const uint8_t* const* mask_ptrs, int frames, int rows, int cols, int stride,
                                    float weak, uint8_t* out, uint8_t* pyr, int hs)
{
    if (bad_geometry(frames, rows, cols, hs, stride, cols)) return -1;
    if (frame_planes_check(plane_ptrs != nullptr, frames, cols, stride, 0)) return -3;
    QSArgs a = common_args(frames, rows, cols, hs, stride, weak, out, pyr, nullptr);
    a.img = reinterpret_cast<const uint8_t*>(plane_ptrs);
    a.mask = reinterpret_cast<const uint8_t*>(mask_ptrs);
    run_stream<QS_WHOLE, true>(a);
    return 0;
}

// the source pass through the plane table (the strided form QS_SOURCE: the plan has no other, returns -2 if it ever says otherwise)
extern "C" int sbm_emu_planes_source(const uint8_t* const* plane_ptrs, int frames, int rows, int cols, int stride, uint8_t* pyr, uint8_t* keep, int hs)
{
    if (bad_geometry(frames, rows, cols, hs, stride, cols) || (rows & 1)) return -1;
    if (frame_planes_source_lines(0, stride, rows, cols, true)) return -2;
    QSArgs a = common_args(frames, rows, cols, hs, stride, 0.f, nullptr, pyr, keep);
    a.img = reinterpret_cast<const uint8_t*>(plane_ptrs);
    run_stream<QS_SOURCE, true>(a);
    return 0;
}

// the interleaved table forms (sbm_match_batch_device_ptrs, three channels): frame f at frame_ptrs[f]
extern "C" int sbm_emu_ptrs3_whole(const uint8_t* const* frame_ptrs, const uint8_t* const* mask_ptrs, int frames, int rows, int cols, int stride,
                                   float weak, uint8_t* out, uint8_t* pyr, int hs)
{
    if (bad_geometry(frames, rows, cols, hs, stride, cols * 3)) return -1;
    QSArgs a = common_args(frames, rows, cols, hs, stride, weak, out, pyr, nullptr);
    a.img = reinterpret_cast<const uint8_t*>(frame_ptrs);
    a.mask = reinterpret_cast<const uint8_t*>(mask_ptrs);
    run_stream<QS_WHOLE, false>(a);
    return 0;
}

extern "C" int sbm_emu_ptrs3_source(const uint8_t* const* frame_ptrs, int frames, int rows, int cols, int stride, uint8_t* pyr, uint8_t* keep, int hs)
{
    if (bad_geometry(frames, rows, cols, hs, stride, cols * 3) || (rows & 1)) return -1;
    QSArgs a = common_args(frames, rows, cols, hs, stride, 0.f, nullptr, pyr, keep);
    a.img = reinterpret_cast<const uint8_t*>(frame_ptrs);
    run_stream<QS_SOURCE, false>(a);
    return 0;
}
