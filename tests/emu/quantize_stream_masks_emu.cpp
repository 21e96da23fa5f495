// quantize_stream_masks_emu.cpp — TEST INFRASTRUCTURE: the SOURCE of the gfx950 row-streaming gradient kernel
// (shape_based_matching_amd/csrc/sbm_quantize_stream.h) compiled for the CPU against tests/emu/wave_emu.h, launched
// the way the engine launches a batch whose frames each bring their own mask (QSArgs::mask_fs).  Built by
// tests/test_emu_quantize_stream_masks.py into a shared object of its own; never loaded by the product.
#define SBM_WAVE_EMU 1
#define SBM_WAVE_HEADER "wave_emu.h"
#include <climits>
#include <cmath>
#include "sbm_quantize_stream.h"

// `frames` contiguous frames, frame f under the mask at masks + f * mask_fs (mask_fs = 0: one shared mask).  With
// pack != 0 the last strip of up to 64 / pack_lanes frames shares a wave (quantize_stream_pack_lanes decides, as on the
// GPU, from the geometry AND the mask stride).  Returns the segment lanes of the packed strip (0: not packed), < 0: bad
// arguments.
extern "C" int sbm_emu_quantize_stream_frame_masks(const uint8_t* img, int frames, int rows, int cols, int stride, int ch, const uint8_t* masks,
                                                   int64_t mask_fs, float weak, uint8_t* out, uint8_t* pyr, int hs, int pack)
{
    if ((ch != 1 && ch != 3) || cols < 4 || (cols & 3) || rows < 1 || hs < 2 || (hs & 1) || frames < 1) return -1;
    if (mask_fs && (!masks || mask_fs < (int64_t)rows * cols)) return -1;
    sbm::QSArgs a{};
    a.img = img;
    a.mask = masks;
    a.out = out;
    a.pyr = pyr;
    a.img_fs = (int64_t)rows * stride;
    a.out_fs = (int64_t)rows * cols;
    a.pyr_fs = (int64_t)(rows / 2) * (cols / 2) * ch;
    a.mask_fs = mask_fs;
    a.rows = rows;
    a.cols = cols;
    a.stride = stride;
    const float thr_sq = weak * weak;
    a.thr_i = thr_sq < 2147483000.f ? (int)floorf(thr_sq) : INT_MAX;
    a.hs = hs;
    a.row_lo = 0;
    a.row_hi = rows;
    a.n_strips = (cols + sbm::QS_USEFUL - 1) / sbm::QS_USEFUL;
    a.n_rblocks = (rows + hs - 1) / hs;
    a.frames = frames;
    a.pack_lanes = pack ? sbm::quantize_stream_pack_lanes(rows, cols, ch, frames, mask_fs) : 0;
    a.pack_groups = a.pack_lanes ? (frames + 64 / a.pack_lanes - 1) / (64 / a.pack_lanes) : 0;
    for (int item = 0; item < sbm::quantize_stream_items(a); ++item) {
        if (ch == 3) sbm::quantize_stream_item<3>(a, item);
        else sbm::quantize_stream_item<1>(a, item);
    }
    return a.pack_lanes;
}

// what quantize_stream_pack_lanes answers for a geometry and a mask stride (the 32-bit per-lane offset rule)
extern "C" int sbm_emu_pack_lanes(int rows, int cols, int ch, int frames, int64_t mask_fs)
{
    return sbm::quantize_stream_pack_lanes(rows, cols, ch, frames, mask_fs);
}
