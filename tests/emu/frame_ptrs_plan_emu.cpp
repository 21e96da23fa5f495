// TEST INFRASTRUCTURE: shape_based_matching_amd/csrc/sbm_frame_ptrs_plan.h -- the argument check and the source-pass form rule of
// sbm_match_batch_device_ptrs -- behind a C interface, beside the rule of the contiguous layout it must agree with
// (sbm_source_lines_plan.h).  Compiled by tests/test_frame_ptrs_plan.py into its temporary directory; never loaded by the product.
#include "sbm_frame_ptrs_plan.h"

using namespace sbm;

extern "C" int sbm_emu_frame_ptrs_check(int have_table, int n_frames, int cols, int stride, int channels, int flags)
{
    return frame_ptrs_check(have_table != 0, n_frames, cols, stride, channels, flags);
}

extern "C" const char* sbm_emu_frame_ptrs_error(int e) { return frame_ptrs_error(e); }

extern "C" int sbm_emu_frame_ptrs_lines(int flags, int64_t stride, int rows, int cols, int ch, int knob)
{
    return frame_ptrs_source_lines(flags, stride, rows, cols, ch, knob != 0) ? 1 : 0;
}

extern "C" int sbm_emu_source_lines_ok(uint64_t base, int64_t stride, int64_t frame_stride, int frames, int rows, int cols, int ch)
{
    return source_lines_ok(base, stride, frame_stride, frames, rows, cols, ch) ? 1 : 0;
}
