// TEST INFRASTRUCTURE: shape_based_matching_amd/csrc/sbm_frame_planes_plan.h -- the argument check and the source-pass form rule of
// sbm_match_batch_device_planes -- behind a C interface.  Compiled by tests/test_frame_planes_plan.py into its temporary directory;
// never loaded by the product.
#include "sbm_frame_planes_plan.h"

using namespace sbm;

extern "C" int sbm_emu_frame_planes_check(int have_table, int n_frames, int cols, int stride, int flags)
{
    return frame_planes_check(have_table != 0, n_frames, cols, stride, flags);
}

extern "C" const char* sbm_emu_frame_planes_error(int e) { return frame_planes_error(e); }

extern "C" int sbm_emu_frame_planes_lines(int flags, int64_t stride, int rows, int cols, int knob)
{
    return frame_planes_source_lines(flags, stride, rows, cols, knob != 0) ? 1 : 0;
}

extern "C" int sbm_emu_frame_planes_channels() { return FPL_CHANNELS; }
