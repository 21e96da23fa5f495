// sbm_frame_planes_plan.h — the host rules of the batched match on planar frames (sbm_match_batch_device_planes: the loop of
// Detector::match, line2Dup.cpp:1078, over frames whose three channels are three planes anywhere in device memory, named by a device
// table of 3 * n_frames addresses).  As with the table of frame pointers (sbm_frame_ptrs_plan.h) the host never reads the table: what
// it decides it decides from the call's integers.  The call travels as a FrameSource of kind FRAMES_PLANES (sbm_frame_source.h); its
// masks, if any, are a table of mask addresses as a _ptrs call's are.  Plain integer code, no HIP types: the entry point and
// sbm_frame_source.h call it, tests/test_frame_planes_plan.py compiles it for the CPU suite.
#pragma once
#include <stdint.h>
#include "sbm_frame_ptrs_plan.h"

namespace sbm {

constexpr int FPL_CHANNELS = 3;    // always three planes per frame (a gray planar frame is a frame of sbm_match_batch_device_ptrs)
constexpr int FPL_KNOWN_FLAGS = 0; // `flags` is reserved

// The argument check, in the order the messages are reported.  0: acceptable.  stride: bytes per row of a PLANE.
enum FramePlanesError : int { FPL_OK = 0, FPL_NULL_TABLE = 1, FPL_NO_FRAMES = 2, FPL_UNKNOWN_FLAGS = 3, FPL_SHORT_STRIDE = 4 };

inline int frame_planes_check(bool have_table, int n_frames, int cols, int stride, int flags)
{
    if (!have_table) return FPL_NULL_TABLE;
    if (n_frames < 1) return FPL_NO_FRAMES;
    if (flags & ~FPL_KNOWN_FLAGS) return FPL_UNKNOWN_FLAGS;
    if (stride < cols) return FPL_SHORT_STRIDE;
    return FPL_OK;
}

inline const char* frame_planes_error(int e)
{
    switch (e) {
    case FPL_NULL_TABLE: return "null table of plane pointers";
    case FPL_NO_FRAMES: return "n_frames must be >= 1";
    case FPL_UNKNOWN_FLAGS: return "flags is reserved and must be 0";
    case FPL_SHORT_STRIDE: return "stride < cols (bytes per row of a plane)";
    default: return "";
    }
}

// The source pass of a plane call: always the strided form (QS_SOURCE, plane form).  k_source_lines moves whole lines of
// interleaved pixels and has no plane form, whatever the layout and whatever SBM_SOURCE_LINES says.
inline bool frame_planes_source_lines(int flags, int64_t stride, int rows, int cols, bool knob)
{
    (void)flags, (void)stride, (void)rows, (void)cols, (void)knob;
    return false;
}

} // namespace sbm
