// sbm_frame_ptrs_plan.h — the host rules of the batched match from a device table of frame pointers
// (sbm_match_batch_device_ptrs: the loop of Detector::match, line2Dup.cpp:1078, over frames that lie anywhere in device memory).
// The host never reads the table, so everything it decides it decides from the call's integers: whether the arguments are
// acceptable, and which form of the sparse path's source pass the call takes.  How the call travels through the host code is
// sbm_frame_source.h's business (a FrameSource of kind FRAMES_TABLE, which holds the flags).  Plain integer code, no HIP types: the
// entry point and sbm_frame_source.h call it, tests/test_frame_ptrs_plan.py compiles it for the CPU suite.
#pragma once
#include <stdint.h>
#include "sbm_source_lines_plan.h"

namespace sbm {

constexpr int FP_ALIGNED4 = 1;            // SBM_PTRS_ALIGNED4: the caller promises that every frame pointer is a multiple of 4
constexpr int FP_KNOWN_FLAGS = FP_ALIGNED4;

// The argument check, in the order the messages are reported.  0: acceptable.
enum FramePtrsError : int { FP_OK = 0, FP_NULL_TABLE = 1, FP_NO_FRAMES = 2, FP_UNKNOWN_FLAGS = 3, FP_SHORT_STRIDE = 4 };

inline int frame_ptrs_check(bool have_table, int n_frames, int cols, int stride, int channels, int flags)
{
    if (!have_table) return FP_NULL_TABLE;
    if (n_frames < 1) return FP_NO_FRAMES;
    if (flags & ~FP_KNOWN_FLAGS) return FP_UNKNOWN_FLAGS;
    if ((int64_t)stride < (int64_t)cols * channels) return FP_SHORT_STRIDE;
    return FP_OK;
}

inline const char* frame_ptrs_error(int e)
{
    switch (e) {
    case FP_NULL_TABLE: return "null table of frame pointers";
    case FP_NO_FRAMES: return "n_frames must be >= 1";
    case FP_UNKNOWN_FLAGS: return "unknown flag bits";
    case FP_SHORT_STRIDE: return "stride < cols*channels";
    default: return "";
    }
}

// The source pass of a table call as whole lines (k_source_lines_ptrs) or in the strided form (QS_SOURCE).  The line form loads
// dwords, so every row of every frame must begin on a 4-byte boundary: the rows' pitch the host sees, the first pixels it cannot --
// the flag stands in for them.  What else the line form asks of a layout is source_lines_ok's business: the rule is that rule
// for ONE frame at an aligned base (a table has no frame stride to ask about).  knob: SBM_SOURCE_LINES is not 0.
inline bool frame_ptrs_source_lines(int flags, int64_t stride, int rows, int cols, int ch, bool knob)
{
    return knob && (flags & FP_ALIGNED4) != 0 && source_lines_ok(0, stride, 0, 1, rows, cols, ch);
}

} // namespace sbm
