// sbm_frame_source.h — where the frames and masks of one gradient launch lie, as a typed record: frames a fixed number of bytes
// apart, a device table of frame addresses (sbm_match_batch_device_ptrs) or a device table of plane addresses
// (sbm_match_batch_device_planes).  Every host function between an entry point and the kernel launch takes the record, asks its
// questions of it here, and the key of a captured graph (GraphKey) holds it field by field.  Plain integer code, no HIP types:
// tests/test_frame_source.py compiles it for the CPU suite.
#pragma once
#include <stdint.h>
#include "sbm_frame_planes_plan.h"

namespace sbm {

enum FrameKind : int { FRAMES_STRIDED, FRAMES_TABLE, FRAMES_PLANES };

struct FrameSource {
    FrameKind kind = FRAMES_STRIDED;
    const void* base = nullptr; // STRIDED: the first frame; TABLE / PLANES: the device array of addresses (the host never reads it)
    int stride = 0;             // bytes per row (of a plane, for PLANES)
    int ch = 0;
    int frames = 1;
    int64_t frame_stride = 0;   // STRIDED: bytes from one frame to the next (any value, also 0 or negative); 0 otherwise
    int flags = 0;              // TABLE: SBM_PTRS_* bits; PLANES: reserved, 0
};

enum MaskKind : int { MASK_NONE, MASK_SHARED, MASK_STRIDED, MASK_TABLE };

struct MaskSource {
    MaskKind kind = MASK_NONE;
    const void* base = nullptr; // SHARED: the one mask; STRIDED: the first frame's; TABLE: the device array of mask addresses
    int64_t stride = 0;         // STRIDED: bytes from one frame's mask to the next; 0 otherwise
};

inline bool operator==(const FrameSource& a, const FrameSource& b)
{
    return a.kind == b.kind && a.base == b.base && a.stride == b.stride && a.ch == b.ch && a.frames == b.frames &&
           a.frame_stride == b.frame_stride && a.flags == b.flags;
}
inline bool operator==(const MaskSource& a, const MaskSource& b) { return a.kind == b.kind && a.base == b.base && a.stride == b.stride; }

// ---- constructors ----
// `frames` frames of rows x cols x ch pixels, packed: the context's own buffers (a pyramid level, the retained level-0 source)
inline FrameSource packed_frames(const void* base, int rows, int cols, int ch, int frames)
{
    FrameSource s;
    s.base = base, s.stride = cols * ch, s.ch = ch, s.frames = frames, s.frame_stride = (int64_t)rows * cols * ch;
    return s;
}
inline FrameSource strided_frames(const void* base, int stride, int ch, int frames, int64_t frame_stride)
{
    FrameSource s;
    s.base = base, s.stride = stride, s.ch = ch, s.frames = frames, s.frame_stride = frame_stride;
    return s;
}
inline FrameSource table_frames(FrameKind kind, const void* table, int stride, int ch, int frames, int flags)
{
    FrameSource s;
    s.kind = kind, s.base = table, s.stride = stride, s.ch = ch, s.frames = frames, s.flags = flags;
    return s;
}
// no mask (null), one mask for all frames (stride 0), or a mask per frame
inline MaskSource strided_masks(const void* base, int64_t stride)
{
    MaskSource m;
    if (base) m.kind = stride ? MASK_STRIDED : MASK_SHARED, m.base = base, m.stride = stride;
    return m;
}
inline MaskSource table_masks(const void* table)
{
    MaskSource m;
    if (table) m.kind = MASK_TABLE, m.base = table;
    return m;
}

// ---- what the host asks of a source ----
// the frames are named by a device table of either kind
inline bool frames_in_table(const FrameSource& s) { return s.kind != FRAMES_STRIDED; }
// a mask per frame (levels >= 1 then hold one resized mask per frame)
inline bool masks_per_frame(const MaskSource& m) { return m.kind == MASK_STRIDED || m.kind == MASK_TABLE; }
// the img_fs / mask_fs a kernel gets: behind a table the kernel reads addresses, and the stride argument is not read
inline int64_t kernel_frame_stride(const FrameSource& s) { return s.kind == FRAMES_STRIDED ? s.frame_stride : 0; }
inline int64_t kernel_mask_stride(const MaskSource& m) { return m.kind == MASK_STRIDED ? m.stride : 0; }
// A launch may share a wave among the narrow last strips of several frames (32-bit lane offsets from the group's first frame).
// Frames named by a table lie anywhere, no such offset reaches from one to the next: the table forms are launched unpacked
// (DESIGN.md section 5 has the measurement behind that choice).
inline bool source_may_pack(const FrameSource& s) { return !frames_in_table(s); }
// The source pass as whole lines (k_source_lines, k_source_lines_ptrs) or in the strided form (QS_SOURCE).  Behind a table the host
// cannot see the frames' addresses: the caller's promise (SBM_PTRS_ALIGNED4) stands in for them.  Planes have no line form.
// knob: SBM_SOURCE_LINES is not 0.
inline bool source_takes_lines(const FrameSource& s, int rows, int cols, bool knob)
{
    switch (s.kind) {
    case FRAMES_PLANES: return frame_planes_source_lines(s.flags, s.stride, rows, cols, knob);
    case FRAMES_TABLE: return frame_ptrs_source_lines(s.flags, s.stride, rows, cols, s.ch, knob);
    default: return knob && source_lines_ok((uint64_t)(uintptr_t)s.base, s.stride, s.frame_stride, s.frames, rows, cols, s.ch);
    }
}

// ---- the key of a captured graph: every argument the recorded launches depend on ----
// kind: 0 a single frame, > 0 the frames of a batch, -1 the template loop alone.  The tables' contents are no part of the key (only
// the kernels read them), their kind and flags are: a _ptrs and a _planes call at one table address record different kernels.
struct GraphKey {
    FrameSource src;
    MaskSource mask;
    int rows = 0, cols = 0;
    uint32_t thr_bits = 0;
    const void* out = nullptr;
    int64_t cap = 0;
    const void* count = nullptr;
    const void* mirror_out = nullptr;
    const void* mirror_count = nullptr;
    int kind = 0;
    int64_t forms_signature = 0; // kind < 0: the form every level is held in (what the template loop's launches depend on); else 0
    bool sparse_grad = false;    // the call's plan makes level 0's map sparsely (another launch sequence at the same geometry)
    bool sparse_rects = false;   // ... with its work items taken from the record of need rectangles (other kernel arguments)
    int sparse_slots = 0;        // ... by that many waves per frame from the lists of working items, 0: a wave per item (another grid)
    int sparse_list_hs = 0;      // ... the lists made on a grid of that many rows per item (other arguments of two launches)
};

inline bool operator==(const GraphKey& a, const GraphKey& b)
{
    return a.src == b.src && a.mask == b.mask && a.rows == b.rows && a.cols == b.cols && a.thr_bits == b.thr_bits && a.out == b.out &&
           a.cap == b.cap && a.count == b.count && a.mirror_out == b.mirror_out && a.mirror_count == b.mirror_count && a.kind == b.kind &&
           a.forms_signature == b.forms_signature && a.sparse_grad == b.sparse_grad && a.sparse_rects == b.sparse_rects &&
           a.sparse_slots == b.sparse_slots && a.sparse_list_hs == b.sparse_list_hs;
}

} // namespace sbm
