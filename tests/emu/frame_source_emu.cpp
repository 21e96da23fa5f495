// TEST INFRASTRUCTURE: shape_based_matching_amd/csrc/sbm_frame_source.h -- the typed record of where a call's frames and masks lie,
// the questions the host asks of it and the key of a captured graph -- behind a C interface, beside the three source-pass form rules
// its one form function must agree with.  Compiled by tests/test_frame_source.py into its temporary directory; never loaded by the
// product.
#include "sbm_frame_source.h"

using namespace sbm;

// a graph key as plain integers: the test sets fields by name, copies and compares
struct EmuKey {
    int32_t src_kind, src_stride, src_ch, src_frames, src_flags;
    int64_t src_base, src_frame_stride;
    int32_t mask_kind;
    int64_t mask_base, mask_stride;
    int32_t rows, cols;
    uint32_t thr_bits;
    int64_t out, cap, count, mirror_out, mirror_count;
    int32_t kind;
    int64_t forms_signature;
    int32_t sparse_grad, sparse_rects;
};

static FrameSource frame_source(int kind, int64_t base, int stride, int ch, int frames, int64_t frame_stride, int flags)
{
    FrameSource s;
    s.kind = (FrameKind)kind, s.base = (const void*)(uintptr_t)base, s.stride = stride, s.ch = ch, s.frames = frames;
    s.frame_stride = frame_stride, s.flags = flags;
    return s;
}

static GraphKey graph_key(const EmuKey& e)
{
    GraphKey k;
    k.src = frame_source(e.src_kind, e.src_base, e.src_stride, e.src_ch, e.src_frames, e.src_frame_stride, e.src_flags);
    k.mask.kind = (MaskKind)e.mask_kind, k.mask.base = (const void*)(uintptr_t)e.mask_base, k.mask.stride = e.mask_stride;
    k.rows = e.rows, k.cols = e.cols, k.thr_bits = e.thr_bits;
    k.out = (const void*)(uintptr_t)e.out, k.cap = e.cap, k.count = (const void*)(uintptr_t)e.count;
    k.mirror_out = (const void*)(uintptr_t)e.mirror_out, k.mirror_count = (const void*)(uintptr_t)e.mirror_count;
    k.kind = e.kind, k.forms_signature = e.forms_signature, k.sparse_grad = e.sparse_grad != 0, k.sparse_rects = e.sparse_rects != 0;
    return k;
}

extern "C" int sbm_emu_graph_key_equal(const EmuKey* a, const EmuKey* b) { return graph_key(*a) == graph_key(*b) ? 1 : 0; }

// the constructors the entry points use, as the key's source / mask fields
extern "C" void sbm_emu_strided_frames(EmuKey* e, int64_t base, int stride, int ch, int frames, int64_t frame_stride)
{
    const FrameSource s = strided_frames((const void*)(uintptr_t)base, stride, ch, frames, frame_stride);
    e->src_kind = s.kind, e->src_base = (int64_t)(uintptr_t)s.base, e->src_stride = s.stride, e->src_ch = s.ch, e->src_frames = s.frames;
    e->src_frame_stride = s.frame_stride, e->src_flags = s.flags;
}
extern "C" void sbm_emu_table_frames(EmuKey* e, int planes, int64_t table, int stride, int ch, int frames, int flags)
{
    const FrameSource s = table_frames(planes ? FRAMES_PLANES : FRAMES_TABLE, (const void*)(uintptr_t)table, stride, ch, frames, flags);
    e->src_kind = s.kind, e->src_base = (int64_t)(uintptr_t)s.base, e->src_stride = s.stride, e->src_ch = s.ch, e->src_frames = s.frames;
    e->src_frame_stride = s.frame_stride, e->src_flags = s.flags;
}
extern "C" void sbm_emu_strided_masks(EmuKey* e, int64_t base, int64_t stride)
{
    const MaskSource m = strided_masks((const void*)(uintptr_t)base, stride);
    e->mask_kind = m.kind, e->mask_base = (int64_t)(uintptr_t)m.base, e->mask_stride = m.stride;
}
extern "C" void sbm_emu_table_masks(EmuKey* e, int64_t table)
{
    const MaskSource m = table_masks((const void*)(uintptr_t)table);
    e->mask_kind = m.kind, e->mask_base = (int64_t)(uintptr_t)m.base, e->mask_stride = m.stride;
}

// the questions the host asks of a source (kind: 0 strided, 1 table, 2 planes)
extern "C" int sbm_emu_frames_in_table(int kind, int64_t frame_stride, int flags)
{
    return frames_in_table(frame_source(kind, 0x1000, 1728, 3, 4, frame_stride, flags)) ? 1 : 0;
}
extern "C" int64_t sbm_emu_kernel_frame_stride(int kind, int64_t frame_stride, int flags)
{
    return kernel_frame_stride(frame_source(kind, 0x1000, 1728, 3, 4, frame_stride, flags));
}
extern "C" int sbm_emu_source_may_pack(int kind, int64_t frame_stride, int flags)
{
    return source_may_pack(frame_source(kind, 0x1000, 1728, 3, 4, frame_stride, flags)) ? 1 : 0;
}
extern "C" int64_t sbm_emu_kernel_mask_stride(int mask_kind, int64_t stride)
{
    MaskSource m;
    m.kind = (MaskKind)mask_kind, m.base = (const void*)(uintptr_t)0x2000, m.stride = stride;
    return kernel_mask_stride(m);
}
extern "C" int sbm_emu_masks_per_frame(int mask_kind)
{
    MaskSource m;
    m.kind = (MaskKind)mask_kind;
    return masks_per_frame(m) ? 1 : 0;
}

// the one source-pass form function, and the three rules it switches between
extern "C" int sbm_emu_source_takes_lines(int kind, int64_t base, int stride, int ch, int frames, int64_t frame_stride, int flags, int rows, int cols,
                                          int knob)
{
    return source_takes_lines(frame_source(kind, base, stride, ch, frames, frame_stride, flags), rows, cols, knob != 0) ? 1 : 0;
}
extern "C" int sbm_emu_source_lines_ok(uint64_t base, int64_t stride, int64_t frame_stride, int frames, int rows, int cols, int ch)
{
    return source_lines_ok(base, stride, frame_stride, frames, rows, cols, ch) ? 1 : 0;
}
extern "C" int sbm_emu_frame_ptrs_lines(int flags, int64_t stride, int rows, int cols, int ch, int knob)
{
    return frame_ptrs_source_lines(flags, stride, rows, cols, ch, knob != 0) ? 1 : 0;
}
extern "C" int sbm_emu_frame_planes_lines(int flags, int64_t stride, int rows, int cols, int knob)
{
    return frame_planes_source_lines(flags, stride, rows, cols, knob != 0) ? 1 : 0;
}
