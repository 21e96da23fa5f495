// TEST INFRASTRUCTURE: what the retained copy of level 0's source depends on, compiled for the CPU against wave_emu.h behind a C
// interface, beside what sparse_list_emu.cpp already offers (the mark, the lists, the launches on packed frames):
//   the decision rule source_pass_retains (sbm_source_lines_plan.h),
//   both forms of the source pass given the two call counters (sbm_quantize_stream.h QS_SOURCE, sbm_source_lines.h),
//   the sparse gradient launch -- a wave per item, or by slots from the lists -- on frames in a caller's layout.
// Compiled by tests/test_source_retention.py into its temporary directory; never loaded by the product.
#include "sparse_list_emu.cpp"

#include "sbm_source_lines.h"

extern "C" int sbm_emu_retains(uint32_t enqueued, uint32_t executed) { return source_pass_retains(enqueued, executed) ? 1 : 0; }

// The source pass over frames in the caller's layout with the counters at (enqueued, executed).  form 0: the strided form, a
// narrow last strip packed; form 1: the line form (-2 where its rule refuses the layout).  note: receives what the launch's first
// work item notes (1 stored, 2 skipped); *note_writes counts the work items that changed it.  counters 0: no counters are given
// (null), the copy is always stored.
extern "C" int sbm_emu_source_counted(int form, const uint8_t* img, int frames, int rows, int cols, int ch, int hs, int stride, int64_t img_fs,
                                      uint8_t* pyr, uint8_t* keep, int counters, uint32_t enqueued, uint32_t executed, uint32_t* note,
                                      int32_t* note_writes)
{
    if (bad_geometry(frames, rows, cols, ch, hs) || stride < cols * ch || img_fs < (int64_t)rows * stride) return -1;
    if (form == 1 && !source_lines_ok((uint64_t)(uintptr_t)img, stride, img_fs, frames, rows, cols, ch)) return -2;
    QSArgs a = batch_args(img, frames, rows, cols, ch, 0.f, hs, form == 0);
    a.stride = stride;
    a.img_fs = img_fs;
    a.pyr = pyr;
    a.keep = keep;
    a.keep_fs = (int64_t)rows * cols * ch;
    if (counters) a.call_enqueued = &enqueued, a.call_executed = &executed;
    a.call_note = note;
    *note_writes = 0;
    const int n = form == 1 ? sl_items(cols, a.n_rblocks, frames) : quantize_stream_items(a);
    for (int item = 0; item < n; ++item) {
        *note = 0;
        if (form == 1) {
            if (ch == 3) source_lines_item<3>(a, item);
            else source_lines_item<1>(a, item);
        } else {
            if (ch == 3) quantize_stream_item<3, QS_SOURCE>(a, item);
            else quantize_stream_item<1, QS_SOURCE>(a, item);
        }
        if (*note) {
            ++*note_writes;
            note[1] = *note;
        }
    }
    *note = note[1];
    return n;
}

// The sparse gradient launch on frames in a caller's layout (rows of `stride` bytes, frames img_fs bytes apart), the narrow last
// strip packed as the host packs it.  slots 0: a wave per item of the grid, each testing itself; slots > 0: by slots from `lists`.
// The frame stride may be any value: the frames of a window of a canvas lie a few columns apart.  Returns the working items, or -1.
extern "C" int sbm_emu_sparse_strided(const uint8_t* img, int frames, int rows, int cols, int ch, float weak, int hs, int stride, int64_t img_fs,
                                      const uint8_t* flags, const int32_t* rects, const int32_t* lists, int64_t list_stride, int list_cap, int slots,
                                      int T, int W, int H, uint8_t* out)
{
    if (bad_geometry(frames, rows, cols, ch, hs) || stride < cols * ch || img_fs < 0) return -1;
    QSArgs a = batch_args(img, frames, rows, cols, ch, weak, hs, 1);
    a.stride = stride;
    a.img_fs = img_fs;
    a.out = out;
    a.tile_flags = flags;
    a.n_tiles = refine_tile_count(W, H);
    a.grid_t = T;
    a.grid_w = W;
    a.grid_h = H;
    a.need_rects = rects;
    a.n_bands = refine_band_count(rows);
    int32_t count = 0;
    a.item_count = &count;
    if (slots > 0) {
        a.item_list = lists;
        a.list_stride = list_stride;
        a.list_cap = list_cap;
        a.slots = slots;
        for (int g = 0; g < quantize_slots_groups(a); ++g)
            for (int q = 0; q < 4; ++q) {
                if (ch == 3) quantize_stream_slot_wave<3>(a, g, q);
                else quantize_stream_slot_wave<1>(a, g, q);
            }
        return count;
    }
    for (int item = 0; item < quantize_stream_items(a); ++item) {
        if (ch == 3) quantize_stream_item<3, QS_SPARSE>(a, item);
        else quantize_stream_item<1, QS_SPARSE>(a, item);
    }
    return count;
}
