// sbm_call_record.h — what a match call leaves in the context (CallRecord): which buffers are resident and in which form, and
// which launches made them.  Every later reader decides by it.  Plain launches write it where they are made; a captured graph
// keeps the record its capture wrote, and a replay restores it (replayed).  No HIP types: tests/test_call_record.py compiles it.
#pragma once
#include <string.h>

#include "sbm_level_forms.h"

namespace sbm {

// Per level, what the last build of its linear memories was (sbm_get_level_build): the LmForm it was made in (LM_BIT_STRIPS_SPARSE
// included), the builder (0 none, 1 k_build_lm_rows, 2 k_build_lm_any, 3 k_build_lm, 4 the unfused path), LmWork's split and allty of
// that launch, and which kernel packed the coarsest level's bit planes since (1 k_pack_bitplanes_spread, 2 k_pack_bitplanes, 0 none).
struct LevelBuild {
    int32_t form = LM_NONE, builder = 0, split = 0, allty = 0, packed = 0;
};

struct CallRecord {
    // ---- what is resident ----
    // which of d_lm[l], d_lmc[l], d_lbits[l], d_blm hold level l's current linear memories (the forms rebuilt on demand: frame 0's only)
    LevelForms forms[LF_MAX_LEVELS];
    int levels_valid = 0;   // number of levels whose linear memories are resident
    bool map0_whole = true; // d_quant[0] holds every frame's whole map (false: a sparse call left it in pieces, ensure_level0_map)
    int src0_ch = 0;        // channels of the retained level-0 source that completes it
    int last_frames = 1;    // frames of the last pyramid built (sbm_get_quantized_frame)
    // ---- what was launched ----
    int32_t coarse_form[4] = {0, 0, 0, 0}; // {kind, P, wide, dw} of the coarse kernel (sbm_get_coarse_form)
    int32_t source_form = 0; // the source pass: 0 none, 1 the strided form QS_SOURCE, 2 k_source_lines (sbm_get_source_form)
    int32_t refine_form[LF_MAX_LEVELS][6] = {}; // {kind, LW, order, t8, sparse, slots} of every level's refinement kernel (sbm_get_refine_form)
    LevelBuild level_build[LF_MAX_LEVELS];
    // the sparse level-0 gradient launch: {selection: 0 none, 1 tiles, 2 need rectangles; working items (-1: not counted); items launched};
    // the count is still on the device (profiling only: never in a captured record); {it ran from item lists, its waves per frame,
    // the rows per item of the grid the lists' entries name (the list grid; the launch's own grid where the two are one)}
    int32_t sparse_items[3] = {0, 0, 0};
    bool sparse_items_pending = false;
    int32_t sparse_list[3] = {0, 0, 0};

    // a call begins to build the pyramid of `frames` frames: no source pass and no sparse launch yet
    void begin_build(int frames)
    {
        last_frames = frames;
        source_form = 0;
        sparse_items[0] = 0, sparse_items[1] = -1, sparse_items[2] = 0;
        sparse_items_pending = false;
        sparse_list[0] = sparse_list[1] = sparse_list[2] = 0;
    }
    void note_level_build(int l, LmForm f, int builder, int split = 0, int allty = 0) { level_build[l] = LevelBuild{(int32_t)f, builder, split, allty, 0}; }
    void note_coarse_form(int kind, int P, bool wide, int dw) { coarse_form[0] = kind, coarse_form[1] = P, coarse_form[2] = wide ? 1 : 0, coarse_form[3] = dw; }
    void note_refine_form(int l, LmForm reads, int LW, int order, bool t8, bool sparse, int slots)
    {
        const int kind = reads == LM_BIT_STRIPS ? 4 : reads == LM_SPREAD_STRIP ? 3 : reads == LM_SPREAD ? 2 : 1;
        const int32_t f[6] = {kind, LW, order, t8 ? 1 : 0, sparse ? 1 : 0, slots};
        memcpy(refine_form[l], f, sizeof f);
    }

    // A graph was replayed whose capture left `captured` (kind: 0 a single frame, > 0 the frames of a batch, < 0 the template
    // loop alone).  A match call's graph makes everything anew: the record is the captured one.  The template loop builds on
    // what is resident -- brought up to date outside the capture, and the same forms as at the capture (forms_signature in the
    // key) -- and notes only its own launches: the coarse pass, the refinement, level 0's strips where it built them sparsely.
    void replayed(const CallRecord& captured, int kind)
    {
        if (kind >= 0) {
            *this = captured;
            return;
        }
        memcpy(coarse_form, captured.coarse_form, sizeof coarse_form);
        memcpy(refine_form, captured.refine_form, sizeof refine_form);
        if (captured.level_build[0].form == LM_BIT_STRIPS_SPARSE) level_build[0] = captured.level_build[0];
    }
};

} // namespace sbm
