// TEST INFRASTRUCTURE: shape_based_matching_amd/csrc/sbm_call_record.h (what a match call leaves in the context, and what a
// graph replay restores of it) behind a C interface, compiled by tests/test_call_record.py into its temporary directory.
// No logic of its own: records in as words, CallRecord::replayed, the record out as words.
//
// A record as REC_WORDS int32: per level l (8 levels, 12 words each) the forms as bits (planes8 1, spread 2, spread_strip 4,
// bit_strips 8, bit_planes 16), level_build {form, builder, split, allty, packed}, refine_form[6]; then levels_valid,
// map0_whole, src0_ch, last_frames, coarse_form[4], source_form, sparse_items[3], sparse_items_pending, sparse_list[2].
#include <stdint.h>

#include "sbm_call_record.h"

using namespace sbm;

constexpr int LEVEL_WORDS = 12, REC_WORDS = LF_MAX_LEVELS * LEVEL_WORDS + 15;

static CallRecord from_words(const int32_t* w)
{
    CallRecord r;
    for (int l = 0; l < LF_MAX_LEVELS; ++l, w += LEVEL_WORDS) {
        LevelForms& f = r.forms[l];
        f.planes8 = w[0] & 1, f.spread = w[0] & 2, f.spread_strip = w[0] & 4, f.bit_strips = w[0] & 8, f.bit_planes = w[0] & 16;
        r.level_build[l] = LevelBuild{w[1], w[2], w[3], w[4], w[5]};
        for (int k = 0; k < 6; ++k) r.refine_form[l][k] = w[6 + k];
    }
    r.levels_valid = w[0], r.map0_whole = w[1] != 0, r.src0_ch = w[2], r.last_frames = w[3];
    for (int k = 0; k < 4; ++k) r.coarse_form[k] = w[4 + k];
    r.source_form = w[8];
    for (int k = 0; k < 3; ++k) r.sparse_items[k] = w[9 + k];
    r.sparse_items_pending = w[12] != 0;
    r.sparse_list[0] = w[13], r.sparse_list[1] = w[14];
    return r;
}

static void to_words(const CallRecord& r, int32_t* w)
{
    for (int l = 0; l < LF_MAX_LEVELS; ++l, w += LEVEL_WORDS) {
        const LevelForms& f = r.forms[l];
        w[0] = (f.planes8 ? 1 : 0) | (f.spread ? 2 : 0) | (f.spread_strip ? 4 : 0) | (f.bit_strips ? 8 : 0) | (f.bit_planes ? 16 : 0);
        const LevelBuild& b = r.level_build[l];
        w[1] = b.form, w[2] = b.builder, w[3] = b.split, w[4] = b.allty, w[5] = b.packed;
        for (int k = 0; k < 6; ++k) w[6 + k] = r.refine_form[l][k];
    }
    w[0] = r.levels_valid, w[1] = r.map0_whole, w[2] = r.src0_ch, w[3] = r.last_frames;
    for (int k = 0; k < 4; ++k) w[4 + k] = r.coarse_form[k];
    w[8] = r.source_form;
    for (int k = 0; k < 3; ++k) w[9 + k] = r.sparse_items[k];
    w[12] = r.sparse_items_pending;
    w[13] = r.sparse_list[0], w[14] = r.sparse_list[1];
}

extern "C" int sbm_emu_record_words() { return REC_WORDS; }

// the context's record after the replay of a graph of `kind` whose capture left `captured`
extern "C" void sbm_emu_record_replayed(const int32_t* context, const int32_t* captured, int kind, int32_t* out)
{
    CallRecord r = from_words(context);
    r.replayed(from_words(captured), kind);
    to_words(r, out);
}

// a fresh record, and one a build of `frames` frames has begun on (begin_build) from `context`
extern "C" void sbm_emu_record_begin(const int32_t* context, int frames, int32_t* fresh, int32_t* out)
{
    to_words(CallRecord{}, fresh);
    CallRecord r = from_words(context);
    r.begin_build(frames);
    to_words(r, out);
}
