// sbm_level_forms.h — which buffers hold a pyramid level's linear memories (LevelForms), in which form a call builds every
// level (plan_build) and which buffer a reader takes (refine_reads, full_lm_source).  Plain data and integer arithmetic,
// no HIP types: the host side (sbm_capi_ctx.inc) launches by it, tests/test_level_forms.py compiles it for the CPU suite.
#pragma once
#include <stdint.h>

namespace sbm {

constexpr int LF_MAX_LEVELS = 8; // SBM_MAX_LEVELS (include/sbm_types.h)

// The forms of a level's linear memories; the values are LmLevelArgs::compact of k_build_lm_rows (sbm_lm_kernels.h).
enum LmForm : int32_t {
    LM_NONE = -1,
    LM_PLANES8 = 0,      // the reference's 8 response planes (d_lm)
    LM_SPREAD = 1,       // one plane of spread bytes, row-major (d_lmc)
    LM_SPREAD_STRIP = 2, // the same plane strip-interleaved (d_lmc, lm_strip_offset)
    LM_BIT_PLANES = 3,   // the coarsest level's 16 bit planes (d_blm, sbm_coarse_bits.h)
    LM_BIT_STRIPS = 4,   // a T = 4 refinement level as bit strips (d_lbits, sbm_local_bits.h)
    // the same strips, but only in the tiles the call's coarse candidates read (sbm_refine_tiles.h): built between the call's
    // coarse pass and its refinement, for that refinement alone -- not a layout of its own, and nothing the call leaves behind
    LM_BIT_STRIPS_SPARSE = 5,
};

// Per level: every field says "this buffer holds the level's current contents" and nothing else.  Several may be set (a
// form rebuilt for a stage entry point stands beside the one it was made from); none is set for a stale buffer.
// Validity is per level, not per frame: a batch build makes every frame current, while the lazy rebuilds (ensure_full_lm,
// ensure_local_forms, ensure_coarse_planes) cover frame 0 only, which is all their readers take.
struct LevelForms {
    bool planes8 = false;      // d_lm[l]
    bool spread = false;       // d_lmc[l] ...
    bool spread_strip = false; // ... strip-interleaved (meaningful only with spread)
    bool bit_strips = false;   // d_lbits[l]
    bool bit_planes = false;   // d_blm (coarsest level only)
    void forget() { *this = LevelForms{}; }
    // the level was rebuilt in form f: every other buffer is stale.  LM_BIT_STRIPS_SPARSE leaves NOTHING current: the strips
    // are whole in no frame, and the orientation map (levels_valid) is what the next reader rebuilds its form from.
    void set(LmForm f)
    {
        forget();
        planes8 = f == LM_PLANES8;
        spread = f == LM_SPREAD || f == LM_SPREAD_STRIP;
        spread_strip = f == LM_SPREAD_STRIP;
        bit_planes = f == LM_BIT_PLANES;
        bit_strips = f == LM_BIT_STRIPS;
    }
};

// What the refinement pass reads of a level: the bit strips, else the spread plane unless the 8 planes are current, else those.
// LM_NONE: nothing is current -- after a sparse match call; the reader rebuilds from the resident orientation map
// (ensure_local_forms), or is that call's own refinement, which builds its tiles (sparse_refine).
inline LmForm refine_reads(const LevelForms& f)
{
    if (f.bit_strips) return LM_BIT_STRIPS;
    if (f.spread && !f.planes8) return f.spread_strip ? LM_SPREAD_STRIP : LM_SPREAD;
    return f.planes8 ? LM_PLANES8 : LM_NONE;
}

// What the 8 response planes of a level are made from when a stage entry point asks for them: themselves, the spread plane
// (expanded), or -- returned as the form that is current, LM_NONE where none is (a sparse match call) -- the resident
// orientation map
inline LmForm full_lm_source(const LevelForms& f)
{
    if (f.planes8) return LM_PLANES8;
    if (f.spread) return f.spread_strip ? LM_SPREAD_STRIP : LM_SPREAD;
    return f.bit_strips ? LM_BIT_STRIPS : (f.bit_planes ? LM_BIT_PLANES : LM_NONE);
}

// Part of the key of a captured template loop, whose kernels and operands follow from the forms: a stage entry point may
// have rebuilt a level in another form since the capture, at the same geometry.
inline int64_t forms_signature(const LevelForms* f, int L)
{
    int64_t sig = 0;
    for (int l = 0; l < L; ++l)
        sig = sig * 32 + ((f[l].planes8 ? 1 : 0) | (f[l].spread ? 2 : 0) | (f[l].spread && f[l].spread_strip ? 4 : 0) | (f[l].bit_strips ? 8 : 0) |
                          (f[l].bit_planes ? 16 : 0));
    return sig;
}

// Everything the choice of forms depends on: geometry, the buffers that exist, modes, threshold, knobs (Tuning) and the caller
struct PlanInputs {
    int L = 0;
    int T[LF_MAX_LEVELS] = {}, rows[LF_MAX_LEVELS] = {}, cols[LF_MAX_LEVELS] = {};
    bool has_spread[LF_MAX_LEVELS] = {}, has_bit_strips[LF_MAX_LEVELS] = {}; // d_lmc[l], d_lbits[l] are allocated
    bool has_bit_planes = false;                                             // d_blm is
    int coarse_mode = 0;  // sbm_set_coarse_mode
    int refine_bits = -1; // sbm_set_refine_bits
    bool have_thr = false;
    float thr = 0.f;
    bool full_lm = false, strip_lm = true, lm_allty = true, fused_bits = true; // SBM_FULL_LM, SBM_STRIP_LM, SBM_LM_ALLTY, SBM_FUSED_BITS
    int local_bits = -1;                                                       // SBM_LOCAL_BITS
    bool sparse_strips = false; // level 0 of a two-level pyramid as LM_BIT_STRIPS_SPARSE (off here; on in a context unless SBM_SPARSE_STRIPS=0)
    // Level 0's gradient stage only where the flagged tiles' strip builders read its map (sbm_quantize_stream.h, QS_SOURCE and
    // QS_SPARSE): the knob (off here; on in a context that holds the retained source buffer unless SBM_SPARSE_GRADIENT=0 or
    // SBM_SPARSE_STRIPS=0), and what the caller says of ONE call: its level-0 launches take the streaming kernel, it brings a
    // mask (a level-0 mask is the caller's memory too, gone when a later reader asks for the whole map), it is banded
    bool sparse_gradient = false;
    bool l0_stream = false, l0_mask = false, banded = false;
    // A batch of frames on a pyramid that the one-launch builder does not take (one_launch false: a stride other than 4 or 8,
    // a level whose width is no multiple of 16), strides up to 16: the batched any-stride builder k_build_lm_any
    // (sbm_lm_any.h) makes every level of every frame.  What one call says; off for a single frame, which keeps the generic
    // single-frame builder and its 8 response planes.
    bool any_batch = false;
    int W(int l) const { return cols[l] / T[l]; }
    int H(int l) const { return rows[l] / T[l]; }
};

// the coarse pass of the current threshold runs on bit planes (sbm_coarse_bits.h): every raw_min >= 1, mode auto or bits
inline bool coarse_on_bits(const PlanInputs& p) { return (p.coarse_mode == 0 || p.coarse_mode == 3) && p.have_thr && p.thr >= 0.f && p.has_bit_planes; }

// The coarse pass on bit planes that are not current packs them from the 8 response planes -- inside the pass, which an
// empty template selection skips
inline bool coarse_packs_planes(const PlanInputs& p, const LevelForms& coarsest, bool empty_selection)
{
    return coarse_on_bits(p) && !empty_selection && !coarsest.bit_planes;
}

// a T = 4 strip level is wanted as bit strips (refined by k_similarity_local_bits) ...
inline bool local_bits_wanted(const PlanInputs& p, int l)
{
    const int mode = p.refine_bits >= 0 ? p.refine_bits : (p.local_bits >= 0 ? p.local_bits : 1);
    return l < p.L - 1 && !p.full_lm && p.strip_lm && p.lm_allty && mode != 0 && p.T[l] == 4 && (p.W(l) & 15) == 0;
}

// In which form a build of the pyramid makes every level.
//   one_launch   every level takes the one-launch builder k_build_lm_rows (T in {4, 8}, 16-column-aligned rows); else -- and
//                in the captured single-frame graph -- the generic builder makes the 8 response planes of every level,
//                unless the call is a batch (PlanInputs::any_batch): then k_build_lm_any makes, in the forms the batched
//                readers take at any stride and width, one plane of spread bytes of a refinement level, the same of the
//                coarsest level of a coarse pass on bit planes (which k_pack_bitplanes_spread packs), else the 8 planes.
//                No strips, no bit strips, no sparse level 0 and no fused bit planes: those need T = 4 and aligned grids.
//   match_entry  a match entry point (it has set the threshold, and its launch resets the counters): refinement levels may
//                become bit strips, the coarsest level its bit planes.  Stage entry points keep to bytes.
struct BuildPlan {
    LmForm form[LF_MAX_LEVELS];
    bool pack_spread; // the coarsest level is LM_SPREAD and k_pack_bitplanes_spread makes the bit planes from it
    // level 0's orientation map is made between the coarse pass and the refinement, in the flagged tiles' reach only: the call
    // leaves the map whole in no frame (the context's "level 0's map is whole" flag goes down; ensure_level0_map)
    bool sparse_gradient;
};
inline BuildPlan plan_build(const PlanInputs& p, bool one_launch, bool match_entry)
{
    BuildPlan b;
    b.pack_spread = false;
    b.sparse_gradient = false;
    for (int l = 0; l < LF_MAX_LEVELS; ++l) b.form[l] = l < p.L ? LM_PLANES8 : LM_NONE;
    if (!one_launch && p.any_batch) {
        for (int l = 0; l < p.L - 1; ++l)
            if (!p.full_lm && p.has_spread[l]) b.form[l] = LM_SPREAD;
        const int lc = p.L - 1;
        if (match_entry && coarse_on_bits(p) && p.fused_bits && !p.full_lm && p.has_spread[lc]) b.form[lc] = LM_SPREAD, b.pack_spread = true;
        return b;
    }
    if (!one_launch) return b;
    // refinement-only levels: ONE plane of spread bytes, strip-interleaved when the grid width allows it (the refinement
    // pass reads 16 x 16 cells per feature: 2 - 4 cache lines instead of 16), or bit strips
    for (int l = 0; l < p.L - 1; ++l) {
        if (p.full_lm || !p.has_spread[l]) continue;
        b.form[l] = p.strip_lm && (p.W(l) & 15) == 0 ? LM_SPREAD_STRIP : LM_SPREAD;
        if (match_entry && local_bits_wanted(p, l) && p.has_bit_strips[l]) b.form[l] = LM_BIT_STRIPS;
    }
    // Two levels: the coarse candidates are the refinement's, so level 0's strips wait for them.  (Deeper pyramids keep the
    // whole build: refinement at an intermediate level moves the candidates before level 0 is read.)
    if (p.sparse_strips && p.L == 2 && b.form[0] == LM_BIT_STRIPS) b.form[0] = LM_BIT_STRIPS_SPARSE;
    b.sparse_gradient = p.sparse_gradient && match_entry && b.form[0] == LM_BIT_STRIPS_SPARSE && p.l0_stream && !p.l0_mask && !p.banded;
    // the coarsest level of a coarse pass on bit planes: those only, inside the launch (a wave's 256 positions must not
    // straddle two sub-planes), else the spread plane and a pack launch; without either, the 8 planes (packed on demand)
    const int lc = p.L - 1;
    if (match_entry && coarse_on_bits(p) && p.fused_bits) {
        if ((((int64_t)p.W(lc) * p.H(lc)) & 255) == 0) b.form[lc] = LM_BIT_PLANES;
        else if (p.has_spread[lc]) b.form[lc] = LM_SPREAD, b.pack_spread = true;
    }
    return b;
}

// what a build by plan b leaves current
inline void record_build(LevelForms* f, int L, const BuildPlan& b)
{
    for (int l = 0; l < L; ++l) f[l].set(b.form[l]);
    if (b.pack_spread) f[L - 1].bit_planes = true;
}

// ... and the coarse pass of a match entry point that packs the coarsest level's bit planes from its 8 response planes
// (coarse_packs_planes; pack_bitplanes): they are current beside those
inline void record_pack(LevelForms& coarsest) { coarsest.bit_planes = true; }

// The two steps in the order a match entry point makes them (enqueue_pyramid, then enqueue_coarse), for the CPU models of a whole
// call (tests/emu).  The host side records each step where it launches it and keeps a graph's record with the graph
// (sbm_call_record.h): nothing there derives a record through this.
inline void record_match(LevelForms* f, const PlanInputs& p, bool one_launch, bool empty_selection)
{
    record_build(f, p.L, plan_build(p, one_launch, true));
    if (coarse_packs_planes(p, f[p.L - 1], empty_selection)) record_pack(f[p.L - 1]);
}

// One level's share of a k_build_lm_rows launch: LmLevelArgs::split and ::allty, and the work items (256 per block).
// split: the items an 8-plane level is cut into per (pixel row, 4 cells): LM_FULL_SPLIT for a few frames, 1 for a batch
struct LmWork {
    int32_t split, allty;
    int64_t items;
};
inline LmWork lm_work(LmForm f, int T, int rows, int W, int H, int split, bool lm_allty)
{
    LmWork w{1, 0, (int64_t)rows * (W >> 2)}; // LM_SPREAD, LM_BIT_PLANES: a thread per (pixel row, 4 cells)
    if (f == LM_PLANES8) {
        w.split = split;
        w.items *= w.split;
    } else if (f == LM_BIT_STRIPS || f == LM_BIT_STRIPS_SPARSE) { // (sparse: the later launch's share; none of the pyramid's)
        w.allty = 1;
        w.items = (int64_t)((W + 31) >> 5) * ((H + 31) >> 5) * 256;
    } else if (f == LM_SPREAD_STRIP) { // a workgroup per 16 grid rows x 64 cells, for all four ty at T = 4 (all-ty threads), else per ty
        w.allty = T == 4 && lm_allty ? 1 : 0;
        w.items = (int64_t)((W + 63) >> 6) * ((H + 15) >> 4) * (w.allty ? 1 : T) * 256;
    }
    return w;
}

} // namespace sbm
