// TEST INFRASTRUCTURE: shape_based_matching_amd/csrc/sbm_refine_tiles.h (where a coarse candidate's refinement looks and which
// bit-strip tiles it reads) behind a C interface, compiled by tests/test_refine_tiles.py into its temporary directory.  No logic
// of its own: candidates in, the header's origins and tile marks out; and the build plan of sbm_level_forms.h with its
// sparse_strips input, which tests/emu/level_forms_emu.cpp leaves at its default.
#include <stdint.h>

#include "sbm_level_forms.h"
#include "sbm_refine_tiles.h"

using namespace sbm;

// cand: n x (cx, cy, width, height).  extra: the features reach this many pixels past the declared box (the footprint is taken
// of the features' extent, the clamp of the declared box, as k_mark_refine_tiles does).  origin: n x (x, y, ox, oy).  mask: per candidate bit t = tile t is marked (the grids of
// the test have at most 64 tiles); returns the tile count of the grid, or -1 if a mark fell outside it.
extern "C" int sbm_emu_refine_tiles(int64_t n, const int32_t* cand, int rows, int cols, int T, int W, int H, int extra, int32_t* origin,
                                    uint64_t* mask)
{
    const int n_tiles = refine_tile_count(W, H);
    bool outside = n_tiles > 64;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t* c = cand + 4 * i;
        const RefineOrigin o = refine_origin(c[0], c[1], c[2], c[3], rows, cols, T);
        origin[4 * i] = o.x, origin[4 * i + 1] = o.y, origin[4 * i + 2] = o.ox, origin[4 * i + 3] = o.oy;
        uint64_t m = 0;
        refine_tiles_for_each(refine_tiles(o, c[2] + extra, c[3] + extra, rows, cols, T, W, H), W, H, [&](int tile) {
            if (tile < 0 || tile >= n_tiles || tile >= 64) outside = true;
            else m |= (uint64_t)1 << tile;
        });
        mask[i] = m;
    }
    return outside ? -1 : n_tiles;
}

// The plan of a build with PlanInputs::sparse_strips as given (every other knob at its default, threshold 90, all buffers
// allocated) and what record_match / record_build leaves.  geo: L, then T, rows, cols of L levels.  out per level: the plan's
// form, refine_reads and full_lm_source of the record, whether anything is current.  Returns the signature.
extern "C" int64_t sbm_emu_sparse_plan(const int32_t* geo, int sparse, int match_entry, int32_t* out)
{
    PlanInputs p;
    p.L = geo[0];
    for (int l = 0; l < p.L; ++l) {
        p.T[l] = geo[1 + l], p.rows[l] = geo[1 + p.L + l], p.cols[l] = geo[1 + 2 * p.L + l];
        p.has_spread[l] = true;
        p.has_bit_strips[l] = l < p.L - 1 && p.T[l] == 4;
    }
    p.has_bit_planes = true;
    p.have_thr = true;
    p.thr = 90.f;
    p.sparse_strips = sparse != 0;
    const BuildPlan b = plan_build(p, true, match_entry != 0);
    LevelForms f[LF_MAX_LEVELS];
    for (int l = 0; l < p.L; ++l) f[l].set(LM_PLANES8); // whatever an earlier call left
    if (match_entry) record_match(f, p, true, false);
    else record_build(f, p.L, b);
    for (int l = 0; l < p.L; ++l) {
        out[4 * l] = b.form[l], out[4 * l + 1] = refine_reads(f[l]), out[4 * l + 2] = full_lm_source(f[l]);
        out[4 * l + 3] = f[l].planes8 || f[l].spread || f[l].bit_strips || f[l].bit_planes;
        // the sparse launch has the whole build's workgroups, one per tile
        const LmForm whole = b.form[l] == LM_BIT_STRIPS_SPARSE ? LM_BIT_STRIPS : b.form[l];
        if (lm_work(b.form[l], p.T[l], p.rows[l], p.W(l), p.H(l), 1, true).items != lm_work(whole, p.T[l], p.rows[l], p.W(l), p.H(l), 1, true).items) return -1;
        if (b.form[l] == LM_BIT_STRIPS_SPARSE && lm_work(whole, p.T[l], p.rows[l], p.W(l), p.H(l), 1, true).items != (int64_t)256 * refine_tile_count(p.W(l), p.H(l))) return -1;
    }
    return forms_signature(f, p.L);
}
