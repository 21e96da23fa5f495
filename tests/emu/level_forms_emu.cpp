// TEST INFRASTRUCTURE: shape_based_matching_amd/csrc/sbm_level_forms.h (the per-level record of current linear-memory
// forms, the build plan and the reader choice) behind a C interface, compiled by tests/test_level_forms.py into its
// temporary directory.  No logic of its own: inputs in, the header's answers out.
#include <stdint.h>

#include "sbm_level_forms.h"

using namespace sbm;

static LevelForms from_bits(int b)
{
    LevelForms f;
    f.planes8 = b & 1, f.spread = b & 2, f.spread_strip = b & 4, f.bit_strips = b & 8, f.bit_planes = b & 16;
    return f;
}
static int to_bits(const LevelForms& f)
{
    return (f.planes8 ? 1 : 0) | (f.spread ? 2 : 0) | (f.spread_strip ? 4 : 0) | (f.bit_strips ? 8 : 0) | (f.bit_planes ? 16 : 0);
}

// one record given as bits (planes8 1, spread 2, spread_strip 4, bit_strips 8, bit_planes 16): out = refine_reads,
// full_lm_source, the bits after set(form); returns the signature of the one-level state
extern "C" int64_t sbm_emu_forms_record(int bits, int form, int32_t* out)
{
    LevelForms f = from_bits(bits);
    out[0] = refine_reads(f);
    out[1] = full_lm_source(f);
    LevelForms g = f;
    g.set((LmForm)form);
    out[2] = to_bits(g);
    return forms_signature(&f, 1);
}

// A build of the pyramid and what it leaves.  geo: L, then T, rows, cols of L levels; knobs: full_lm, strip_lm, lm_allty,
// fused_bits, local_bits; thr_state: 0 no threshold yet, 1 a threshold < 0, 2 one >= 0.  A match caller's record includes
// its coarse pass (record_match); a stage caller's is the build alone.  out per level: the plan's form, the record's bits,
// refine_reads; then pack_spread, coarse_on_bits.  Returns the signature.
extern "C" int64_t sbm_emu_forms_build(const int32_t* geo, const int32_t* knobs, int coarse_mode, int refine_bits, int thr_state, int has_spread,
                                       int one_launch, int match_entry, int empty_selection, int32_t* out)
{
    PlanInputs p;
    p.L = geo[0];
    for (int l = 0; l < p.L; ++l) {
        p.T[l] = geo[1 + l], p.rows[l] = geo[1 + p.L + l], p.cols[l] = geo[1 + 2 * p.L + l];
        p.has_spread[l] = has_spread != 0;
        p.has_bit_strips[l] = l < p.L - 1 && p.T[l] == 4; // as ensure_geometry allocates them
    }
    p.has_bit_planes = true;
    p.coarse_mode = coarse_mode;
    p.refine_bits = refine_bits;
    p.have_thr = thr_state != 0;
    p.thr = thr_state == 1 ? -1.f : 90.f;
    p.full_lm = knobs[0], p.strip_lm = knobs[1], p.lm_allty = knobs[2], p.fused_bits = knobs[3], p.local_bits = knobs[4];
    const BuildPlan b = plan_build(p, one_launch != 0, match_entry != 0);
    LevelForms f[LF_MAX_LEVELS];
    for (int l = 0; l < p.L; ++l) f[l] = from_bits(31); // whatever an earlier call left
    if (match_entry) record_match(f, p, one_launch != 0, empty_selection != 0);
    else record_build(f, p.L, b);
    for (int l = 0; l < p.L; ++l) out[3 * l] = b.form[l], out[3 * l + 1] = to_bits(f[l]), out[3 * l + 2] = refine_reads(f[l]);
    out[3 * p.L] = b.pack_spread;
    out[3 * p.L + 1] = coarse_on_bits(p);
    return forms_signature(f, p.L);
}
