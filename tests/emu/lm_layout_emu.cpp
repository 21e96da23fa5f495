// TEST INFRASTRUCTURE: the stored layouts of a refinement level (shape_based_matching_amd/csrc/sbm_lm_layout.h), the build plan
// (sbm_level_forms.h) and the any-stride builder's workgroup shape (sbm_lm_any_plan.h) behind a C interface, compiled by
// tests/test_lm_form_cases.py into its temporary directory.  No logic of its own: inputs in, the headers' answers out.
#include <stdint.h>

#include "sbm_level_forms.h"
#include "sbm_lm_any_plan.h"
#include "sbm_lm_layout.h"

using namespace sbm;

// out[(sub * H + gy) * W + gx] = lm_strip_offset(sub, gy, gx): every cell of a [subs][H][W] plane
extern "C" void sbm_emu_lml_strip_offsets(int subs, int W, int H, int64_t* out)
{
    for (int sub = 0; sub < subs; ++sub)
        for (int gy = 0; gy < H; ++gy)
            for (int gx = 0; gx < W; ++gx) out[((int64_t)sub * H + gy) * W + gx] = lm_strip_offset(sub, gy, gx, W, H);
}

// out[(plane * (W / 16) + strip) * H + gy] = lm_bits_offset(plane, strip, gy), plane-major as the caller's own array; returns lm_bits_dwords
extern "C" int64_t sbm_emu_lml_bits_offsets(int planes, int W, int H, int64_t* out)
{
    const int S = W >> 4;
    for (int p = 0; p < planes; ++p)
        for (int s = 0; s < S; ++s)
            for (int gy = 0; gy < H; ++gy) out[((int64_t)p * S + s) * H + gy] = lm_bits_offset(p, s, gy, W, H);
    return lm_bits_dwords(W, H);
}

// out = {cells, grows} of the any-stride builder's workgroup at stride T
extern "C" void sbm_emu_lml_any_shape(int T, int32_t* out)
{
    const LmaShape s = lma_shape(T);
    out[0] = s.cells, out[1] = s.grows;
}

// The plan of one build.  geo: L, then T, rows, cols of L levels; knobs: full_lm, strip_lm, lm_allty, fused_bits, local_bits,
// sparse_strips; the buffers as ensure_geometry allocates them.  out per level: the form, LmWork's split and allty for `frames`
// frames; then pack_spread.
extern "C" void sbm_emu_lml_plan(const int32_t* geo, const int32_t* knobs, int coarse_mode, int refine_bits, int one_launch, int any_batch,
                                 int match_entry, int frames, int32_t* out)
{
    PlanInputs p;
    p.L = geo[0];
    for (int l = 0; l < p.L; ++l) {
        p.T[l] = geo[1 + l], p.rows[l] = geo[1 + p.L + l], p.cols[l] = geo[1 + 2 * p.L + l];
        p.has_spread[l] = true;
        p.has_bit_strips[l] = l < p.L - 1 && p.T[l] == 4;
    }
    p.has_bit_planes = true;
    p.coarse_mode = coarse_mode;
    p.refine_bits = refine_bits;
    p.have_thr = match_entry != 0;
    p.thr = 90.f;
    p.full_lm = knobs[0], p.strip_lm = knobs[1], p.lm_allty = knobs[2], p.fused_bits = knobs[3], p.local_bits = knobs[4];
    p.sparse_strips = knobs[5] && p.has_bit_strips[0];
    p.any_batch = any_batch != 0;
    const BuildPlan b = plan_build(p, one_launch != 0, match_entry != 0);
    for (int l = 0; l < p.L; ++l) {
        const LmWork w = lm_work(b.form[l], p.T[l], p.rows[l], p.W(l), p.H(l), frames < 4 ? 4 : 1, p.lm_allty);
        out[3 * l] = b.form[l], out[3 * l + 1] = one_launch ? w.split : 0, out[3 * l + 2] = one_launch ? w.allty : 0;
    }
    out[3 * p.L] = b.pack_spread;
}
