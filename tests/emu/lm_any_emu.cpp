// TEST INFRASTRUCTURE: shape_based_matching_amd/csrc/sbm_lm_any_plan.h (the index arithmetic of the batched any-stride
// linear-memory builder k_build_lm_any) behind a C interface, compiled by tests/test_lm_any_plan.py into its temporary
// directory.  sbm_emu_lma_build walks one level the way the kernel does -- block by block, the three LDS stages, then the
// aligned destination dwords of every (grid row, sub-plane) run -- with every size, block, destination and piece taken from
// the header, and counts what the kernel must never do: a store outside the level's T * T * W * H bytes, a byte stored
// twice, a dword store that is not aligned or hangs over its run, an LDS index outside the footprint.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "sbm_lm_any_plan.h"

using namespace sbm;

extern "C" void sbm_emu_lma_shape(int T, int32_t* out)
{
    const LmaShape s = lma_shape(T);
    out[0] = s.cells, out[1] = s.grows, out[2] = lma_lds_bytes(T, s.cells, s.grows), out[3] = lma_pitch(T, s.cells);
}

extern "C" int sbm_emu_lma_level_blocks(int T, int W, int H) { return lma_level_blocks(W, H, lma_shape(T)); }

// block blk of a W x H level: gx0, n_cells, gy0, n_rows
extern "C" void sbm_emu_lma_block(int T, int W, int H, int blk, int32_t* out)
{
    const LmaBlock b = lma_block(blk, W, H, lma_shape(T));
    out[0] = b.gx0, out[1] = b.n_cells, out[2] = b.gy0, out[3] = b.n_rows;
}

extern "C" int sbm_emu_lma_find_level(const int32_t* block_begin, int n_levels, int blk) { return lma_find_level(block_begin, n_levels, blk); }

extern "C" int64_t sbm_emu_lma_dst(int sub, int gy, int gx, int W, int H) { return lma_dst(sub, gy, gx, W, H); }

// One level of one frame.  q: rows x cols one-hot map; out: T * T * W * H + tail bytes of spread bytes (linear-memory order),
// preset by the caller; hits: as many counters, incremented per stored byte.  Returns the number of violations.
extern "C" int64_t sbm_emu_lma_build(const uint8_t* q, int rows, int cols, int T, uint8_t* out, int32_t* hits, int64_t out_bytes)
{
    const int W = cols / T, H = rows / T;
    const LmaShape sh = lma_shape(T);
    const int G = sh.cells, pitch = lma_pitch(T, G), pw = pitch >> 2;
    const int lds = lma_lds_bytes(T, G, sh.grows);
    std::vector<uint8_t> smem((size_t)lds);
    int64_t bad = 0;
    const int64_t level_bytes = (int64_t)T * T * W * H;
    auto lds_ok = [&](int64_t i) {
        if (i < 0 || i >= lds) {
            ++bad;
            return false;
        }
        return true;
    };
    const int n_blocks = lma_level_blocks(W, H, sh);
    for (int blk = 0; blk < n_blocks; ++blk) {
        const LmaBlock b = lma_block(blk, W, H, sh);
        const int lh = (b.n_rows + 1) * T - 1, vh = b.n_rows * T;
        const int o_q = 0, o_v = ((sh.grows + 1) * T - 1) * pitch, o_sp = o_v + sh.grows * T * pitch;
        const int pr0 = b.gy0 * T, pc0 = b.gx0 * T;
        std::fill(smem.begin(), smem.end(), (uint8_t)0xEE); // stale LDS: nothing may depend on it
        for (int idx = 0; idx < lh * pitch; ++idx) {
            const int r = idx / pitch, c = idx - r * pitch;
            const int gr = pr0 + r, gc = pc0 + c;
            if (lds_ok(o_q + idx)) smem[o_q + idx] = (gr < rows && gc < cols) ? q[(size_t)gr * cols + gc] : (uint8_t)0;
        }
        for (int idx = 0; idx < vh * pw; ++idx) {
            const int y = idx / pw, cw = idx - y * pw;
            for (int k = 0; k < 4; ++k) {
                uint8_t v = 0;
                for (int d = 0; d < T; ++d)
                    if (lds_ok(o_q + ((y + d) * pw + cw) * 4 + k)) v |= smem[o_q + ((y + d) * pw + cw) * 4 + k];
                if (lds_ok(o_v + idx * 4 + k)) smem[o_v + idx * 4 + k] = v;
            }
        }
        const int tw = b.n_cells * T;
        for (int idx = 0; idx < vh * tw; ++idx) {
            const int y = idx / tw, c = idx - y * tw;
            uint8_t v = 0;
            for (int d = 0; d < T; ++d)
                if (lds_ok(o_v + y * pitch + c + d)) v |= smem[o_v + y * pitch + c + d];
            const int r = y / T, ty = y - r * T, g = c / T, tx = c - g * T;
            if (lds_ok(o_sp + ((r * T + ty) * T + tx) * G + g)) smem[o_sp + ((r * T + ty) * T + tx) * G + g] = v;
        }
        const int G4 = G >> 2, TT = T * T, per_run = G4 + 1;
        for (int it = 0; it < b.n_rows * TT * per_run; ++it) {
            const int run = it / per_run, j = it - run * per_run;
            const int r = run / TT, sub = run - r * TT;
            const int64_t dst0 = lma_dst(sub, b.gy0 + r, b.gx0, W, H);
            if (j >= lma_pieces(dst0, b.n_cells)) continue;
            const LmaPiece pc = lma_piece(dst0, j);
            if (pc.dst & 3) ++bad;
            if (4 * j - pc.k0 < 0 || 4 * j - pc.k0 > 3) ++bad;
            for (int k = 0; k < 4; ++k) {
                const int cell = pc.k0 + k;
                if (cell < 0 || cell >= b.n_cells) continue; // byte-wise piece: the cells inside only
                const int64_t d = pc.dst + k;
                if (d < 0 || d >= level_bytes || d >= out_bytes) {
                    ++bad;
                    continue;
                }
                if (!lds_ok(o_sp + run * G + cell)) continue;
                out[d] = smem[o_sp + run * G + cell];
                ++hits[d];
            }
        }
    }
    return bad;
}

// ---- the plan of a batch through this builder (sbm_level_forms.h, PlanInputs::any_batch) ----
#include "sbm_level_forms.h"

// geo: L, then T, rows, cols of L levels; knobs: full_lm, fused_bits; thr_state: 0 no threshold yet, 1 one < 0, 2 one >= 0.
// out per level: the plan's form, the record's bits (planes8 1, spread 2, spread_strip 4, bit_strips 8, bit_planes 16) after a
// match entry point's launches (or the build alone), refine_reads; then pack_spread, sparse_gradient.  Returns the signature.
extern "C" int64_t sbm_emu_lma_plan(const int32_t* geo, const int32_t* knobs, int coarse_mode, int thr_state, int has_spread, int any_batch,
                                    int match_entry, int empty_selection, int32_t* out)
{
    PlanInputs p;
    p.L = geo[0];
    for (int l = 0; l < p.L; ++l) {
        p.T[l] = geo[1 + l], p.rows[l] = geo[1 + p.L + l], p.cols[l] = geo[1 + 2 * p.L + l];
        p.has_spread[l] = has_spread != 0;
        p.has_bit_strips[l] = l < p.L - 1 && p.T[l] == 4;
    }
    p.has_bit_planes = true;
    p.coarse_mode = coarse_mode;
    p.have_thr = thr_state != 0;
    p.thr = thr_state == 1 ? -1.f : 90.f;
    p.full_lm = knobs[0], p.fused_bits = knobs[1];
    p.sparse_strips = true, p.sparse_gradient = true, p.l0_stream = true;
    p.any_batch = any_batch != 0;
    const BuildPlan b = plan_build(p, false, match_entry != 0);
    LevelForms f[LF_MAX_LEVELS];
    for (int l = 0; l < p.L; ++l) f[l].planes8 = f[l].spread = f[l].spread_strip = f[l].bit_strips = f[l].bit_planes = true;
    if (match_entry) record_match(f, p, false, empty_selection != 0);
    else record_build(f, p.L, b);
    for (int l = 0; l < p.L; ++l) {
        out[3 * l] = b.form[l];
        out[3 * l + 1] = (f[l].planes8 ? 1 : 0) | (f[l].spread ? 2 : 0) | (f[l].spread_strip ? 4 : 0) | (f[l].bit_strips ? 8 : 0) | (f[l].bit_planes ? 16 : 0);
        out[3 * l + 2] = refine_reads(f[l]);
    }
    out[3 * p.L] = b.pack_spread;
    out[3 * p.L + 1] = b.sparse_gradient;
    return forms_signature(f, p.L);
}
