// sbm_lm_any.h — gfx950 kernel that builds the linear memories of EVERY level of EVERY frame of a batch in one launch, for
// any stride T in 1 .. 16 and any level the reference takes (rows % T == 0, cols % T == 0, rows * cols % 16 == 0): grid
// widths that are no multiple of 4, odd widths, map rows that start on any byte.  The batched counterpart of k_build_lm for
// the pyramids that the register-only builder k_build_lm_rows does not take (sbm_lm_kernels.h).
// Reference functions replaced (file:line in ddcr/shape_based_matching):
//   k_build_lm_any   spread + computeResponseMaps + linearize, fused   line2Dup.cpp:616-630, 637-747, 749-777
// The index arithmetic (cells and grid rows per workgroup, LDS footprint, block -> level / rows / cells, destinations and
// their cut into aligned dwords) is sbm_lm_any_plan.h.
#pragma once
#include "sbm_common.h"
#include "sbm_lm_kernels.h"
#include "sbm_lm_any_plan.h"

namespace sbm {

struct LmaLevel {
    const uint8_t* q; // orientation maps, q_fs bytes from frame to frame
    uint8_t* lm;      // form 1: the spread plane (d_lmc), form 0: the 8 response planes (d_lm), lm_fs bytes from frame to frame
    int64_t lm_stride, q_fs, lm_fs;
    int32_t rows, cols, W, H, T;
    int32_t cells, grows; // lma_shape(T)
    int32_t form;         // LM_SPREAD (1) or LM_PLANES8 (0)
};
struct LmaArgs {
    LmaLevel lv[SBM_MAX_LEVELS];
    int32_t block_begin[SBM_MAX_LEVELS]; // first block of each level's range
    int32_t n_levels;
    int32_t* counters;  // may be null: else the launch zeroes the per-frame counters ...
    int32_t* out_count; // ... and the caller's {n_matches, overflow} pairs (may be null)
};

// One block = lma_block(): `cells` grid cells x `grows` grid rows of level l of frame blockIdx.y.  The one-hot tile with
// its T - 1 halo rows and columns (zero outside the image: the window of spread() clipped at the bottom and the right,
// :626-627) is OR-reduced in LDS, T rows downwards on dwords and then T columns to the right, which also transposes it
// into linear-memory order; a thread then takes one aligned destination dword of one (grid row, sub-plane) run
// (lma_piece) and stores the spread bytes, or their 8 orientation responses.
__global__ __launch_bounds__(LMA_THREADS) void k_build_lm_any(const LmaArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lma_smem[];
    const int tid = threadIdx.x;
    const size_t frame = blockIdx.y;
    if (blockIdx.x == 0 && a.counters) {
        if (tid < CTR_STRIDE) a.counters[frame * CTR_STRIDE + tid] = 0;
        if (tid < 2 && a.out_count) a.out_count[frame * 2 + tid] = 0;
    }
    const int l = lma_find_level(a.block_begin, a.n_levels, (int)blockIdx.x);
    const LmaLevel& p = a.lv[l];
    const int T = p.T, W = p.W, H = p.H, rows = p.rows, cols = p.cols, G = p.cells;
    const LmaBlock b = lma_block((int)blockIdx.x - a.block_begin[l], W, H, LmaShape{G, p.grows});
    const int pitch = lma_pitch(T, G), pw = pitch >> 2;
    const int lh = (b.n_rows + 1) * T - 1; // pixel rows loaded
    const int vh = b.n_rows * T;           // pixel rows of the block's own grid rows
    uint8_t* s_q = lma_smem;                                   // [(grows + 1) * T - 1][pitch]
    uint8_t* s_v = s_q + ((p.grows + 1) * T - 1) * pitch;      // [grows * T][pitch]
    uint8_t* s_sp = s_v + p.grows * T * pitch;                 // [grows][T * T][G]
    const uint8_t* q = p.q + frame * p.q_fs;
    const int pr0 = b.gy0 * T, pc0 = b.gx0 * T;
    if ((cols & 3) == 0) {
        // every map row, the frame and the block's first column start on a dword (q_fs = rows * cols is a multiple of 16,
        // gx0 of 8): a dword lies wholly inside a row or wholly past it
        for (int idx = tid; idx < lh * pw; idx += LMA_THREADS) {
            const int r = idx / pw, c = (idx - r * pw) * 4;
            const int gr = pr0 + r, gc = pc0 + c;
            uint32_t v = 0;
            if (gr < rows && gc < cols) v = *(const uint32_t*)(q + (size_t)gr * cols + gc);
            ((uint32_t*)s_q)[idx] = v;
        }
    } else {
        for (int idx = tid; idx < lh * pitch; idx += LMA_THREADS) {
            const int r = idx / pitch, c = idx - r * pitch;
            const int gr = pr0 + r, gc = pc0 + c;
            s_q[idx] = (gr < rows && gc < cols) ? q[(size_t)gr * cols + gc] : (uint8_t)0;
        }
    }
    __syncthreads();
    // T rows downwards, four pixels at a time
    for (int idx = tid; idx < vh * pw; idx += LMA_THREADS) {
        const int y = idx / pw, cw = idx - y * pw;
        uint32_t v = 0;
        for (int d = 0; d < T; ++d) v |= ((const uint32_t*)s_q)[(y + d) * pw + cw];
        ((uint32_t*)s_v)[idx] = v;
    }
    __syncthreads();
    // T columns to the right; pixel (y, c) is cell g = c / T of grid row y / T, sub-plane (y % T, c % T)
    const int tw = b.n_cells * T;
    for (int idx = tid; idx < vh * tw; idx += LMA_THREADS) {
        const int y = idx / tw, c = idx - y * tw;
        uint8_t v = 0;
        for (int d = 0; d < T; ++d) v |= s_v[y * pitch + c + d];
        const int r = y / T, ty = y - r * T, g = c / T, tx = c - g * T;
        s_sp[((r * T + ty) * T + tx) * G + g] = v;
    }
    __syncthreads();
    const int G4 = G >> 2, TT = T * T, per_run = G4 + 1;
    uint8_t* lm = p.lm + frame * p.lm_fs;
    const int items = b.n_rows * TT * per_run;
    for (int it = tid; it < items; it += LMA_THREADS) {
        const int run = it / per_run, j = it - run * per_run; // run = r * TT + sub
        const int r = run / TT, sub = run - r * TT;
        const int64_t dst0 = lma_dst(sub, b.gy0 + r, b.gx0, W, H);
        if (j >= lma_pieces(dst0, b.n_cells)) continue;
        const LmaPiece pc = lma_piece(dst0, j);
        // cells k0 .. k0 + 3 of the run: with a = dst0 & 3 = 4 j - k0, bytes 4 - a .. 7 - a of the row's dwords j - 1 and j
        const uint32_t* row = (const uint32_t*)s_sp + run * G4;
        const uint32_t lo = j > 0 ? row[j - 1] : 0u, hi = j < G4 ? row[j] : 0u;
        const uint32_t v = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (4 - (4 * j - pc.k0))));
        const bool whole = pc.k0 >= 0 && pc.k0 + 3 < b.n_cells;
        if (p.form == 1) {
            if (whole) *(uint32_t*)(lm + pc.dst) = v;
            else
                for (int k = 0; k < 4; ++k)
                    if (pc.k0 + k >= 0 && pc.k0 + k < b.n_cells) lm[pc.dst + k] = (uint8_t)(v >> (8 * k));
        } else {
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                const uint32_t rsp = response4(v, o);
                uint8_t* d = lm + o * p.lm_stride + pc.dst;
                if (whole) *(uint32_t*)d = rsp;
                else
                    for (int k = 0; k < 4; ++k)
                        if (pc.k0 + k >= 0 && pc.k0 + k < b.n_cells) d[k] = (uint8_t)(rsp >> (8 * k));
            }
        }
    }
}

} // namespace sbm
