// sbm_lm_any_plan.h — the index arithmetic of the batched any-stride linear-memory builder k_build_lm_any (sbm_lm_any.h):
// how many grid cells and grid rows a workgroup owns for a stride T, its LDS footprint, which (level, grid rows, cell run) a
// block number names, where a (sub-plane, cell) lands in the linear memories, and how a run of cells whose destination is
// not dword-aligned is cut into aligned dwords.  Plain integer code, no HIP types: the kernel and the host use it,
// tests/test_lm_any_plan.py compiles it for the CPU suite.
//
// A WORKGROUP owns `cells` consecutive grid cells of `grows` consecutive grid rows of one level of one frame.  It holds in LDS
//     s_q   [(grows + 1) * T - 1][pitch]   the one-hot pixels of its grid rows plus the T - 1 rows below and columns right
//                                          of them that the clipped T x T window of spread() reaches (zero outside the image)
//     s_v   [grows * T][pitch]             the OR of T rows downwards
//     s_sp  [grows][T * T][cells]          then of T columns to the right, already in linear-memory order [ty][tx][gx]
// with pitch = cells * T + T - 1 rounded up to a dword.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBM_LMA_HD __host__ __device__ __forceinline__
#else
#define SBM_LMA_HD inline
#endif

namespace sbm {

constexpr int LMA_MAX_T = 16;            // strides the builder takes: 1 .. 16
constexpr int LMA_THREADS = 256;         // threads of a workgroup
// LDS a workgroup may take.  A quarter of a CU's 160 KiB: four workgroups of any stride are resident per CU, and the
// footprint stays far below the 64 KiB a kernel gets without asking for more.
constexpr int LMA_LDS_BUDGET = 40 * 1024;

SBM_LMA_HD int lma_pitch(int T, int cells) { return (cells * T + T - 1 + 3) & ~3; }
SBM_LMA_HD int lma_lds_bytes(int T, int cells, int grows)
{
    const int p = lma_pitch(T, cells);
    return ((grows + 1) * T - 1) * p + grows * T * p + grows * T * T * cells;
}

// The sizing rule: 64 cells per workgroup (a 64-byte run per store instruction and sub-plane), halved until one grid row
// fits the budget (T >= 13: 32 cells); then as many grid rows -- 8, 4 or 2 -- as still fit, because every workgroup loads
// T - 1 rows below its own: one grid row per workgroup reads the map (2T - 1) / T times, eight read it (9T - 1) / 8T times.
struct LmaShape {
    int cells, grows;
};
SBM_LMA_HD LmaShape lma_shape(int T)
{
    LmaShape s{64, 1};
    while (s.cells > 8 && lma_lds_bytes(T, s.cells, 1) > LMA_LDS_BUDGET) s.cells >>= 1;
    for (int g = 8; g > 1; g >>= 1)
        if (lma_lds_bytes(T, s.cells, g) <= LMA_LDS_BUDGET) {
            s.grows = g;
            break;
        }
    return s;
}

// blocks of one level: cell runs along x times groups of grid rows along y, x fastest
SBM_LMA_HD int lma_level_blocks(int W, int H, LmaShape s) { return ((W + s.cells - 1) / s.cells) * ((H + s.grows - 1) / s.grows); }

// what block `blk` of a level owns: cells gx0 .. gx0 + n_cells - 1 of grid rows gy0 .. gy0 + n_rows - 1
struct LmaBlock {
    int gx0, n_cells, gy0, n_rows;
};
SBM_LMA_HD LmaBlock lma_block(int blk, int W, int H, LmaShape s)
{
    const int runs = (W + s.cells - 1) / s.cells;
    const int gyb = blk / runs, run = blk - gyb * runs;
    LmaBlock b;
    b.gx0 = run * s.cells;
    b.n_cells = W - b.gx0 < s.cells ? W - b.gx0 : s.cells;
    b.gy0 = gyb * s.grows;
    b.n_rows = H - b.gy0 < s.grows ? H - b.gy0 : s.grows;
    return b;
}

// the level whose block range holds block `blk`: the one with the largest first block <= blk (ranges in any order)
SBM_LMA_HD int lma_find_level(const int32_t* block_begin, int n_levels, int blk)
{
    int l = 0, lb = -1;
    for (int i = 0; i < n_levels; ++i)
        if (blk >= block_begin[i] && block_begin[i] > lb) l = i, lb = block_begin[i];
    return l;
}

// offset of cell (gx, gy) of sub-plane sub = ty * T + tx in one plane of linear memories: linearize()'s order
// [ty][tx][gy][gx] (line2Dup.cpp:749-777)
SBM_LMA_HD int64_t lma_dst(int sub, int gy, int gx, int W, int H) { return ((int64_t)sub * H + gy) * W + gx; }

// A run of n cells of one (sub-plane, grid row) goes to bytes dst0 .. dst0 + n - 1, and dst0 is dword-aligned only where
// W % 4 == 0.  The run is therefore written as the ALIGNED dwords that cover it: piece j = 0 .. lma_pieces() - 1 is the
// dword at dst0 - (dst0 & 3) + 4 j and holds cells k0 .. k0 + 3 of the run, k0 = 4 j - (dst0 & 3).  A piece whose four
// cells all lie in 0 .. n - 1 is one dword store; the first and the last piece of a row may hang over its ends and are
// written byte by byte, the cells inside only -- the bytes beside them belong to the neighbouring run or row, or are the
// zero tail behind the last sub-plane, which nothing may touch.
SBM_LMA_HD int lma_pieces(int64_t dst0, int n) { return (int)(((dst0 & 3) + n + 3) >> 2); }
struct LmaPiece {
    int k0;      // first cell of the piece, relative to the run (may be negative)
    int64_t dst; // where cell k0 goes: a multiple of 4
};
SBM_LMA_HD LmaPiece lma_piece(int64_t dst0, int j)
{
    const int a = (int)(dst0 & 3);
    return LmaPiece{4 * j - a, dst0 - a + 4 * j};
}

} // namespace sbm
