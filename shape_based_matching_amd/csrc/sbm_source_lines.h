// sbm_source_lines.h — the source pass of the sparse level-0 path (sbm_quantize_stream.h, QS_SOURCE) in a form made for the
// memory pipeline: k_source_lines.  Same outputs, bit for bit: the packed retained copy of the level-0 image (QSArgs::keep) and
// cv::pyrDown of it (QSArgs::pyr, ColorGradientPyramid::pyrDown, line2Dup.cpp:424-444).  The index arithmetic and the rule that
// says which layouts it takes are in sbm_source_lines_plan.h; a layout it does not take stays with QS_SOURCE.
//
// What differs from QS_SOURCE is the shape of the memory operations, not the arithmetic's result:
//   strips     256 source columns per wave and no halo lanes: a wave-row is 768 contiguous bytes of BGR (256 of gray), loaded
//              with ONE 96-bit (32-bit) buffer load per lane and stored to the copy with one streamed store of the same width
//   edges      the horizontal [1 4 6 4 1] reaches two pixels left of the strip and one right of it: lane 0 and lane 63 fetch
//              them with one extra load per row (every other lane's offset is dropped by the range check); the interior lanes
//              get their neighbours' raw dwords by DPP; at the image border REFLECT_101 folds the taps onto the lane's own pixels
//   order      the horizontal pass and the decimation first, per source row, on the raw bytes; then the vertical 5-tap on the
//              half-width rows -- one packed u16 pair per channel and row in the window instead of two.  All sums are integers
//              <= 16 * 16 * 255 = 65 280 and there is one rounding (s + 128) >> 8, so the order changes no bit
//   pyrDown    an even lane stores its own two output pixels and its right neighbour's as three dwords (gray: one): 384 (128)
//              contiguous bytes per wave and row, no 2-byte store
//   rows       the rows a moved-up last block shares with the block above are stored by that block alone
// The loop keeps what the QS_SOURCE loop learned: straight-line code with no branch around a load or a store, a row or a
// cv::pyrDown row that is not the item's own dropped by its offset, SL_PREFETCH rows of loads in flight, no constant-row test.
#pragma once
#include "sbm_quantize_stream.h"
#include "sbm_source_lines_plan.h"

#ifdef SBM_WAVE_EMU
// the buffer loads and the plain 96-bit store in terms of the emulation's memory (sbm_wave_gfx950.h has the instructions): a
// dropped lane reads 0; a kept lane that would read outside the buffer, or off a dword boundary, is a kernel bug -> abort
namespace wv {
inline V buf_load_dword(const Buf& b, const V& voff, uint32_t soff, uint32_t k, uint32_t n)
{
    V r;
    for (int i = 0; i < WAVE; ++i) {
        r.l[i] = 0;
        if ((uint64_t)voff.l[i] + 4 * n > b.bytes) continue;
        if ((uint64_t)voff.l[i] + soff + 4 * n > b.bytes || ((voff.l[i] + soff) & 3) || ((uintptr_t)b.base & 3)) __builtin_trap();
        memcpy(&r.l[i], b.base + voff.l[i] + soff + 4 * k, 4);
    }
    return r;
}
inline void sched_fence() {}
inline V buf_load_u32(const Buf& b, const V& voff, uint32_t soff) { return buf_load_dword(b, voff, soff, 0, 1); }
inline void buf_load_u32x2(const Buf& b, const V& voff, uint32_t soff, V& v0, V& v1)
{
    v0 = buf_load_dword(b, voff, soff, 0, 2);
    v1 = buf_load_dword(b, voff, soff, 1, 2);
}
inline void buf_load_u32x3(const Buf& b, const V& voff, uint32_t soff, V& v0, V& v1, V& v2)
{
    v0 = buf_load_dword(b, voff, soff, 0, 3);
    v1 = buf_load_dword(b, voff, soff, 1, 3);
    v2 = buf_load_dword(b, voff, soff, 2, 3);
}
inline void buf_store_u32x3(const Buf& b, const V& voff, uint32_t soff, const V& v0, const V& v1, const V& v2)
{
    // all three dwords or none: the range check is on the 12 bytes
    V off = voff;
    for (int i = 0; i < WAVE; ++i)
        if ((uint64_t)voff.l[i] + 12 > b.bytes) off.l[i] = BUF_DROP;
    buf_store_u32(b, off, soff, v0);
    buf_store_u32(b, off, soff + 4, v1);
    buf_store_u32(b, off, soff + 8, v2);
}
} // namespace wv
#endif

namespace sbm {

constexpr int SL_PREFETCH = 4; // source rows in flight ahead of the one being consumed (the ring holds 6)

// One work item: strip `strip` (256 columns), rows sl_rows(rb, ...) of frame `frame`.
// PTRS: the table form (sbm_quantize_stream.h) -- a.img is a device array of frame addresses, each a multiple of 4 by the caller's promise.
template <int CH, bool PTRS = false>
__device__ __forceinline__ void source_lines_wave(const QSArgs& a, int strip, int rb, int frame)
{
    using namespace wv;
    constexpr int ND = CH == 3 ? 3 : 1; // source dwords per lane and row
    constexpr int NE = CH == 3 ? 2 : 1; // ... of the edge load
    const int rows = a.rows, cols = a.cols;
    const SlRows rr = sl_rows(rb, a.hs, a.row_lo, a.row_hi);
    const int R0 = rr.r0, R1 = rr.r1, own0 = rr.own0;
    const int drows = rows >> 1, dcols = cols >> 1;

    // ---- per-lane constants: sl_lane_col, sl_row_off and sl_pyr_off of the plan header over the 64 lanes, BUF_DROP for their -1 ----
    const V lane = lane_id();
    const V c0 = splat((uint32_t)(strip * SL_STRIP)) + (lane << 2); // first column of this lane
    const P in_img = lt_i(c0, splat((uint32_t)cols));               // not a lane of the cut
    const V row_off = select(in_img, CH == 3 ? c0 + (c0 << 1) : c0, BUF_DROP); // the lane's bytes in a source row and in a row of the copy
    const uint8_t* img = PTRS ? qs_table_entry(a.img, frame) : a.img + (int64_t)frame * a.img_fs;
    const Buf src_buf = make_buf(const_cast<uint8_t*>(img), sl_frame_bytes(rows, cols, CH, a.stride));
    const Buf keep_buf = make_buf(a.keep + (int64_t)frame * a.keep_fs, source_keep_range(a, (uint32_t)rows * (uint32_t)cols * CH, strip == 0 && rb == 0 && frame == 0));
    const Buf pyr_buf = make_buf(a.pyr + (int64_t)frame * a.pyr_fs, (uint32_t)drows * (uint32_t)dcols * CH);
    const V pyr_off = select(p_and(in_img, eq(lane & 1u, splat(0u))), CH == 3 ? (c0 >> 1) + ((c0 >> 1) << 1) : (c0 >> 1), BUF_DROP);
    // the edge load: lane 0 and lane 63 of a strip with a neighbour on that side
    const P is_l0 = eq(lane, splat(0u)), is_l63 = eq(lane, splat(63u));
    const int64_t e_left = sl_edge_left(strip, CH), e_right = sl_edge_right(strip, cols, CH);
    const V edge_off = select(is_l0, e_left >= 0 ? (uint32_t)e_left : BUF_DROP, select(is_l63, e_right >= 0 ? (uint32_t)e_right : BUF_DROP, BUF_DROP));
    // REFLECT_101 at the left / right image border: the lane holding column 0 / column cols - 4
    const bool left_border = e_left < 0, right_border = e_right < 0;
    const P first = eq(c0, splat(0u)), last = eq(c0, splat((uint32_t)(cols - 4)));
    const uint32_t K4 = opaque(QS_K(4, 4));

    V hw[6][CH]; // horizontally filtered, decimated rows: (out_a, out_b) <= 4080 as a u16 pair, row i of the item in slot i % 6
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int c = 0; c < CH; ++c) hw[k][c] = splat(0u);
    V dq[6][ND], de[6][NE]; // rows in flight: the lane's own dwords, the edge dwords
    auto issue_load = [&](int i, V (&d)[ND], V (&e)[NE]) {
        int y = R0 - 2 + i;
        y = y < 0 ? 0 : (y > rows - 1 ? rows - 1 : y);
        const uint32_t soff = (uint32_t)y * (uint32_t)a.stride;
        // the edge load first: the wait for the row's own dwords then covers it.  Fenced: left alone, the scheduler sorts the
        // prologue's loads by width, the loop's first wait must then assume the worst of both orders, and every group of rows
        // begins by draining the queue
        if (CH == 3) {
            buf_load_u32x2(src_buf, edge_off, soff, e[0], e[1 % NE]);
            buf_load_u32x3(src_buf, row_off, soff, d[0], d[1 % ND], d[2 % ND]);
        } else {
            e[0] = buf_load_u32(src_buf, edge_off, soff);
            d[0] = buf_load_u32(src_buf, row_off, soff);
        }
        sched_fence();
    };
    const int n_iter = R1 - R0 + 3; // source rows R0 - 2 .. R1
#pragma unroll
    for (int p = 0; p < SL_PREFETCH; ++p) issue_load(p, dq[p], de[p]);
    const int n_groups = (n_iter + 5) / 6;
    for (int grp = 0; grp < n_groups; ++grp) {
        const int i0 = grp * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int i = i0 + k, y = R0 - 2 + i;
            issue_load(i + SL_PREFETCH, dq[(k + SL_PREFETCH) % 6], de[(k + SL_PREFETCH) % 6]);
            const V d0 = dq[k][0], d1 = dq[k][1 % ND], d2 = dq[k][2 % ND], e0 = de[k][0], e1 = de[k][1 % NE];
            // ---- the retained copy: the lane's dwords as loaded ----
            const V koff = y >= own0 && y < R1 ? row_off : splat(BUF_DROP);
            if (CH == 3) buf_store_u32x3_nt(keep_buf, koff, (uint32_t)(y * cols * CH), d0, d1, d2);
            else buf_store_u32_nt(keep_buf, koff, (uint32_t)(y * cols * CH), d0);
            // ---- horizontal [1 4 6 4 1] at the lane's pixels 0 and 2: out_a = m2 + 4 m1 + 6 p0 + 4 p1 + p2,
            //      out_b = p0 + 4 p1 + 6 p2 + 4 p3 + n0, with m2, m1 the left neighbour's pixels 2, 3 and n0 the right one's pixel 0 ----
            if (CH == 3) {
                // bytes: d0 = b0 g0 r0 b1, d1 = g1 r1 b2 g2, d2 = r2 b3 g3 r3; of the left neighbour's dwords 1 and 2 (pd1: its b2 g2,
                // pd2: r2 b3 g3 r3) and the right one's dword 0 (nd0: b0 g0 r0) only those bytes are read
                V pd1 = select(is_l0, e0, from_left(d1)), pd2 = select(is_l0, e1, from_left(d2)), nd0 = select(is_l63, e0, from_right(d0));
                if (left_border) { // columns -2, -1 are columns 2, 1
                    pd1 = select(first, d1, pd1);
                    pd2 = select(first, perm(d2, perm(d1, d0, 0x0504030cu), 0x03020104u), pd2);
                }
                if (right_border) nd0 = select(last, perm(d2, d1, 0x0c040302u), nd0); // column cols is column cols - 2
                const V E[3] = {perm(d1, d0, 0x0c060c00u), perm(d1, d0, 0x0c070c01u), perm(d2, d0, 0x0c040c02u)};    // (p0, p2)
                const V O[3] = {perm(d2, d0, 0x0c050c03u), perm(d2, d1, 0x0c060c00u), perm(d2, d1, 0x0c070c01u)};    // (p1, p3)
                const V M2[3] = {perm(pd1, d0, 0x0c000c06u), perm(pd1, d0, 0x0c010c07u), perm(pd2, d0, 0x0c020c04u)}; // (m2, p0)
                const V M1[3] = {perm(pd2, d0, 0x0c030c05u), perm(pd2, d1, 0x0c000c06u), perm(pd2, d1, 0x0c010c07u)}; // (m1, p1)
                const V P2[3] = {perm(nd0, d1, 0x0c040c02u), perm(nd0, d1, 0x0c050c03u), perm(nd0, d2, 0x0c060c00u)}; // (p2, n0)
#pragma unroll
                for (int c = 0; c < CH; ++c) // halves stay below 2^16: plain 32-bit adds
                    hw[k][c] = pk_mad(E[c % 3], QS_K(6, 6), pk_mad(M1[c % 3] + O[c % 3], K4, M2[c % 3] + P2[c % 3]));
            } else {
                V pd = select(is_l0, e0, from_left(d0)), nd = select(is_l63, e0, from_right(d0)); // pd: bytes 2, 3 = m2, m1; nd: byte 0 = n0
                if (left_border) pd = select(first, perm(d0, d0, 0x01020c0cu), pd);
                if (right_border) nd = select(last, perm(d0, d0, 0x0c0c0c02u), nd);
                const V E = perm(d0, d0, 0x0c020c00u), O = perm(d0, d0, 0x0c030c01u);
                const V M2 = perm(pd, d0, 0x0c000c06u), M1 = perm(pd, d0, 0x0c010c07u), P2 = perm(nd, d0, 0x0c040c02u);
                hw[k][0] = pk_mad(E, QS_K(6, 6), pk_mad(M1 + O, K4, M2 + P2));
            }
            sched_fence();
            if ((k & 1) != 0) continue; // i odd: y odd (the item's first loaded row R0 - 2 is even)
            // ---- cv::pyrDown row oy: the vertical [1 4 6 4 1] over source rows 2oy-2 .. 2oy+2 = item rows i-4 .. i ----
            const int oy = (y - 2) >> 1;
            const bool mine = oy >= (own0 >> 1) && oy < (R1 >> 1) && oy < drows;
            // REFLECT_101 at the top / bottom of the image folds taps onto rows inside the window: {0 0 6 8 2} in row 0 ({0 0 8 8 0}
            // when the image has two rows), {1 4 7 4 0} in the last row of an image of even height.  Scalar selects, not branches: a
            // join in front of the stores would make their wait counts those of the worst path
            const bool top = oy == 0, bot = !top && 2 * oy + 2 >= rows, two = top && rows == 2;
            const uint32_t wr[5] = {top ? 0u : 1u, top ? 0u : 4u, two ? 8u : (bot ? 7u : 6u), top ? 8u : 4u, top ? (two ? 0u : 2u) : (bot ? 0u : 1u)};
            V ob[CH]; // (out_a, out_b) per channel, bytes in the low half of each u16
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                V s = pk_mul(hw[(k + 2) % 6][c], wr[0] * 0x00010001u);
#pragma unroll
                for (int t = 1; t < 5; ++t) s = pk_mad(hw[(k + 2 + t) % 6][c], wr[t] * 0x00010001u, s);
                ob[c] = pk_lshr(s + QS_K(128, 128), 8);
            }
            const V poff = mine ? pyr_off : splat(BUF_DROP);
            const uint32_t prow = (uint32_t)(oy * dcols * CH);
            if (CH == 3) {
                // the lane's bytes (b_a g_a r_a b_b) (g_b r_b); an even lane adds its right neighbour's six
                const V A = perm(ob[2 % CH], perm(ob[1 % CH], ob[0], 0x020c0400u), 0x03040100u), B = perm(ob[2 % CH], ob[1 % CH], 0x0c0c0602u);
                const V nA = from_right(A), nB = from_right(B);
                buf_store_u32x3(pyr_buf, poff, prow, A, perm(nA, B, 0x05040100u), perm(nB, nA, 0x05040302u));
            } else {
                buf_store_u32(pyr_buf, poff, prow, perm(from_right(ob[0]), ob[0], 0x06040200u));
            }
            sched_fence();
        }
    }
}

template <int CH, bool PTRS = false>
__device__ __forceinline__ void source_lines_item(const QSArgs& a, int item)
{
    const int n_strips = sl_strips(a.cols);
    if (item >= n_strips * a.n_rblocks * a.frames) return;
    const SlItem it = sl_item(item, n_strips, a.frames);
    source_lines_wave<CH, PTRS>(a, it.strip, it.rb, it.frame);
}

#ifndef SBM_WAVE_EMU
// grid = ceil(work items / 4), block = 256 = four independent waves
template <int CH>
__global__ __launch_bounds__(256) void k_source_lines(const QSArgs a)
{
    const int item = (int)blockIdx.x * 4 + (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    source_lines_item<CH>(a, item);
}

// the table form
template <int CH>
__global__ __launch_bounds__(256) void k_source_lines_ptrs(const QSArgs a)
{
    const int item = (int)blockIdx.x * 4 + (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    source_lines_item<CH, true>(a, item);
}
#endif

} // namespace sbm
