// sbm_source_lines_plan.h — the index arithmetic of the line-shaped source pass k_source_lines (sbm_source_lines.h): when a
// caller's layout admits it, which (strip, row block, frame) a work item names, which rows it loads and which it owns, where a
// lane's bytes of the retained copy and of cv::pyrDown go, and where the two edge lanes find the neighbour pixels of their
// strip.  Plain integer code, no HIP types: the kernel and the host use it, tests/test_source_pass.py compiles it for the CPU
// suite.
//
// A WAVE owns a strip of SL_STRIP = 256 source columns, 4 per lane and no halo lanes, of `hs` rows of one frame.  Per row it
// moves 768 contiguous bytes of BGR (256 of gray): one 96-bit (32-bit) load and one streamed store of the same width per lane.
// Per cv::pyrDown row it writes 384 (128) contiguous bytes: the EVEN lanes store their own two output pixels and their right
// neighbour's as three dwords (one).  The last strip of a row may be cut; cols % 64 == 0 makes the cut a whole number of
// 16-lane groups, so a pair of lanes is never split and every offset below is a multiple of 4.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBM_SL_HD __host__ __device__ __forceinline__
#else
#define SBM_SL_HD inline
#endif

namespace sbm {

constexpr int SL_STRIP = 256;  // source columns of a strip
constexpr int SL_LANE_PX = 4;  // ... of a lane
constexpr int64_t SL_MAX_FRAME_BYTES = 0x7ff00000ll; // a frame's bytes in the caller's layout: lane offsets are 32-bit, BUF_DROP lies above

// The selection rule.  base: the address of frame 0's first pixel; stride: bytes per row; frame_stride: bytes from one frame
// to the next (ignored for a single frame).  The dword loads need every row of every frame on a 4-byte boundary, the lane
// offsets a frame that fits 31 bits, the lane pairs of cv::pyrDown a width of whole 16-lane groups; rows and rows per item are
// even in every launch of the source pass (the present form asks the same).
SBM_SL_HD bool source_lines_ok(uint64_t base, int64_t stride, int64_t frame_stride, int frames, int rows, int cols, int ch)
{
    if ((ch != 1 && ch != 3) || rows < 2 || (rows & 1) || cols < 64 || (cols & 63) || frames < 1) return false;
    if (stride < (int64_t)cols * ch || (base & 3) || (stride & 3)) return false;
    if (frames > 1 && (frame_stride & 3)) return false;
    return (rows - 1) * stride + (int64_t)cols * ch < SL_MAX_FRAME_BYTES;
}

// Whether a work item of the source pass (either form) stores its rows of the retained copy.  enqueued: match calls the host has
// fully enqueued on the context, this one included once its enqueue has ended; executed: calls whose launches up to the
// linear-memory builder have run -- every call before this one.  The copy's readers need the copy of the
// last call enqueued only, so a call keeps its copy unless a later one has been enqueued behind it.  A stale low `enqueued` keeps
// once too often; the word never runs ahead.  The counters wrap: the difference is what counts.
SBM_SL_HD bool source_pass_retains(uint32_t enqueued, uint32_t executed) { return (int32_t)(enqueued - executed) <= 1; }

// bytes of one frame that the pass may load: the buffer the lane offsets are checked against
SBM_SL_HD uint32_t sl_frame_bytes(int rows, int cols, int ch, int stride) { return (uint32_t)((int64_t)(rows - 1) * stride + (int64_t)cols * ch); }

SBM_SL_HD int sl_strips(int cols) { return (cols + SL_STRIP - 1) / SL_STRIP; }
SBM_SL_HD int sl_row_blocks(int row_lo, int row_hi, int hs) { return (row_hi - row_lo + hs - 1) / hs; }
SBM_SL_HD int sl_items(int cols, int n_rblocks, int frames) { return sl_strips(cols) * n_rblocks * frames; }

// Work item order: row block slowest, then frame, then strip -- the order of quantize_stream_item, for its reason (a CU's
// resident workgroups come from different regions of the image).
struct SlItem {
    int strip, rb, frame;
};
SBM_SL_HD SlItem sl_item(int item, int n_strips, int frames)
{
    const int per_rb = n_strips * frames, rb = item / per_rb, r = item - rb * per_rb;
    return SlItem{r % n_strips, rb, r / n_strips};
}

// Rows of a work item.  It LOADS source rows r0 - 2 .. r1 (clamped to the image) with r1 - r0 = min(hs, row_hi - row_lo) for
// every item of a launch: the last block is moved up to end at row_hi.  It OWNS rows [own0, r1) -- the rows of the block above
// that a moved block passes again are stored by that block alone, so every byte of a launch is written once.
struct SlRows {
    int r0, r1, own0;
};
SBM_SL_HD SlRows sl_rows(int rb, int hs, int row_lo, int row_hi)
{
    SlRows r;
    r.own0 = row_lo + rb * hs;
    r.r0 = r.own0;
    if (r.r0 + hs > row_hi) r.r0 = row_hi - row_lo > hs ? row_hi - hs : row_lo;
    r.r1 = r.r0 + hs < row_hi ? r.r0 + hs : row_hi;
    return r;
}

// first column of a lane; the lane is cut when it is not below cols
SBM_SL_HD int sl_lane_col(int strip, int lane) { return strip * SL_STRIP + lane * SL_LANE_PX; }
// byte offset of the lane's 4 pixels in a row, source or packed copy (4 * ch bytes); -1: cut
SBM_SL_HD int64_t sl_row_off(int strip, int lane, int cols, int ch) { return sl_lane_col(strip, lane) < cols ? (int64_t)sl_lane_col(strip, lane) * ch : -1; }
// byte offset in a cv::pyrDown row of the 4 * ch bytes an EVEN lane stores (its two pixels and its right neighbour's); -1: the
// lane stores nothing
SBM_SL_HD int64_t sl_pyr_off(int strip, int lane, int cols, int ch)
{
    return (lane & 1) == 0 && sl_lane_col(strip, lane) < cols ? (int64_t)(sl_lane_col(strip, lane) >> 1) * ch : -1;
}
// The horizontal [1 4 6 4 1] of a strip reaches 2 pixels to its left and 1 to its right.  Lane 0 loads the 8 (gray: 4) bytes that
// END at the strip's first byte -- the dwords a left neighbour lane would hand over --, lane 63 the 8 (4) bytes that BEGIN behind
// its last one.  Byte offsets in the source row; -1: the strip touches the image border there (REFLECT_101 folds the taps onto
// the lane's own pixels) or is cut, and nothing is loaded.
SBM_SL_HD int sl_edge_bytes(int ch) { return ch == 3 ? 8 : 4; }
SBM_SL_HD int64_t sl_edge_left(int strip, int ch) { return strip > 0 ? (int64_t)strip * SL_STRIP * ch - sl_edge_bytes(ch) : -1; }
SBM_SL_HD int64_t sl_edge_right(int strip, int cols, int ch) { return (strip + 1) * SL_STRIP < cols ? (int64_t)(strip + 1) * SL_STRIP * ch : -1; }

} // namespace sbm
