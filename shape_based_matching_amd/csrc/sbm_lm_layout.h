// sbm_lm_layout.h — where a cell of a refinement level lies in its two stored forms that are not row-major: the
// strip-interleaved plane of spread bytes (d_lmc, LM_SPREAD_STRIP) and the bit strips (d_lbits, LM_BIT_STRIPS).  Plain
// integer code, no HIP types: the builders (sbm_lm_kernels.h), the readers and the host use it,
// tests/test_lm_form_cases.py compiles it for the CPU suite.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBM_LML_HD __host__ __device__ __forceinline__
#else
#define SBM_LML_HD inline
#endif

namespace sbm {

// Strip-interleaved compact plane of a refinement-only level (needs W % 16 == 0): inside sub-plane
// sub = (y%T)*T + x%T the W x H grid is cut into W/16 column strips of 16 cells, and a strip is stored row after
// row, 16 bytes per row:  offset = sub*W*H + ((gx / 16) * H + gy) * 16 + gx % 16.
// similarityLocal (line2Dup.cpp:860-922) reads 16 x 16 cells per feature; row-major that is 16 pieces of 16 bytes in
// 16 different 128-byte lines, here it is two runs of 256 contiguous bytes at most (one when gx % 16 == 0).
SBM_LML_HD int64_t lm_strip_offset(int sub, int gy, int gx, int W, int H)
{
    return (int64_t)sub * W * H + ((int64_t)(gx >> 4) * H + gy) * 16 + (gx & 15);
}

// Bit strips of a T = 4 level (built by build_lm_strip4_allty<true>, read by k_similarity_local_bits, sbm_local_bits.h):
// per (sub-plane, orientation o, strip of 16 columns, grid row) one dword = "response > 0" bits of the 16 cells (spread
// bits o-1, o, o+1) in the low half, "response == 4" bits (spread bit o) in the high half:
//     dword index = ((sub * 8 + o) * (W / 16) + strip) * H + gy            (2 bytes per pixel, zero tail behind)
// with plane = sub * 8 + o.
SBM_LML_HD int64_t lm_bits_offset(int plane, int strip, int gy, int W, int H)
{
    return ((int64_t)plane * (W >> 4) + strip) * H + gy;
}
// dwords of a level stored as bit strips, without the zero tail
SBM_LML_HD int64_t lm_bits_dwords(int W, int H) { return (int64_t)128 * (W >> 4) * H; }

} // namespace sbm
