// sbm_nms_math.h — the arithmetic of the NMS stage (sbm_nms_kernels.h): the overlap of two boxes, the adaptive threshold
// and the in-chunk greedy resolution.  Plain scalar code, host and device: tests/test_nms_math.py compiles the host pass
// for the CPU suite and checks it against the Python restatement of the reference (test_nms.py::py_nms), which
// tests/test_reference_nms.py pins, with this file's overlap bits and chunked walk, to the reference's own nms.hpp
// compiled as a test binary.
//
// Reference: include/nms.hpp (cv_dnn::NMSBoxes / rectOverlap, nms.hpp:21-96 of the reference), the step every caller runs
// after Detector::match (test.cpp:491, test_jabil.cpp:148).  Built with -ffp-contract=off -fno-fast-math: the double
// division is the IEEE one and nothing is fused, so the device computes the host's bits.
#pragma once
#include <stdint.h>

namespace sbm {

#if defined(__HIPCC__)
#define SBM_NMS_HD __host__ __device__ __forceinline__
#else
#define SBM_NMS_HD inline
#endif

// rectOverlap(a, b) of nms.hpp on cv::Rect(x, y, w, h): integer areas, integer intersection (empty when it has no
// extent), the Jaccard distance in double, 1 - (float)distance; 1 when both boxes are empty.
SBM_NMS_HD float nms_rect_overlap(int ax, int ay, int aw, int ah, int bx, int by, int bw, int bh)
{
    const int area_a = aw * ah, area_b = bw * bh;
    if (area_a + area_b <= 0) return 1.f;
    const int x1 = ax > bx ? ax : bx, y1 = ay > by ? ay : by;
    const int ax2 = ax + aw, bx2 = bx + bw, ay2 = ay + ah, by2 = by + bh;
    const int x2 = ax2 < bx2 ? ax2 : bx2, y2 = ay2 < by2 ? ay2 : by2;
    const double inter = (x2 <= x1 || y2 <= y1) ? 0.0 : (double)((x2 - x1) * (y2 - y1));
    const double distance = 1.0 - inter / ((double)(area_a + area_b) - inter);
    return 1.f - (float)distance;
}

// the threshold after a kept box (nms.hpp: `if (eta < 1 && threshold > 0.5) threshold *= eta;`)
SBM_NMS_HD float nms_next_threshold(float thr, float eta) { return (eta < 1.f && thr > 0.5f) ? thr * eta : thr; }

// The greedy walk over one chunk of n <= 64 candidates, in order.  over(i, t) returns the 64-bit mask of the j with
// overlap(candidate i, candidate j) > t for j < i, and in bit i whether candidate i overlaps some box kept in an EARLIER
// chunk by more than t (max overlap > t; "every overlap <= t" is "the maximum <= t").  Bits j > i are ignored.
// Candidate i is kept iff no kept candidate of the chunk and no earlier kept box suppresses it at the threshold of its
// turn; *thr is advanced after every kept candidate.  Returns the kept mask.  On the device over() is one ballot of the
// wave (lane j compares its column of the chunk's overlap matrix), on the host a loop: the same walk either way.
template <class Over>
SBM_NMS_HD uint64_t nms_resolve_chunk(int n, float* thr, float eta, Over over)
{
    uint64_t kept = 0;
    float t = *thr;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        if (i < n) {
            const uint64_t bit = (uint64_t)1 << i;
            if ((over(i, t) & (kept | bit)) == 0) {
                kept |= bit;
                t = nms_next_threshold(t, eta);
            }
        }
    }
    *thr = t;
    return kept;
}

} // namespace sbm
