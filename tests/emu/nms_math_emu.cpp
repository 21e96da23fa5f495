// TEST INFRASTRUCTURE: the host pass of shape_based_matching_amd/csrc/sbm_nms_math.h (the NMS stage's overlap, threshold
// and in-chunk resolution), compiled by tests/test_nms_math.py into its temporary directory.  The walk below is the
// kernel's (k_nms_frames, sbm_nms_kernels.h) with the wave's ballot replaced by a loop over the 64 lanes.
#include <stdint.h>

#include "sbm_nms_math.h"

using namespace sbm;

extern "C" float sbm_emu_nms_overlap(const int32_t* a, const int32_t* b)
{
    return nms_rect_overlap(a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]);
}

// boxes: n x (x, y, w, h) in walk order (already score-filtered and sorted); keep_out: the kept positions.  Returns their
// number.  Chunks of 64: every candidate's maximum overlap with the boxes kept in earlier chunks, the chunk's overlap
// matrix, then nms_resolve_chunk.
extern "C" int sbm_emu_nms_walk(const int32_t* boxes, int n, float nms_threshold, float eta, int32_t* keep_out)
{
    float thr = nms_threshold;
    int n_kept = 0;
    static float ov[64][64];
    for (int s = 0; s < n; s += 64) {
        const int cn = n - s < 64 ? n - s : 64;
        for (int i = 0; i < cn; ++i) {
            const int32_t* a = boxes + 4 * (s + i);
            float mx = 0.f;
            for (int k = 0; k < n_kept; ++k) {
                const int32_t* b = boxes + 4 * keep_out[k];
                const float o = nms_rect_overlap(a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]);
                mx = o > mx ? o : mx;
            }
            ov[i][i] = mx;
            for (int j = 0; j < i; ++j) {
                const int32_t* b = boxes + 4 * (s + j);
                ov[i][j] = nms_rect_overlap(a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]);
            }
        }
        const int nk0 = n_kept;
        const uint64_t km = nms_resolve_chunk(cn, &thr, eta, [&](int i, float t) {
            uint64_t m = 0;
            for (int j = 0; j <= i; ++j) {
                const bool v = (j == i && nk0 == 0) ? false : ov[i][j] > t;
                m |= (uint64_t)v << j;
            }
            return m;
        });
        for (int j = 0; j < cn; ++j)
            if ((km >> j) & 1) keep_out[n_kept++] = s + j;
    }
    return n_kept;
}
