// TEST INFRASTRUCTURE: the host pass of shape_based_matching_amd/csrc/sbm_verify_math.h (the verify stage's gray,
// min-max normalisation and normalised correlation), compiled by tests/test_verify_math.py into its temporary directory.
#include <stdint.h>

#include "sbm_verify_math.h"

using namespace sbm;

// n pixels of B, G, R bytes -> n gray bytes
extern "C" void sbm_emu_verify_gray(const uint8_t* bgr, int64_t n, uint8_t* out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = (uint8_t)verify_gray(bgr[3 * i], bgr[3 * i + 1], bgr[3 * i + 2]);
}

// the 256-entry table of every pair lo < hi, in the order (0,1), (0,2), ..., (254,255); and of lo == hi = 7 last
extern "C" int64_t sbm_emu_verify_tables(uint8_t* out)
{
    int64_t k = 0;
    for (int lo = 0; lo < 256; ++lo)
        for (int hi = lo + 1; hi < 256; ++hi, ++k)
            for (int g = 0; g < 256; ++g) out[k * 256 + g] = (uint8_t)verify_norm_entry(g, lo, hi);
    for (int g = 0; g < 256; ++g) out[k * 256 + g] = (uint8_t)verify_norm_entry(g, 7, 7);
    return k + 1;
}

extern "C" float sbm_emu_verify_score(uint64_t sab, uint64_t saa, uint64_t sbb) { return verify_score(sab, saa, sbb); }

extern "C" int sbm_emu_verify_keeps(float score, double min_corr) { return verify_keeps(score, min_corr) ? 1 : 0; }

extern "C" int sbm_emu_verify_inside(int x, int y, int w0, int h0, int rows, int cols) { return verify_roi_inside(x, y, w0, h0, rows, cols) ? 1 : 0; }

extern "C" uint64_t sbm_emu_verify_normalise(const uint8_t* gray, int w, int h, int64_t stride, uint8_t* out)
{
    return verify_normalise_image(gray, w, h, stride, out);
}

// a gray ROI against a RAW gray patch: the patch normalised as the upload does, then the ROI's score
extern "C" float sbm_emu_verify_pair(const uint8_t* roi, const uint8_t* patch, int w, int h, uint8_t* scratch)
{
    const uint64_t sbb = verify_normalise_image(patch, w, h, w, scratch);
    return verify_roi_score(roi, w, h, w, scratch, sbb);
}
