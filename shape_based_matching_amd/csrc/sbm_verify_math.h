// sbm_verify_math.h — the arithmetic of the verify stage (sbm_verify_kernels.h): the gray of a pixel, the min-max
// normalisation of a gray image to 0..255 and the normalised correlation of two equally sized images.  Plain scalar code,
// host and device: tests/test_verify_math.py compiles the host pass for the CPU suite and checks it against a numpy
// restatement of the same rule.
//
// Reference: the HCORR stage of the production driver (test_jabil.cpp:152-207 of the reference): cvtColor(BGR2GRAY),
// cv::normalize(NORM_MINMAX, 0, 255, CV_8U) and matchTemplate(TM_CCORR_NORMED) on two images of one size, whose result
// map is one number.  The rule below restates those three OpenCV calls as closely as can be told without OpenCV at hand
// ("The verify stage", has its standing); it is the definition here.  Built with -ffp-contract=off
// -fno-fast-math: every float operation is rounded on its own and nothing is fused, so the device computes the host's bits.
#pragma once
#include <math.h>
#include <stdint.h>

namespace sbm {

#if defined(__HIPCC__)
#define SBM_VERIFY_HD __host__ __device__ __forceinline__
#else
#define SBM_VERIFY_HD inline
#endif

// records of a stage call: what a record's score slot holds when it could not be verified, and why (the flag bits of the
// frame's output pair, sbm.h)
constexpr int VERIFY_OK = 0, VERIFY_NO_PATCH = 4, VERIFY_OUTSIDE = 8;

// rule 1: cvtColor's fixed-point BGR -> gray (the expression of sbm_cvlite.h)
SBM_VERIFY_HD int verify_gray(int b, int g, int r) { return (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14; }

// rule 2: the coefficients of a gray image with minimum lo < maximum hi: scale and shift in double, applied in float
SBM_VERIFY_HD void verify_norm_coeffs(int lo, int hi, float* a, float* b)
{
    const double scale = 255.0 * (1.0 / (double)(hi - lo));
    const double shift = 0.0 - (double)lo * scale;
    *a = (float)scale;
    *b = (float)shift;
}

// ... and the value g becomes: one rounded multiply, one rounded add, round to nearest even, clamp to 0..255
SBM_VERIFY_HD int verify_norm_value(int g, float a, float b)
{
    const float t = (float)g * a;
    const float u = t + b;
    const float v = rintf(u);
    return v < 0.f ? 0 : (v > 255.f ? 255 : (int)v);
}

// ... as entry g of the 256-entry table of an image with extremes (lo, hi); a constant image becomes 0 everywhere
SBM_VERIFY_HD int verify_norm_entry(int g, int lo, int hi)
{
    if (hi == lo) return 0;
    float a, b;
    verify_norm_coeffs(lo, hi, &a, &b);
    return verify_norm_value(g, a, b);
}

// rule 3: the score from the three integer sums; every double operation the correctly rounded IEEE one
SBM_VERIFY_HD float verify_score(uint64_t sab, uint64_t saa, uint64_t sbb)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const double den = __dsqrt_rn(__dmul_rn((double)saa, (double)sbb));
    double q = den == 0.0 ? 0.0 : __ddiv_rn((double)sab, den);
#else
    const double den = sqrt((double)saa * (double)sbb);
    double q = den == 0.0 ? 0.0 : (double)sab / den;
#endif
    if (q > 1.0) q = 1.0;
    return (float)q;
}

// rule 4
SBM_VERIFY_HD bool verify_keeps(float score, double min_corr) { return (double)score >= min_corr; }

// rule 5: the ROI (x, y, w0, h0) of a record is wholly inside a frame of rows x cols pixels
SBM_VERIFY_HD bool verify_roi_inside(int x, int y, int w0, int h0, int rows, int cols)
{
    if (x < 0 || y < 0 || w0 <= 0 || h0 <= 0) return false;
    return (int64_t)x + w0 <= cols && (int64_t)y + h0 <= rows;
}

// ---- the host pass: what a workgroup of k_verify_rois does for one ROI, sequentially ----
// A w x h gray image (rows stride bytes apart) normalised by rule 2 into out (dense); returns the sum of its squares.
inline uint64_t verify_normalise_image(const uint8_t* gray, int w, int h, int64_t stride, uint8_t* out)
{
    int lo = 255, hi = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int g = gray[(int64_t)y * stride + x];
            lo = g < lo ? g : lo;
            hi = g > hi ? g : hi;
        }
    uint8_t tab[256];
    for (int g = 0; g < 256; ++g) tab[g] = (uint8_t)verify_norm_entry(g, lo, hi);
    uint64_t s = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const uint32_t n = tab[gray[(int64_t)y * stride + x]];
            out[(int64_t)y * w + x] = (uint8_t)n;
            s += n * n;
        }
    return s;
}

// The score of a gray ROI (w x h, rows stride bytes apart) against a normalised patch (dense) whose squares sum to sbb.
inline float verify_roi_score(const uint8_t* gray, int w, int h, int64_t stride, const uint8_t* patch, uint64_t sbb)
{
    int lo = 255, hi = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int g = gray[(int64_t)y * stride + x];
            lo = g < lo ? g : lo;
            hi = g > hi ? g : hi;
        }
    uint64_t sab = 0, saa = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const uint32_t n = (uint32_t)verify_norm_entry(gray[(int64_t)y * stride + x], lo, hi);
            sab += n * (uint32_t)patch[(int64_t)y * w + x];
            saa += n * n;
        }
    return verify_score(sab, saa, sbb);
}

} // namespace sbm
