// TEST INFRASTRUCTURE: fastAtan2 in degrees (cv::phase) evaluated element by element in two forms, for
// tests/test_gradient_spec.py: `fused` = 0 rounds every multiply and add on its own (OpenCV's scalar and SSE paths,
// the oracle, the HIP kernels); `fused` = 1 evaluates the polynomial with fmaf as OpenCV's AVX2 dispatch does
// (v_fma in v_atan_f32).  Built with -ffp-contract=off so that only the explicit fmaf calls fuse.
#include <cfloat>
#include <cmath>
#include <cstdint>

namespace {
const float kDeg = (float)(180.0 / 3.14159265358979323846);
const float kP1 = 0.9997878412794807f * kDeg, kP3 = -0.3258083974640975f * kDeg, kP5 = 0.1555786518463281f * kDeg,
            kP7 = -0.04432655554792128f * kDeg;

inline float atan_deg(float y, float x, bool fused)
{
    const float ax = std::fabs(x), ay = std::fabs(y);
    const float c = std::fmin(ax, ay) / (std::fmax(ax, ay) + (float)DBL_EPSILON);
    const float cc = c * c;
    float a;
    if (fused) {
        a = std::fmaf(std::fmaf(std::fmaf(cc, kP7, kP5), cc, kP3), cc, kP1) * c;
    } else {
        a = kP7 * cc;
        a = a + kP5;
        a = a * cc;
        a = a + kP3;
        a = a * cc;
        a = a + kP1;
        a = a * c;
    }
    if (!(ax >= ay)) a = 90.f - a;
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}
} // namespace

extern "C" void sbm_emu_fast_atan2(const float* y, const float* x, int64_t n, int fused, float* out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = atan_deg(y[i], x[i], fused != 0);
}
