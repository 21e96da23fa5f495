// sbm_rotate_math.h — the scalar rule of batched template rotation (sbm_rotate_kernels.h): Detector::addTemplate_rotate
// (line2Dup.cpp:1395-1451) with every rounding step kept, the angle table the host makes for the kernel, the domain in
// which the rule's wrap loops end, and the verdict on a base before any of its features is read.  Plain C++, host and
// device: tests/test_rotate_math.py compiles the host pass (tests/emu/train_rotate_emu.cpp walks the kernel's two passes
// with these functions) and checks it against the checker's add_template_rotate, bit for bit.  The crop arithmetic is
// sbm_train_math.h's.  References are file:line of the reference's line2Dup.cpp.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sbm.h"
#include "sbm_train_math.h"

namespace sbm {

// ---- the domain ---------------------------------------------------------------------------------------------------------
// The wrap of the orientation is two `while` loops on a float (:1435-1436).  They end, and every intermediate fits its
// type, where |theta| <= 36000, a base feature's theta lies in [-720, 720], a centre component in [-65536, 65536] and
// a base coordinate (feature + tl) in 0 .. 32767.  Then |f.theta - theta| <= 36720 = 102 * 360, so either loop takes at
// most 102 steps and one more covers the rounding of the steps themselves: ROTATE_WRAP_STEPS.  A rotated coordinate
// is below 2^18 in magnitude and its level-0 equivalent below 2^25.
#define SBM_ROTATE_THETA_MAX 36000.0f
#define SBM_ROTATE_FEATURE_THETA_MAX 720.0f
#define SBM_ROTATE_CENTER_MAX 65536.0f
enum { ROTATE_COORD_MAX = 32767, ROTATE_LEVEL_FEATURES_MAX = 8191, ROTATE_WRAP_STEPS = 103 };

// status[0] of a pair, and status[1] where status[0] is ROTATE_NOT_ROTATABLE
enum { ROTATE_OK = 0, ROTATE_BASE_FAILED = 1, ROTATE_CAPACITY = 2, ROTATE_NOT_ROTATABLE = 3 };
enum {
    ROTATE_REASON_BASE_STATUS = 1, // the base's status pair says its features overflowed their block (or is no status)
    ROTATE_REASON_COUNT = 2,       // no feature at all, or a level's n_features outside 0 .. 8191
    ROTATE_REASON_FEATURE = 3      // a feature outside the domain above
};

// a NaN fails either comparison, an infinity one of them
SBM_TRAIN_HD bool rotate_in_range(float v, float bound) { return v >= -bound && v <= bound; }
SBM_TRAIN_HD bool rotate_theta_ok(float theta) { return rotate_in_range(theta, SBM_ROTATE_THETA_MAX); }
SBM_TRAIN_HD bool rotate_center_ok(float c) { return rotate_in_range(c, SBM_ROTATE_CENTER_MAX); }

// ---- the angle: once per theta, on the host ---------------------------------------------------------------------------------
// ang = -theta / 180 * CV_PI (:1428): a float division, then a double product.  cos and sin are the host library's;
// the kernel takes them from a table and never computes them, so the result does not depend on a device libm.
struct RotateAngle {
    double cs, sn;
    float theta;
    int32_t reserved;
};
inline RotateAngle rotate_angle(float theta)
{
    const double ang = -theta / 180 * 3.1415926535897932384626433832795; // CV_PI
    RotateAngle a;
    a.cs = cos(ang);
    a.sn = sin(ang);
    a.theta = theta;
    a.reserved = 0;
    return a;
}

// the centre of level l: halved cumulatively as a float (:1422)
SBM_TRAIN_HD float rotate_center_at(float c, int level)
{
    for (int l = 0; l < level; ++l) c /= 2;
    return c;
}

// a float quotient rounded to nearest, whatever the device's default division is
SBM_TRAIN_HD float rotate_div(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// ---- one feature (:1424-1442) -------------------------------------------------------------------------------------------
// f of a level whose template has (tl_x, tl_y), about the level's centre (cx, cy).  False, with *g untouched, where the
// feature is outside the domain or a wrap loop has not ended within its bound.  Products and sums of the rotation are
// rounded one by one (no fused multiply-add), each as a double, then the pair to float (rotate2d, :1395-1402).
SBM_TRAIN_HD bool rotate_feature(const sbm_train_feature& f, int tl_x, int tl_y, float cx, float cy, const RotateAngle& a, sbm_train_feature* g)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int64_t ax = (int64_t)f.x + tl_x, ay = (int64_t)f.y + tl_y;
    if (ax < 0 || ax > ROTATE_COORD_MAX || ay < 0 || ay > ROTATE_COORD_MAX) return false;
    if (!rotate_in_range(f.theta, SBM_ROTATE_FEATURE_THETA_MAX)) return false;
    const float px = (float)(int)ax, py = (float)(int)ay;
    const float qx = px - cx, qy = py - cy;
    const double cqx = a.cs * (double)qx, sqy = a.sn * (double)qy, sqx = a.sn * (double)qx, cqy = a.cs * (double)qy;
    float rx = (float)(cqx - sqy);
    float ry = (float)(sqx + cqy);
    rx = rx + cx;
    ry = ry + cy;
    float t = f.theta - a.theta;
    int steps = 0;
    while (t > 360 && steps < ROTATE_WRAP_STEPS) t -= 360, ++steps;
    if (t > 360) return false;
    steps = 0;
    while (t < 0 && steps < ROTATE_WRAP_STEPS) t += 360, ++steps;
    if (t < 0) return false;
    g->x = (int)(rx + 0.5f); // truncates toward zero (:1431)
    g->y = (int)(ry + 0.5f);
    g->theta = t;
    g->label = (int)(rotate_div(t * 16, 360) + 0.5f) & 7;
    return true;
}

// x << level of cropTemplates (:129) for a coordinate that may be negative
SBM_TRAIN_HD int rotate_scaled(int v, int level) { return v * (1 << level); }

// ---- the verdict on a base, from its status pair and its level records alone ------------------------------------------------
// {ROTATE_OK, features} | {ROTATE_BASE_FAILED, level} | {ROTATE_CAPACITY, features} | {ROTATE_NOT_ROTATABLE, reason}.
// The level records of a base whose training did not succeed are not read: training zeroes them.
struct RotateVerdict {
    int32_t code, value;
};
SBM_TRAIN_HD RotateVerdict rotate_base_verdict(const int32_t* base_status, const sbm_template_level* levels, int n_levels, int64_t out_cap)
{
    RotateVerdict v;
    if (base_status && base_status[0] != 0) {
        const bool failed = base_status[0] == 1;
        v.code = failed ? ROTATE_BASE_FAILED : ROTATE_NOT_ROTATABLE;
        v.value = failed ? base_status[1] : ROTATE_REASON_BASE_STATUS;
        return v;
    }
    int64_t total = 0;
    bool bad = false;
    for (int l = 0; l < n_levels; ++l) {
        const int n = levels[l].n_features;
        bad = bad || n < 0 || n > ROTATE_LEVEL_FEATURES_MAX;
        total += n;
    }
    if (bad || total == 0) {
        v.code = ROTATE_NOT_ROTATABLE;
        v.value = ROTATE_REASON_COUNT;
    } else if (total > out_cap) {
        v.code = ROTATE_CAPACITY;
        v.value = (int32_t)total;
    } else {
        v.code = ROTATE_OK;
        v.value = (int32_t)total;
    }
    return v;
}

} // namespace sbm
