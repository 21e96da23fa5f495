// TEST INFRASTRUCTURE: the dataflow of the rotation kernel (csrc/sbm_rotate_kernels.h, k_train_rotate) on the CPU, built
// from the scalar rule the kernel shares (csrc/sbm_rotate_math.h): the workgroup's 256 threads as a loop, the LDS
// atomics as plain min / max on four words.  tests/test_rotate_math.py compiles this file (-ffp-contract=off -Wall
// -Wextra -Werror) and checks it against the checker's add_template_rotate.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>

#include "sbm_rotate_math.h"

using namespace sbm;

namespace {
enum { THREADS = 256 };
}

extern "C" {

// One (base, angle) pair, as one workgroup of k_train_rotate makes it: out_levels[L], the pair's block `out` of out_cap
// records, status[2].  The verdict first, then pass 1 (rotate, write uncropped, reduce min / max, flag a feature
// outside the domain), then pass 2 (subtract the level's tl, level records).
void sbm_emu_train_rotate(const sbm_template_level* levels, const sbm_train_feature* feats, const int32_t* base_status, int L, float center_x, float center_y,
                          float theta, int64_t out_cap, sbm_template_level* out_levels, sbm_train_feature* out, int32_t* status)
{
    const RotateAngle ang = rotate_angle(theta);
    RotateVerdict v = rotate_base_verdict(base_status, levels, L, out_cap);
    int s_mm[4] = {INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN};
    int s_bad = 0;
    if (v.code == ROTATE_OK) {
        for (int tid = 0; tid < THREADS; ++tid) {
            int64_t off = 0;
            for (int l = 0; l < L; ++l) {
                const sbm_template_level lv = levels[l];
                const sbm_train_feature* in = feats + lv.feature_offset;
                const float cx = rotate_center_at(center_x, l), cy = rotate_center_at(center_y, l);
                for (int j = tid; j < lv.n_features; j += THREADS) {
                    sbm_train_feature g;
                    if (!rotate_feature(in[j], lv.tl_x, lv.tl_y, cx, cy, ang, &g)) {
                        s_bad |= 1;
                        continue;
                    }
                    out[off + j] = g;
                    const int x = rotate_scaled(g.x, l), y = rotate_scaled(g.y, l);
                    s_mm[0] = std::min(s_mm[0], x), s_mm[1] = std::min(s_mm[1], y);
                    s_mm[2] = std::max(s_mm[2], x), s_mm[3] = std::max(s_mm[3], y);
                }
                off += lv.n_features;
            }
        }
        if (s_bad) {
            v.code = ROTATE_NOT_ROTATABLE;
            v.value = ROTATE_REASON_FEATURE;
        }
    }
    if (v.code == ROTATE_OK) {
        const int min_x = train_crop_even(s_mm[0]), min_y = train_crop_even(s_mm[1]);
        int64_t off = 0;
        for (int l = 0; l < L; ++l) {
            const int nl = levels[l].n_features;
            const TrainBox box = train_crop_level(min_x, min_y, s_mm[2], s_mm[3], l);
            sbm_template_level t;
            t.width = box.width;
            t.height = box.height;
            t.tl_x = box.tl_x;
            t.tl_y = box.tl_y;
            t.pyramid_level = l;
            t.n_features = nl;
            t.feature_offset = off;
            out_levels[l] = t;
            for (int tid = 0; tid < THREADS; ++tid)
                for (int j = tid; j < nl; j += THREADS) {
                    out[off + j].x -= box.tl_x;
                    out[off + j].y -= box.tl_y;
                }
            off += nl;
        }
    } else {
        memset(out_levels, 0, (size_t)L * sizeof(sbm_template_level));
    }
    status[0] = v.code;
    status[1] = v.value;
}

// the host's verdict on an angle and on a centre component, and the angle table's entry
int sbm_emu_rotate_theta_ok(float theta) { return rotate_theta_ok(theta) ? 1 : 0; }
int sbm_emu_rotate_center_ok(float c) { return rotate_center_ok(c) ? 1 : 0; }
void sbm_emu_rotate_angle(float theta, double* cs, double* sn)
{
    const RotateAngle a = rotate_angle(theta);
    *cs = a.cs;
    *sn = a.sn;
}
int sbm_emu_rotate_wrap_steps(void) { return ROTATE_WRAP_STEPS; }

} // extern "C"
