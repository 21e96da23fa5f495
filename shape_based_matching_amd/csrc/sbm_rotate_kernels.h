// sbm_rotate_kernels.h — rotated template families on the device (gfx950): Detector::addTemplate_rotate
// (line2Dup.cpp:1395-1451) for every (angle, base) pair of a call, one workgroup per pair in the shape of k_train_crop.
// The scalar rule is sbm_rotate_math.h's, which the CPU test walks in the same two passes; the host side
// (sbm_train_rotate_device) is in sbm_capi_train.inc.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sbm.h"
#include "sbm_rotate_math.h"

namespace sbm {

// grid (n_thetas, min(n_bases, 65535)); pair p = b * n_thetas + k writes levels[p * L ...], status[2p], status[2p + 1]
// and the block [out_first + k * out_cap, + out_cap) of feats.  `bases` and `angles` are indexed by blockIdx only, so
// a record is wave-uniform.
//   pass 1: every feature of every level rotated and written uncropped into the pair's block; the pair's min / max of
//           x * 2^level, y * 2^level reduced through LDS atomics; a feature outside the domain raises a flag
//   pass 2: behind a barrier the same threads subtract the level's tl from what they wrote; level records and status
__global__ __launch_bounds__(256) void k_train_rotate(const sbm_rotate_base* __restrict__ bases, const RotateAngle* __restrict__ angles, int L, int n_bases,
                                                      sbm_template_level* __restrict__ levels, sbm_train_feature* __restrict__ feats,
                                                      int32_t* __restrict__ status)
{
    __shared__ int s_mm[4];
    __shared__ int s_bad;
    const int k = blockIdx.x, n_thetas = gridDim.x, tid = threadIdx.x;
    const RotateAngle ang = angles[k];
    for (int b = blockIdx.y; b < n_bases; b += gridDim.y) {
        const sbm_rotate_base& base = bases[b];
        const int64_t pair = (int64_t)b * n_thetas + k;
        sbm_template_level* __restrict__ out_levels = levels + pair * L;
        sbm_train_feature* __restrict__ out = feats + base.out_first + (int64_t)k * base.out_cap;
        RotateVerdict v = rotate_base_verdict(base.status, base.levels, L, base.out_cap);
        if (v.code == ROTATE_OK) {
            if (tid == 0) {
                s_mm[0] = s_mm[1] = INT32_MAX;
                s_mm[2] = s_mm[3] = INT32_MIN;
                s_bad = 0;
            }
            __syncthreads();
            int mn_x = INT32_MAX, mn_y = INT32_MAX, mx_x = INT32_MIN, mx_y = INT32_MIN;
            bool bad = false;
            int64_t off = 0;
            for (int l = 0; l < L; ++l) {
                const sbm_template_level lv = base.levels[l];
                const sbm_train_feature* __restrict__ in = base.feats + lv.feature_offset;
                const float cx = rotate_center_at(base.center_x, l), cy = rotate_center_at(base.center_y, l);
                for (int j = tid; j < lv.n_features; j += 256) {
                    sbm_train_feature g;
                    if (!rotate_feature(in[j], lv.tl_x, lv.tl_y, cx, cy, ang, &g)) {
                        bad = true;
                        continue;
                    }
                    out[off + j] = g;
                    const int x = rotate_scaled(g.x, l), y = rotate_scaled(g.y, l);
                    mn_x = min(mn_x, x), mn_y = min(mn_y, y), mx_x = max(mx_x, x), mx_y = max(mx_y, y);
                }
                off += lv.n_features;
            }
            atomicMin(&s_mm[0], mn_x);
            atomicMin(&s_mm[1], mn_y);
            atomicMax(&s_mm[2], mx_x);
            atomicMax(&s_mm[3], mx_y);
            if (bad) atomicOr(&s_bad, 1);
            __syncthreads();
            if (s_bad) {
                v.code = ROTATE_NOT_ROTATABLE;
                v.value = ROTATE_REASON_FEATURE;
            }
        }
        if (v.code == ROTATE_OK) {
            const int min_x = train_crop_even(s_mm[0]), min_y = train_crop_even(s_mm[1]);
            int64_t off = 0;
            for (int l = 0; l < L; ++l) {
                const int nl = base.levels[l].n_features;
                const TrainBox box = train_crop_level(min_x, min_y, s_mm[2], s_mm[3], l);
                if (tid == 0) {
                    sbm_template_level t;
                    t.width = box.width;
                    t.height = box.height;
                    t.tl_x = box.tl_x;
                    t.tl_y = box.tl_y;
                    t.pyramid_level = l;
                    t.n_features = nl;
                    t.feature_offset = off;
                    out_levels[l] = t;
                }
                for (int j = tid; j < nl; j += 256) { // the thread that wrote the feature
                    out[off + j].x -= box.tl_x;
                    out[off + j].y -= box.tl_y;
                }
                off += nl;
            }
        } else if (tid < L) {
            sbm_template_level z;
            z.width = z.height = z.tl_x = z.tl_y = z.pyramid_level = z.n_features = 0;
            z.feature_offset = 0;
            out_levels[tid] = z;
        }
        if (tid == 0) {
            status[2 * pair] = v.code;
            status[2 * pair + 1] = v.value;
        }
        __syncthreads(); // the next base of this workgroup reuses the LDS words
    }
}

} // namespace sbm
