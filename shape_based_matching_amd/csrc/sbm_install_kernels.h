// sbm_install_kernels.h — the kernels of sbm_upload_templates_device (gfx950): trained pyramids that lie in device memory
// become the context's template tables without a feature crossing to the host.
//
//   k_install_scan      one workgroup strides over the pyramids of all sources: which are kept (status, level counts and
//                       ranges), their template index and feature base by a prefix sum with a carry between the chunks of
//                       256, the level records, class and template_id of the kept ones (the records step is folded in)
//   k_install_features  one workgroup per (kept template, level): bounds, the packed tables, the level's extent, and the
//                       class-sorted copies by a two-pass counting sort that reproduces sbm_upload_templates' host loop
//
// The scalar rules are sbm_install_math.h's, the tables' layout sbm_install_plan.h's.  Every loop ends on a count read from
// a record and clamped (install_clamp_nf) or on the call's own sizes; no kernel waits for another workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sbm_common.h"
#include "sbm_install_math.h"
#include "sbm_install_plan.h"

namespace sbm {

// lanes below this one whose bit is set in a wave's ballot
__device__ __forceinline__ uint32_t install_rank_below(uint64_t ballot)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ uint32_t install_wave_scan(uint32_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

// n_pyramids pyramids, flat over the sources.  Outputs at the kept pyramid's template index t: items[t], tls[t * L ..],
// d_class[t], d_tid[t]; per pyramid index[j] = t or -1; the header's counts.  src_kept arrives zeroed, the header with
// empty verdicts.  A kept pyramid with a faulty level record is reported and then treated as skipped, so that nothing
// downstream follows its counts; the host discards the whole call on the report.
__global__ __launch_bounds__(256) void k_install_scan(const InstallSource* __restrict__ src, int n_sources, int n_pyramids, int L, InstallHeader* hdr,
                                                      int32_t* __restrict__ index, InstallItem* __restrict__ items, int32_t* src_t0, int32_t* src_kept,
                                                      int32_t* src_base, DevTL* __restrict__ tls, int32_t* __restrict__ d_class, int32_t* __restrict__ d_tid)
{
    __shared__ uint32_t s_wk[4], s_wf[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int32_t carry_k = 0; // kept pyramids and their features in the chunks before this one (the same in every thread)
    int64_t carry_f = 0;
    for (int base = 0; base < n_pyramids; base += INSTALL_CHUNK) {
        const int j = base + tid;
        bool kept = false;
        uint32_t nfsum = 0;
        int s = 0, i = 0;
        const sbm_template_level* lv = nullptr;
        if (j < n_pyramids) {
            s = install_source_of(src, n_sources, j);
            i = j - src[s].pyr_first;
            lv = src[s].levels + (int64_t)i * L;
            kept = install_keeps(src[s].status ? src[s].status[2 * (int64_t)i] : 0);
            if (kept) {
                const int64_t cap = src[s].feat_cap;
                for (int l = 0; l < L; ++l) {
                    const int fault = install_level_fault(lv[l].n_features, lv[l].feature_offset, cap);
                    if (fault) {
                        atomicMin((unsigned long long*)&hdr->level_verdict, (unsigned long long)install_level_verdict(j, L, l, fault));
                        kept = false;
                        break;
                    }
                    nfsum += (uint32_t)lv[l].n_features;
                }
            }
        }
        // the chunk's exclusive prefix of (kept, features): ballot and scan inside the wave, the waves' totals through LDS
        const uint64_t m = __ballot(kept);
        const uint32_t mine = kept ? nfsum : 0u;
        const uint32_t finc = install_wave_scan(mine, lane);
        if (lane == 63) {
            s_wk[w] = (uint32_t)__popcll(m);
            s_wf[w] = finc;
        }
        __syncthreads();
        uint32_t kb = 0, fb = 0, kt = 0, ft = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            if (v < w) kb += s_wk[v], fb += s_wf[v];
            kt += s_wk[v], ft += s_wf[v];
        }
        const int32_t t = carry_k + (int32_t)(kb + install_rank_below(m));
        if (j < n_pyramids) {
            index[j] = kept ? t : -1;
            if (i == 0) src_t0[s] = t; // kept pyramids in front of the source
            if (kept) {
                InstallItem it;
                it.levels = lv;
                it.feats = src[s].feats + (src[s].feat_first + (int64_t)i * src[s].feat_pitch);
                it.pyramid = j;
                it.source = s;
                items[t] = it;
                int64_t f = carry_f + (int64_t)(fb + finc - mine);
                for (int l = 0; l < L; ++l) {
                    DevTL d;
                    d.width = lv[l].width;
                    d.height = lv[l].height;
                    d.nf = lv[l].n_features;
                    d.feat_off = (int32_t)f; // 2^31 - 1 features or more: the host refuses the call before anything reads this
                    tls[(int64_t)t * L + l] = d;
                    f += lv[l].n_features;
                }
                d_class[t] = src[s].class_idx;
                atomicAdd(&src_kept[s], 1);
            }
        }
        carry_k += (int32_t)kt;
        carry_f += (int64_t)ft;
        __syncthreads(); // the waves' totals are rewritten by the next chunk
    }
    // template_id: kept pyramids of the class in the sources before this one, then the kept ones before it in its own.
    // Sources are few (one per producer call, base or image), so every source sums over the ones before it.
    __syncthreads();
    for (int s = tid; s < n_sources; s += INSTALL_CHUNK) {
        const int32_t cls = src[s].class_idx;
        int32_t before = 0;
        for (int u = 0; u < s; ++u)
            if (src[u].class_idx == cls) before += __hip_atomic_load(&src_kept[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (counted by atomics)
        src_base[s] = before;
    }
    __syncthreads();
    for (int j = tid; j < n_pyramids; j += INSTALL_CHUNK) {
        const int32_t t = index[j];
        if (t < 0) continue;
        const int s = items[t].source;
        d_tid[t] = src_base[s] + (t - src_t0[s]);
    }
    if (tid == 0) {
        hdr->n_kept = carry_k;
        hdr->total_features = carry_f;
    }
}

struct InstallGeo {
    int32_t log2t[SBM_MAX_LEVELS]; // install_log2t of every level's T
};

// One feature of the chunk a thread holds: packed position, label, class (0 where the level is not sorted)
struct InstallFeat {
    uint32_t xy;
    int32_t label;
    int k;
    bool ok;
};
// The record of a lane in one load.  The address comes out of a table, which makes it a generic pointer (flat_load, a 64-bit
// address per lane); it is device memory by the call's contract, so the load is a global one (as wv::load_u32_global).  Records
// are 16 bytes but only dword-aligned by their type; theta's dword is dead, and the compiler may leave it out of the load.
typedef int32_t install_i32x4 __attribute__((ext_vector_type(4)));
typedef install_i32x4 __attribute__((aligned(4))) install_i32x4_a4;
__device__ __forceinline__ InstallFeat install_load(const sbm_train_feature* __restrict__ src, int i, int log2t)
{
    const install_i32x4 v = *((__attribute__((address_space(1))) const install_i32x4_a4*)src + i);
    sbm_train_feature f;
    f.x = v.x, f.y = v.y, f.label = v.z;
    InstallFeat r;
    r.ok = install_feature_ok(f.x, f.y, f.label);
    r.xy = install_pack_xy(f.x, f.y);
    r.label = f.label;
    r.k = log2t >= 0 ? install_class(r.xy, log2t) : 0;
    return r;
}

// grid: kept templates * L workgroups of 256.  tls, items: as k_install_scan left them.
__global__ __launch_bounds__(256) void k_install_features(const InstallItem* __restrict__ items, const DevTL* __restrict__ tls, int L, InstallGeo geo,
                                                          InstallHeader* hdr, uint32_t* __restrict__ fxy, uint8_t* __restrict__ flabel,
                                                          uint8_t* __restrict__ flevel, uint32_t* __restrict__ fxy_s, uint8_t* __restrict__ flabel_s,
                                                          uint16_t* __restrict__ fcls, uint32_t* __restrict__ fext)
{
    __shared__ uint32_t s_cnt[INSTALL_CLASSES];     // features per class
    __shared__ uint32_t s_run[INSTALL_CLASSES];     // where the class's next feature goes (the host loop's pos[])
    __shared__ uint32_t s_wcnt[4][INSTALL_CLASSES]; // a chunk's features per wave and class
    __shared__ uint32_t s_ext[2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t b = blockIdx.x;
    const int t = (int)(b / (uint32_t)L), l = (int)(b - (uint32_t)t * (uint32_t)L);
    const DevTL d = tls[b];
    const int nf = install_clamp_nf(d.nf);
    const int log2t = geo.log2t[l];
    const sbm_train_feature* __restrict__ src = items[t].feats + items[t].levels[l].feature_offset;
    const int64_t dst = d.feat_off;
    if (tid < INSTALL_CLASSES) s_cnt[tid] = 0;
    if (tid < 2) s_ext[tid] = 0;
    __syncthreads();

    // pass 1: bounds, the tables in the caller's order, the extent, the class counts
    uint32_t ext = 0, count = 0; // lane c of a wave counts the wave's features of class c
    for (int c0 = 0; c0 < nf; c0 += INSTALL_CHUNK) {
        const int i = c0 + tid;
        const bool valid = i < nf;
        InstallFeat f{0u, 0, 0, true};
        if (valid) {
            f = install_load(src, i, log2t);
            if (!f.ok) atomicMin(&hdr->feature_verdict, (uint32_t)(dst + i));
            fxy[dst + i] = f.xy;
            flabel[dst + i] = (uint8_t)f.label;
            flevel[dst + i] = (uint8_t)l;
            if (log2t < 0) { // never read sorted (the strip plane exists for T = 4 and 8 only): the copies keep the order
                fxy_s[dst + i] = f.xy;
                flabel_s[dst + i] = (uint8_t)f.label;
            }
            if (f.ok) ext = install_ext_merge(ext, f.xy);
        }
        if (log2t >= 0) {
#pragma unroll
            for (int c = 0; c < INSTALL_CLASSES; ++c) {
                const uint64_t m = __ballot(valid && f.k == c);
                if (lane == c) count += (uint32_t)__popcll(m);
            }
        }
    }
#pragma unroll
    for (int dlt = 32; dlt >= 1; dlt >>= 1) ext = install_ext_merge(ext, __shfl_xor(ext, dlt, 64));
    if (lane == 0) {
        atomicMax(&s_ext[0], ext & 0xffffu);
        atomicMax(&s_ext[1], ext >> 16);
    }
    if (lane < INSTALL_CLASSES && count) atomicAdd(&s_cnt[lane], count);
    __syncthreads();

    // the 17 offsets
    if (tid == 0) {
        uint16_t* cl = fcls + (int64_t)b * (INSTALL_CLASSES + 1);
        uint32_t at = 0;
        cl[0] = 0;
        for (int c = 0; c < INSTALL_CLASSES; ++c) {
            s_run[c] = at;
            at += s_cnt[c];
            cl[c + 1] = (uint16_t)(log2t >= 0 ? at : (uint32_t)nf);
        }
        fext[b] = s_ext[0] | (s_ext[1] << 16);
    }
    if (log2t < 0) return; // (uniform)
    __syncthreads();

    // pass 2: a feature goes to its class's offset + the features of the class before it -- in the chunks before (s_run), in the
    // waves before within the chunk (s_wcnt), in the lanes before within the wave (ballot): the stable counting sort of the host
    for (int c0 = 0; c0 < nf; c0 += INSTALL_CHUNK) {
        const int i = c0 + tid;
        const bool valid = i < nf;
        InstallFeat f{0u, 0, 0, true};
        if (valid) f = install_load(src, i, log2t);
        uint32_t rank = 0, wave_total = 0;
#pragma unroll
        for (int c = 0; c < INSTALL_CLASSES; ++c) {
            const uint64_t m = __ballot(valid && f.k == c);
            if (valid && f.k == c) rank = install_rank_below(m);
            if (lane == c) wave_total = (uint32_t)__popcll(m);
        }
        if (lane < INSTALL_CLASSES) s_wcnt[w][lane] = wave_total;
        __syncthreads();
        if (valid) {
            uint32_t pos = s_run[f.k] + rank;
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (v < w) pos += s_wcnt[v][f.k];
            if (pos < (uint32_t)nf) { // (always, while the source holds still between the passes: a store stays inside its level)
                fxy_s[dst + pos] = f.xy;
                flabel_s[dst + pos] = (uint8_t)f.label;
            }
        }
        __syncthreads();
        if (tid < INSTALL_CLASSES) s_run[tid] += s_wcnt[0][tid] + s_wcnt[1][tid] + s_wcnt[2][tid] + s_wcnt[3][tid];
        __syncthreads();
    }
}

} // namespace sbm
