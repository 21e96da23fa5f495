// TEST INFRASTRUCTURE: the dataflow of the kernels of sbm_upload_templates_device (shape_based_matching_amd/csrc/
// sbm_install_kernels.h) walked on the CPU with the scalar rules the kernels use (sbm_install_math.h, sbm_install_plan.h): a
// workgroup is 4 waves of 64 lanes, a ballot is a 64-bit mask over a wave's lanes, an LDS array is an array, a barrier is the
// end of a loop over the lanes.  Compiled by tests/test_install_math.py into its temporary directory, and with INSTALL_EMU_MAIN
// as a stand-alone program for the sanitizers; never loaded by the product.  The sources' addresses are host addresses here.
#include <string.h>

#include <vector>

#include "sbm_install_plan.h"

using namespace sbm;

namespace {

enum { WAVES = 4, LANES = 64 };
struct TL {
    int32_t width, height, nf, feat_off;
};

int popcount64(uint64_t m) { return __builtin_popcountll(m); }
uint32_t rank_below(uint64_t m, int lane) { return (uint32_t)popcount64(m & ((lane ? ((uint64_t)1 << lane) : 1) - 1)); }

} // namespace

// k_install_scan.  header: {level_verdict, total_features, n_kept} as int64.  index [P]; item_pyramid, item_source, d_class, d_tid
// [P]; tls [P * L] records of 4 int32.
extern "C" int sbm_emu_install_scan(const sbm_template_source* sources, int n_sources, int L, int64_t* header, int32_t* index, int32_t* item_pyramid,
                                    int32_t* item_source, int32_t* tls_out, int32_t* d_class, int32_t* d_tid)
{
    const InstallPlan p = install_plan(sources, n_sources, L);
    if (p.error) return p.error;
    const InstallSource* src = p.table.data();
    const int n_pyramids = (int)p.n_pyramids;
    TL* tls = (TL*)tls_out;
    uint64_t level_verdict = INSTALL_NO_LEVEL_FAULT;
    std::vector<int32_t> src_t0((size_t)n_sources, -1), src_kept((size_t)n_sources, 0), src_base((size_t)n_sources, 0);
    int32_t carry_k = 0;
    int64_t carry_f = 0;
    for (int base = 0; base < n_pyramids; base += INSTALL_CHUNK) {
        bool kept[INSTALL_CHUNK];
        uint32_t nfsum[INSTALL_CHUNK], finc[INSTALL_CHUNK];
        int s_of[INSTALL_CHUNK], i_of[INSTALL_CHUNK];
        uint64_t ballot[WAVES] = {};
        uint32_t s_wk[WAVES], s_wf[WAVES];
        for (int tid = 0; tid < INSTALL_CHUNK; ++tid) {
            const int j = base + tid;
            kept[tid] = false, nfsum[tid] = 0, s_of[tid] = 0, i_of[tid] = 0;
            if (j >= n_pyramids) continue;
            const int s = install_source_of(src, n_sources, j), i = j - src[s].pyr_first;
            s_of[tid] = s, i_of[tid] = i;
            const sbm_template_level* lv = src[s].levels + (int64_t)i * L;
            kept[tid] = install_keeps(src[s].status ? src[s].status[2 * (int64_t)i] : 0);
            if (!kept[tid]) continue;
            for (int l = 0; l < L; ++l) {
                const int fault = install_level_fault(lv[l].n_features, lv[l].feature_offset, src[s].feat_cap);
                if (fault) {
                    const uint64_t v = install_level_verdict(j, L, l, fault);
                    if (v < level_verdict) level_verdict = v; // atomicMin
                    kept[tid] = false;
                    break;
                }
                nfsum[tid] += (uint32_t)lv[l].n_features;
            }
        }
        for (int w = 0; w < WAVES; ++w) { // the ballot and the inclusive scan inside each wave
            uint32_t run = 0;
            for (int lane = 0; lane < LANES; ++lane) {
                const int tid = w * LANES + lane;
                if (kept[tid]) ballot[w] |= (uint64_t)1 << lane;
                run += kept[tid] ? nfsum[tid] : 0u;
                finc[tid] = run;
            }
            s_wk[w] = (uint32_t)popcount64(ballot[w]);
            s_wf[w] = finc[w * LANES + LANES - 1];
        }
        uint32_t kt = 0, ft = 0;
        for (int w = 0; w < WAVES; ++w) kt += s_wk[w], ft += s_wf[w];
        for (int tid = 0; tid < INSTALL_CHUNK; ++tid) {
            const int j = base + tid, w = tid / LANES, lane = tid % LANES;
            if (j >= n_pyramids) continue;
            uint32_t kb = 0, fb = 0;
            for (int v = 0; v < w; ++v) kb += s_wk[v], fb += s_wf[v];
            const int32_t t = carry_k + (int32_t)(kb + rank_below(ballot[w], lane));
            const int s = s_of[tid], i = i_of[tid];
            index[j] = kept[tid] ? t : -1;
            if (i == 0) src_t0[(size_t)s] = t;
            if (!kept[tid]) continue;
            const sbm_template_level* lv = src[s].levels + (int64_t)i * L;
            item_pyramid[t] = j;
            item_source[t] = s;
            int64_t f = carry_f + (int64_t)(fb + finc[tid] - nfsum[tid]);
            for (int l = 0; l < L; ++l) {
                tls[(int64_t)t * L + l] = TL{lv[l].width, lv[l].height, lv[l].n_features, (int32_t)f};
                f += lv[l].n_features;
            }
            d_class[t] = src[s].class_idx;
            ++src_kept[(size_t)s];
        }
        carry_k += (int32_t)kt;
        carry_f += (int64_t)ft;
    }
    for (int s = 0; s < n_sources; ++s) {
        int32_t before = 0;
        for (int u = 0; u < s; ++u)
            if (src[u].class_idx == src[s].class_idx) before += src_kept[(size_t)u];
        src_base[(size_t)s] = before;
    }
    for (int j = 0; j < n_pyramids; ++j) {
        const int32_t t = index[j];
        if (t < 0) continue;
        const int s = item_source[t];
        d_tid[t] = src_base[(size_t)s] + (t - src_t0[(size_t)s]);
    }
    header[0] = (int64_t)level_verdict;
    header[1] = carry_f;
    header[2] = carry_k;
    return 0;
}

// k_install_features for one (template, level): nf_record features at src (the level record's count, clamped as the kernel
// clamps it), the level's T and number, its installed feature_offset.  The tables are indexed as the kernel indexes them
// (from feat_off); fcls: this level's 17 offsets; *fext, *verdict (merged by minimum, as the atomic does).
extern "C" void sbm_emu_install_features(const sbm_train_feature* src, int32_t nf_record, int T, int level, int32_t feat_off, uint32_t* fxy, uint8_t* flabel,
                                         uint8_t* flevel, uint32_t* fxy_s, uint8_t* flabel_s, uint16_t* fcls, uint32_t* fext, uint32_t* verdict)
{
    const int nf = install_clamp_nf(nf_record), log2t = install_log2t(T);
    const int64_t dst = feat_off;
    uint32_t s_cnt[INSTALL_CLASSES] = {}, s_run[INSTALL_CLASSES] = {}, s_ext[2] = {0, 0};
    uint32_t count[WAVES][LANES] = {}; // lane c of a wave counts the wave's features of class c
    uint32_t ext[WAVES][LANES] = {};
    struct Feat {
        uint32_t xy;
        int32_t label;
        int k;
        bool ok;
    };
    auto load = [&](int i) {
        const sbm_train_feature f = src[i];
        Feat r;
        r.ok = install_feature_ok(f.x, f.y, f.label);
        r.xy = install_pack_xy(f.x, f.y);
        r.label = f.label;
        r.k = log2t >= 0 ? install_class(r.xy, log2t) : 0;
        return r;
    };
    // pass 1
    for (int c0 = 0; c0 < nf; c0 += INSTALL_CHUNK)
        for (int w = 0; w < WAVES; ++w) {
            Feat f[LANES];
            bool valid[LANES];
            for (int lane = 0; lane < LANES; ++lane) {
                const int i = c0 + w * LANES + lane;
                valid[lane] = i < nf;
                f[lane] = Feat{0u, 0, 0, true};
                if (!valid[lane]) continue;
                f[lane] = load(i);
                if (!f[lane].ok && (uint32_t)(dst + i) < *verdict) *verdict = (uint32_t)(dst + i);
                fxy[dst + i] = f[lane].xy;
                flabel[dst + i] = (uint8_t)f[lane].label;
                flevel[dst + i] = (uint8_t)level;
                if (log2t < 0) {
                    fxy_s[dst + i] = f[lane].xy;
                    flabel_s[dst + i] = (uint8_t)f[lane].label;
                }
                if (f[lane].ok) ext[w][lane] = install_ext_merge(ext[w][lane], f[lane].xy);
            }
            if (log2t >= 0)
                for (int c = 0; c < INSTALL_CLASSES; ++c) {
                    uint64_t m = 0;
                    for (int lane = 0; lane < LANES; ++lane)
                        if (valid[lane] && f[lane].k == c) m |= (uint64_t)1 << lane;
                    count[w][c] += (uint32_t)popcount64(m);
                }
        }
    for (int w = 0; w < WAVES; ++w) {
        uint32_t e = 0;
        for (int lane = 0; lane < LANES; ++lane) e = install_ext_merge(e, ext[w][lane]); // the butterfly's result
        if ((e & 0xffffu) > s_ext[0]) s_ext[0] = e & 0xffffu;
        if ((e >> 16) > s_ext[1]) s_ext[1] = e >> 16;
        for (int c = 0; c < INSTALL_CLASSES; ++c) s_cnt[c] += count[w][c];
    }
    // the 17 offsets
    uint32_t at = 0;
    fcls[0] = 0;
    for (int c = 0; c < INSTALL_CLASSES; ++c) {
        s_run[c] = at;
        at += s_cnt[c];
        fcls[c + 1] = (uint16_t)(log2t >= 0 ? at : (uint32_t)nf);
    }
    *fext = s_ext[0] | (s_ext[1] << 16);
    if (log2t < 0) return;
    // pass 2
    for (int c0 = 0; c0 < nf; c0 += INSTALL_CHUNK) {
        uint32_t s_wcnt[WAVES][INSTALL_CLASSES] = {};
        Feat f[INSTALL_CHUNK];
        bool valid[INSTALL_CHUNK];
        uint32_t rank[INSTALL_CHUNK] = {};
        for (int w = 0; w < WAVES; ++w) {
            for (int lane = 0; lane < LANES; ++lane) {
                const int tid = w * LANES + lane, i = c0 + tid;
                valid[tid] = i < nf;
                f[tid] = valid[tid] ? load(i) : Feat{0u, 0, 0, true};
            }
            for (int c = 0; c < INSTALL_CLASSES; ++c) {
                uint64_t m = 0;
                for (int lane = 0; lane < LANES; ++lane)
                    if (valid[w * LANES + lane] && f[w * LANES + lane].k == c) m |= (uint64_t)1 << lane;
                for (int lane = 0; lane < LANES; ++lane)
                    if (valid[w * LANES + lane] && f[w * LANES + lane].k == c) rank[w * LANES + lane] = rank_below(m, lane);
                s_wcnt[w][c] = (uint32_t)popcount64(m);
            }
        }
        for (int tid = 0; tid < INSTALL_CHUNK; ++tid) {
            if (!valid[tid]) continue;
            uint32_t pos = s_run[f[tid].k] + rank[tid];
            for (int v = 0; v < tid / LANES; ++v) pos += s_wcnt[v][f[tid].k];
            if (pos < (uint32_t)nf) {
                fxy_s[dst + pos] = f[tid].xy;
                flabel_s[dst + pos] = (uint8_t)f[tid].label;
            }
        }
        for (int c = 0; c < INSTALL_CLASSES; ++c)
            for (int w = 0; w < WAVES; ++w) s_run[c] += s_wcnt[w][c];
    }
}

extern "C" int sbm_emu_install_feature_ok(int32_t x, int32_t y, int32_t label) { return install_feature_ok(x, y, label) ? 1 : 0; }
extern "C" int sbm_emu_install_class(uint32_t xy, int T) { return install_class(xy, install_log2t(T)); }
extern "C" uint32_t sbm_emu_install_ext_merge(uint32_t a, uint32_t b) { return install_ext_merge(a, b); }

#ifdef INSTALL_EMU_MAIN
// The same walks over a small family with tight buffers, for the sanitizers: every table exactly as large as the sizes of
// sbm_install_plan.h say, the feature counts at the chunk's edges, a skipped pyramid, a level without features.
#include <stdio.h>
int main()
{
    const int L = 3, T[3] = {4, 8, 16};
    const int counts[][3] = {{257, 64, 1}, {0, 0, 0}, {8191, 255, 65}, {63, 0, 256}};
    const int n = 4;
    std::vector<sbm_template_level> levels((size_t)n * L);
    std::vector<int32_t> status((size_t)n * 2, 0);
    status[2] = 1; // the pyramid without features failed its training
    int64_t cap = 0;
    for (int i = 0; i < n; ++i) cap = std::max<int64_t>(cap, counts[i][0] + counts[i][1] + counts[i][2]);
    std::vector<sbm_train_feature> feats((size_t)(cap * n));
    uint32_t seed = 12345;
    for (int i = 0; i < n; ++i) {
        int64_t off = 0;
        for (int l = 0; l < L; ++l) {
            levels[(size_t)i * L + l] = sbm_template_level{100 + i, 50 + l, 0, 0, l, counts[i][l], off};
            for (int k = 0; k < counts[i][l]; ++k) {
                seed = seed * 1664525u + 1013904223u;
                feats[(size_t)(i * cap + off + k)] = sbm_train_feature{(int32_t)((seed >> 8) & 0xffff), (int32_t)((seed >> 3) & 0x3ff), (int32_t)(seed >> 29), 1.f};
            }
            off += counts[i][l];
        }
    }
    const sbm_template_source source{levels.data(), feats.data(), status.data(), n, 7, 0, cap, cap};
    int64_t header[3];
    std::vector<int32_t> index((size_t)n), ip((size_t)n), is((size_t)n), tls((size_t)n * L * 4), cls((size_t)n), tid((size_t)n);
    if (sbm_emu_install_scan(&source, 1, L, header, index.data(), ip.data(), is.data(), tls.data(), cls.data(), tid.data())) return 1;
    const int64_t K = header[2], NF = header[1];
    if (K != 3 || header[0] != -1) return 2;
    std::vector<uint32_t> fxy((size_t)install_table_bytes(INSTALL_T_FXY, K, L, NF) / 4), fxy_s(fxy.size());
    std::vector<uint8_t> flabel((size_t)install_table_bytes(INSTALL_T_FLABEL, K, L, NF)), flevel(flabel.size()), flabel_s(flabel.size());
    std::vector<uint16_t> fcls((size_t)install_table_bytes(INSTALL_T_FCLS, K, L, NF) / 2);
    std::vector<uint32_t> fext((size_t)install_table_bytes(INSTALL_T_FEXT, K, L, NF) / 4);
    uint32_t verdict = INSTALL_NO_FEATURE_FAULT;
    for (int64_t t = 0; t < K; ++t)
        for (int l = 0; l < L; ++l) {
            const int32_t* d = &tls[(size_t)(t * L + l) * 4];
            const sbm_template_level& lv = levels[(size_t)ip[(size_t)t] * L + l];
            sbm_emu_install_features(feats.data() + ip[(size_t)t] * cap + lv.feature_offset, d[2], T[l], l, d[3], fxy.data(), flabel.data(), flevel.data(),
                                     fxy_s.data(), flabel_s.data(), &fcls[(size_t)(t * L + l) * 17], &fext[(size_t)(t * L + l)], &verdict);
        }
    if (verdict != INSTALL_NO_FEATURE_FAULT) return 3;
    // the sorted copy of every level is a permutation of the level that is ordered by class
    for (int64_t r = 0; r < K * L; ++r) {
        const int32_t* d = &tls[(size_t)r * 4];
        const int log2t = install_log2t(T[r % L]);
        uint64_t a = 0, b = 0;
        for (int k = 0; k < d[2]; ++k) {
            a += fxy[(size_t)(d[3] + k)] + flabel[(size_t)(d[3] + k)], b += fxy_s[(size_t)(d[3] + k)] + flabel_s[(size_t)(d[3] + k)];
            if (log2t >= 0 && k && install_class(fxy_s[(size_t)(d[3] + k - 1)], log2t) > install_class(fxy_s[(size_t)(d[3] + k)], log2t)) return 4;
        }
        if (a != b || fcls[(size_t)r * 17 + 16] != d[2]) return 5;
    }
    printf("install emulation ok: %lld templates, %lld features\n", (long long)K, (long long)NF);
    return 0;
}
#endif
