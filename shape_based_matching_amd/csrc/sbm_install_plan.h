// sbm_install_plan.h — the host rules of sbm_upload_templates_device: the argument verdict, the table of sources the scan
// kernel reads, the layout of the call's scratch, the sizes of the ten template tables and how a verdict word of the
// kernels names its source, pyramid and level.  Plain C++, no HIP: tests/test_install_plan.py compiles it for the CPU
// (tests/emu/install_plan_emu.cpp).  The host never reads a level record or a feature of a source, so everything here
// follows from the call's integers and from what the kernels report.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/sbm.h"
#include "sbm_install_math.h"

namespace sbm {

// A source as the scan kernel reads it: the caller's record with its addresses typed, then the flat index of its first pyramid
struct InstallSource { // 64 bytes
    const sbm_template_level* levels;
    const sbm_train_feature* feats;
    const int32_t* status;
    int32_t n_pyramids, class_idx;
    int64_t feat_first, feat_pitch, feat_cap;
    int32_t pyr_first, reserved;
};

// a kept pyramid, at its template index: where its level records and its feature block lie, and which pyramid it was
struct InstallItem { // 24 bytes
    const sbm_template_level* levels;
    const sbm_train_feature* feats;
    int32_t pyramid, source;
};

// what the kernels report, 32 bytes at the front of the scratch; the host writes it with both verdicts empty
struct InstallHeader {
    uint64_t level_verdict; // install_level_verdict of the first faulty level record, or INSTALL_NO_LEVEL_FAULT
    int64_t total_features; // of the kept pyramids
    int32_t n_kept;
    uint32_t feature_verdict; // installed index of the first feature out of bounds, or INSTALL_NO_FEATURE_FAULT
    int32_t reserved[2];
};

enum InstallError {
    INP_OK = 0,
    INP_COUNT,    // n_sources < 1
    INP_NEGATIVE, // a negative n_pyramids, feat_first, feat_pitch or feat_cap
    INP_NULL,     // a source with pyramids and no level records, or with room for features and no feature array
    INP_SPAN,     // the last block's end does not fit 63-bit byte arithmetic
    INP_PYRAMIDS, // more than 2^31 / n_levels pyramids
    INP_ERRORS
};

inline const char* install_error(int e)
{
    switch (e) {
    case INP_COUNT: return "at least one source";
    case INP_NEGATIVE: return "negative n_pyramids, feat_first, feat_pitch or feat_cap";
    case INP_NULL: return "null d_levels or d_feats";
    case INP_SPAN: return "feature blocks beyond the addressable range";
    case INP_PYRAMIDS: return "more than 2^31 / n_levels pyramids";
    default: return "";
    }
}

inline int64_t install_round256(int64_t v) { return (v + 255) / 256 * 256; }

enum InstallTable { // sbm_get_template_table's `which`
    INSTALL_T_TLS = 0, INSTALL_T_FXY, INSTALL_T_FLABEL, INSTALL_T_FLEVEL, INSTALL_T_FXY_S, INSTALL_T_FLABEL_S, INSTALL_T_FCLS, INSTALL_T_FEXT,
    INSTALL_T_CLASS, INSTALL_T_TID, INSTALL_TABLES
};
// bytes of a table for n_templates templates of L levels and n_features features; -1: no such table
inline int64_t install_table_bytes(int which, int64_t n_templates, int L, int64_t n_features)
{
    const int64_t tl = n_templates * L;
    switch (which) {
    case INSTALL_T_TLS: return tl * 16;
    case INSTALL_T_FXY: case INSTALL_T_FXY_S: return n_features * 4;
    case INSTALL_T_FLABEL: case INSTALL_T_FLEVEL: case INSTALL_T_FLABEL_S: return n_features;
    case INSTALL_T_FCLS: return tl * (INSTALL_CLASSES + 1) * 2;
    case INSTALL_T_FEXT: return tl * 4;
    case INSTALL_T_CLASS: case INSTALL_T_TID: return n_templates * 4;
    default: return -1;
    }
}

struct InstallPlan {
    int error = INP_OK;
    int error_source = -1; // the first source the reported rule fails on (-1: a rule of the whole call)
    int L = 0, n_sources = 0;
    int64_t n_pyramids = 0;
    std::vector<InstallSource> table; // [n_sources]
    // byte offsets in the scratch: the header, the table and the per-source kept counts travel from the host in one copy
    // ([0, o_index)); behind them what only the kernels write
    int64_t o_header = 0, o_table = 0, o_src_kept = 0, o_index = 0, o_items = 0, o_src_t0 = 0, o_src_base = 0, total = 0;
};

// sources: read for counts, sizes and whether the addresses are null; never dereferenced
inline InstallPlan install_plan(const sbm_template_source* sources, int n_sources, int L)
{
    InstallPlan p;
    p.L = L, p.n_sources = n_sources;
    auto bad = [&](int e, int s) {
        p.error = e, p.error_source = s;
        return p;
    };
    if (n_sources < 1 || !sources) return bad(INP_COUNT, -1);
    for (int s = 0; s < n_sources; ++s)
        if (sources[s].n_pyramids < 0 || sources[s].feat_first < 0 || sources[s].feat_pitch < 0 || sources[s].feat_cap < 0) return bad(INP_NEGATIVE, s);
    for (int s = 0; s < n_sources; ++s)
        if (sources[s].n_pyramids > 0 && (!sources[s].d_levels || (sources[s].feat_cap > 0 && !sources[s].d_feats))) return bad(INP_NULL, s);
    const int64_t max_records = INT64_MAX / (int64_t)sizeof(sbm_train_feature);
    for (int s = 0; s < n_sources; ++s) {
        const sbm_template_source& r = sources[s];
        if (r.n_pyramids == 0) continue;
        // feat_first + (n - 1) * feat_pitch + feat_cap records, in bytes, stays below 2^63
        if (r.feat_cap > max_records || r.feat_first > max_records - r.feat_cap) return bad(INP_SPAN, s);
        const int64_t room = max_records - r.feat_cap - r.feat_first;
        if (r.n_pyramids > 1 && r.feat_pitch > room / (r.n_pyramids - 1)) return bad(INP_SPAN, s);
    }
    p.table.resize((size_t)n_sources);
    for (int s = 0; s < n_sources; ++s) {
        const sbm_template_source& r = sources[s];
        if (p.n_pyramids + r.n_pyramids > (((int64_t)1 << 31) - 1) / L) return bad(INP_PYRAMIDS, s);
        InstallSource& v = p.table[(size_t)s];
        v.levels = (const sbm_template_level*)r.d_levels;
        v.feats = (const sbm_train_feature*)r.d_feats;
        v.status = (const int32_t*)r.d_status;
        v.n_pyramids = r.n_pyramids;
        v.class_idx = r.class_idx;
        v.feat_first = r.feat_first;
        v.feat_pitch = r.feat_pitch;
        v.feat_cap = r.feat_cap;
        v.pyr_first = (int32_t)p.n_pyramids;
        v.reserved = 0;
        p.n_pyramids += r.n_pyramids;
    }
    const int64_t S = n_sources, P = p.n_pyramids;
    p.o_header = 0;
    p.o_table = install_round256((int64_t)sizeof(InstallHeader));
    p.o_src_kept = p.o_table + install_round256(S * (int64_t)sizeof(InstallSource));
    p.o_index = p.o_src_kept + install_round256(S * 4);
    p.o_items = p.o_index + install_round256(P * 4);
    p.o_src_t0 = p.o_items + install_round256(P * (int64_t)sizeof(InstallItem));
    p.o_src_base = p.o_src_t0 + install_round256(S * 4);
    p.total = p.o_src_base + install_round256(S * 4);
    return p;
}

// the source of flat pyramid j (0 <= j < n_pyramids): the last source whose first pyramid is not behind j -- a source without
// pyramids shares its first with the next one and is never the last such.  The scan kernel searches the same way.
template <class Table>
SBM_INSTALL_HD int install_source_of(const Table* table, int n_sources, int32_t j)
{
    int lo = 0, hi = n_sources;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (table[mid].pyr_first <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct InstallWhere {
    int source, pyramid, level, fault; // pyramid: inside its source
};
// a level verdict of k_install_scan (not INSTALL_NO_LEVEL_FAULT)
inline InstallWhere install_where_level(const InstallPlan& p, uint64_t verdict)
{
    InstallWhere w;
    w.fault = (int)(verdict & 3);
    const int64_t jl = (int64_t)(verdict >> 2);
    const int32_t j = (int32_t)(jl / p.L);
    w.level = (int)(jl % p.L);
    w.source = install_source_of(p.table.data(), p.n_sources, j);
    w.pyramid = j - p.table[(size_t)w.source].pyr_first;
    return w;
}

// A feature verdict of k_install_features: the installed index of a feature.  feat_off: the installed feature_offset of every
// (template, level), n of them `stride` int32 apart, non-decreasing; the record that holds the feature is the last one that starts at or before it
// (a level without features starts where the next one does).  Returns the record's index, *feature: the feature inside it.
inline int64_t install_where_feature(const int32_t* feat_off, int64_t stride, int64_t n, uint32_t verdict, int32_t* feature)
{
    int64_t lo = 0, hi = n; // feat_off[lo] <= verdict (feat_off[0] = 0)
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((uint32_t)feat_off[mid * stride] <= verdict) lo = mid;
        else hi = mid;
    }
    *feature = (int32_t)(verdict - (uint32_t)feat_off[lo * stride]);
    return lo;
}

} // namespace sbm
