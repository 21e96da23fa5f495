// TEST INFRASTRUCTURE: shape_based_matching_amd/csrc/sbm_install_plan.h -- the argument verdict, the table of sources, the scratch
// layout, the table sizes and the decoding of the kernels' verdict words of sbm_upload_templates_device -- behind a C interface.
// Compiled by tests/test_install_plan.py into its temporary directory; never loaded by the product.
#include "sbm_install_plan.h"

using namespace sbm;

enum { PLAN_FIELDS = 9 };

// fields: n_pyramids, o_header, o_table, o_src_kept, o_index, o_items, o_src_t0, o_src_base, total;  pyr_first: per source
extern "C" int sbm_emu_install_plan(const sbm_template_source* sources, int n, int L, int64_t* fields, int32_t* pyr_first, int32_t* error_source)
{
    const InstallPlan p = install_plan(sources, n, L);
    *error_source = p.error_source;
    if (p.error) return p.error;
    const int64_t f[PLAN_FIELDS] = {p.n_pyramids, p.o_header, p.o_table, p.o_src_kept, p.o_index, p.o_items, p.o_src_t0, p.o_src_base, p.total};
    for (int j = 0; j < PLAN_FIELDS; ++j) fields[j] = f[j];
    for (int s = 0; s < n; ++s) {
        const InstallSource& v = p.table[(size_t)s];
        const sbm_template_source& r = sources[s];
        if (v.levels != r.d_levels || v.feats != r.d_feats || v.status != r.d_status || v.n_pyramids != r.n_pyramids || v.class_idx != r.class_idx ||
            v.feat_first != r.feat_first || v.feat_pitch != r.feat_pitch || v.feat_cap != r.feat_cap)
            return -1; // the table is the caller's records
        pyr_first[s] = v.pyr_first;
    }
    return 0;
}

extern "C" const char* sbm_emu_install_error(int e) { return install_error(e); }
extern "C" int sbm_emu_install_errors() { return INP_ERRORS; }
extern "C" int sbm_emu_sizeof_template_source() { return (int)sizeof(sbm_template_source); }
extern "C" int sbm_emu_sizeof_install_source() { return (int)sizeof(InstallSource); }
extern "C" int sbm_emu_sizeof_install_item() { return (int)sizeof(InstallItem); }
extern "C" int sbm_emu_sizeof_install_header() { return (int)sizeof(InstallHeader); }
extern "C" int64_t sbm_emu_install_table_bytes(int which, int64_t n_templates, int L, int64_t n_features)
{
    return install_table_bytes(which, n_templates, L, n_features);
}

extern "C" uint64_t sbm_emu_install_level_verdict(int64_t pyramid, int L, int level, int fault) { return install_level_verdict(pyramid, L, level, fault); }
// out: source, pyramid inside it, level, fault
extern "C" int sbm_emu_install_where_level(const sbm_template_source* sources, int n, int L, uint64_t verdict, int32_t* out)
{
    const InstallPlan p = install_plan(sources, n, L);
    if (p.error) return p.error;
    const InstallWhere w = install_where_level(p, verdict);
    out[0] = w.source, out[1] = w.pyramid, out[2] = w.level, out[3] = w.fault;
    return 0;
}
extern "C" int64_t sbm_emu_install_where_feature(const int32_t* feat_off, int64_t stride, int64_t n, uint32_t verdict, int32_t* feature)
{
    return install_where_feature(feat_off, stride, n, verdict, feature);
}
extern "C" int sbm_emu_install_level_fault(int32_t n_features, int64_t feature_offset, int64_t feat_cap)
{
    return install_level_fault(n_features, feature_offset, feat_cap);
}
extern "C" int32_t sbm_emu_install_number(const uint8_t* kept, const int32_t* cls, int64_t n, int32_t* index_out, int32_t* class_out, int32_t* id_out)
{
    return install_number(kept, cls, n, index_out, class_out, id_out);
}
