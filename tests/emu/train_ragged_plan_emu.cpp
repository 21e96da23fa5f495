// TEST INFRASTRUCTURE: shape_based_matching_amd/csrc/sbm_train_plan.h -- the argument check, the per-image level records, the
// scratch layout and the grid sizes of sbm_train_ragged_device -- behind a C interface.  Compiled by
// tests/test_train_ragged_plan.py into its temporary directory; never loaded by the product.
#include "sbm_train_plan.h"

using namespace sbm;

enum { REC_FIELDS = 12, SUM_FIELDS = 15 };

// rec: [n * L][REC_FIELDS] = rows, cols, cand_cap, nf, pix_off, cand_off, sort_off, img_off, mask_off, stride, feat_first, feat_cap
// sums: img_bytes, pix_elems, cand_elems, sort_elems, o_mag, o_ori, o_quant, o_flags, o_cand, o_keys, o_sel, o_kept, o_counts, o_table, total
// grids: k_train_maxima's x, then the level steps' x per level
extern "C" int sbm_emu_train_ragged_plan(const sbm_train_image* images, int n, int ch, int L, int64_t* rec, int64_t* sums, int32_t* grids,
                                         int32_t* error_image)
{
    const TrainRaggedPlan p = train_ragged_plan(images, n, ch, L);
    *error_image = p.error_image;
    if (p.error) return p.error;
    for (size_t k = 0; k < p.table.size(); ++k) {
        const TrainRecord& v = p.table[k];
        const int64_t f[REC_FIELDS] = {v.rows,     v.cols,       v.cand_cap,    (int64_t)v.nf, v.pix_off,    v.cand_off,
                                       v.sort_off, p.img_off[k], p.mask_off[k], v.stride,      v.feat_first, v.feat_cap};
        for (int j = 0; j < REC_FIELDS; ++j) rec[k * REC_FIELDS + j] = f[j];
    }
    const int64_t s[SUM_FIELDS] = {p.img_bytes, p.pix_elems, p.cand_elems, p.sort_elems, p.o_mag,    p.o_ori,   p.o_quant, p.o_flags,
                                   p.o_cand,    p.o_keys,    p.o_sel,      p.o_kept,     p.o_counts, p.o_table, p.total};
    for (int j = 0; j < SUM_FIELDS; ++j) sums[j] = s[j];
    grids[0] = p.grid_maxima;
    for (int l = 0; l < SBM_MAX_LEVELS; ++l) grids[1 + l] = p.grid_level[l];
    return 0;
}

extern "C" const char* sbm_emu_train_ragged_error(int e) { return train_ragged_error(e); }
extern "C" int sbm_emu_train_ragged_errors() { return TRP_ERRORS; }
extern "C" int sbm_emu_sizeof_train_image() { return (int)sizeof(sbm_train_image); }
extern "C" int sbm_emu_sizeof_train_scale() { return (int)sizeof(sbm_train_scale); }
extern "C" int sbm_emu_sizeof_train_record() { return (int)sizeof(TrainRecord); }
extern "C" int sbm_emu_sizeof_train_cand() { return (int)sizeof(TrainCand); }
extern "C" int64_t sbm_emu_train_cand_bound(int rows, int cols) { return train_cand_bound(rows, cols); }
