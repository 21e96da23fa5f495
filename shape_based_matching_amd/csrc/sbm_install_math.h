// sbm_install_math.h — the scalar rules of installing device-trained pyramids as the match set (sbm_upload_templates_device,
// sbm_install_kernels.h): which pyramid is kept, what a level record must satisfy, the bounds of a feature, how it is packed,
// the class key of the refinement pass's sorted copies, the merge of a level's feature extent and the numbering of the kept
// pyramids.  Plain C++, host and device: tests/test_install_math.py compiles the host pass (tests/emu/install_math_emu.cpp walks
// the kernels' dataflow with these functions) and checks it against a restatement of sbm_upload_templates' host loop.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <unordered_map>

#include "../../include/sbm.h"

namespace sbm {

#if defined(__HIPCC__)
#define SBM_INSTALL_HD __host__ __device__ __forceinline__
#else
#define SBM_INSTALL_HD inline
#endif

enum { INSTALL_CLASSES = 16, INSTALL_CHUNK = 256 }; // classes of the sorted copies; features a workgroup takes per step

// A pyramid is kept when its status pair begins with 0 (no status array: every pyramid is ok).  Any other pair is a pyramid
// addTemplate returned -1 for, or one that never came to be: it adds nothing (line2Dup.cpp:1343).
SBM_INSTALL_HD bool install_keeps(int32_t status0) { return status0 == 0; }

// a level record's feature count as the kernels loop on it: never beyond the reference's bound, whatever the record says
SBM_INSTALL_HD int32_t install_clamp_nf(int32_t nf) { return nf < 0 ? 0 : (nf > SBM_MAX_FEATURES ? SBM_MAX_FEATURES : nf); }

// what is wrong with a kept pyramid's level record (the order of the tests is the order of the messages)
enum InstallLevelFault { INSTALL_LEVEL_OK = 0, INSTALL_LEVEL_COUNT = 1, INSTALL_LEVEL_RANGE = 2 };
SBM_INSTALL_HD int install_level_fault(int32_t n_features, int64_t feature_offset, int64_t feat_cap)
{
    if (n_features < 0 || n_features > SBM_MAX_FEATURES) return INSTALL_LEVEL_COUNT; // CV_Error line2Dup.cpp:1195, :1260
    if (feature_offset < 0 || feature_offset > feat_cap - n_features) return INSTALL_LEVEL_RANGE;
    return INSTALL_LEVEL_OK;
}

// feature_in_bounds of sbm_upload_templates: what fits 16 + 16 bits and the eight orientation labels
SBM_INSTALL_HD bool install_feature_ok(int32_t x, int32_t y, int32_t label)
{
    return x >= 0 && y >= 0 && x <= 65535 && y <= 65535 && label >= 0 && label < 8;
}
SBM_INSTALL_HD uint32_t install_pack_xy(int32_t x, int32_t y) { return (uint32_t)x | ((uint32_t)y << 16); }

// log2 of a level's T where the strip plane exists (T = 4 and 8), -1 elsewhere: such a level is copied unsorted
SBM_INSTALL_HD int install_log2t(int T) { return T == 4 ? 2 : (T == 8 ? 3 : -1); }
// the class of a packed feature: the strip column of its x, modulo the 16 columns of a strip
SBM_INSTALL_HD int install_class(uint32_t xy, int log2t) { return (int)(((xy & 0xffffu) >> log2t) & 15u); }

// largest x | largest y << 16 of a level, merged pairwise (0 for a level without features)
SBM_INSTALL_HD uint32_t install_ext_merge(uint32_t a, uint32_t b)
{
    const uint32_t ax = a & 0xffffu, bx = b & 0xffffu, ay = a >> 16, by = b >> 16;
    return (ax > bx ? ax : bx) | ((ay > by ? ay : by) << 16);
}

// The verdict words.  A level fault: (flat pyramid * n_levels + level) * 4 + fault, so the minimum over all faults is the
// first faulty level in source order with its first failing test.  A feature fault: the feature's installed index, which
// runs in source order too.  No fault: all ones.
SBM_INSTALL_HD uint64_t install_level_verdict(int64_t pyramid, int n_levels, int level, int fault)
{
    return (uint64_t)((pyramid * n_levels + level) * 4 + fault);
}
constexpr uint64_t INSTALL_NO_LEVEL_FAULT = ~(uint64_t)0;
constexpr uint32_t INSTALL_NO_FEATURE_FAULT = ~(uint32_t)0;

// ---- numbering ---------------------------------------------------------------------------------------------------------
// The kept pyramids become templates 0, 1, ... in source order; a kept pyramid's template_id is the number of kept pyramids
// of its class before it (line2Dup.cpp:1312: the id is the class's size when the pyramid is added).  kept[j]: pyramid j of
// the flat list is kept; cls[j]: its class.  index_out[j]: its template index or -1; class_out / id_out: per template.
// The host's form of what k_install_scan computes with a prefix sum per class: the kernel's numbering is tested against it.
inline int32_t install_number(const uint8_t* kept, const int32_t* cls, int64_t n, int32_t* index_out, int32_t* class_out, int32_t* id_out)
{
    std::unordered_map<int32_t, int32_t> count; // kept pyramids per class so far
    int32_t t = 0;
    for (int64_t j = 0; j < n; ++j) {
        if (!kept[j]) {
            if (index_out) index_out[j] = -1;
            continue;
        }
        if (index_out) index_out[j] = t;
        class_out[t] = cls[j];
        id_out[t] = count[cls[j]]++;
        ++t;
    }
    return t;
}

} // namespace sbm
