// sbm_train_plan.h — the host rules of ragged batched training (sbm_train_ragged_device, sbm_train_sweep_device): from
// the call's integers to the per-image level records the kernels read, the layout of the training scratch (a running
// sum over the images, where the one-geometry call has n * stride), the grid sizes and the argument verdict.  Plain
// C++, no HIP: tests/test_train_ragged_plan.py compiles it for the CPU (tests/emu/train_ragged_plan_emu.cpp).  The
// host never reads an image, so everything here follows from sizes and counts alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/sbm.h"
#include "sbm_train_math.h"

namespace sbm {

struct TrainCand {
    int32_t xy;    // x | y << 16
    int32_t label; // bit index of the one-hot orientation
    float score;   // squared magnitude
    float theta;   // angle_ori
};

struct TrainLevel {
    int32_t rows, cols;
    int32_t cand_cap;    // train_cand_bound(rows, cols)
    uint32_t nf;         // features asked of this level
    int64_t pix_off;     // of this level in an image's pixel space
    int64_t cand_off;    // ... candidate space
    int64_t sort_off;    // ... key space (a power of two >= cand_cap keys per level)
    const uint8_t* mask; // level's masks (nullptr: none), mask_fs bytes apart (0: one for all images)
    int64_t mask_fs;
};

// The ragged form's record of (image, level), at [image * L + level] of a device table: the level as above with
// pix_off, cand_off and sort_off counted from the start of the batch's spaces (the per-image strides are 0) and the
// mask this image's own, then where the level's image lies and where the image's features go.  rows == 0: the level is
// not built (the image is too small for it); it yields no candidate, which fails the level.
struct TrainRecord : TrainLevel {
    const uint8_t* img;           // the level's image, rows of `stride` bytes (level 0: the caller's)
    int32_t stride, reserved;
    int64_t feat_first, feat_cap; // the image's block of the feature array, in records (the same at every level)
};

// One scale of the sweep's resize launch (k_resize_sweep_u8): the scaled size, where its coefficient tables start in the
// concatenated arrays (x_off, y_off: in destination coordinates; the tables of sbm_resize_table.h) and where the scaled
// image and mask go.
struct TrainSweepScale {
    int32_t rows, cols;
    int64_t x_off, y_off;
    uint8_t* img;
    uint8_t* mask; // nullptr: the sweep has no mask
};

enum { TRAIN_MIN_SIDE = 5 }; // the 5 x 5 scan of extractTemplate has no pixel in a smaller level
// The fewest features a level may be asked for.  With ONE, selectScatteredFeatures (line2Dup.cpp:163-212) never returns
// once the level has a candidate: the first candidate is always taken, so every sweep of the growing phase has "enough",
// clears and widens the distance again -- and the device selection follows it step by step.  The ragged calls refuse such
// a count instead of starting a kernel that cannot end.
enum { TRAIN_MIN_FEATURES = 2 };

enum TrainRaggedError {
    TRP_OK = 0,
    TRP_COUNT,      // n < 1 or n > 65535
    TRP_CHANNELS,   // not 1 or 3
    TRP_GEOMETRY,   // rows or cols outside [1, 32767]
    TRP_STRIDE,     // stride < cols * channels
    TRP_FEATURES,   // num_features < 1, or halved to fewer than TRAIN_MIN_FEATURES at the last level
    TRP_FEAT_CAP,   // negative feat_cap (or a block that does not start at a record >= 0)
    TRP_OVERLAP,    // two feature blocks share a record
    TRP_NULL_IMAGE, // an image without pixels
    TRP_ERRORS
};

inline const char* train_ragged_error(int e)
{
    switch (e) {
    case TRP_COUNT: return "number of images out of range (1 .. 65535)";
    case TRP_CHANNELS: return "channels must be 1 or 3";
    case TRP_GEOMETRY: return "image size out of range (1 .. 32767: positions are 15-bit)";
    case TRP_STRIDE: return "stride below cols * channels";
    case TRP_FEATURES: return "num_features leaves fewer than two features for the last pyramid level";
    case TRP_FEAT_CAP: return "negative feature capacity or block start";
    case TRP_OVERLAP: return "feature blocks overlap";
    case TRP_NULL_IMAGE: return "null image";
    default: return "";
    }
}

inline int64_t train_round256(int64_t v) { return (v + 255) / 256 * 256; }

struct TrainRaggedPlan {
    int error = TRP_OK;
    int error_image = -1; // the first image the reported rule fails on (-1: a rule of the whole call)
    int L = 0, n = 0, ch = 0;
    std::vector<TrainRecord> table; // [n * L]; img and mask of the levels the engine builds are set by train_ragged_bind
    std::vector<int64_t> img_off;   // [n * L] byte offset of the level's image in the scratch; -1: the caller's (level 0) or none
    std::vector<int64_t> mask_off;  // ... of the level's mask; -1: the caller's or none
    // the running sums: bytes of level images and masks, elements of the pixel / candidate / key spaces
    int64_t img_bytes = 0, pix_elems = 0, cand_elems = 0, sort_elems = 0;
    // byte offsets of the sections behind the level images, and the whole
    int64_t o_mag = 0, o_ori = 0, o_quant = 0, o_flags = 0, o_cand = 0, o_keys = 0, o_sel = 0, o_kept = 0, o_counts = 0, o_table = 0, total = 0;
    int grid_maxima = 1;               // grid x of k_train_maxima: the largest level-0 image
    int grid_level[SBM_MAX_LEVELS] = {}; // grid x of the level steps that make level l (0: nothing to make)
    int any_mask = 0;
};

// bytes of the sections from the four sums (every sum is a multiple of 256)
inline void train_ragged_sections(TrainRaggedPlan& p)
{
    const int64_t N = (int64_t)p.n * p.L;
    p.o_mag = p.img_bytes;
    p.o_ori = p.o_mag + p.pix_elems * 4;
    p.o_quant = p.o_ori + p.pix_elems * 4;
    p.o_flags = p.o_quant + p.pix_elems;
    p.o_cand = p.o_flags + p.pix_elems;
    p.o_keys = p.o_cand + p.cand_elems * (int64_t)sizeof(TrainCand);
    p.o_sel = p.o_keys + p.sort_elems * 8;
    p.o_kept = p.o_sel + p.cand_elems * 4;
    p.o_counts = p.o_kept + p.cand_elems * 4;
    p.o_table = p.o_counts + train_round256(N * 2 * 4);
    p.total = p.o_table + train_round256(N * (int64_t)sizeof(TrainRecord));
}

inline int train_grid_x(int64_t items) { return (int)std::min<int64_t>(std::max<int64_t>((items + 255) / 256, 1), 4096); }

// images: read for sizes, counts and whether the pointers are null; never dereferenced
inline TrainRaggedPlan train_ragged_plan(const sbm_train_image* images, int n, int ch, int L)
{
    TrainRaggedPlan p;
    p.L = L, p.n = n, p.ch = ch;
    auto bad = [&](int e, int i) {
        p.error = e, p.error_image = i;
        return p;
    };
    if (n < 1 || n > 65535 || !images) return bad(TRP_COUNT, -1);
    if (ch != 1 && ch != 3) return bad(TRP_CHANNELS, -1);
    for (int i = 0; i < n; ++i)
        if (images[i].rows < 1 || images[i].cols < 1 || images[i].rows > 32767 || images[i].cols > 32767) return bad(TRP_GEOMETRY, i);
    for (int i = 0; i < n; ++i)
        if (images[i].stride < images[i].cols * ch) return bad(TRP_STRIDE, i);
    for (int i = 0; i < n; ++i)
        if (images[i].num_features < 1 || train_level_features((size_t)images[i].num_features, L - 1) < TRAIN_MIN_FEATURES) return bad(TRP_FEATURES, i);
    for (int i = 0; i < n; ++i)
        if (images[i].feat_cap < 0 || images[i].feat_first < 0 || images[i].feat_first > INT64_MAX - images[i].feat_cap) return bad(TRP_FEAT_CAP, i);
    {
        std::vector<std::pair<int64_t, int>> blocks; // (first, image) of the blocks that hold a record
        for (int i = 0; i < n; ++i)
            if (images[i].feat_cap > 0) blocks.push_back(std::make_pair(images[i].feat_first, i));
        std::sort(blocks.begin(), blocks.end());
        for (size_t k = 1; k < blocks.size(); ++k) {
            const sbm_train_image& a = images[blocks[k - 1].second];
            if (a.feat_first + a.feat_cap > blocks[k].first) return bad(TRP_OVERLAP, std::max(blocks[k - 1].second, blocks[k].second));
        }
    }
    for (int i = 0; i < n; ++i)
        if (!images[i].img) return bad(TRP_NULL_IMAGE, i);

    const size_t N = (size_t)n * (size_t)L;
    p.table.resize(N);
    p.img_off.assign(N, -1);
    p.mask_off.assign(N, -1);
    int64_t max_px[SBM_MAX_LEVELS] = {};
    for (int i = 0; i < n; ++i) {
        const sbm_train_image& im = images[i];
        p.any_mask = p.any_mask || im.mask != nullptr;
        int r = im.rows, c = im.cols;
        bool built = true;
        for (int l = 0; l < L; ++l) {
            if (l) r /= 2, c /= 2;
            built = built && r >= TRAIN_MIN_SIDE && c >= TRAIN_MIN_SIDE;
            const size_t k = (size_t)i * L + l;
            TrainRecord& v = p.table[k];
            v.rows = built ? r : 0;
            v.cols = built ? c : 0;
            v.cand_cap = built ? (int32_t)train_cand_bound(r, c) : 0;
            v.nf = (uint32_t)train_level_features((size_t)im.num_features, l);
            v.pix_off = p.pix_elems;
            v.cand_off = p.cand_elems;
            v.sort_off = p.sort_elems;
            v.mask = nullptr;
            v.mask_fs = 0;
            v.img = nullptr;
            v.stride = l ? v.cols * ch : im.stride;
            v.reserved = 0;
            v.feat_first = im.feat_first;
            v.feat_cap = im.feat_cap;
            if (!built) continue;
            const int64_t npx = (int64_t)r * c;
            int64_t pow2 = 1;
            while (pow2 < v.cand_cap) pow2 <<= 1;
            p.pix_elems += train_round256(npx);
            p.cand_elems += train_round256(v.cand_cap);
            p.sort_elems += train_round256(pow2);
            max_px[l] = std::max(max_px[l], npx);
            if (l > 0) { // the level's image (pyrDown) and mask (nearest neighbour) live in the scratch
                p.img_off[k] = p.img_bytes;
                p.img_bytes += train_round256(npx * ch + 64);
                if (im.mask) {
                    p.mask_off[k] = p.img_bytes;
                    p.img_bytes += train_round256(npx);
                }
            }
        }
    }
    p.grid_maxima = train_grid_x(max_px[0]);
    for (int l = 1; l < L; ++l) p.grid_level[l] = max_px[l] ? train_grid_x(max_px[l]) : 0;
    train_ragged_sections(p);
    return p;
}

// the addresses: level 0 from the caller's descriptors, the levels below from the scratch at `base`
inline void train_ragged_bind(TrainRaggedPlan& p, const sbm_train_image* images, uint8_t* base)
{
    for (int i = 0; i < p.n; ++i)
        for (int l = 0; l < p.L; ++l) {
            const size_t k = (size_t)i * p.L + l;
            TrainRecord& v = p.table[k];
            if (l == 0) {
                v.img = (const uint8_t*)images[i].img;
                v.mask = (const uint8_t*)images[i].mask;
            } else {
                v.img = p.img_off[k] >= 0 ? base + p.img_off[k] : nullptr;
                v.mask = p.mask_off[k] >= 0 ? base + p.mask_off[k] : nullptr;
            }
        }
}

} // namespace sbm
