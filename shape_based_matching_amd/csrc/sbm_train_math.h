// sbm_train_math.h — the scalar pieces of batched template training (sbm_train_kernels.h): the candidate order, the
// distance predicate and pass control of selectScatteredFeatures, the row-major tie resolution among equal local maxima
// and the arithmetic of cropTemplates.  Plain C++, host and device: tests/test_train_select.py compiles the host pass
// (tests/emu/train_select_emu.cpp walks the kernels' dataflow with these functions) and checks it against the oracle's
// add_template.  References are file:line of the reference's line2Dup.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sbm {

#if defined(__HIPCC__)
#define SBM_TRAIN_HD __host__ __device__ __forceinline__
#else
#define SBM_TRAIN_HD inline
#endif

// No two accepted maxima lie within Chebyshev distance 2 of each other, so every 3 x 3 cell of the level holds at most
// one: the bound on accepted maxima, hence on candidates and on selected features, that the scratch is sized from.
SBM_TRAIN_HD int64_t train_cand_bound(int rows, int cols) { return (int64_t)((rows + 2) / 3) * ((cols + 2) / 3); }

// num_features of pyramid level `level`: halved per level as size_t (:427)
SBM_TRAIN_HD size_t train_level_features(size_t num_features, int level)
{
    for (int l = 0; l < level; ++l) num_features /= 2;
    return num_features;
}

// ---- order of the candidates: std::stable_sort by score, descending (:522), of a row-major list -------------------------
// One 64-bit key per candidate, sorted in DESCENDING order: the score's bits (scores are positive floats, whose bits
// order as the values do) above the complement of the row-major index, so equal scores keep row-major order.  0 is below
// every key of a candidate (padding).
SBM_TRAIN_HD uint64_t train_key(uint32_t score_bits, uint32_t index) { return ((uint64_t)score_bits << 32) | (uint64_t)(0xffffffffu - index); }
SBM_TRAIN_HD uint32_t train_key_index(uint64_t key) { return 0xffffffffu - (uint32_t)key; }

// ---- selectScatteredFeatures (:163-212) -------------------------------------------------------------------------------
// a candidate is taken when it is at least `distance` away from every feature taken so far: compared as floats (:189)
SBM_TRAIN_HD bool train_far(int ax, int ay, int bx, int by, float distance_sq)
{
    const int dx = ax - bx, dy = ay - by;
    return (float)(dx * dx + dy * dy) >= distance_sq;
}

// the level fails, and with it the template, when there are at most four candidates and fewer than asked for
SBM_TRAIN_HD bool train_level_fails(size_t n_candidates, size_t num_features) { return n_candidates <= 4 && n_candidates < num_features; }

struct TrainSelect {
    float distance;
    bool growing;
};
enum { TRAIN_PASS_STOP = 0, TRAIN_PASS_KEEP = 1, TRAIN_PASS_RESTART = 2 };

// num_features >= 1
SBM_TRAIN_HD TrainSelect train_select_begin(size_t n_candidates, size_t num_features)
{
    TrainSelect s;
    s.distance = (float)(n_candidates / num_features + 1); // integer division (:525)
    s.growing = true;
    return s;
}

// After one sweep over the candidates at s.distance that left `kept` features: while growing, a sweep that yields enough
// clears them and runs again one further apart; the first that does not starts the shrinking phase, which keeps what is
// chosen and sweeps again one closer until there are enough or the distance falls below 3.
SBM_TRAIN_HD int train_select_next(TrainSelect& s, size_t kept, size_t num_features)
{
    const bool enough = kept >= num_features;
    if (s.growing) {
        if (enough) {
            s.distance += 1.0f;
            return TRAIN_PASS_RESTART;
        }
        s.growing = false;
    }
    s.distance -= 1.0f;
    return (enough || s.distance < 3) ? TRAIN_PASS_STOP : TRAIN_PASS_KEEP;
}

// ---- row-major tie resolution ----------------------------------------------------------------------------------------
// Within a row, walking left to right over the pixels that are `available` (in S and not within two rows and two columns
// of a pixel kept in the two rows above): a pixel is kept iff no pixel was kept in the two columns before it.  The state
// is the number of columns the last kept pixel still blocks (0, 1, 2); a column is a map of the state, packed as three
// 2-bit values (the image of state s in bits 2s, 2s+1), and maps compose associatively: a prefix composition over the
// row gives every column its incoming state.
enum { TRAIN_TIE_IDENTITY = 0x24 }; // 0 -> 0, 1 -> 1, 2 -> 2
SBM_TRAIN_HD uint32_t train_tie_fn(bool available) { return available ? 0x12u : 0x10u; } // 0 -> 2 (kept) | 0; 1 -> 0; 2 -> 1
SBM_TRAIN_HD uint32_t train_tie_apply(uint32_t f, uint32_t state) { return (f >> (2 * state)) & 3u; }
SBM_TRAIN_HD bool train_tie_keeps(bool available, uint32_t state) { return available && state == 0; }
// f first, then g
SBM_TRAIN_HD uint32_t train_tie_compose(uint32_t f, uint32_t g)
{
    return train_tie_apply(g, train_tie_apply(f, 0)) | (train_tie_apply(g, train_tie_apply(f, 1)) << 2) | (train_tie_apply(g, train_tie_apply(f, 2)) << 4);
}

// ---- cropTemplates (:115-161) ------------------------------------------------------------------------------------------
// min / max over the features of every level of x << level, y << level; the minima made even
SBM_TRAIN_HD int train_crop_even(int v) { return (v % 2 == 1) ? v - 1 : v; }
struct TrainBox {
    int width, height, tl_x, tl_y;
};
// min_x, min_y already even
SBM_TRAIN_HD TrainBox train_crop_level(int min_x, int min_y, int max_x, int max_y, int level)
{
    TrainBox b;
    b.width = (max_x - min_x) >> level;
    b.height = (max_y - min_y) >> level;
    b.tl_x = min_x >> level;
    b.tl_y = min_y >> level;
    return b;
}

} // namespace sbm
