// TEST INFRASTRUCTURE: the dataflow of the batched training kernels (csrc/sbm_train_kernels.h) on the CPU, built from
// the scalar pieces the kernels share (csrc/sbm_train_math.h): 64 lanes as loops, the wave's prefix scans as array
// scans, a ballot as a 64-bit mask.  tests/test_train_select.py compiles this file (-Wall -Wextra -Werror) and checks it
// against the oracle's add_template.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <vector>

#include "sbm_train_math.h"

using namespace sbm;

namespace {

struct Cand {
    int32_t xy, label;
    float score, theta;
};

// k_train_maxima: the dense flag plane of S
std::vector<uint8_t> maxima_flags(const float* mag, const uint8_t* mask, int rows, int cols, float thr_sq)
{
    std::vector<uint8_t> flags((size_t)rows * cols, 0);
    for (int r = 2; r < rows - 2; ++r)
        for (int c = 2; c < cols - 2; ++c) {
            const int idx = r * cols + c;
            const float s = mag[idx];
            bool in = s > thr_sq;
            if (in && mask)
                for (int dr = -1; dr <= 1; ++dr)
                    for (int dc = -1; dc <= 1; ++dc) in = in && mask[idx + dr * cols + dc] != 0;
            if (in)
                for (int dr = -2; dr <= 2; ++dr)
                    for (int dc = -2; dc <= 2; ++dc) in = in && !(s < mag[idx + dr * cols + dc]);
            flags[idx] = in ? 1 : 0;
        }
    return flags;
}

// k_train_resolve: lane i owns the columns [i * K, (i + 1) * K)
std::vector<Cand> resolve(std::vector<uint8_t>& flags, const float* mag, const uint8_t* quant, const float* ori, int rows, int cols)
{
    std::vector<Cand> cand;
    const int K = (cols + 63) / 64;
    for (int r = 2; r < rows - 2; ++r) {
        uint8_t* f0 = flags.data() + (size_t)r * cols;
        const uint8_t* f1 = f0 - cols;
        const uint8_t* f2 = f1 - cols;
        auto available = [&](int c) {
            if (!(f0[c] & 1)) return false;
            uint32_t above = 0;
            for (int d = -2; d <= 2; ++d) above |= (uint32_t)f1[c + d] | (uint32_t)f2[c + d];
            return (above & 2u) == 0;
        };
        uint32_t f[64];
        for (int lane = 0; lane < 64; ++lane) {
            const int c0 = std::min(lane * K, cols), c1 = std::min(c0 + K, cols);
            f[lane] = TRAIN_TIE_IDENTITY;
            for (int c = c0; c < c1; ++c) f[lane] = train_tie_compose(f[lane], train_tie_fn(available(c)));
        }
        for (int d = 1; d < 64; d <<= 1) { // the wave's inclusive scan, step by step as the shuffles do it
            uint32_t g[64];
            for (int lane = 0; lane < 64; ++lane) g[lane] = lane >= d ? f[lane - d] : 0;
            for (int lane = 0; lane < 64; ++lane)
                if (lane >= d) f[lane] = train_tie_compose(g[lane], f[lane]);
        }
        for (int lane = 0; lane < 64; ++lane) {
            const int c0 = std::min(lane * K, cols), c1 = std::min(c0 + K, cols);
            uint32_t state = lane ? train_tie_apply(f[lane - 1], 0) : 0u;
            for (int c = c0; c < c1; ++c) {
                const bool a = available(c);
                if (train_tie_keeps(a, state)) f0[c] = 3;
                state = train_tie_apply(train_tie_fn(a), state);
            }
        }
        for (int c = 0; c < cols; ++c) { // the lanes' segments in lane order are the row in column order
            const uint32_t a = quant[(size_t)r * cols + c];
            if ((f0[c] & 2) && a) {
                int label = 0;
                while (!((a >> label) & 1)) ++label;
                cand.push_back(Cand{c | (r << 16), label, mag[(size_t)r * cols + c], ori[(size_t)r * cols + c]});
            }
        }
    }
    return cand;
}

// k_train_sort + k_train_select
int select(const std::vector<Cand>& cand, size_t nf, std::vector<int32_t>& sel)
{
    const int n = (int)cand.size();
    sel.clear();
    if (train_level_fails((size_t)n, nf)) return -1;
    std::vector<uint64_t> keys((size_t)n);
    for (int i = 0; i < n; ++i) {
        uint32_t bits;
        memcpy(&bits, &cand[(size_t)i].score, 4);
        keys[(size_t)i] = train_key(bits, (uint32_t)i);
    }
    std::sort(keys.begin(), keys.end(), [](uint64_t a, uint64_t b) { return a > b; });
    std::vector<uint32_t> kept;
    TrainSelect st = train_select_begin((size_t)n, nf);
    for (;;) {
        const float d2 = st.distance * st.distance;
        for (int first = 0; first < n; first += 64) {
            int idx[64] = {}, xy[64] = {};
            uint64_t m = 0;
            const size_t before = kept.size();
            for (int lane = 0; lane < 64 && first + lane < n; ++lane) {
                idx[lane] = (int)train_key_index(keys[(size_t)(first + lane)]);
                xy[lane] = cand[(size_t)idx[lane]].xy;
                bool alive = true;
                for (size_t j = 0; j < before; ++j) alive = alive && train_far(xy[lane] & 0xffff, xy[lane] >> 16, (int)(kept[j] & 0xffffu), (int)(kept[j] >> 16), d2);
                if (alive) m |= 1ull << lane;
            }
            while (m) {
                const int k = __builtin_ctzll(m);
                kept.push_back((uint32_t)xy[k]);
                sel.push_back(idx[k]);
                m &= ~(1ull << k);
                for (int lane = 0; lane < 64; ++lane)
                    if (((m >> lane) & 1) && !train_far(xy[lane] & 0xffff, xy[lane] >> 16, xy[k] & 0xffff, xy[k] >> 16, d2)) m &= ~(1ull << lane);
            }
        }
        const int next = train_select_next(st, kept.size(), nf);
        if (next == TRAIN_PASS_STOP) break;
        if (next == TRAIN_PASS_RESTART) {
            kept.clear();
            sel.clear();
        }
    }
    return (int)sel.size();
}

} // namespace

extern "C" {

// One image: per level l the planes at mag[l] / quant[l] / ori[l] / mask[l] (mask: NULL or an array with NULL entries = no
// mask).  levels_out: [n_levels][6] width, height, tl_x, tl_y, pyramid_level, n_features; feats_out: [cap][4] x, y,
// label, theta bits, level after level.  Returns the number of features, -1 - l when level l fails, INT_MIN when cap is
// too small.
int sbm_emu_train_image(int n_levels, const float* const* mag, const uint8_t* const* quant, const float* const* ori, const uint8_t* const* mask,
                        const int32_t* rows, const int32_t* cols, int32_t num_features, float strong, int32_t* levels_out, int32_t* feats_out,
                        int64_t cap)
{
    std::vector<std::vector<Cand>> cands((size_t)n_levels);
    std::vector<std::vector<int32_t>> sels((size_t)n_levels);
    int failed = -1;
    for (int l = 0; l < n_levels; ++l) {
        std::vector<uint8_t> flags = maxima_flags(mag[l], mask ? mask[l] : nullptr, rows[l], cols[l], strong * strong);
        cands[(size_t)l] = resolve(flags, mag[l], quant[l], ori[l], rows[l], cols[l]);
        if ((int64_t)cands[(size_t)l].size() > train_cand_bound(rows[l], cols[l])) return INT_MIN + 1; // the bound the scratch is sized from
        if (select(cands[(size_t)l], train_level_features((size_t)num_features, l), sels[(size_t)l]) < 0 && failed < 0) failed = l;
    }
    if (failed >= 0) return -1 - failed;
    // k_train_crop
    int64_t total = 0;
    int min_x = INT_MAX, min_y = INT_MAX, max_x = INT_MIN, max_y = INT_MIN;
    for (int l = 0; l < n_levels; ++l) {
        total += (int64_t)sels[(size_t)l].size();
        for (int32_t i : sels[(size_t)l]) {
            const int xy = cands[(size_t)l][(size_t)i].xy;
            const int x = (xy & 0xffff) << l, y = (xy >> 16) << l;
            min_x = std::min(min_x, x), min_y = std::min(min_y, y), max_x = std::max(max_x, x), max_y = std::max(max_y, y);
        }
    }
    if (total > cap) return INT_MIN;
    min_x = train_crop_even(min_x);
    min_y = train_crop_even(min_y);
    int64_t off = 0;
    for (int l = 0; l < n_levels; ++l) {
        const TrainBox b = train_crop_level(min_x, min_y, max_x, max_y, l);
        const int32_t rec[6] = {b.width, b.height, b.tl_x, b.tl_y, l, (int32_t)sels[(size_t)l].size()};
        memcpy(levels_out + 6 * l, rec, sizeof rec);
        for (int32_t i : sels[(size_t)l]) {
            const Cand& c = cands[(size_t)l][(size_t)i];
            int32_t* f = feats_out + 4 * off++;
            f[0] = (c.xy & 0xffff) - b.tl_x;
            f[1] = (c.xy >> 16) - b.tl_y;
            f[2] = c.label;
            memcpy(&f[3], &c.theta, 4);
        }
    }
    return (int)total;
}

} // extern "C"
