// sbm_quantize_rows_plan.h — rows per work item of the streaming gradient kernel (sbm_quantize_stream.h) for one launch: the
// arithmetic of quantize_stream_rows (sbm_capi_ctx.inc).  Plain integer code, no HIP types: the host uses it,
// tests/test_sparse_list_grids.py compiles it for the CPU suite.
//
// A launch has per_rb waves per row block (one per strip and frame, a packed last strip shared by several frames) and
// ceil(out_rows / hs) row blocks.  Every wave runs whole groups of 7 row iterations: its hs rows and 10 of warm-up and drain,
// rounded up -- so the candidates differ only where hs + 10 passes a multiple of 7 (32 rows: 42 iterations, 24: 35, 18: 28, 10: 21).
#pragma once
#include <stdint.h>

namespace sbm {

constexpr int QS_ROWS_THROUGHPUT_MAX = 32; // items longer than 42 iterations stopped paying (profiles/r03_rows_per_item_sweep.txt)
constexpr int QS_ROWS_LATENCY_MAX = 130;

inline int64_t qs_rows_waves(int64_t per_rb, int out_rows, int h) { return per_rb * ((out_rows + h - 1) / h); }
inline int64_t qs_rows_iterations(int out_rows, int h) { return ((h < out_rows ? h : out_rows) + 10 + 6) / 7 * 7; }

// Latency sizing (one batch at a time): every work item resident at once, as few row iterations as that allows.
// slots: the waves the chip holds of this kernel (3 per SIMD at the BGR kernel's registers, 6 gray)
inline int qs_rows_latency(int64_t per_rb, int out_rows, int64_t slots)
{
    int hs = 0;
    int64_t best = INT64_MAX;
    for (int h = 4; h <= QS_ROWS_LATENCY_MAX; h += 2) {
        const int64_t cost = ((qs_rows_waves(per_rb, out_rows, h) + slots - 1) / slots) * qs_rows_iterations(out_rows, h);
        if (cost <= best) best = cost, hs = h;
    }
    return hs;
}

// The least total work of a launch, waves x row iterations, among even h in 4 .. 32 whose launch has at least min_waves waves
// (min_waves 0: among all of them).  0: no h has that many.
inline int qs_rows_least_work(int64_t per_rb, int out_rows, int64_t min_waves)
{
    int hs = 0;
    int64_t best = INT64_MAX;
    for (int h = 4; h <= QS_ROWS_THROUGHPUT_MAX; h += 2) {
        const int64_t waves = qs_rows_waves(per_rb, out_rows, h);
        if (waves < min_waves) continue;
        const int64_t cost = waves * qs_rows_iterations(out_rows, h);
        if (cost <= best) best = cost, hs = h;
    }
    return hs;
}

// Throughput sizing (the caller keeps several batches in flight): the least total work among the launches that put a wave on every
// SIMD.  The launches of a match call are a chain, each waiting for the one before, and a launch lasts as long as one of its
// waves: with fewer waves than SIMDs the item's length is paid in the chain while part of the chip holds none of its waves, and
// the other batches in flight do not make that up (profiles/gradient_item_sizing.txt).  A launch whose least-work form already
// has a wave per SIMD keeps it -- level 0 of a whole build at 4 Mpixel and more --; where no h reaches a wave per SIMD, the
// launch with the most waves, the shortest items.
// What the bound can cost: quantize_stream_rows sends launches of less than 4 Mpixel to the tile kernel unless the stream mode is
// forced, and a launch of 4 Mpixel has at least 576 waves at 32 rows (4 frames of 1024^2: 18 per row block; one frame of 2048^2: 9
// per row block, 64 blocks), so it reaches a wave per SIMD of a 1024-SIMD chip at 16 - 18 rows, 28 iterations, for 1.2 - 1.35
// times the least total work.  The shortest items, 14 iterations for 4 rows and 2.7 times the work, come up only where a caller
// forces the streaming kernel on a launch too small for it.
inline int qs_rows_throughput(int64_t per_rb, int out_rows, int n_simd)
{
    const int any = qs_rows_least_work(per_rb, out_rows, 0);
    if (qs_rows_waves(per_rb, out_rows, any) >= n_simd) return any;
    const int filled = qs_rows_least_work(per_rb, out_rows, n_simd);
    return filled ? filled : 4;
}

} // namespace sbm
