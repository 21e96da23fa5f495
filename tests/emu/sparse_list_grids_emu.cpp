// TEST INFRASTRUCTURE: the sparse level-0 gradient launch with its lists of working items made on a row grid of their own
// (sbm_quantize_stream.h: QSArgs::list_hs, quantize_stream_slot_wave) and the rows-per-item rules of the gradient launches
// (sbm_quantize_rows_plan.h), compiled for the CPU against wave_emu.h behind a C interface, beside what sparse_list_emu.cpp already
// offers (the mark, the lists on any grid, the whole map).  Compiled by tests/test_sparse_list_grids.py into its temporary
// directory; never loaded by the product.
#include "sparse_list_emu.cpp"

#include "sbm_quantize_rows_plan.h"

// The sparse pass by slots as the host launches it, on two row grids: the launch's own, `hs` rows per item -- what a frame whose
// count is RT_LIST_NONE walks, what the packed last-strip waves run, what the waves launched follow -- and the lists', `list_hs`
// rows per item, whose row blocks the entries name.  Otherwise sbm_emu_sparse_slots_pass.
extern "C" int sbm_emu_sparse_grids_pass(const uint8_t* keep, int frames, int rows, int cols, int ch, float weak, int hs, int list_hs,
                                         const uint8_t* flags, const int32_t* rects, const int32_t* lists, int64_t list_stride, int list_cap,
                                         int slots, int T, int W, int H, uint8_t* out, int32_t* waves)
{
    if (bad_geometry(frames, rows, cols, ch, hs) || slots < 1 || list_hs < 2 || (list_hs & 1)) return -1;
    QSArgs a = batch_args(keep, frames, rows, cols, ch, weak, hs, 1);
    a.out = out;
    a.tile_flags = flags;
    a.n_tiles = refine_tile_count(W, H);
    a.grid_t = T;
    a.grid_w = W;
    a.grid_h = H;
    a.need_rects = rects;
    a.n_bands = refine_band_count(rows);
    a.item_list = lists;
    a.list_stride = list_stride;
    a.list_cap = list_cap;
    a.slots = slots;
    a.list_hs = list_hs;
    a.list_n_rblocks = (rows + list_hs - 1) / list_hs;
    int32_t count = 0;
    a.item_count = &count;
    if (waves) *waves = frames * slots + quantize_slots_packed(a);
    for (int g = 0; g < quantize_slots_groups(a); ++g)
        for (int q = 0; q < 4; ++q) {
            if (ch == 3) quantize_stream_slot_wave<3>(a, g, q);
            else quantize_stream_slot_wave<1>(a, g, q);
        }
    return count;
}

// waves per row block of a whole-level launch on packed frames: one per strip and frame, a narrow last strip shared
extern "C" int sbm_emu_waves_per_row_block(int frames, int rows, int cols, int ch)
{
    const int n_strips = (cols + QS_USEFUL - 1) / QS_USEFUL;
    const int pack = quantize_stream_pack_lanes(rows, cols, ch, frames);
    return pack ? (n_strips - 1) * frames + (frames + 64 / pack - 1) / (64 / pack) : n_strips * frames;
}
extern "C" int sbm_emu_rows_throughput(int per_rb, int out_rows, int n_simd) { return qs_rows_throughput(per_rb, out_rows, n_simd); }
extern "C" int sbm_emu_rows_latency(int per_rb, int out_rows, int slots) { return qs_rows_latency(per_rb, out_rows, slots); }
