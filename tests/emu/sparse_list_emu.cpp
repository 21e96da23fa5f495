// TEST INFRASTRUCTURE: the lists of working items of the sparse level-0 gradient pass (sbm_refine_tiles.h: gradient_rect_list) and
// the launch that runs from them by slots (sbm_quantize_stream.h: quantize_stream_slot_wave), compiled for the CPU against
// wave_emu.h behind a C interface, beside what sparse_rects_emu.cpp already offers (the mark, the items of the fixed grid, the whole
// map).  Compiled by tests/test_sparse_list.py into its temporary directory; never loaded by the product.
#include "sparse_rects_emu.cpp"

// One frame's list as k_mark_refine_tiles writes it: list = RT_LIST_HEAD + RT_LIST_ENTRY * capacity int32, the count in front (cut
// to the capacity), then {k, rb, x_first, 0} per working item of the n_full x ceil(rows / hs) grid.  Returns the working items found.
extern "C" int sbm_emu_list(const int32_t* rects, const uint8_t* flags, int rows, int cols, int hs, int n_full, int T, int W, int H, int32_t* list,
                            int capacity)
{
    const int n_rblocks = (rows + hs - 1) / hs;
    int n = 0;
    gradient_rect_list(rects, flags, n_full, n_rblocks, hs, QS_USEFUL, rows, cols, T, W, H, 0, 1, [&](int k, int rb, int x0) {
        const int slot = n++;
        if (slot >= capacity) return;
        int32_t* e = list + RT_LIST_HEAD + RT_LIST_ENTRY * (int64_t)slot;
        e[0] = k, e[1] = rb, e[2] = x0, e[3] = 0;
    });
    list[0] = n < capacity ? n : capacity;
    return n;
}

// the strips of this geometry that get a wave per frame in a launch of `frames` frames (a narrow last strip is packed)
extern "C" int sbm_emu_n_full(int frames, int rows, int cols, int ch)
{
    const int n_strips = (cols + QS_USEFUL - 1) / QS_USEFUL;
    return quantize_stream_pack_lanes(rows, cols, ch, frames) ? n_strips - 1 : n_strips;
}

// The sparse pass by slots, as the host launches it: every wave of every workgroup of the grid.  lists: frames x list_stride int32
// (a frame whose count is RT_LIST_NONE tests its own items), list_cap: what the kernel cuts a count to.  waves (may be null):
// receives the waves launched.  Returns the working items (counted as under profiling), or -1.
extern "C" int sbm_emu_sparse_slots_pass(const uint8_t* keep, int frames, int rows, int cols, int ch, float weak, int hs, const uint8_t* flags,
                                         const int32_t* rects, const int32_t* lists, int64_t list_stride, int list_cap, int slots, int T, int W, int H,
                                         uint8_t* out, int32_t* waves)
{
    if (bad_geometry(frames, rows, cols, ch, hs) || slots < 1) return -1;
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
