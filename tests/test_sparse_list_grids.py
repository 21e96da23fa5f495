"""CPU (not gpu): the sparse level-0 gradient launch on two row grids, and the rows-per-item rules of the gradient launches.

A frame of few candidates has a list of its working items, and those items are better short: k_mark_refine_tiles makes the lists
on a row grid of their own, the LIST grid (QSArgs::list_hs rows per item).  A frame without a list -- more than 256 candidates, or
none -- walks the launch's own grid, the FIXED grid (QSArgs::hs), as do the packed last-strip waves; the waves launched are the
fixed grid's.  Compiled here for the CPU (tests/emu/sparse_list_grids_emu.cpp):

  list        gradient_rect_list on the list grid lists exactly the items of that grid that meet the need: the plain enumeration of
              gradient_rect_item_needed over every (k, rb) of that grid, each once with its x_first, and the listed items' rectangles
              cover every pixel of every need rectangle
  emulation   quantize_stream_slot_wave with (fixed, list) = (32, 18), (32, 16), (24, 10), (32, 32) gives the whole kernel's map
              on every pixel of every need rectangle and writes nothing else that differs -- three frames of 96 x 576 x 3 with a whole
              and a partial group of the packed strip, 448 x 576 BGR (448 is no multiple of 18 or 10: the last block is moved up;
              the last tile column is cut), 512 x 704 gray -- with one frame listed, one on RT_LIST_NONE and one empty in the same
              launch, a list count of 0, and an entry in the last, moved-up row block
  sizing      qs_rows_throughput / qs_rows_latency (sbm_quantize_rows_plan.h) as a table over n_simd 4 / 1024, 1 / 16 / 64 frames,
              512^2 and 1024^2 levels, BGR and gray, against the rule restated here; with one batch at a time (depth 1) every row
              has the value of the rule as it was before the launches were sized by the SIMDs"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_sparse_list import ENTRY, HEAD, NONE, USEFUL, check_map, enumerate_items, make_list, mark
from test_sparse_rects import BAND, GEOMETRIES, POISON, T, make_frames

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
GRIDS = [(32, 18), (32, 16), (24, 10), (32, 32)]  # (rows per item of the fixed grid, of the list grid)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("sparse_list_grids_emu") / "libsparse_list_grids_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-variable",
                           "-Wno-unused-but-set-variable", "-Wno-unknown-pragmas", "-I", EMU_DIR, "-I", CSRC, "-o", so,
                           os.path.join(EMU_DIR, "sparse_list_grids_emu.cpp")])
    L = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    L.sbm_emu_mark.argtypes = [C.c_int64, vp, i, i, i, i, i, vp, vp, vp]
    L.sbm_emu_items.argtypes = [vp, vp, i, i, i, i, i, i, vp]
    L.sbm_emu_whole_map.argtypes = [vp, i, i, i, i, C.c_float, i, vp]
    L.sbm_emu_list.argtypes = [vp, vp, i, i, i, i, i, i, i, vp, i]
    L.sbm_emu_n_full.argtypes = [i, i, i, i]
    L.sbm_emu_sparse_grids_pass.argtypes = [vp, i, i, i, i, C.c_float, i, i, vp, vp, vp, C.c_int64, i, i, i, i, i, vp, vp]
    L.sbm_emu_waves_per_row_block.argtypes = [i, i, i, i]
    L.sbm_emu_rows_throughput.argtypes = [i, i, i]
    L.sbm_emu_rows_latency.argtypes = [i, i, i]
    return L


def item_rows(rb, hs, rows):
    """output rows of row block rb (sbm_refine_tiles.h: gradient_item_rows): the last block is moved up to end at the last row"""
    r0 = rb * hs
    if r0 + hs > rows:
        r0 = rows - hs if rows > hs else 0
    return r0, min(r0 + hs, rows)


@pytest.fixture(scope="module")
def scenes(emu):
    """per geometry of test_sparse_rects: frames, flags, hulls, the whole kernel's map (computed once) and the needed pixels"""
    out = {}
    for (rows, cols, ch), per_frame in GEOMETRIES.items():
        n = len(per_frame)
        frames = make_frames(n, rows, cols, ch, 31 + rows + ch)
        marks = [mark(emu, c, rows, cols) for c in per_frame]
        flags = np.ascontiguousarray(np.stack([m[0] for m in marks]))
        rects = np.ascontiguousarray(np.stack([m[1] for m in marks]))
        want = np.full((n, rows, cols), POISON, np.uint8)
        assert emu.sbm_emu_whole_map(frames.ctypes.data, n, rows, cols, ch, 30.0, 32, want.ctypes.data) == 0
        needed = np.zeros((n, rows, cols), bool)
        for f in range(n):
            for b, (lo, hi) in enumerate(rects[f]):
                if lo < hi:
                    needed[f, b * BAND: (b + 1) * BAND, lo:hi] = True
        assert needed.any()
        want.setflags(write=False)
        out[(rows, cols, ch)] = dict(frames=frames, flags=flags, rects=rects, want=want, needed=needed, n=n, per_frame=per_frame)
    return out


# ---- the list on the list grid ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols,ch", list(GEOMETRIES), ids=["96x576x3", "448x576x3", "512x704x1"])
@pytest.mark.parametrize("list_hs", [10, 16, 18, 32])
def test_the_list_holds_exactly_the_items_of_its_own_grid_that_meet_the_need(emu, scenes, rows, cols, ch, list_hs):
    sc = scenes[(rows, cols, ch)]
    n_strips = (cols + USEFUL - 1) // USEFUL
    n_rb = (rows + list_hs - 1) // list_hs
    room = n_strips * ((rows + 1) // 2)
    assert n_strips * n_rb <= room  # the lists have room for every item of any grid of even rows per item
    for f in range(sc["n"]):
        want = enumerate_items(emu, sc["rects"][f], sc["flags"][f], rows, cols, list_hs, n_strips)
        lst, n = make_list(emu, sc["rects"][f], sc["flags"][f], rows, cols, list_hs, n_strips, room)
        ent = lst[HEAD: HEAD + ENTRY * n].reshape(n, ENTRY)
        got = {(int(k), int(rb)): int(x) for k, rb, x, _ in ent}
        assert n == lst[0] == len(want) and len(got) == n and got == want, (f, list_hs)
        assert all(0 <= rb < n_rb and 0 <= k < n_strips for k, rb in got)
        # every needed pixel lies in a listed item's rectangle: rows of ITS grid, `useful` columns from its x_first
        covered = np.zeros((rows, cols), bool)
        for (k, rb), x in got.items():
            r0, r1 = item_rows(rb, list_hs, rows)
            covered[r0:r1, x: x + USEFUL] = True
        assert not (sc["needed"][f] & ~covered).any(), (f, list_hs)
        assert bool(got) == bool(sc["per_frame"][f])


# ---- the launch on two grids in the wave emulation ------------------------------------------------------------------------------

def run_grids(emu, sc, rows, cols, ch, hs, list_hs, slots=None, sentinel=(), hide=()):
    """the launch by slots with the lists made on the list grid; frames in `sentinel` keep RT_LIST_NONE, frames in `hide` get a
    list of count 0 whatever their candidates.  Returns the map, the working items counted, the waves launched, the items expected"""
    n = sc["n"]
    W, H = cols // T, rows // T
    n_strips = (cols + USEFUL - 1) // USEFUL
    n_full = emu.sbm_emu_n_full(n, rows, cols, ch)
    n_rb = (rows + hs - 1) // hs
    S = n_full * n_rb if slots is None else slots  # the fixed grid's items per frame
    room = n_strips * ((rows + 1) // 2)
    stride = HEAD + ENTRY * room
    lists = np.zeros((n, stride), np.int32)
    expect = 0
    for f in range(n):
        lst, cnt = make_list(emu, sc["rects"][f], sc["flags"][f], rows, cols, list_hs, n_full, room)
        lists[f] = lst
        if f in sentinel:
            lists[f, 0] = NONE  # its waves test the items of the FIXED grid themselves
            expect += len(enumerate_items(emu, sc["rects"][f], sc["flags"][f], rows, cols, hs, n_full))
        elif f in hide:
            lists[f, 0] = 0
        else:
            expect += cnt
        # the packed last-strip waves keep the fixed grid and their own test, listed frame or not
        if n_full < n_strips:
            expect += sum(1 for (k, _) in enumerate_items(emu, sc["rects"][f], sc["flags"][f], rows, cols, hs, n_strips) if k == n_strips - 1)
    GUARD = 4096
    buf = np.full(GUARD + n * rows * cols + GUARD, POISON, np.uint8)
    got = buf[GUARD: GUARD + n * rows * cols].reshape(n, rows, cols)
    waves = C.c_int32(0)
    working = emu.sbm_emu_sparse_grids_pass(sc["frames"].ctypes.data, n, rows, cols, ch, 30.0, hs, list_hs, sc["flags"].ctypes.data,
                                            sc["rects"].ctypes.data, lists.ctypes.data, stride, room, S, T, W, H, got.ctypes.data, C.byref(waves))
    assert (buf[:GUARD] == POISON).all() and (buf[-GUARD:] == POISON).all()  # no byte outside the level
    per_wave = 64 // ((cols - USEFUL * (n_strips - 1)) // 4 + 4)  # frames that share a wave of the packed last strip
    packed = 0 if n_full == n_strips else n_rb * -(-n // per_wave)
    assert waves.value == n * S + packed  # the waves launched are the fixed grid's, whatever the list grid
    return got, working, expect, lists


@pytest.mark.parametrize("rows,cols,ch", list(GEOMETRIES), ids=["96x576x3", "448x576x3", "512x704x1"])
@pytest.mark.parametrize("hs,list_hs", GRIDS, ids=["%d-%d" % g for g in GRIDS])
def test_listed_frames_run_the_items_of_the_list_grid(emu, scenes, rows, cols, ch, hs, list_hs):
    sc = scenes[(rows, cols, ch)]
    got, working, expect, lists = run_grids(emu, sc, rows, cols, ch, hs, list_hs)
    check_map(sc, got)  # byte for byte the whole kernel's map wherever it is needed, nothing else written that differs
    assert working == expect and working > 0
    if not sc["per_frame"][-1]:
        assert lists[-1, 0] == 0  # the empty frame of the batch: a list of count 0
    # fewer slots than entries: the waves loop over the entries of the list grid
    got3, working3, expect3, _ = run_grids(emu, sc, rows, cols, ch, hs, list_hs, slots=3)
    assert np.array_equal(got3, got) and working3 == expect3 == expect


@pytest.mark.parametrize("hs,list_hs", GRIDS, ids=["%d-%d" % g for g in GRIDS])
def test_a_listed_frame_a_frame_without_a_list_and_an_empty_frame_in_one_launch(emu, scenes, hs, list_hs):
    rows, cols, ch = 96, 576, 3
    sc = scenes[(rows, cols, ch)]
    assert sc["per_frame"][0] and sc["per_frame"][1] and not sc["per_frame"][2]
    base, _, _, _ = run_grids(emu, sc, rows, cols, ch, hs, list_hs)
    for sentinel in ((1,), (0,), (0, 1), (2,), (0, 1, 2)):
        got, working, expect, lists = run_grids(emu, sc, rows, cols, ch, hs, list_hs, sentinel=sentinel)
        check_map(sc, got)
        assert working == expect, sentinel
        for f in range(sc["n"]):  # a listed frame's bytes do not depend on what its neighbours are
            if f not in sentinel:
                assert np.array_equal(got[f], base[f]), (sentinel, f)
    # ... and the fixed grid alone gives the map a frame on the sentinel gets
    fixed, _, _, _ = run_grids(emu, sc, rows, cols, ch, hs, hs)
    got, _, _, _ = run_grids(emu, sc, rows, cols, ch, hs, list_hs, sentinel=(0, 1, 2))
    assert np.array_equal(got, fixed)


@pytest.mark.parametrize("hs,list_hs", GRIDS, ids=["%d-%d" % g for g in GRIDS])
def test_a_list_of_count_0_runs_nothing_of_its_frame(emu, scenes, hs, list_hs):
    rows, cols, ch = 512, 704, 1  # (one frame, no packed strip: nothing else could write)
    sc = scenes[(rows, cols, ch)]
    got, working, expect, _ = run_grids(emu, sc, rows, cols, ch, hs, list_hs, hide=(0,))
    assert working == expect == 0 and (got == POISON).all()


@pytest.mark.parametrize("hs,list_hs", GRIDS, ids=["%d-%d" % g for g in GRIDS])
def test_an_entry_in_the_last_moved_up_row_block(emu, scenes, hs, list_hs):
    rows, cols, ch = 448, 576, 3
    sc = scenes[(rows, cols, ch)]
    n_rb = (rows + list_hs - 1) // list_hs
    got, working, expect, lists = run_grids(emu, sc, rows, cols, ch, hs, list_hs)
    ent = lists[0, HEAD: HEAD + ENTRY * lists[0, 0]].reshape(-1, ENTRY)
    last = ent[ent[:, 1] == n_rb - 1]
    assert len(last) > 0  # the object at the bottom edge
    r0, r1 = item_rows(n_rb - 1, list_hs, rows)
    assert r1 == rows and r1 - r0 == list_hs
    if rows % list_hs:
        assert r0 < (n_rb - 1) * list_hs  # moved up: it passes rows of the block above again
    for _, _, x, _ in last:  # its rows are written, down to the last one, and are the whole kernel's
        x1 = min(int(x) + USEFUL, cols)
        assert np.array_equal(got[0, r0:r1, int(x):x1], sc["want"][0, r0:r1, int(x):x1])
    check_map(sc, got)


# ---- the rows per work item of a launch ------------------------------------------------------------------------------------------

def iterations(h, out_rows):
    return (min(h, out_rows) + 10 + 6) // 7 * 7  # whole groups of 7: the item's rows and 10 of warm-up and drain


def least_work(per_rb, out_rows, min_waves):
    best, hs = None, 0
    for h in range(4, 33, 2):
        waves = per_rb * -(-out_rows // h)
        if waves < min_waves:
            continue
        cost = waves * iterations(h, out_rows)
        if best is None or cost <= best:
            best, hs = cost, h
    return hs


def throughput_rule(per_rb, out_rows, n_simd):
    """the least total work among the launches with a wave for every SIMD; the least-work launch itself where it has them; the
    most waves where none has"""
    any_h = least_work(per_rb, out_rows, 0)
    if per_rb * -(-out_rows // any_h) >= n_simd:
        return any_h
    return least_work(per_rb, out_rows, n_simd) or 4


def latency_rule(per_rb, out_rows, slots):
    """every work item resident at once, as few row iterations as that allows (one batch at a time; unchanged)"""
    best, hs = None, 0
    for h in range(4, 131, 2):
        waves = per_rb * -(-out_rows // h)
        cost = -(-waves // slots) * iterations(h, out_rows)
        if best is None or cost <= best:
            best, hs = cost, h
    return hs


SIZING = [(n_simd, frames, side, ch) for n_simd in (4, 1024) for frames in (1, 16, 64) for side in (512, 1024) for ch in (3, 1)]
# worked by hand.  16 x 512^2 x 3: 2 strips x 16 frames + 4 packed groups = 36 waves per row block; 32 rows: 16 blocks, 576 waves
# < 1024; 20 rows: 26 blocks, 936; 18 rows: 29 blocks, 1044 waves of 28 iterations = 29232, and every shorter item costs more
# (10 rows: 1872 x 21 = 39312).  16 x 1024^2 x 3: 70 per row block, 32 rows: 2240 waves -- it keeps 32.
# Gray packs its last strip like BGR: the same 36.  One frame of 1024^2 (5 strips, nothing to pack): 32 rows give 160 waves; only
# 4 rows reach 1024 (256 blocks x 5 = 1280; 6 rows: 171 x 5 = 855).  One frame of 512^2: 3 per row block, 4 rows give 384 -- no
# size has a wave per SIMD, the shortest items.  64 x 512^2: 2 x 64 + 13 = 141 per row block, 2256 waves at 32 rows.
PINNED = {(1024, 16, 512, 3): 18, (1024, 16, 1024, 3): 32, (1024, 64, 512, 3): 32, (1024, 64, 1024, 1): 32, (4, 16, 512, 3): 32, (4, 1, 1024, 1): 32,
          (1024, 16, 512, 1): 18, (1024, 1, 1024, 3): 4, (1024, 1, 512, 3): 4, (1024, 1, 512, 1): 4, (1024, 64, 512, 1): 32, (1024, 16, 1024, 1): 32,
          (4, 1, 512, 3): 32, (4, 64, 1024, 3): 32}
PINNED_LATENCY = {(1024, 16, 1024, 3): 24, (1024, 16, 512, 3): 10}


@pytest.mark.parametrize("n_simd,frames,side,ch", SIZING, ids=["simd%d-%dx%d^2x%d" % s for s in SIZING])
def test_rows_per_item_table(emu, n_simd, frames, side, ch):
    per_rb = emu.sbm_emu_waves_per_row_block(frames, side, side, ch)
    n_strips = (side + USEFUL - 1) // USEFUL
    assert (n_strips - 1) * frames < per_rb <= n_strips * frames
    # several batches in flight
    got = emu.sbm_emu_rows_throughput(per_rb, side, n_simd)
    assert got == throughput_rule(per_rb, side, n_simd), (per_rb, got)
    assert got == PINNED.get((n_simd, frames, side, ch), got)
    before = least_work(per_rb, side, 0)  # the rule before the launches knew the SIMDs: the fewest waves x iterations
    if per_rb * -(-side // before) >= n_simd:
        assert got == before  # a launch that has a wave per SIMD at that size keeps it
    else:
        assert got <= before and (per_rb * -(-side // got) >= n_simd or got == 4)
    # one batch at a time (depth 1): the value it always had
    slots = n_simd * (3 if ch == 3 else 6)
    lat = emu.sbm_emu_rows_latency(per_rb, side, slots)
    assert lat == latency_rule(per_rb, side, slots), (per_rb, lat)
    assert lat == PINNED_LATENCY.get((n_simd, frames, side, ch), lat)
