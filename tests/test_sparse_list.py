"""CPU (not gpu): the sparse level-0 gradient launch runs from per-frame lists of its working items.

k_mark_refine_tiles, which holds a frame's hulls and tile flags, tests every item (k, rb) of the launch's grid once and compacts the
working ones behind a count (sbm_refine_tiles.h: gradient_rect_list); the launch then runs S waves per frame over the entries
(sbm_quantize_stream.h: quantize_stream_slot_wave) and no wave tests anything.  Compiled here for the CPU
(tests/emu/sparse_list_emu.cpp):

  list        for constructed candidates -- the object against each border, two objects in the same rows, none, widths 448 / 576 /
              704 (the last tile column cut), 8 / 18 / 32 rows per item, H < 16 -- the list holds exactly the items that a plain
              enumeration of gradient_rect_item_needed over every (k, rb) finds, each once, with its x_first, and their count
  emulation   sbm_quantize_stream.h on wave_emu.h: the launch by slots gives the whole kernel's map on every pixel of every need
              rectangle and writes nothing else that differs -- with S >= count, S = 3 and S = 1 (waves loop), with one frame of
              the batch on the sentinel (its waves test themselves), and with a count larger than the capacity (cut, no item
              beyond it runs)"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_sparse_rects import BAND, GEOMETRIES, POISON, T, make_frames

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
HEAD, ENTRY, NONE = 4, 4, -1  # sbm_refine_tiles.h: RT_LIST_HEAD, RT_LIST_ENTRY, RT_LIST_NONE
USEFUL = 240


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("sparse_list_emu") / "libsparse_list_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-variable",
                           "-Wno-unused-but-set-variable", "-Wno-unknown-pragmas", "-I", EMU_DIR, "-I", CSRC, "-o", so,
                           os.path.join(EMU_DIR, "sparse_list_emu.cpp")])
    L = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    L.sbm_emu_mark.argtypes = [C.c_int64, vp, i, i, i, i, i, vp, vp, vp]
    L.sbm_emu_items.argtypes = [vp, vp, i, i, i, i, i, i, vp]
    L.sbm_emu_whole_map.argtypes = [vp, i, i, i, i, C.c_float, i, vp]
    L.sbm_emu_list.argtypes = [vp, vp, i, i, i, i, i, i, i, vp, i]
    L.sbm_emu_n_full.argtypes = [i, i, i, i]
    L.sbm_emu_sparse_slots_pass.argtypes = [vp, i, i, i, i, C.c_float, i, vp, vp, vp, C.c_int64, i, i, i, i, i, vp, vp]
    return L


def mark(emu, cands, rows, cols):
    W, H = cols // T, rows // T
    cand = np.ascontiguousarray(np.asarray(cands, np.int32).reshape(-1, 6))
    flags = np.full(((W + 31) // 32) * ((H + 31) // 32), 7, np.uint8)
    rects = np.full(((rows + BAND - 1) // BAND, 2), 5, np.int32)
    assert emu.sbm_emu_mark(len(cand), cand.ctypes.data, rows, cols, T, W, H, flags.ctypes.data, rects.ctypes.data, None) == 0
    return flags, rects


def enumerate_items(emu, rects, flags, rows, cols, hs, n_full):
    """{(k, rb): x_first} by gradient_rect_item_needed over every item of the grid of n_full strips"""
    n_strips, n_rb = (cols + USEFUL - 1) // USEFUL, (rows + hs - 1) // hs
    out = np.zeros((n_rb, n_strips), np.int32)
    emu.sbm_emu_items(rects.ctypes.data, flags.ctypes.data, rows, cols, hs, T, cols // T, rows // T, out.ctypes.data)
    return {(k, rb): int(out[rb, k]) for rb in range(n_rb) for k in range(n_full) if out[rb, k] >= 0}


def make_list(emu, rects, flags, rows, cols, hs, n_full, capacity):
    lst = np.full(HEAD + ENTRY * capacity, -77, np.int32)
    n = emu.sbm_emu_list(rects.ctypes.data, flags.ctypes.data, rows, cols, hs, n_full, T, cols // T, rows // T, lst.ctypes.data, capacity)
    return lst, n


# ---- the list against a plain enumeration ---------------------------------------------------------------------------------

# (name, rows, cols, candidates): (cx, cy, declared width, declared height, feature extent x, feature extent y) at the coarse level
LIST_CASES = [
    ("left-top", 160, 448, [(0, 0, 60, 40, 61, 41)]),
    ("right-bottom", 160, 448, [(400, 400, 60, 40, 61, 41)]),
    ("left-bottom", 160, 576, [(0, 400, 60, 40, 61, 41)]),
    ("right-top", 160, 704, [(400, 0, 60, 40, 61, 41)]),
    ("inside", 160, 704, [(150, 21, 60, 40, 61, 41)]),
    ("inside, ox = 4 mod 16", 160, 576, [(18, 20, 60, 40, 61, 41)]),
    ("two objects in the same rows", 160, 704, [(5, 20, 60, 40, 61, 41), (330, 20, 60, 40, 61, 41)]),
    ("two objects, rows apart", 448, 576, [(18, 40, 120, 90, 121, 91), (400, 400, 120, 90, 121, 91)]),
    ("no candidate", 160, 576, []),
    ("H < 16", 48, 448, [(100, 3, 60, 10, 61, 40)]),
    ("H < 16, right", 56, 576, [(400, 5, 60, 10, 61, 30)]),
    ("patch passes row H - 1", 160, 576, [(100, 400, 60, 40, 61, 90)]),
]


@pytest.mark.parametrize("name,rows,cols,cands", LIST_CASES, ids=[c[0] for c in LIST_CASES])
def test_the_list_is_the_enumeration_of_the_item_rule(emu, name, rows, cols, cands):
    flags, rects = mark(emu, cands, rows, cols)
    n_strips = (cols + USEFUL - 1) // USEFUL
    for hs in (8, 18, 32):
        for n_full in (n_strips, n_strips - 1):  # every strip a wave per frame | the last one packed
            want = enumerate_items(emu, rects, flags, rows, cols, hs, n_full)
            capacity = n_strips * ((rows + 1) // 2)
            lst, n = make_list(emu, rects, flags, rows, cols, hs, n_full, capacity)
            assert n == lst[0] == len(want), (name, hs, n_full, n, lst[0], len(want))
            ent = lst[HEAD: HEAD + ENTRY * n].reshape(n, ENTRY)
            got = {(int(k), int(rb)): int(x) for k, rb, x, _ in ent}
            assert len(got) == n and got == want, (name, hs, n_full)  # the same items, each once, with the right x_first
            assert (ent[:, 3] == 0).all() and (lst[HEAD + ENTRY * n:] == -77).all() and (lst[1:HEAD] == -77).all()
            if cands:
                assert n > 0 and (ent[:, 2] % 4 == 0).all()
            else:
                assert n == 0


def test_a_list_longer_than_its_room_is_cut_and_nothing_is_written_behind_it(emu):
    rows, cols = 448, 576
    flags, rects = mark(emu, [(18, 40, 120, 90, 121, 91), (400, 400, 120, 90, 121, 91)], rows, cols)
    want = enumerate_items(emu, rects, flags, rows, cols, 8, 3)
    assert len(want) > 6
    lst, n = make_list(emu, rects, flags, rows, cols, 8, 3, 5)
    assert n == len(want) and lst[0] == 5 and len(lst) == HEAD + ENTRY * 5
    got = {(int(k), int(rb)): int(x) for k, rb, x, _ in lst[HEAD:].reshape(5, ENTRY)}
    assert len(got) == 5 and all(want[key] == x for key, x in got.items())


# ---- the launch by slots in the wave emulation ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scenes(emu):
    """per geometry of test_sparse_rects: frames, flags, hulls, the whole kernel's map and the needed pixels"""
    out = {}
    for (rows, cols, ch), per_frame in GEOMETRIES.items():
        n = len(per_frame)
        frames = make_frames(n, rows, cols, ch, 31 + rows + ch)
        marks = [mark(emu, c, rows, cols) for c in per_frame]
        flags = np.ascontiguousarray(np.stack([m[0] for m in marks]))
        rects = np.ascontiguousarray(np.stack([m[1] for m in marks]))
        hs = 18 if rows == 96 else 32
        want = np.full((n, rows, cols), POISON, np.uint8)
        assert emu.sbm_emu_whole_map(frames.ctypes.data, n, rows, cols, ch, 30.0, hs, want.ctypes.data) == 0
        needed = np.zeros((n, rows, cols), bool)
        for f in range(n):
            for b, (lo, hi) in enumerate(rects[f]):
                if lo < hi:
                    needed[f, b * BAND: (b + 1) * BAND, lo:hi] = True
        assert needed.any()
        out[(rows, cols, ch)] = dict(frames=frames, flags=flags, rects=rects, hs=hs, want=want, needed=needed, n=n, per_frame=per_frame)
    return out


def run_slots(emu, sc, rows, cols, ch, slots, sentinel=(), count_plus=0):
    """the launch by `slots` waves per frame; frames in `sentinel` keep RT_LIST_NONE; count_plus: every list's count says that many
    more than its capacity holds, and the entries behind it name items that must not run"""
    n, hs = sc["n"], sc["hs"]
    W, H = cols // T, rows // T
    n_full = emu.sbm_emu_n_full(n, rows, cols, ch)
    n_strips, n_rb = (cols + USEFUL - 1) // USEFUL, (rows + hs - 1) // hs
    room = n_strips * ((rows + 1) // 2)
    stride = HEAD + ENTRY * room
    lists = np.zeros((n, stride), np.int32)
    counts = []
    cap = room
    for f in range(n):
        lst, cnt = make_list(emu, sc["rects"][f], sc["flags"][f], rows, cols, hs, n_full, room)
        lists[f] = lst
        counts.append(cnt)
    if count_plus:
        cap = max(counts)  # what the kernel is told the lists have room for: the longest list is full
        for f in range(n):
            # behind every list: in-range items of the grid, none of which the launch may run
            tail = lists[f, HEAD + ENTRY * counts[f]:].reshape(-1, ENTRY)
            tail[:] = [(0, 0, 0, 0)]
            tail[:, 1] = np.arange(len(tail)) % n_rb
            if counts[f] == cap:
                lists[f, 0] = cap + count_plus
    for f in sentinel:
        lists[f, 0] = NONE
    GUARD = 4096
    buf = np.full(GUARD + n * rows * cols + GUARD, POISON, np.uint8)
    got = buf[GUARD: GUARD + n * rows * cols].reshape(n, rows, cols)
    waves = C.c_int32(0)
    working = emu.sbm_emu_sparse_slots_pass(sc["frames"].ctypes.data, n, rows, cols, ch, 30.0, hs, sc["flags"].ctypes.data, sc["rects"].ctypes.data,
                                            lists.ctypes.data, stride, cap, slots, T, W, H, got.ctypes.data, C.byref(waves))
    assert (buf[:GUARD] == POISON).all() and (buf[-GUARD:] == POISON).all()  # no byte outside the level
    return got, working, waves.value, counts, n_full, n_rb


def check_map(sc, got):
    want, needed = sc["want"], sc["needed"]
    assert ((got == want) | (got == POISON)).all()  # written = right, everything else untouched
    assert np.array_equal(got[needed], want[needed]), np.argwhere(needed & (got != want))[:5]
    if not sc["per_frame"][-1]:
        assert (got[-1] == POISON).all()  # a frame without candidates: nothing runs


def packed_working(emu, sc, rows, cols, n_full):
    """what the packed last-strip waves count: one per frame and row block whose last strip works"""
    n_strips = (cols + USEFUL - 1) // USEFUL
    if n_full == n_strips:
        return 0
    total = 0
    for f in range(sc["n"]):
        all_items = enumerate_items(emu, sc["rects"][f], sc["flags"][f], rows, cols, sc["hs"], n_strips)
        total += sum(1 for (k, _) in all_items if k == n_strips - 1)
    return total


@pytest.mark.parametrize("rows,cols,ch", list(GEOMETRIES), ids=["96x576x3", "448x576x3", "512x704x1"])
@pytest.mark.parametrize("slots", ["all", 3, 1])
def test_the_launch_by_slots_reproduces_the_whole_kernel_where_it_is_needed(emu, scenes, rows, cols, ch, slots):
    sc = scenes[(rows, cols, ch)]
    n_full = emu.sbm_emu_n_full(sc["n"], rows, cols, ch)
    per_frame = n_full * ((rows + sc["hs"] - 1) // sc["hs"])
    S = per_frame if slots == "all" else slots
    got, working, waves, counts, n_full, n_rb = run_slots(emu, sc, rows, cols, ch, S)
    assert max(counts) > 0 and (slots != "all" or S >= max(counts)) and (slots == "all" or S < max(counts))
    check_map(sc, got)
    assert working == sum(counts) + packed_working(emu, sc, rows, cols, n_full), (working, counts)
    n_strips = (cols + USEFUL - 1) // USEFUL
    assert waves <= sc["n"] * S + n_rb * sc["n"] and (n_full < n_strips or waves == sc["n"] * S)


@pytest.mark.parametrize("slots", [64, 3])
def test_a_frame_on_the_sentinel_tests_its_own_items_beside_frames_with_lists(emu, scenes, slots):
    rows, cols, ch = 96, 576, 3
    sc = scenes[(rows, cols, ch)]
    base, working0, _, counts, n_full, _ = run_slots(emu, sc, rows, cols, ch, slots)
    for sentinel in ((0,), (1, 2), (0, 1, 2)):
        got, working, _, _, _, _ = run_slots(emu, sc, rows, cols, ch, slots, sentinel=sentinel)
        check_map(sc, got)
        assert np.array_equal(got, base) and working == working0, sentinel  # the same items either way


@pytest.mark.parametrize("rows,cols,ch", [(96, 576, 3), (448, 576, 3)], ids=["96x576x3", "448x576x3"])
def test_a_count_larger_than_the_capacity_is_cut(emu, scenes, rows, cols, ch):
    sc = scenes[(rows, cols, ch)]
    base, working0, _, counts, n_full, _ = run_slots(emu, sc, rows, cols, ch, 3)
    got, working, _, _, _, _ = run_slots(emu, sc, rows, cols, ch, 3, count_plus=1000)
    check_map(sc, got)
    assert working == working0 and np.array_equal(got, base)  # no entry behind the capacity ran
