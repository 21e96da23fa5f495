"""CPU (not gpu): the retained copy of level 0's source is stored by the last call enqueued only.

Compiled here for the CPU (tests/emu/source_retention_emu.cpp), on wave_emu.h:

  rule        source_pass_retains as a table: (enqueued, executed) in {(n, n), (n+1, n), (n+2, n), (n+5, n)} gives keep, keep,
              skip, skip -- also where the counters wrap
  source      both forms of the source pass with the decision "skip" write no byte of the copy, which stays a poison pattern, and
              write cv::pyrDown byte for byte as with "keep"; the launch's first work item alone notes the decision; without
              counters the copy is stored
  sparse      the sparse gradient launch -- a wave per item, and by slots from the lists -- reading a caller's layout (row pad
              13 and 64, a frame pad, a window of a larger canvas) writes the map of the same launch on the packed copy, byte for
              byte, with a whole and a partial group of the packed last strip"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_source_pass import layout, make_frames
from test_sparse_list import ENTRY, HEAD, make_list, mark
from test_sparse_rects import POISON, T

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
USEFUL = 240


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("source_retention_emu") / "libsource_retention_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-variable",
                           "-Wno-unused-but-set-variable", "-Wno-unknown-pragmas", "-I", EMU_DIR, "-I", CSRC, "-o", so,
                           os.path.join(EMU_DIR, "source_retention_emu.cpp")])
    L = C.CDLL(so)
    vp, i, i64, u32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint32
    L.sbm_emu_retains.argtypes = [u32, u32]
    L.sbm_emu_source_counted.argtypes = [i, vp, i, i, i, i, i, i, i64, vp, vp, i, u32, u32, vp, vp]
    L.sbm_emu_sparse_strided.argtypes = [vp, i, i, i, i, C.c_float, i, i, i64, vp, vp, vp, i64, i, i, i, i, i, vp]
    L.sbm_emu_mark.argtypes = [i64, vp, i, i, i, i, i, vp, vp, vp]
    L.sbm_emu_list.argtypes = [vp, vp, i, i, i, i, i, i, i, vp, i]
    L.sbm_emu_n_full.argtypes = [i, i, i, i]
    return L


# ---- the rule -------------------------------------------------------------------------------------------------------------

def test_decision_rule_table(emu):
    for n in (0, 1, 7, 1000, 2**31 - 3, 2**31 - 1, 2**31, 2**32 - 6, 2**32 - 2, 2**32 - 1):
        for ahead, want in ((0, 1), (1, 1), (2, 0), (5, 0)):
            assert emu.sbm_emu_retains((n + ahead) % 2**32, n) == want, (n, ahead)


# ---- the source pass ------------------------------------------------------------------------------------------------------

SOURCE_CASES = [(96, 576, 3, 18), (448, 576, 3, 32), (512, 704, 1, 32)]  # rows, cols, channels, rows per item; three frames each
KEEP, SKIP = (5, 4), (6, 4)  # (enqueued, executed): this call is the last one enqueued | a later one is enqueued behind it


def run_source(emu, form, buf, stride, fs, n, rows, cols, ch, hs, counters):
    pyr = np.full((n, rows // 2, cols // 2 * ch), POISON, np.uint8)
    keep = np.full((n, rows, cols * ch), POISON, np.uint8)
    note = np.zeros(2, np.uint32)
    writes = C.c_int32(-1)
    enq, exe = counters if counters else (0, 0)
    items = emu.sbm_emu_source_counted(form, buf.ctypes.data, n, rows, cols, ch, hs, stride, fs, pyr.ctypes.data, keep.ctypes.data,
                                       1 if counters else 0, enq, exe, note.ctypes.data, C.byref(writes))
    assert items > 0, items
    return pyr, keep, int(note[0]), writes.value


@pytest.mark.parametrize("rows,cols,ch,hs", SOURCE_CASES, ids=["96x576x3", "448x576x3", "512x704x1"])
@pytest.mark.parametrize("form", [0, 1], ids=["strided", "lines"])
def test_a_skipping_source_pass_writes_pyrdown_and_no_byte_of_the_copy(emu, form, rows, cols, ch, hs):
    n = 3
    frames = make_frames(n, rows, cols, ch, 11 + rows + ch)
    flat = frames.reshape(n, rows, cols * ch)
    for row_pad, frame_pad in ((0, 0), (64, 1000)):
        buf, stride, fs = layout(frames, row_pad, frame_pad)
        pyr_k, keep_k, note_k, writes_k = run_source(emu, form, buf, stride, fs, n, rows, cols, ch, hs, KEEP)
        assert np.array_equal(keep_k, flat) and note_k == 1 and writes_k == 1
        assert len(np.unique(pyr_k)) > 50 and not (pyr_k == POISON).all()
        pyr_s, keep_s, note_s, writes_s = run_source(emu, form, buf, stride, fs, n, rows, cols, ch, hs, SKIP)
        assert (keep_s == POISON).all()  # not one byte of the copy
        assert np.array_equal(pyr_s, pyr_k)
        assert note_s == 2 and writes_s == 1  # the first work item alone notes the decision
        pyr_0, keep_0, note_0, _ = run_source(emu, form, buf, stride, fs, n, rows, cols, ch, hs, None)
        assert np.array_equal(keep_0, flat) and np.array_equal(pyr_0, pyr_k) and note_0 == 1  # no counters: always stored


# ---- the sparse launch on a caller's layout --------------------------------------------------------------------------------

# (rows, cols, channels, rows per item, per frame the candidates (cx, cy, declared w, h, feature extent x, y) at the coarse level)
A96 = [(0, 0, 60, 24, 61, 25), (400, 2, 60, 24, 61, 25)]
B96 = [(18, 2, 60, 24, 61, 25), (241, 2, 60, 24, 61, 25)]
SPARSE_CASES = [
    ("96x576x3, a whole group of the packed strip", 96, 576, 3, 18, [A96, B96]),
    ("96x576x3, a whole and a partial group", 96, 576, 3, 18, [A96, B96, A96]),
    ("448x576x3", 448, 576, 3, 32, [[(18, 40, 120, 90, 121, 91), (400, 400, 120, 90, 121, 91)], [(400, 40, 120, 90, 121, 91)], []]),
]


def caller_layouts(frames):
    """(name, buffer, row stride, frame stride) of the frames in four layouts of a caller's"""
    n, rows = frames.shape[:2]
    line = frames[0].size // rows
    out = []
    for name, row_pad, frame_pad in (("row pad 13", 13, 0), ("row pad 64", 64, 0), ("frame pad", 0, 1000), ("row pad 13 + frame pad", 13, 777)):
        buf, stride, fs = layout(frames, row_pad, frame_pad)
        out.append((name, buf, stride, fs))
    # a window of a larger canvas: every frame a region of one wide image, the frames side by side in it
    stride = n * line + 40
    canvas = np.full(rows * stride + 64, 0xA5, np.uint8)
    for f in range(n):
        canvas[: rows * stride].reshape(rows, stride)[:, f * line: (f + 1) * line] = frames[f].reshape(rows, line)
    out.append(("window of a canvas", canvas, stride, line))
    return out


@pytest.mark.parametrize("name,rows,cols,ch,hs,per_frame", SPARSE_CASES, ids=[c[0] for c in SPARSE_CASES])
def test_the_sparse_launch_on_a_callers_layout_writes_the_packed_copys_map(emu, name, rows, cols, ch, hs, per_frame):
    n = len(per_frame)
    W, H = cols // T, rows // T
    frames = make_frames(n, rows, cols, ch, 5 + rows + n)
    marks = [mark(emu, c, rows, cols) for c in per_frame]
    flags = np.ascontiguousarray(np.stack([m[0] for m in marks]))
    rects = np.ascontiguousarray(np.stack([m[1] for m in marks]))
    n_full = emu.sbm_emu_n_full(n, rows, cols, ch)
    n_strips = (cols + USEFUL - 1) // USEFUL
    assert n_full == n_strips - 1  # the last strip is packed: 96 of 576 columns, two frames to a wave
    room = n_strips * ((rows + 1) // 2)
    list_stride = HEAD + ENTRY * room
    lists = np.zeros((n, list_stride), np.int32)
    for f in range(n):
        lists[f], _ = make_list(emu, rects[f], flags[f], rows, cols, hs, n_full, room)
    per_frame_items = n_full * ((rows + hs - 1) // hs)

    def run(buf, stride, fs, slots):
        out = np.full((n, rows, cols), POISON, np.uint8)
        working = emu.sbm_emu_sparse_strided(buf.ctypes.data, n, rows, cols, ch, 30.0, hs, stride, fs, flags.ctypes.data, rects.ctypes.data,
                                             lists.ctypes.data, list_stride, room, slots, T, W, H, out.ctypes.data)
        assert working > 0
        return out, working

    packed = np.ascontiguousarray(frames.reshape(n, -1))
    for slots in (0, per_frame_items, 3):
        want, working = run(packed, cols * ch, rows * cols * ch, slots)
        assert (want != POISON).any() and (want == POISON).any()  # a sparse map
        for lname, buf, stride, fs in caller_layouts(frames):
            got, w = run(buf, stride, fs, slots)
            assert w == working, (lname, slots)
            assert np.array_equal(got, want), (lname, slots, np.argwhere(got != want)[:5])
