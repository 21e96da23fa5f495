"""CPU (not gpu): the line-shaped source pass (sbm_source_lines.h) against the present one (sbm_quantize_stream.h, QS_SOURCE).

Three parts, all compiled here for the CPU (tests/emu/source_pass_emu.cpp):
  emulation   both forms on wave_emu.h write the same bytes: the packed retained copy -- the input itself, no padding byte in
              it -- and cv::pyrDown, over poisoned outputs, at every width, height, item height, frame count, channel count and
              padding the line form has a case for, with the object against every image border
  plan        sbm_source_lines_plan.h walked on its own: every byte of the copy and of cv::pyrDown is written exactly once and
              none outside, every offset is dword aligned, every owned cv::pyrDown row finds its window among the loaded rows
  selection   the rule as a table: 4-byte aligned base, row stride and frame stride, cols % 64 == 0, a frame within 31 bits;
              a row pad of 13 bytes and an odd frame stride fall back"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from shape_based_matching_amd import synth

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
POISON = 0xAA
PAD = 0xA5


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("source_pass_emu") / "libsource_pass_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-variable",
                           "-Wno-unused-but-set-variable", "-Wno-unknown-pragmas", "-I", EMU_DIR, "-I", CSRC, "-o", so,
                           os.path.join(EMU_DIR, "source_pass_emu.cpp")])
    L = C.CDLL(so)
    vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
    L.sbm_emu_source_present.argtypes = [vp, i, i, i, i, i, i, i, i64, vp, vp]
    L.sbm_emu_source_lines.argtypes = [vp, i, i, i, i, i, i, i64, vp, vp]
    L.sbm_emu_source_lines_ok.argtypes = [C.c_uint64, i64, i64, i, i, i, i]
    L.sbm_emu_source_lines_walk.argtypes = [i, i, i, i, i, vp, vp]
    L.sbm_emu_source_lines_walk.restype = i64
    return L


# ---- emulation ------------------------------------------------------------------------------------------------------------

def make_frames(n, rows, cols, ch, seed):
    """per frame a scene with noise whose object -- a bright textured box -- touches the top and the left border (frame 0), the
    bottom and the right border (frame 1), or all four (frame 2: pure noise), so that REFLECT_101 folds real texture in rows
    and in columns"""
    rs = np.random.RandomState(seed)
    out = []
    for f in range(n):
        a = (synth.scene_bgr(seed + f, rows, cols) if ch == 3 else synth.scene_gray(seed + f, rows, cols)).copy()
        box = rs.randint(0, 256, (rows // 2, cols // 2) + a.shape[2:]).astype(np.uint8)
        if f % 3 == 0:
            a[: rows // 2, : cols // 2] = box
        elif f % 3 == 1:
            a[rows - rows // 2:, cols - cols // 2:] = box
        else:
            a = rs.randint(0, 256, a.shape).astype(np.uint8)
        out.append(a)
    return np.ascontiguousarray(np.stack(out))


def layout(frames, row_pad, frame_pad):
    """the frames in a caller's buffer whose first byte is 64-byte aligned: `row_pad` bytes of 0xA5 behind every row, `frame_pad`
    behind every frame -> (buffer, row stride, frame stride)"""
    n, rows = frames.shape[:2]
    line = frames[0].size // rows
    stride = line + row_pad
    fs = rows * stride + frame_pad
    raw = np.full(n * fs + 64, PAD, np.uint8)
    o = (-raw.ctypes.data) % 64
    buf = raw[o: o + n * fs]
    for f in range(n):
        buf[f * fs: f * fs + rows * stride].reshape(rows, stride)[:, :line] = frames[f].reshape(rows, line)
    return buf, stride, fs


COLS = [64, 256, 320, 576, 704]  # one cut strip; exactly one strip; a strip and a 64-column rest; 2 + 64 columns; 2 + 192 columns
ROWS_HS = [(32, 32), (48, 32), (48, 8), (48, 20), (32, 20)]  # (48, 32), (48, 20), (32, 20): the last block is moved up


@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("cols", COLS)
def test_line_form_equals_the_present_form_byte_for_byte(emu, cols, n, ch):
    for rows, hs in ROWS_HS:
        frames = make_frames(n, rows, cols, ch, 7 + rows + cols + ch)
        shape_p = (n, rows // 2, cols // 2) + ((3,) if ch == 3 else ())
        want_pyr = np.full(shape_p, POISON, np.uint8)
        want_keep = np.full(frames.shape, POISON, np.uint8)
        assert emu.sbm_emu_source_present(frames.ctypes.data, n, rows, cols, ch, hs, 1, cols * ch, rows * cols * ch, want_pyr.ctypes.data,
                                          want_keep.ctypes.data) == 0
        assert np.array_equal(want_keep, frames)
        assert len(np.unique(want_pyr)) > 50  # a textured result, not a flat one
        for row_pad, frame_pad in ((0, 0), (64, 1000), (64, 0), (0, 1000)):
            buf, stride, fs = layout(frames, row_pad, frame_pad)
            pyr = np.full(shape_p, POISON, np.uint8)
            keep = np.full(frames.shape, POISON, np.uint8)
            items = emu.sbm_emu_source_lines(buf.ctypes.data, n, rows, cols, ch, hs, stride, fs, pyr.ctypes.data, keep.ctypes.data)
            assert items == -(-cols // 256) * -(-rows // hs) * n, (rows, hs, row_pad, frame_pad, items)
            assert np.array_equal(keep, frames), (rows, hs, row_pad, frame_pad, np.argwhere(keep != frames)[:5])
            assert np.array_equal(pyr, want_pyr), (rows, hs, row_pad, frame_pad, np.argwhere(pyr != want_pyr)[:5])


def test_line_form_refuses_what_the_rule_refuses(emu):
    frames = make_frames(2, 32, 64, 3, 3)
    pyr = np.zeros((2, 16, 32, 3), np.uint8)
    keep = np.zeros_like(frames)
    for row_pad, frame_pad in ((13, 0), (0, 1001)):
        buf, stride, fs = layout(frames, row_pad, frame_pad)
        assert emu.sbm_emu_source_lines(buf.ctypes.data, 2, 32, 64, 3, 32, stride, fs, pyr.ctypes.data, keep.ctypes.data) == -2


# ---- plan -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("cols", COLS + [1024])
def test_plan_writes_every_byte_exactly_once(emu, cols, ch):
    for frames in (1, 3):
        for rows in (2, 8, 32, 48, 70, 128):
            for hs in (2, 8, 18, 20, 32, 64):
                copy_cnt = np.zeros((frames, rows, cols * ch), np.int32)
                pyr_cnt = np.zeros((frames, rows // 2, cols // 2 * ch), np.int32)
                bad = emu.sbm_emu_source_lines_walk(frames, rows, cols, ch, hs, copy_cnt.ctypes.data, pyr_cnt.ctypes.data)
                assert bad == 0, (frames, rows, cols, hs, bad)
                assert (copy_cnt == 1).all(), (frames, rows, cols, hs, np.argwhere(copy_cnt != 1)[:5])
                assert (pyr_cnt == 1).all(), (frames, rows, cols, hs, np.argwhere(pyr_cnt != 1)[:5])


# ---- selection ------------------------------------------------------------------------------------------------------------

def test_selection_rule_table(emu):
    ok = emu.sbm_emu_source_lines_ok
    base = 0x7F0000001000
    # (base, row pad, frame pad, frames, rows, cols, ch) -> chosen
    table = [
        ((base, 0, 0, 16, 1024, 1024, 3), 1),       # the headline batch
        ((base, 0, 0, 1, 1024, 1024, 3), 1),
        ((base, 0, 0, 3, 448, 576, 3), 1),
        ((base, 0, 0, 3, 512, 704, 1), 1),
        ((base, 64, 1000, 3, 512, 768, 3), 1),      # a 4-byte aligned padded layout
        ((base, 4, 4, 3, 512, 768, 1), 1),
        ((base + 4, 0, 0, 2, 64, 64, 3), 1),
        ((base, 13, 0, 3, 448, 576, 3), 0),         # a row pad of 13 bytes
        ((base, 13, 0, 1, 448, 576, 3), 0),
        ((base, 0, 1001, 3, 448, 576, 3), 0),       # an odd frame stride
        ((base, 0, 1001, 1, 448, 576, 3), 1),       # ... which a single frame never uses
        ((base, 0, 2, 2, 448, 576, 1), 0),          # a frame stride that is even, not a multiple of 4
        ((base + 1, 0, 0, 1, 448, 576, 3), 0),      # the base off a dword boundary
        ((base + 2, 0, 0, 1, 448, 576, 1), 0),
        ((base, 0, 0, 1, 512, 544, 3), 0),          # cols % 64 == 32
        ((base, 0, 0, 1, 512, 32, 1), 0),
        ((base, 0, 0, 1, 70, 260, 3), 0),
        ((base, 0, 0, 1, 63, 64, 3), 0),            # odd rows: no launch of the source pass has them
        ((base, 0, 0, 1, 512, 512, 2), 0),
        ((base, 0, 0, 2, 16384, 16384, 3), 1),      # 805 306 368 bytes a frame: within the 32-bit lane offsets
        ((base, 0, 0, 2, 32768, 32768, 3), 0),      # 3 221 225 472: not
        ((base, 0, 0, 2, 32768, 32768, 1), 1),      # 1 073 741 824
        ((base, 1 << 20, 0, 1, 2048, 1024, 1), 0),  # a row stride that carries the last row past 2^31 - 2^20
    ]
    for (b, row_pad, frame_pad, frames, rows, cols, ch), want in table:
        stride = cols * ch + row_pad
        assert ok(b, stride, rows * stride + frame_pad, frames, rows, cols, ch) == want, (hex(b), row_pad, frame_pad, frames, rows, cols, ch)
    assert ok(base, 64 * 3 - 4, 64 * 64 * 3, 1, 64, 64, 3) == 0  # a row stride below the row's bytes
