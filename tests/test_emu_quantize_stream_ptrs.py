"""CPU (not gpu): the TABLE forms of the gfx950 gradient kernels (sbm_quantize_stream.h, sbm_source_lines.h: PTRS) on the wave
emulation of tests/emu/wave_emu.h -- the kernels behind sbm_match_batch_device_ptrs, which take a frame's first pixel from
table[frame] instead of base + frame * stride, and its mask likewise.

The frames are separately allocated host buffers; the table lists them in reverse order with one frame listed twice.  What the
table forms write -- the one-hot map, the cv::pyrDown image, the retained copy of the source pass -- must equal, bit for bit,
(a) what the existing contiguous forms write for the same frames in table order (packed last strip and all), and
(b) oracle.Pyramid.build(frame, T, weak, mask) / oracle.pyrdown(frame) / the frame itself, frame by frame
    (Detector::match's loop, line2Dup.cpp:1078; quantize() :446-450; pyrDown() :424-444)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frame_mask_cases as FM
from conftest import ROOT
from test_emu_quantize_stream_masks import CASES

EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
HS = 8


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """the kernel sources + the table harness as a shared object of this test's own (flags of tests/emu/Makefile)"""
    so = str(tmp_path_factory.mktemp("emu_ptrs") / "libsbm_emu_ptrs.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-variable",
                           "-Wno-unused-but-set-variable", "-Wno-unknown-pragmas", "-I" + EMU_DIR, "-I" + CSRC, "-o", so,
                           os.path.join(EMU_DIR, "quantize_stream_ptrs_emu.cpp")])
    L = C.CDLL(so)
    vp, i, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
    L.sbm_emu_ptrs_whole.argtypes = [vp, vp, i, i, i, i, i, f32, vp, vp, i]
    L.sbm_emu_block_whole.argtypes = [vp, i64, vp, i64, i, i, i, i, i, f32, vp, vp, i]
    L.sbm_emu_ptrs_source.argtypes = [vp, i, i, i, i, i, vp, vp, i, i]
    L.sbm_emu_block_source.argtypes = [vp, i64, i, i, i, i, i, vp, vp, i, i]
    return L


class World:
    """n separately allocated frames (and masks), the table order -- reversed, frame 1 listed twice -- and the oracle's answers"""

    def __init__(self, oracle, rows, cols, n, ch):
        self.rows, self.cols, self.n, self.ch = rows, cols, n, ch
        src = FM.textured_frames(rows * 1000 + cols + ch, n, rows, cols, ch)
        self.frames = [np.array(src[f], copy=True) for f in range(n)]  # one allocation each
        m = FM.frame_masks(cols + n, n, rows, cols)
        self.masks = [np.array(m[f], copy=True) for f in range(n)]
        order = list(range(n - 1, -1, -1))
        order.insert(1, 1 if n > 1 else 0)  # one frame twice
        self.order = order
        self.T = FM.pyramid_T(rows, cols)
        listed = [self.frames[f] for f in order]
        self.want_plain = [w[0] for w in FM.oracle_maps(oracle, listed, None, self.T)]
        self.want_masked = [w[0] for w in FM.oracle_maps(oracle, listed, [self.masks[f] for f in order], self.T)]
        self.want_pyr = [oracle.pyrdown(x) for x in listed]
        # the same frames as one block in table order: what the contiguous entry points are given
        self.block = np.ascontiguousarray(np.stack(listed))
        self.mask_block = np.ascontiguousarray(np.stack([self.masks[f] for f in order]))
        self.frame_tab = np.array([self.frames[f].ctypes.data for f in order], np.uint64)
        self.mask_tab = np.array([self.masks[f].ctypes.data for f in order], np.uint64)

    def outputs(self):
        k = len(self.order)
        pshape = (k, self.rows // 2, self.cols // 2) + ((3,) if self.ch == 3 else ())
        return (np.full((k, self.rows, self.cols), 0xAA, np.uint8), np.full(pshape, 0xAA, np.uint8),
                np.full(self.block.shape, 0xAA, np.uint8))


@pytest.fixture(scope="module")
def worlds(oracle):
    cache = {}

    def get(rows, cols, n, ch):
        key = (rows, cols, n, ch)
        if key not in cache:
            cache[key] = World(oracle, rows, cols, n, ch)
        return cache[key]

    return get


@pytest.mark.parametrize("ch", [1, 3], ids=["gray", "bgr"])
@pytest.mark.parametrize("rows,cols,n,lanes", CASES)
def test_whole_row_loop_through_the_table(emu, worlds, rows, cols, n, lanes, ch):
    w = worlds(rows, cols, n, ch)
    k, stride = len(w.order), cols * ch
    for masked in (False, True):
        out, pyr, _ = w.outputs()
        rc = emu.sbm_emu_ptrs_whole(w.frame_tab.ctypes.data, w.mask_tab.ctypes.data if masked else None, k, rows, cols, stride, ch, FM.WEAK,
                                    out.ctypes.data, pyr.ctypes.data, HS)
        assert rc == 0
        out_b, pyr_b, _ = w.outputs()
        got_lanes = emu.sbm_emu_block_whole(w.block.ctypes.data, rows * stride, w.mask_block.ctypes.data if masked else None, rows * cols, k, rows,
                                            cols, stride, ch, FM.WEAK, out_b.ctypes.data, pyr_b.ctypes.data, HS)
        # the contiguous side packs its last strip (one more frame than CASES counts: the same lanes, one more segment)
        assert got_lanes == lanes, (got_lanes, lanes)
        assert np.array_equal(out, out_b) and np.array_equal(pyr, pyr_b), (rows, cols, ch, masked)
        want = w.want_masked if masked else w.want_plain
        for f in range(k):
            assert np.array_equal(out[f], want[f]), (masked, f, np.argwhere(out[f] != want[f])[:5])
            assert np.array_equal(pyr[f], w.want_pyr[f]), (masked, f)
    # the masks matter: the masked and the plain maps of some listed frame differ
    assert any(not np.array_equal(a, b) for a, b in zip(w.want_masked, w.want_plain))


@pytest.mark.parametrize("ch", [1, 3], ids=["gray", "bgr"])
@pytest.mark.parametrize("rows,cols,n,lanes", CASES)
def test_source_pass_through_the_table(emu, worlds, rows, cols, n, lanes, ch):
    """QS_SOURCE and k_source_lines: the retained copy is the frames in table order, packed; the next level's image cv::pyrDown"""
    w = worlds(rows, cols, n, ch)
    k, stride = len(w.order), cols * ch
    ran_lines = False
    for lines in (0, 1):
        _, pyr, keep = w.outputs()
        rc = emu.sbm_emu_ptrs_source(w.frame_tab.ctypes.data, k, rows, cols, stride, ch, pyr.ctypes.data, keep.ctypes.data, HS, lines)
        _, pyr_b, keep_b = w.outputs()
        rc_b = emu.sbm_emu_block_source(w.block.ctypes.data, rows * stride, k, rows, cols, stride, ch, pyr_b.ctypes.data, keep_b.ctypes.data, HS, lines)
        assert rc == rc_b, (rc, rc_b)
        if lines and rc == -2:  # the rule refuses the layout (a width that is no multiple of 64) for both
            assert cols % 64 != 0
            continue
        assert rc >= 0
        ran_lines = ran_lines or bool(lines)
        assert np.array_equal(keep, keep_b) and np.array_equal(pyr, pyr_b), (rows, cols, ch, lines)
        assert np.array_equal(keep, w.block), lines
        for f in range(k):
            assert np.array_equal(pyr[f], w.want_pyr[f]), (lines, f)
    assert ran_lines == (cols % 64 == 0)


def test_windows_of_larger_canvases(emu, oracle):
    """equal-sized windows cut out of larger canvases at another place in each: the stride is the canvas row, and no byte of the
    canvas outside a window reaches a border pixel (BORDER_REPLICATE / REFLECT_101 are the window's, not the canvas's)"""
    rows, cols, ch = 16, 256, 3
    rs = np.random.RandomState(11)
    frames = FM.textured_frames(77, 3, rows, cols, ch)
    canvases = [rs.randint(0, 256, (rows + 8, cols + 16, ch)).astype(np.uint8) for _ in range(3)]
    at = [(0, 4), (5, 7), (8, 16)]  # (y, x): byte offsets 12, 21 + ..., 48 -- the middle one is odd
    for cv, fr, (y, x) in zip(canvases, frames, at):
        cv[y:y + rows, x:x + cols] = fr
    stride = (cols + 16) * ch
    tab = np.array([cv.ctypes.data + y * stride + x * ch for cv, (y, x) in zip(canvases, at)], np.uint64)
    out = np.full((3, rows, cols), 0xAA, np.uint8)
    pyr = np.full((3, rows // 2, cols // 2, ch), 0xAA, np.uint8)
    keep = np.full((3, rows, cols, ch), 0xAA, np.uint8)
    assert emu.sbm_emu_ptrs_whole(tab.ctypes.data, None, 3, rows, cols, stride, ch, FM.WEAK, out.ctypes.data, pyr.ctypes.data, HS) == 0
    want = FM.oracle_maps(oracle, frames, None, [4, 8])
    for f in range(3):
        assert np.array_equal(out[f], want[f][0]), f
        assert np.array_equal(pyr[f], oracle.pyrdown(frames[f])), f
    pyr[:] = 0xAA
    assert emu.sbm_emu_ptrs_source(tab.ctypes.data, 3, rows, cols, stride, ch, pyr.ctypes.data, keep.ctypes.data, HS, 0) == 0
    assert np.array_equal(keep, frames)
    for f in range(3):
        assert np.array_equal(pyr[f], oracle.pyrdown(frames[f])), f
    # the line form refuses the odd pointer (the harness checks the promise the GPU cannot) ...
    assert emu.sbm_emu_ptrs_source(tab.ctypes.data, 3, rows, cols, stride, ch, pyr.ctypes.data, keep.ctypes.data, HS, 1) == -2
    # ... and takes the windows at x offsets that are multiples of 4 pixels
    at4 = [(0, 4), (5, 8), (8, 16)]
    for cv, fr, (y, x) in zip(canvases, frames, at4):
        cv[:] = rs.randint(0, 256, cv.shape)
        cv[y:y + rows, x:x + cols] = fr
    tab4 = np.array([cv.ctypes.data + y * stride + x * ch for cv, (y, x) in zip(canvases, at4)], np.uint64)
    keep[:] = 0xAA
    pyr[:] = 0xAA
    assert emu.sbm_emu_ptrs_source(tab4.ctypes.data, 3, rows, cols, stride, ch, pyr.ctypes.data, keep.ctypes.data, HS, 1) > 0
    assert np.array_equal(keep, frames)
    for f in range(3):
        assert np.array_equal(pyr[f], oracle.pyrdown(frames[f])), f
