"""CPU (not gpu): the PLANE forms of the gfx950 gradient kernel (sbm_quantize_stream.h: PLANES, the whole row loop and the source
pass) on the wave emulation of tests/emu/wave_emu.h -- the kernels behind sbm_match_batch_device_planes, which take channel c of
frame f from table[3 f + c], one dword per plane and lane, where the interleaved forms take 12 consecutive bytes.

Every plane is a separately allocated host buffer.  What the plane forms write -- the one-hot map, the cv::pyrDown image, the
retained copy of the source pass -- must equal, bit for bit,
(a) what the interleaved table forms (sbm_match_batch_device_ptrs) write for np.stack(planes, -1), and
(b) oracle.Pyramid.build / oracle.pyrdown of that interleaved frame, and the frame itself for the retained copy
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
GEOMETRIES = [(rows, cols) for rows, cols, _, _ in CASES]  # 16x256, 12x320, 20x512, 16x480, 16x128


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """the kernel source + the plane harness as a shared object of this test's own (flags of tests/emu/Makefile)"""
    so = str(tmp_path_factory.mktemp("emu_planes") / "libsbm_emu_planes.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-variable",
                           "-Wno-unused-but-set-variable", "-Wno-unknown-pragmas", "-I" + EMU_DIR, "-I" + CSRC, "-o", so,
                           os.path.join(EMU_DIR, "quantize_stream_planes_emu.cpp")])
    L = C.CDLL(so)
    vp, i, f32 = C.c_void_p, C.c_int, C.c_float
    L.sbm_emu_planes_whole.argtypes = [vp, vp, i, i, i, i, f32, vp, vp, i]
    L.sbm_emu_planes_source.argtypes = [vp, i, i, i, i, vp, vp, i]
    L.sbm_emu_ptrs3_whole.argtypes = [vp, vp, i, i, i, i, f32, vp, vp, i]
    L.sbm_emu_ptrs3_source.argtypes = [vp, i, i, i, i, vp, vp, i]
    return L


def planes_of(frame):
    """the three channels of an interleaved frame as three separate allocations"""
    return [np.array(frame[..., c], copy=True) for c in range(3)]


def table(listed):
    """listed: per frame its three plane arrays, in the order the matcher is to see them"""
    return np.array([p.ctypes.data for planes in listed for p in planes], np.uint64)


def outputs(k, rows, cols):
    return (np.full((k, rows, cols), 0xAA, np.uint8), np.full((k, rows // 2, cols // 2, 3), 0xAA, np.uint8),
            np.full((k, rows, cols, 3), 0xAA, np.uint8))


def run_planes(emu, listed, masks, rows, cols, stride=None):
    """(map, pyr of the whole row loop, pyr and retained copy of the source pass) of the plane forms"""
    k = len(listed)
    tab = table(listed)
    mtab = np.array([m.ctypes.data for m in masks], np.uint64) if masks is not None else None
    stride = cols if stride is None else stride
    out, pyr, keep = outputs(k, rows, cols)
    assert emu.sbm_emu_planes_whole(tab.ctypes.data, mtab.ctypes.data if masks is not None else None, k, rows, cols, stride, FM.WEAK, out.ctypes.data,
                                    pyr.ctypes.data, HS) == 0
    _, pyr_s, _ = outputs(k, rows, cols)
    assert emu.sbm_emu_planes_source(tab.ctypes.data, k, rows, cols, stride, pyr_s.ctypes.data, keep.ctypes.data, HS) == 0
    return out, pyr, pyr_s, keep


def run_interleaved(emu, frames, masks, rows, cols):
    """the same of the interleaved table forms on separately allocated interleaved frames"""
    k = len(frames)
    tab = np.array([f.ctypes.data for f in frames], np.uint64)
    mtab = np.array([m.ctypes.data for m in masks], np.uint64) if masks is not None else None
    out, pyr, keep = outputs(k, rows, cols)
    assert emu.sbm_emu_ptrs3_whole(tab.ctypes.data, mtab.ctypes.data if masks is not None else None, k, rows, cols, cols * 3, FM.WEAK, out.ctypes.data,
                                   pyr.ctypes.data, HS) == 0
    _, pyr_s, _ = outputs(k, rows, cols)
    assert emu.sbm_emu_ptrs3_source(tab.ctypes.data, k, rows, cols, cols * 3, pyr_s.ctypes.data, keep.ctypes.data, HS) == 0
    return out, pyr, pyr_s, keep


def tie_frame(rows, cols):
    """a frame whose map depends on the ORDER of its channels: channel 0 a ramp along x (a triangle wave, slope 4 per pixel),
    channel 2 the same slope along y, channel 1 flat.  Away from the wave's kinks both gradients are (8 * 4)^2 = 1024 > weak^2, an
    exact tie that the reference gives to the LOWER channel (line2Dup.cpp:370-387): the horizontal gradient as listed, the vertical
    one with the planes reversed.  (On textured frames the channel of maximum magnitude is the same whatever the order.)"""
    x = np.arange(cols)
    tri = 4 * np.minimum(x % 128, 127 - x % 128)  # 0 .. 252
    f = np.empty((rows, cols, 3), np.uint8)
    f[..., 0] = tri[None, :]
    f[..., 1] = 100
    f[..., 2] = (4 * np.arange(rows))[:, None]
    return f


class World:
    """three textured BGR frames as nine separately allocated planes, and the four frames a table lists from them:
    frame 0 as it is, frame 1 with its planes in (2, 1, 0) order, frame 2 as it is, and plane 1 of frame 0 three times"""

    def __init__(self, oracle, rows, cols):
        self.rows, self.cols = rows, cols
        src = FM.textured_frames(rows * 1000 + cols + 3, 3, rows, cols, 3)
        src[1] = tie_frame(rows, cols)
        self.planes = [planes_of(src[f]) for f in range(3)]
        p = self.planes
        self.listed = [p[0], p[1][::-1], p[2], [p[0][1]] * 3]
        # what the matcher is to see, interleaved: the oracle's input and the interleaved kernels'
        self.seen = [np.ascontiguousarray(np.stack(planes, -1)) for planes in self.listed]
        assert np.array_equal(self.seen[0], src[0]) and np.array_equal(self.seen[1], src[1][..., ::-1])
        assert np.array_equal(self.seen[3], np.repeat(src[0][..., 1:2], 3, axis=-1))
        m = FM.frame_masks(cols + 4, 4, rows, cols)
        self.masks = [np.array(m[f], copy=True) for f in range(4)]
        self.T = FM.pyramid_T(rows, cols)
        self.want_plain = [w[0] for w in FM.oracle_maps(oracle, self.seen, None, self.T)]
        self.want_masked = [w[0] for w in FM.oracle_maps(oracle, self.seen, self.masks, self.T)]
        self.want_pyr = [oracle.pyrdown(x) for x in self.seen]
        # the order matters: frame 1 as it is gives another map than frame 1 reversed
        self.straight1 = FM.oracle_maps(oracle, [np.ascontiguousarray(src[1])], None, self.T)[0][0]


@pytest.fixture(scope="module")
def worlds(oracle):
    cache = {}

    def get(rows, cols):
        if (rows, cols) not in cache:
            cache[(rows, cols)] = World(oracle, rows, cols)
        return cache[(rows, cols)]

    return get


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masks"])
@pytest.mark.parametrize("rows,cols", GEOMETRIES)
def test_planes_equal_the_interleaved_form_and_the_oracle(emu, worlds, rows, cols, masked):
    """agreement, channel order (listed frame 1) and equal entries (listed frame 3) in one table"""
    w = worlds(rows, cols)
    masks = w.masks if masked else None
    out, pyr, pyr_s, keep = run_planes(emu, w.listed, masks, rows, cols)
    out_i, pyr_i, pyr_si, keep_i = run_interleaved(emu, w.seen, masks, rows, cols)
    assert np.array_equal(out, out_i) and np.array_equal(pyr, pyr_i) and np.array_equal(pyr_s, pyr_si) and np.array_equal(keep, keep_i)
    want = w.want_masked if masked else w.want_plain
    for f in range(4):
        assert np.array_equal(out[f], want[f]), (f, np.argwhere(out[f] != want[f])[:5])
        assert np.array_equal(pyr[f], w.want_pyr[f]) and np.array_equal(pyr_s[f], w.want_pyr[f]), f
        assert np.array_equal(keep[f], w.seen[f]), f  # the retained copy is the interleaved frame
    # the checks are telling: the reversed order is another map than the straight one, the masks change the maps, nothing is empty
    assert not np.array_equal(w.want_plain[1], w.straight1)
    assert any(not np.array_equal(a, b) for a, b in zip(w.want_masked, w.want_plain))
    assert all(m.any() for m in w.want_plain)


def test_windows_of_larger_planar_canvases(emu, oracle):
    """windows of [3, H, W] noise canvases at odd byte offsets: the stride is the canvas's W, and no canvas byte outside a window
    reaches a border pixel (BORDER_REPLICATE / REFLECT_101 are the window's, not the canvas's)"""
    rows, cols = 16, 256
    rs = np.random.RandomState(12)
    frames = FM.textured_frames(78, 3, rows, cols, 3)
    crows, ccols = rows + 8, cols + 16
    at = [(0, 1), (5, 7), (8, 16)]  # (y, x): plane byte offsets 1, 5 * 272 + 7 (odd), 8 * 272 + 16
    canvases = [rs.randint(0, 256, (3, crows, ccols)).astype(np.uint8) for _ in range(3)]
    listed = []
    for cv, fr, (y, x) in zip(canvases, frames, at):
        cv[:, y:y + rows, x:x + cols] = np.moveaxis(fr, -1, 0)
        listed.append([cv[c, y:, x:] for c in range(3)])  # views: their first byte is the window's
    assert any(p.ctypes.data % 2 for planes in listed for p in planes)
    out, pyr, pyr_s, keep = run_planes(emu, listed, None, rows, cols, stride=ccols)
    want = FM.oracle_maps(oracle, frames, None, [4, 8])
    assert np.array_equal(keep, frames)
    for f in range(3):
        assert np.array_equal(out[f], want[f][0]), f
        assert np.array_equal(pyr[f], oracle.pyrdown(frames[f])) and np.array_equal(pyr_s[f], oracle.pyrdown(frames[f])), f
    # other noise around the same windows: the same bytes out
    for cv, fr, (y, x) in zip(canvases, frames, at):
        cv[:] = rs.randint(0, 256, cv.shape)
        cv[:, y:y + rows, x:x + cols] = np.moveaxis(fr, -1, 0)
    out2, pyr2, pyr_s2, keep2 = run_planes(emu, listed, None, rows, cols, stride=ccols)
    assert np.array_equal(out, out2) and np.array_equal(pyr, pyr2) and np.array_equal(pyr_s, pyr_s2) and np.array_equal(keep, keep2)


def test_constant_rows_in_three_different_channel_values(emu, oracle):
    """the constant-row shortcut derives its closed-form state and its cv::pyrDown row from flat_key = b | g << 8 | r << 16, and a row
    is flat only if ALL THREE plane dwords are, in every lane.  Frame 0: its first 14 rows and a 14-row band in the middle are the
    colour (10, 200, 90).  Frame 1: the same, but one pixel of the band leaves that colour in plane 2 alone -- a test that looks at
    plane 0 (or at planes 0 and 1) takes the shortcut there wrongly.  Both against the oracle."""
    rows, cols = 64, 256
    colour = (10, 200, 90)
    base = FM.textured_frames(91, 1, rows, cols, 3)[0]
    a = base.copy()
    a[:14] = colour
    a[30:44] = colour
    b = a.copy()
    b[37, 130, 2] = 255  # plane 2, inside the band (strip 0, a lane in the middle)
    frames = [a, b]
    listed = [planes_of(f) for f in frames]
    # hs = 32: a work item's rows 0 .. 31 start inside the constant region (the warm-up shortcut) and run through the band
    k = 2
    tab = table(listed)
    for hs in (32, 8):
        out, pyr, keep = outputs(k, rows, cols)
        assert emu.sbm_emu_planes_whole(tab.ctypes.data, None, k, rows, cols, cols, FM.WEAK, out.ctypes.data, pyr.ctypes.data, hs) == 0
        want = FM.oracle_maps(oracle, frames, None, [4, 8])
        for f in range(2):
            assert np.array_equal(out[f], want[f][0]), (hs, f, np.argwhere(out[f] != want[f][0])[:5])
            assert np.array_equal(pyr[f], oracle.pyrdown(frames[f])), (hs, f)
        # the pixel matters: the two frames' pyrDown images differ, and the constant rows are the colour
        assert not np.array_equal(pyr[0], pyr[1]) and not out[0][35:39].any()
        assert (pyr[0][:6] == np.array(colour, np.uint8)).all()
