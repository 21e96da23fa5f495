"""CPU (not gpu): the SOURCE of the gfx950 row-streaming gradient kernel (sbm_quantize_stream.h) on the wave emulation
of tests/emu/wave_emu.h, with one mask per frame of a batch (QSArgs::mask_fs) -- in particular the packed last strip,
where one wave holds that strip of several frames side by side and every segment has to read its own frame's mask.

Reference, frame by frame and bit for bit: oracle.Pyramid.build(frame, T, weak, mask=masks[f]) (Detector::match's mask
belongs to the call, line2Dup.cpp:1078; quantize() :446-450; pyrDown() resizes it with INTER_NEAREST, :439).  T is
[4, 8] and both levels are checked where the reference's preconditions (line2Dup.cpp:639, :751-752) admit the geometry;
12 and 20 rows halve to 6 and 10, which no T = 8 level takes, so those two geometries are checked at level 0 against
the pyramid [4].  Level 1 runs the kernel a second time, on its own fused pyrDown output and the masks sampled as
pyrDown() samples them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frame_mask_cases as FM
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")

# rows, cols, frames, segment lanes of the packed last strip (0: a wave per frame)
CASES = [
    (16, 256, 9, 8),    # 8 frames per packed wave: a full group plus a group of one
    (12, 320, 5, 24),   # 2 frames per wave
    (20, 512, 7, 12),   # 5 per wave
    (16, 480, 3, 0),    # the last strip is full and not packed
    (16, 128, 3, 0),    # a single strip
]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """the kernel source + its per-frame-mask harness as a shared object of this test's own (flags of tests/emu/Makefile)"""
    so = str(tmp_path_factory.mktemp("emu_masks") / "libsbm_emu_masks.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-variable",
                           "-Wno-unused-but-set-variable", "-Wno-unknown-pragmas", "-I" + EMU_DIR, "-I" + CSRC, "-o", so,
                           os.path.join(EMU_DIR, "quantize_stream_masks_emu.cpp")])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.sbm_emu_quantize_stream_frame_masks.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int64, C.c_float, vp, vp,
                                                      C.c_int, C.c_int]
    L.sbm_emu_pack_lanes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64]

    def run(frames, mask_buf, mask_fs, hs, pack=1):
        frames = np.ascontiguousarray(frames)
        n, r, c = frames.shape[:3]
        ch = 1 if frames.ndim == 3 else 3
        out = np.full((n, r, c), 0xAA, np.uint8)
        pyr = np.full((n, r // 2, c // 2) + (() if ch == 1 else (3,)), 0xAA, np.uint8)
        lanes = L.sbm_emu_quantize_stream_frame_masks(frames.ctypes.data, n, r, c, c * ch, ch, mask_buf.ctypes.data, mask_fs, FM.WEAK,
                                                      out.ctypes.data, pyr.ctypes.data, hs, pack)
        assert lanes >= 0
        return out, pyr, lanes

    run.lib = L
    return run


def check_level(emu, frames, masks, want, level, hs, expect_lanes, what):
    """the kernel on `frames` under masks[f], dense and at a stride of two masks with garbage in between, packed and
    not: frame f's map is want[f][level]"""
    n, rows, cols = masks.shape
    buf, fs = FM.strided(masks)
    for mask_buf, mask_fs in ((np.ascontiguousarray(masks), rows * cols), (buf, fs)):
        out, pyr, lanes = emu(frames, mask_buf, mask_fs, hs, pack=1)
        assert lanes == expect_lanes, (what, lanes)
        for f in range(n):
            assert np.array_equal(out[f], want[f][level]), (what, level, mask_fs, f, np.argwhere(out[f] != want[f][level])[:5])
        out1, pyr1, lanes1 = emu(frames, mask_buf, mask_fs, hs, pack=0)  # a wave per frame: the same bytes
        assert lanes1 == 0 and np.array_equal(out1, out) and np.array_equal(pyr1, pyr), what
    return pyr


@pytest.mark.parametrize("ch", [1, 3], ids=["gray", "bgr"])
@pytest.mark.parametrize("rows,cols,n,lanes", CASES)
def test_every_frame_under_its_own_mask(emu, oracle, rows, cols, n, lanes, ch):
    frames = FM.textured_frames(rows * 1000 + cols + ch, n, rows, cols, ch)
    T = FM.pyramid_T(rows, cols)
    # batches of three have no room for both special frames beside two telling ones: a second mask set carries the all-255 one
    mask_sets = [FM.frame_masks(cols + n, n, rows, cols)]
    if n == 3:
        second = FM.frame_masks(cols + n + 1, n, rows, cols)
        second[1] = 255
        mask_sets.append(second)
    for masks in mask_sets:
        want = FM.assert_masks_matter(oracle, frames, masks, T)
        pyr = check_level(emu, frames, masks, want, 0, 8, lanes, (rows, cols, n, ch))
        if len(T) == 2:
            # level 1: the next level's image is the kernel's own pyrDown output, its masks pyrDown()'s nearest samples
            m1 = np.ascontiguousarray(masks[:, ::2, ::2])
            lanes1 = emu.lib.sbm_emu_pack_lanes(rows // 2, cols // 2, ch, n, m1[0].size)
            check_level(emu, pyr, m1, want, 1, 4, lanes1, (rows // 2, cols // 2, n, ch))


def test_shared_mask_is_stride_zero(emu, oracle):
    """mask_fs = 0: every frame, packed or not, under the one mask -- the launch every existing entry point makes"""
    rows, cols, n = 16, 256, 9
    frames = FM.textured_frames(5, n, rows, cols, 3)
    mask = FM.rect_mask(np.random.RandomState(6), rows, cols)
    out, _, lanes = emu(frames, mask, 0, 8)
    assert lanes == 8
    want = FM.oracle_maps(oracle, frames, [mask] * n, [4, 8])
    for f in range(n):
        assert np.array_equal(out[f], want[f][0]), f


def test_pack_refused_when_mask_offsets_leave_32_bits(emu):
    """per-lane offsets are 32-bit: the masks of a packed group must lie within 2 GiB of the group's first (as the
    frames must); past that the last strip gets a wave per frame"""
    L = emu.lib
    per = 8  # 16 x 256: 8 frames per wave
    assert L.sbm_emu_pack_lanes(16, 256, 1, 9, 16 * 256) == 8
    limit = 0x7FF00000 // per
    assert L.sbm_emu_pack_lanes(16, 256, 1, 9, limit - 1) == 8
    assert L.sbm_emu_pack_lanes(16, 256, 1, 9, limit) == 0
    assert L.sbm_emu_pack_lanes(16, 256, 1, 9, 1 << 40) == 0
    assert L.sbm_emu_pack_lanes(16, 256, 1, 9, -4096) == 0
    assert L.sbm_emu_pack_lanes(16, 256, 1, 9, 0) == 8
