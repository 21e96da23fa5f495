"""CPU (not gpu): level 0's gradient stage made only where the flagged refinement tiles' strip builders read its map.

Three parts, all compiled here for the CPU (tests/emu/sparse_gradient_emu.cpp):
  footprint   sbm_refine_tiles.h: for every single flagged tile the gradient work items that gradient_item_needed keeps write
              every pixel that the tile's workgroup of build_lm_strip4_allty<true> loads (the loads enumerated thread by thread
              from that kernel's index arithmetic), and a single tile never keeps more than a bounded share of the items
  emulation   sbm_quantize_stream.h on wave_emu.h: the source pass (QS_SOURCE) gives the whole kernel's cv::pyrDown output and
              an exact, packed copy of the input -- also from padded rows and padded or interleaved frames; the sparse pass (QS_SPARSE) over that copy gives the whole kernel's map bit for bit
              with every tile flagged, and with some tiles flagged the map on every pixel those tiles' builders load and a
              poison pattern wherever it wrote nothing
  plan        sbm_level_forms.h: BuildPlan::sparse_gradient is set exactly when level 0 is planned LM_BIT_STRIPS_SPARSE by a
              match entry point, the knob is on, the launch takes the streaming kernel, and the call has no mask and no bands"""
import ctypes as C
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from shape_based_matching_amd import synth

sys.path.insert(0, os.path.join(ROOT, "tools"))
from fuzz_sequence import padded_layout  # noqa: E402

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
POISON = 0xAA  # no orientation byte (0 or one bit) looks like it
T = 4


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("sparse_gradient_emu") / "libsparse_gradient_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-variable",
                           "-Wno-unused-but-set-variable", "-Wno-unknown-pragmas", "-I", EMU_DIR, "-I", CSRC, "-o", so,
                           os.path.join(EMU_DIR, "sparse_gradient_emu.cpp")])
    L = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    L.sbm_emu_whole_pass.argtypes = [vp, i, i, i, i, C.c_float, i, i, vp, vp]
    L.sbm_emu_source_pass.argtypes = [vp, i, i, i, i, i, i, i, C.c_int64, vp, vp]
    L.sbm_emu_sparse_pass.argtypes = [vp, i, i, i, i, C.c_float, i, i, vp, i, i, i, vp]
    L.sbm_emu_footprint.argtypes = [i, i, i, i, i, vp, vp]
    L.sbm_emu_footprint.restype = C.c_int64
    L.sbm_emu_sparse_gradient_plan.argtypes = [vp] + [i] * 7 + [vp]
    return L


# ---- footprint ------------------------------------------------------------------------------------------------------------

# rows per gradient work item: everything the host's two sizing rules can return (even, 4 .. 130), the 2 and the large values
# that sbm_set_quantize_mode / SBM_QS_HS may force
HS = list(range(2, 132, 2)) + [256, 1024]


@pytest.mark.parametrize("cols", [512, 640, 1024, 448, 576, 704])
def test_kept_items_cover_every_pixel_a_flagged_tiles_builder_loads(emu, cols):
    """widths: 512 (two full strips and a 32-column last strip, the packed one), 640, 1024, and 448, 576, 704, whose last tile
    column is cut to 16 cells; 3 .. 8 tile rows, the last one whole and cut; every hs; every single flagged tile"""
    kept, loaded = C.c_int32(0), C.c_int64(0)
    n_cb = (cols // T + 31) // 32
    assert n_cb == {512: 4, 640: 5, 1024: 8, 448: 4, 576: 5, 704: 6}[cols]
    assert ((cols // T) % 32 == 16) == (cols in (448, 576, 704))
    for tile_rows in range(3, 9):
        for rows in (tile_rows * 128, tile_rows * 128 - 80):
            n_rb = (rows // T + 31) // 32
            assert n_rb == tile_rows
            for hs in HS:
                n_items = ((cols + 239) // 240) * ((rows + hs - 1) // hs)
                for ty in range(n_rb):
                    for tx in range(n_cb):
                        missing = emu.sbm_emu_footprint(rows, cols, hs, tx, ty, C.byref(kept), C.byref(loaded))
                        assert missing == 0, (rows, cols, hs, tx, ty, missing)
                        assert loaded.value > 0
                        # not by keeping everything: a tile's 132 x 131 pixels meet at most 2 strips (3 where two strip borders
                        # fall inside it: never at 240 columns per strip) and ceil(131 / hs) + 1 row blocks, + 1 for the moved last block
                        assert 0 < kept.value <= 2 * (-(-131 // hs) + 2), (rows, cols, hs, tx, ty, kept.value)
                        if hs <= 32 and n_rb >= 4:
                            assert kept.value < n_items // 2, (rows, cols, hs, tx, ty, kept.value, n_items)


# ---- emulation ------------------------------------------------------------------------------------------------------------

def tile_rect(tx, ty, rows, cols):
    """refine_tile_pixels restated: the pixels the builder of tile (tx, ty) loads, T = 4"""
    W, H = cols // T, rows // T
    gx1, gy1 = min((tx + 1) * 32, W), min((ty + 1) * 32, H)
    return tx * 128, ty * 128, min(cols, gx1 * T + T), min(rows, gy1 * T + T - 1)


def make_frames(n, rows, cols, ch, seed):
    """scenes with noise, a constant band (the constant-row shortcut of both forms) and one frame of pure noise"""
    rs = np.random.RandomState(seed)
    out = []
    for f in range(n):
        a = synth.scene_bgr(seed + f, rows, cols) if ch == 3 else synth.scene_gray(seed + f, rows, cols)
        a = a.copy()
        if f == 1:
            a = rs.randint(0, 256, a.shape).astype(np.uint8)
        else:
            a[rows // 3: rows // 3 + 20] = 37
            a[:, cols // 2: cols // 2 + 8] = rs.randint(0, 256, a[:, cols // 2: cols // 2 + 8].shape)
        out.append(a)
    return np.ascontiguousarray(np.stack(out))


CASES = [(96, 512, 3, 1), (96, 512, 3, 3), (96, 512, 1, 3), (96, 512, 1, 1), (70, 260, 3, 1), (70, 260, 3, 3), (70, 260, 1, 1), (70, 260, 1, 3),
         (272, 512, 1, 2),  # three tile rows, so that whole row blocks are skipped
         (96, 576, 3, 3)]   # a cut tile column; the 96-column last strip packed two frames per wave: a whole group and a partial one


@pytest.mark.parametrize("rows,cols,ch,n", CASES)
def test_the_two_forms_reproduce_the_whole_kernel(emu, rows, cols, ch, n):
    frames = make_frames(n, rows, cols, ch, 11 + rows + ch)
    shape_p = (n, rows // 2, cols // 2) + ((3,) if ch == 3 else ())
    W, H = cols // T, rows // T
    n_cb, n_rb = (W + 31) // 32, (H + 31) // 32
    for hs, hs_src, pack in ((18, 32, 1), (32, 18, 1), (8, 4, 0)):
        want = np.full((n, rows, cols), POISON, np.uint8)
        want_pyr = np.full(shape_p, POISON, np.uint8)
        assert emu.sbm_emu_whole_pass(frames.ctypes.data, n, rows, cols, ch, 30.0, hs, pack, want.ctypes.data, want_pyr.ctypes.data) >= 0
        assert (want != POISON).all() and (want != 0).sum() > 500

        pyr = np.full(shape_p, POISON, np.uint8)
        keep = np.full(frames.shape, POISON, np.uint8)
        lanes = emu.sbm_emu_source_pass(frames.ctypes.data, n, rows, cols, ch, hs_src, pack, cols * ch, rows * cols * ch, pyr.ctypes.data,
                                        keep.ctypes.data)
        assert lanes >= 0 and (lanes > 0) == (pack == 1 and n > 1 and cols in (260, 512, 576))
        if cols == 576 and lanes:
            assert 64 // lanes == 2 and n % 2 == 1  # the last group holds one frame
        assert np.array_equal(pyr, want_pyr), np.argwhere(pyr != want_pyr)[:5]
        assert np.array_equal(keep, frames), np.argwhere(keep != frames)[:5]

        # every tile flagged (and no flag array at all): the whole map
        for flags in (np.ones((n, n_cb * n_rb), np.uint8), None):
            got = np.full((n, rows, cols), POISON, np.uint8)
            assert emu.sbm_emu_sparse_pass(keep.ctypes.data, n, rows, cols, ch, 30.0, hs, pack, None if flags is None else flags.ctypes.data, T, W, H,
                                           got.ctypes.data) >= 0
            assert np.array_equal(got, want), np.argwhere(got != want)[:5]

        # a random quarter of the tiles (at least one per call, other ones per frame)
        rs = np.random.RandomState(hs)
        flags = np.zeros((n, n_cb * n_rb), np.uint8)
        for f in range(n):
            flags[f, rs.choice(n_cb * n_rb, max(1, n_cb * n_rb // 4), replace=False)] = 1
        got = np.full((n, rows, cols), POISON, np.uint8)
        assert emu.sbm_emu_sparse_pass(keep.ctypes.data, n, rows, cols, ch, 30.0, hs, pack, flags.ctypes.data, T, W, H, got.ctypes.data) >= 0
        needed = np.zeros((n, rows, cols), bool)
        for f in range(n):
            for t in np.flatnonzero(flags[f]):
                x0, y0, x1, y1 = tile_rect(t % n_cb, t // n_cb, rows, cols)
                needed[f, y0:y1, x0:x1] = True
        assert needed.any() and np.array_equal(got[needed], want[needed])
        assert ((got == want) | (got == POISON)).all()  # written = right, everything else untouched
        if n_cb * n_rb >= 4 and hs <= 18:
            assert (got == POISON).sum() > got.size // 8, (got == POISON).mean()  # ... and work was skipped


LAYOUTS = [(13, 0), (64, 0), (0, 1000), (0, -1), (13, -1), (64, 1000)]  # (row pad, frame pad; -1: a whole, inverted frame between)


@pytest.mark.parametrize("rows,cols,ch,n", [(96, 576, 3, 3), (96, 576, 1, 3), (70, 260, 3, 3), (70, 260, 1, 2), (70, 260, 3, 1)])
def test_source_pass_reads_the_callers_layout_and_writes_packed(emu, rows, cols, ch, n):
    """the source pass on padded rows and padded or interleaved frames: the retained copy is the packed input, cv::pyrDown is
    the whole kernel's on the packed frames, and no byte of the padding (0xA5, or the inverted frame) shows in either"""
    frames = make_frames(n, rows, cols, ch, 23 + rows + ch)
    shape_p = (n, rows // 2, cols // 2) + ((3,) if ch == 3 else ())
    for hs_src, pack in ((32, 1), (18, 1), (4, 0)):
        want_pyr = np.full(shape_p, POISON, np.uint8)
        scratch = np.full((n, rows, cols), POISON, np.uint8)
        assert emu.sbm_emu_whole_pass(frames.ctypes.data, n, rows, cols, ch, 30.0, 18, pack, scratch.ctypes.data, want_pyr.ctypes.data) >= 0
        for row_pad, frame_pad in LAYOUTS:
            buf, stride, fs = padded_layout(list(frames), row_pad, frame_pad)
            assert buf.size > frames.size and stride == cols * ch + row_pad
            pyr = np.full(shape_p, POISON, np.uint8)
            keep = np.full(frames.shape, POISON, np.uint8)
            lanes = emu.sbm_emu_source_pass(buf.ctypes.data, n, rows, cols, ch, hs_src, pack, stride, fs, pyr.ctypes.data, keep.ctypes.data)
            assert lanes >= 0 and (lanes > 0) == (pack == 1 and n > 1), (row_pad, frame_pad, lanes)
            assert np.array_equal(keep, frames), (row_pad, frame_pad, hs_src, np.argwhere(keep != frames)[:5])
            assert np.array_equal(pyr, want_pyr), (row_pad, frame_pad, hs_src, np.argwhere(pyr != want_pyr)[:5])


# ---- plan -----------------------------------------------------------------------------------------------------------------

def test_plan_makes_level_0_sparsely_exactly_under_its_conditions(emu):
    SPARSE = 5
    seen = {0: 0, 1: 0}
    for Ts, rows0, cols0 in (((4, 8), 1024, 1024), ((4, 8), 512, 640), ((4, 8), 480, 672), ((8, 8), 1024, 1024), ((4, 4, 8), 1024, 1024), ((4,), 512, 512)):
        L = len(Ts)
        geo = np.array([L, *Ts, *[rows0 >> l for l in range(L)], *[cols0 >> l for l in range(L)]], np.int32)
        for strips, grad, stream, mask, banded, one_launch, match in itertools.product((0, 1), repeat=7):
            form0 = C.c_int32(0)
            got = emu.sbm_emu_sparse_gradient_plan(geo.ctypes.data, strips, grad, stream, mask, banded, one_launch, match, C.byref(form0))
            # level 0 is planned sparse: two levels, T = 4 on a grid of whole 16-cell strips, the one-launch builder, a match entry point
            level0_sparse = bool(strips and one_launch and match and L == 2 and Ts[0] == 4 and (cols0 // 4) % 16 == 0)
            assert (form0.value == SPARSE) == level0_sparse, (Ts, rows0, cols0, strips, one_launch, match)
            want = int(level0_sparse and grad and stream and not mask and not banded)
            assert got == want, (Ts, rows0, cols0, strips, grad, stream, mask, banded, one_launch, match)
            seen[got] += 1
    assert seen[1] == 2 and seen[0] > 700  # (4, 8) at 1024 x 1024 and at 512 x 640, every condition met
