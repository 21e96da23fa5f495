"""CPU (not gpu): the sparse level-0 gradient pass takes its work items from a record of need rectangles.

k_mark_refine_tiles keeps, beside the tile flags, per band of 8 pixel rows the hull {xmin, xmax} of the map columns that some
candidate's refinement can depend on (sbm_refine_tiles.h: refine_need); the sparse form of the streaming gradient kernel places
its strips from the left end of the hull of its rows (gradient_rect_item_needed).  Compiled here for the CPU
(tests/emu/sparse_rects_emu.cpp):

  footprint   for constructed candidates every map pixel a response can depend on is recomputed from the refinement kernel's own
              index arithmetic, restated in numpy -- every in-bounds feature x the 256 window positions x the T x T spread, with
              the flat dword index of local_best_bits and its two wrap cases -- and found inside the hull of its band; without a
              wrap the hull is no wider than the feature extent + 66 + 3 pixels; the rect-driven launch never has more working items
              than the tile-driven one
  emulation   sbm_quantize_stream.h on wave_emu.h: with the record the sparse form gives the whole kernel's map on every pixel
              of every need rectangle, writes nothing else that differs and no byte outside the level; an empty record runs no
              item, a null record is the tile-driven launch"""
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
POISON = 0xAA  # no orientation byte (0 or one bit) looks like it
T = 4
BAND = 8
INT_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("sparse_rects_emu") / "libsparse_rects_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-variable",
                           "-Wno-unused-but-set-variable", "-Wno-unknown-pragmas", "-I", EMU_DIR, "-I", CSRC, "-o", so,
                           os.path.join(EMU_DIR, "sparse_rects_emu.cpp")])
    L = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    L.sbm_emu_mark.argtypes = [C.c_int64, vp, i, i, i, i, i, vp, vp, vp]
    L.sbm_emu_items.argtypes = [vp, vp, i, i, i, i, i, i, vp]
    L.sbm_emu_whole_map.argtypes = [vp, i, i, i, i, C.c_float, i, vp]
    L.sbm_emu_sparse_rect_pass.argtypes = [vp, i, i, i, i, C.c_float, i, vp, vp, i, i, i, vp]
    return L


def mark(emu, cands, rows, cols):
    """(flags, rects, origins) of one frame's candidates: n x (cx, cy, width, height, feature extent x, feature extent y)"""
    W, H = cols // T, rows // T
    cand = np.ascontiguousarray(np.asarray(cands, np.int32).reshape(-1, 6))
    flags = np.full(((W + 31) // 32) * ((H + 31) // 32), 7, np.uint8)
    rects = np.full(((rows + BAND - 1) // BAND, 2), 5, np.int32)
    origin = np.zeros((len(cand), 4), np.int32)
    assert emu.sbm_emu_mark(len(cand), cand.ctypes.data, rows, cols, T, W, H, flags.ctypes.data, rects.ctypes.data, origin.ctypes.data) == 0
    return flags, rects, origin


def items(emu, rects, flags, rows, cols, hs):
    n_strips, n_rb = (cols + 239) // 240, (rows + hs - 1) // hs
    out = np.zeros((n_rb, n_strips), np.int32)
    n = emu.sbm_emu_items(None if rects is None else rects.ctypes.data, flags.ctypes.data, rows, cols, hs, T, cols // T, rows // T, out.ctypes.data)
    assert n == (out >= 0).sum()
    return out


# ---- footprint ------------------------------------------------------------------------------------------------------------

def dependent_pixels(ox, oy, fw, fh, rows, cols, label):
    """local_best_bits (sbm_local_bits.h) and build_lm_strip4_allty (sbm_lm_kernels.h) restated: the map pixels that the 256
    responses of a candidate with window origin (ox, oy) depend on, for a feature of orientation `label` at every (fx, fy) of
    fw x fh.  A feature at pixel (x, y) inside the level reads, for patch row r and window column i, bit (gx0 & 15) + i of the dword
    pair at index ((plane * ns + strip) * H + gy0 + r) and + H, plane = ((y & 3) * 4 + (x & 3)) * 8 + label -- the index is
    flat, whatever row, strip or plane it lands in; past the 128 planes lies the zero tail.  Bit c of the dword of (plane', strip',
    row') is the response at pixel ((strip' * 16 + c) * 4 + dx', row' * 4 + dy') of sub-plane (dy', dx') = divmod(plane' // 8, 4),
    and that is spread from the T x T map pixels from there on, cut to the level."""
    W, H = cols // T, rows // T
    ns = W >> 4
    fy, fx = np.mgrid[0:fh, 0:fw]
    x, y = (fx + ox).ravel(), (fy + oy).ravel()
    ok = (x >= 0) & (y >= 0) & (x < cols) & (y < rows)
    x, y = x[ok].astype(np.int64), y[ok].astype(np.int64)
    need = np.zeros((rows, cols), bool)
    if x.size == 0:
        return need
    gx0, gy0 = x >> 2, y >> 2
    plane = (((y & 3) << 2) | (x & 3)) * 8 + label
    base = ((plane * ns + (gx0 >> 4)) * H + gy0)[:, None, None]
    r = np.arange(16)[None, :, None]
    bit = (gx0 & 15)[:, None, None] + np.arange(16)[None, None, :]
    d = base + r + np.where(bit >= 16, H, 0)
    c = bit & 15
    live = d < 128 * ns * H
    d, c = d[live], np.broadcast_to(c, live.shape)[live]
    plane2, rem = d // (ns * H), d % (ns * H)
    s2, gy2 = rem // H, rem % H
    sub2 = plane2 // 8
    px, py = (s2 * 16 + c) * 4 + (sub2 & 3), gy2 * 4 + (sub2 >> 2)
    for dy in range(T):
        for dx in range(T):
            qx, qy = px + dx, py + dy
            inside = (qx < cols) & (qy < rows)
            need[qy[inside], qx[inside]] = True
    return need


# (name, rows, cols, (cx, cy, width, height, feature extent x, feature extent y), wrap): the declared box clamps, the extent is
# the features' own -- one past the box as in the reference's templates (features AT x = width), or far past it for the wrap cases
FOOTPRINT_CASES = [
    ("left-top", 160, 448, (0, 0, 60, 40, 61, 41), False),
    # (clamped to the right border, the feature column AT x = width starts the last strip: its patches read the strip behind it)
    ("right-bottom", 160, 448, (400, 400, 60, 40, 61, 41), True),
    ("left-bottom", 160, 576, (0, 400, 60, 40, 61, 41), False),
    ("right-top", 160, 704, (400, 0, 60, 40, 61, 41), True),
    ("right-top, features inside the box", 160, 704, (400, 0, 60, 40, 60, 40), False),
    ("inside, ox = 4 mod 16", 160, 576, (18, 20, 60, 40, 61, 41), False),
    ("inside", 160, 704, (150, 21, 60, 40, 61, 41), False),
    ("patch passes row H - 1", 160, 576, (100, 400, 60, 40, 61, 90), True),
    ("strip past the last strip", 160, 448, (400, 20, 60, 40, 120, 41), True),
    ("both wraps", 160, 448, (400, 400, 60, 40, 120, 90), True),
    ("H < 16", 48, 448, (100, 3, 60, 10, 61, 40), True),
    ("H < 16, right", 56, 576, (400, 5, 60, 10, 61, 30), True),
]


@pytest.mark.parametrize("name,rows,cols,cand,wrap", FOOTPRINT_CASES, ids=[c[0] for c in FOOTPRINT_CASES])
def test_every_pixel_a_response_depends_on_lies_in_the_hull_of_its_band(emu, name, rows, cols, cand, wrap):
    flags, rects, origin = mark(emu, [cand], rows, cols)
    x, y, ox, oy = (int(v) for v in origin[0])
    assert ox % T == 0 and oy % T == 0
    need = np.zeros((rows, cols), bool)
    for label in (0, 7):  # label 7 of the last strip wraps into the next SUB-PLANE, label 0 into the next orientation
        need |= dependent_pixels(ox, oy, cand[4], cand[5], rows, cols, label)
    assert need.any()
    ys, xs = np.nonzero(need)
    lo, hi = rects[ys // BAND, 0], rects[ys // BAND, 1]
    miss = (xs < lo) | (xs >= hi)
    assert not miss.any(), (name, list(zip(ys[miss][:5], xs[miss][:5])), rects[np.unique(ys[miss] // BAND)[:5]])
    live = rects[:, 0] < rects[:, 1]
    assert (rects[~live] == [INT_MAX, 0]).all() and (rects[live, 0] >= 0).all() and (rects[live, 1] <= cols).all()
    if not wrap:
        # at cell precision: the hull is the extent + the 15 further cells + the spread's reach, and only the bands of such rows
        assert (rects[live, 1] - rects[live, 0]).max() <= cand[4] + 3 + 66, rects[live]
        assert live.sum() <= (cand[5] + 3 + 66) // BAND + 2
        band_rows = np.unique(ys // BAND)
        # no band without a dependence, but for the one that the rows under the last cell row's first sub-plane may reach into
        assert set(band_rows) <= set(np.flatnonzero(live)) and live.sum() <= len(band_rows) + 1
        # ... and tight: the first needed column is the hull's, the last one within a cell's sub-plane columns of it
        assert xs.min() == rects[live, 0].min()
        assert 0 <= rects[live, 1].max() - (xs.max() + 1) <= 3
    # the rect-driven launch never runs more items than the tile-driven one, and each of its items meets a flagged tile
    for hs in (18, 24, 32):
        by_rect, by_tile = items(emu, rects, flags, rows, cols, hs), items(emu, None, flags, rows, cols, hs)
        assert ((by_rect >= 0).sum(axis=1) <= (by_tile >= 0).sum(axis=1)).all(), (name, hs, by_rect, by_tile)
        assert (by_rect >= 0).any() and (by_rect[by_rect >= 0] % 4 == 0).all()
        # every needed pixel is written by a working item
        cov = np.zeros((rows, cols), bool)
        for rb, k in zip(*np.nonzero(by_rect >= 0)):
            r0 = rb * hs if rb * hs + hs <= rows else max(rows - hs, 0)
            cov[r0: r0 + hs, by_rect[rb, k]: by_rect[rb, k] + 240] = True
        assert not (need & ~cov).any(), (name, hs, np.argwhere(need & ~cov)[:5])


def test_two_distant_objects_share_a_hull_and_the_tile_test_cuts_the_middle(emu):
    rows, cols = 160, 704
    flags, rects, _ = mark(emu, [(5, 20, 60, 40, 61, 41), (330, 20, 60, 40, 61, 41)], rows, cols)
    live = rects[:, 0] < rects[:, 1]
    assert (rects[live, 1] - rects[live, 0]).max() > 600  # wider than two strips
    by_rect, by_tile = items(emu, rects, flags, rows, cols, 32), items(emu, None, flags, rows, cols, 32)
    assert ((by_rect >= 0).sum(axis=1) <= (by_tile >= 0).sum(axis=1)).all()
    assert (by_rect[:, 1] < 0).all() and (by_rect[:, 0] >= 0).any() and (by_rect[:, 2] >= 0).any(), by_rect  # the middle strip never works


def test_item_strips_start_at_a_multiple_of_4(emu):
    """a record whose left end is no multiple of 4 (no T = 4 candidate writes one; the header takes any): the strip is moved left"""
    rows, cols = 160, 576
    flags = np.ones(((cols // T + 31) // 32) * ((rows // T + 31) // 32), np.uint8)
    rects = np.full(((rows + 7) // 8, 2), 0, np.int32)
    rects[:, 0] = INT_MAX
    rects[3] = (6, 300)
    rects[9] = (251, 576)
    got = items(emu, rects, flags, rows, cols, 32)
    assert got[0].tolist() == [4, 244, -1] and got[1].tolist() == [-1, -1, -1] and got[2].tolist() == [248, 488, -1], got


# ---- emulation ------------------------------------------------------------------------------------------------------------

def make_frames(n, rows, cols, ch, seed):
    rs = np.random.RandomState(seed)
    out = []
    for f in range(n):
        a = (synth.scene_bgr(seed + f, rows, cols) if ch == 3 else synth.scene_gray(seed + f, rows, cols)).copy()
        if f == 1:
            a = rs.randint(0, 256, a.shape).astype(np.uint8)
        else:
            a[rows // 3: rows // 3 + 20] = 37  # the constant-row shortcut
        out.append(a)
    return np.ascontiguousarray(np.stack(out))


# per geometry and frame the candidates: xa at 0 and a hull that ends at cols (a candidate at the right border reads the last strip's
# neighbour, a wrap: its rows keep every column) | xa = 4 mod 16 and a hull wider than two strips | none
GEOMETRIES = {
    (96, 576, 3): [[(0, 0, 60, 24, 61, 25), (400, 2, 60, 24, 61, 25)], [(18, 2, 60, 24, 61, 25), (241, 2, 60, 24, 61, 25)], []],
    (448, 576, 3): [[(18, 40, 120, 90, 121, 91), (400, 400, 120, 90, 121, 91)]],
    (512, 704, 1): [[(0, 100, 120, 90, 121, 91), (300, 120, 120, 90, 121, 91)]],
}


@pytest.mark.parametrize("rows,cols,ch", list(GEOMETRIES), ids=["96x576x3", "448x576x3", "512x704x1"])
def test_the_rect_driven_pass_reproduces_the_whole_kernel_where_it_is_needed(emu, rows, cols, ch):
    per_frame = GEOMETRIES[(rows, cols, ch)]
    n = len(per_frame)
    W, H = cols // T, rows // T
    frames = make_frames(n, rows, cols, ch, 31 + rows + ch)
    marks = [mark(emu, c, rows, cols) for c in per_frame]
    flags = np.ascontiguousarray(np.stack([m[0] for m in marks]))
    rects = np.ascontiguousarray(np.stack([m[1] for m in marks]))
    # the cases the geometries are chosen for
    first = [r[r[:, 0] < r[:, 1]] for r in rects]
    if rows == 96:
        assert first[0][:, 0].min() == 0 and first[0][:, 1].max() == cols and first[1][:, 0].min() % 16 == 4 and len(first[2]) == 0
        assert (first[1][:, 1] - first[1][:, 0]).max() > 480
    else:
        assert first[0][:, 1].max() == cols or first[0][:, 0].min() == 0
    GUARD = 4096
    for hs in ((18, 32) if rows == 96 else (32,)):
        want = np.full((n, rows, cols), POISON, np.uint8)
        assert emu.sbm_emu_whole_map(frames.ctypes.data, n, rows, cols, ch, 30.0, hs, want.ctypes.data) == 0
        assert (want != POISON).all()
        for use_rects in (True, False):
            buf = np.full(GUARD + n * rows * cols + GUARD, POISON, np.uint8)
            got = buf[GUARD: GUARD + n * rows * cols].reshape(n, rows, cols)
            count = emu.sbm_emu_sparse_rect_pass(frames.ctypes.data, n, rows, cols, ch, 30.0, hs, flags.ctypes.data,
                                                 rects.ctypes.data if use_rects else None, T, W, H, got.ctypes.data)
            assert (buf[:GUARD] == POISON).all() and (buf[-GUARD:] == POISON).all()  # no byte outside the level
            assert ((got == want) | (got == POISON)).all()  # written = right, everything else untouched
            needed = np.zeros((n, rows, cols), bool)
            working = 0
            for f in range(n):
                if use_rects:
                    for b, (lo, hi) in enumerate(rects[f]):
                        if lo < hi:
                            needed[f, b * BAND: (b + 1) * BAND, lo:hi] = True
                    working += (items(emu, rects[f], flags[f], rows, cols, hs) >= 0).sum()
                else:
                    n_cb = (W + 31) // 32
                    for t in np.flatnonzero(flags[f]):
                        tx, ty = t % n_cb, t // n_cb
                        needed[f, ty * 128: min(rows, min((ty + 1) * 32, H) * T + T - 1), tx * 128: min(cols, min((tx + 1) * 32, W) * T + T)] = True
            assert needed.any() and np.array_equal(got[needed], want[needed]), (hs, use_rects, np.argwhere(needed & (got != want))[:5])
            if use_rects:
                assert count == working > 0
                rect_written = (got != POISON).sum()
            else:
                assert count > 0 and (got != POISON).sum() >= rect_written  # the tile-driven launch, as before: never less
            if not per_frame[-1]:
                assert (got[-1] == POISON).all()  # an empty record (and no flag): no item runs, nothing is written


def test_an_empty_record_runs_no_item_even_under_flagged_tiles(emu):
    rows, cols, ch = 96, 576, 3
    frames = make_frames(1, rows, cols, ch, 5)
    flags = np.ones((1, ((cols // T + 31) // 32) * ((rows // T + 31) // 32)), np.uint8)
    for empty in ((INT_MAX, 0), (0, 0)):  # as cleared, and as allocated
        rects = np.ascontiguousarray(np.tile(np.array(empty, np.int32), ((rows + 7) // 8, 1))[None])
        got = np.full((1, rows, cols), POISON, np.uint8)
        assert emu.sbm_emu_sparse_rect_pass(frames.ctypes.data, 1, rows, cols, ch, 30.0, 32, flags.ctypes.data, rects.ctypes.data, T, cols // T,
                                            rows // T, got.ctypes.data) == 0
        assert (got == POISON).all()
