"""CPU (not gpu): the footprint arithmetic of the sparse level-0 strip build (shape_based_matching_amd/csrc/sbm_refine_tiles.h),
compiled here for the CPU.  For every candidate the test recomputes, from lm_bits_offset restated below, the dword indices
that local_best_bits (sbm_local_bits.h) loads for the extreme in-bounds features of the template box -- rows 0 .. 15 of
both loads, the `pitch` load included, for the first and the last plane (the first wraps past the last strip into the next
plane, the last runs into the zero tail) -- and asserts that each index lies in a marked tile or at or beyond lm_bits_dwords.

Grids: W in {16, 32, 48, 80}, H in {16, 33, 40, 64, 67}, T = 4, boxes from 1 x 1 up to the level size minus the border,
every candidate position (the clamps move most of them).  The literal product of both axes is ~10^9 cases per grid, so it is
enumerated in two parts.  (1) Every case of one axis against three fixed cases of the other.  (2) The product of the two
axes' CLASSES: what is loaded depends on a case only through the cells of its two extreme features on that axis, so the
cases of an axis are grouped by those cells (computed by the test) and one case of every class meets one of every class of
the other axis.  A 256 x 256 grid (8 x 8 tiles) with boxes of at most 32 px is added for the cap below, which the small grids
(at most 3 x 3 tiles) cannot violate.

A cap keeps the test from passing by marking everything: for boxes of at most 32 px no candidate may mark more than 4 x 4
tiles (the reference formula -- bbox / 4 cells + 16 + one strip -- stays within that); it is checked before anything else."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "refine_tiles_emu.cpp")
T = 4
BORDER = 8 * T


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("tiles_emu") / "libtiles_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so, EMU_SRC])
    L = C.CDLL(so)
    L.sbm_emu_refine_tiles.argtypes = [C.c_int64, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
    L.sbm_emu_refine_tiles.restype = C.c_int
    L.sbm_emu_sparse_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.sbm_emu_sparse_plan.restype = C.c_int64
    return L


def trunc_div(a, b):
    """C integer division"""
    return np.where(a >= 0, a // b, -((-a) // b))


def axis_origin(c, size, length):
    """the clamp of similarity_local_body on one axis: candidate coordinate c one level up, box size, level length"""
    x = 2 * c + 1
    x = np.maximum(x, BORDER)
    x = np.minimum(x, length - size - BORDER)
    return x, (trunc_div(x, T) - 8) * T


def axis_cases(length, max_size, extra=0):
    """every (candidate coordinate, box size) of one axis, and per case the cells of its two extreme in-bounds features;
    extra: the features reach that many pixels past the declared box, which alone the clamp sees"""
    c, size = np.meshgrid(np.arange(length // 2), np.arange(1, max_size + 1), indexing="ij")
    c, size = c.ravel(), size.ravel()
    _, o = axis_origin(c, size, length)
    lo, hi = np.maximum(0, -o), np.minimum(size + extra - 1, length - 1 - o)  # extreme in-bounds feature coordinates
    valid = lo <= hi
    g_lo, g_hi = np.where(valid, (lo + o) >> 2, -1), np.where(valid, (hi + o) >> 2, -1)
    return c, size, g_lo, g_hi


def class_representatives(g_lo, g_hi):
    key = (g_lo.astype(np.int64) + 1) * 100000 + (g_hi + 1)
    _, first = np.unique(key, return_index=True)
    return first


def need_table(W, H, n_cb):
    """need[gx, gy]: bit t set = a feature at cell (gx, gy) loads a dword of tile t (lm_bits_offset, restated)"""
    ns = W >> 4
    total = 128 * ns * H  # lm_bits_dwords
    gx = np.arange(W, dtype=np.int64)[:, None, None, None, None]
    gy = np.arange(H, dtype=np.int64)[None, :, None, None, None]
    plane = np.array([0, 127], np.int64)[None, None, :, None, None]
    load = np.arange(2, dtype=np.int64)[None, None, None, :, None]  # the row's dword, and the one `pitch` = H dwords on
    r = np.arange(16, dtype=np.int64)[None, None, None, None, :]
    idx = (plane * ns + (gx >> 4)) * H + gy + r + load * H
    strip, row = (idx // H) % ns, idx % H
    tile = (row >> 5) * n_cb + (strip >> 1)
    bits = np.where(idx < total, np.uint64(1) << np.minimum(tile, 63).astype(np.uint64), np.uint64(0))
    return np.bitwise_or.reduce(bits.reshape(W, H, -1), axis=2)


def popcount(m):
    m = m.copy()
    n = np.zeros(m.shape, np.int64)
    while m.any():
        n += (m & np.uint64(1)).astype(np.int64)
        m >>= np.uint64(1)
    return n


def check(emu, W, H, xs, ys, need, n_cb, n_rb, extra=0):
    """the product of the x cases xs and the y cases ys (each: c, size, g_lo, g_hi)"""
    rows, cols = H * T, W * T
    cx, w, gx_lo, gx_hi = (np.repeat(a, len(ys[0])) for a in xs)
    cy, h, gy_lo, gy_hi = (np.tile(a, len(xs[0])) for a in ys)
    n = len(cx)
    cand = np.ascontiguousarray(np.stack([cx, cy, w, h], axis=1).astype(np.int32))
    origin = np.zeros((n, 4), np.int32)
    mask = np.zeros(n, np.uint64)
    assert emu.sbm_emu_refine_tiles(n, cand.ctypes.data, rows, cols, T, W, H, extra, origin.ctypes.data, mask.ctypes.data) == n_cb * n_rb
    # the cap first: boxes of at most 32 px mark at most 4 x 4 tiles
    small = (w + extra <= 32) & (h + extra <= 32)
    col_any = np.zeros(n, np.int64)
    for tx in range(n_cb):
        col_bits = np.uint64(sum(1 << (ty * n_cb + tx) for ty in range(n_rb)))
        col_any += (mask & col_bits) != 0
    row_any = np.zeros(n, np.int64)
    for ty in range(n_rb):
        row_any += (mask & np.uint64(((1 << n_cb) - 1) << (ty * n_cb))) != 0
    assert (col_any[small] <= 4).all() and (row_any[small] <= 4).all() and (popcount(mask[small]) <= 16).all(), (W, H)
    # the clamp is the reference's (line2Dup.cpp:1240-1250), restated per axis
    x, ox = axis_origin(cx, w, cols)
    y, oy = axis_origin(cy, h, rows)
    assert np.array_equal(origin, np.stack([x, y, ox, oy], axis=1).astype(np.int32)), (W, H)
    # every dword of the four extreme in-bounds features lies in a marked tile
    inb = (gx_lo >= 0) & (gy_lo >= 0)
    needed = np.zeros(n, np.uint64)
    for gx in (gx_lo, gx_hi):
        for gy in (gy_lo, gy_hi):
            needed |= np.where(inb, need[np.maximum(gx, 0), np.maximum(gy, 0)], np.uint64(0))
    missing = needed & ~mask
    bad = np.flatnonzero(missing)
    assert bad.size == 0, (W, H, cand[bad[0]].tolist(), hex(int(needed[bad[0]])), hex(int(mask[bad[0]])))
    return n, int(inb.sum())


def run_grid(emu, W, H, max_w, max_h, extra=0):
    n_cb, n_rb = (W + 31) // 32, (H + 31) // 32
    need = need_table(W, H, n_cb)
    xa, ya = axis_cases(W * T, max_w, extra), axis_cases(H * T, max_h, extra)
    pick = lambda a, i: tuple(v[i] for v in a)  # noqa: E731
    # three fixed cases of the other axis: a small box mid-level, the largest box, a box that the far clamp moves
    def fixed(a, length, max_size):
        c, size = a[0], a[1]
        want = [(length // 4, 1), (0, max_size), (length // 2 - 1, min(33, max_size))]
        return np.array([int(np.flatnonzero((c == wc) & (size == ws))[0]) for wc, ws in want])
    n = inb = 0
    for xs, ys in ((xa, pick(ya, fixed(ya, H * T, max_h))), (pick(xa, fixed(xa, W * T, max_w)), ya)):
        a, b = check(emu, W, H, xs, ys, need, n_cb, n_rb, extra)
        n, inb = n + a, inb + b
    xr, yr = pick(xa, class_representatives(xa[2], xa[3])), pick(ya, class_representatives(ya[2], ya[3]))
    step = max(1, 2000000 // max(1, len(yr[0])))
    for i in range(0, len(xr[0]), step):
        a, b = check(emu, W, H, pick(xr, slice(i, i + step)), yr, need, n_cb, n_rb, extra)
        n, inb = n + a, inb + b
    return n, inb


@pytest.mark.parametrize("W", [16, 32, 48, 80])
def test_every_loaded_dword_lies_in_a_marked_tile(emu, W):
    for H in (16, 33, 40, 64, 67):
        n, inb = run_grid(emu, W, H, W * T - BORDER, H * T - BORDER)
        assert n > 1000, (W, H)
        if W > 16 and H > 16:
            assert inb > n // 4, (W, H, n, inb)  # most cases do have in-bounds features: the check is not vacuous


@pytest.mark.parametrize("extra", [1, 96])
def test_features_past_the_declared_box(emu, extra):
    """The reference's templates hold features AT x = width, y = height (cropTemplates: width = max_x - min_x), and an
    uploaded template may declare any box: the footprint is taken of the features' extent.  With features 96 px past the
    box the clamps let patches pass the last grid row (the flat overrun into the next strip) and the last strip (the wrap
    into the next plane); both must have been seen."""
    seen_wrap = seen_over = False
    for W, H in ((32, 33), (48, 40), (80, 67)):
        n, inb = run_grid(emu, W, H, W * T - BORDER, H * T - BORDER, extra)
        assert n > 1000 and inb > n // 4
        xa, ya = axis_cases(W * T, W * T - BORDER, extra), axis_cases(H * T, H * T - BORDER, extra)
        seen_wrap = seen_wrap or bool(((xa[3] >> 4) + 1 >= W >> 4).any())
        seen_over = seen_over or bool((ya[3] + 15 >= H).any())
    assert (seen_wrap and seen_over) == (extra == 96)


def test_cap_on_a_grid_of_8_by_8_tiles(emu):
    n, inb = run_grid(emu, 256, 256, 32, 32)
    assert n > 100000 and inb == n


def test_plan_holds_level_0_sparsely_only_for_two_level_match_calls(emu):
    """sbm_level_forms.h: with PlanInputs::sparse_strips a match entry point plans level 0 of a TWO-level pyramid as
    LM_BIT_STRIPS_SPARSE where it would have been bit strips, the record then calls nothing of the level current (readers
    rebuild from the orientation map) and its signature differs from the whole build's; stage entry points, deeper
    pyramids, T = 8 and grids that are no multiple of 16 cells are planned as without the input"""
    NONE, BIT_STRIPS, SPARSE = -1, 4, 5
    sigs = {}
    for Ts, rows0, cols0 in (((4, 8), 1024, 1024), ((4, 8), 512, 640), ((4, 8), 480, 672), ((8, 8), 1024, 1024), ((4, 4, 8), 1024, 1024),
                             ((4, 8, 8), 1024, 1024)):
        L = len(Ts)
        geo = np.array([L, *Ts, *[rows0 >> l for l in range(L)], *[cols0 >> l for l in range(L)]], np.int32)
        for match in (1, 0):
            out = {}
            for sparse in (0, 1):
                o = np.zeros(4 * L, np.int32)
                sig = emu.sbm_emu_sparse_plan(geo.ctypes.data, sparse, match, o.ctypes.data)
                assert sig >= 0
                out[sparse] = (o.reshape(L, 4).tolist(), sig)
            whole, sp = out[0], out[1]
            eligible = L == 2 and match and whole[0][0][0] == BIT_STRIPS
            assert eligible == (L == 2 and bool(match) and Ts[0] == 4 and (cols0 // 4) % 16 == 0), (Ts, rows0, cols0, match)
            if not eligible:
                assert sp == whole, (Ts, rows0, cols0, match)
                continue
            assert sp[0][0] == [SPARSE, NONE, NONE, 0] and whole[0][0][:2] == [BIT_STRIPS, BIT_STRIPS] and whole[0][0][3] == 1
            assert sp[0][1:] == whole[0][1:] and sp[1] != whole[1]
            sigs[(Ts, rows0, cols0)] = sp[1]
    assert len(sigs) == 2
