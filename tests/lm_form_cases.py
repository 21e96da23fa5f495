"""Inputs, layout decoders, oracle expectations and numpy mutants for the linear-memory builders in every stored form, the shared
check of tests/test_gpu_lm_forms.py and its child worker (``python tests/lm_form_cases.py --run FORM``).
tests/test_lm_form_cases.py proves the inputs and the decoders without a GPU.

The builders turn a one-hot orientation map q into what the two match passes read.  With sp = spread(q, T) (OR over the T x T
window that starts at the pixel, clipped at the image, line2Dup.cpp:616-630), the response of orientation o (:632-747) is 4 where
sp has bit o, else 3 where it has bit o - 1 or o + 1 (mod 8), else 0, and linearize (:749-777) orders a map as
[ty * T + tx][gy][gx] = map[gy * T + ty][gx * T + tx] on the W x H grid, W = cols / T, H = rows / T.  The stored forms, each as
the product's comments describe it, restated here:

  8 planes      d_lm    [8][lm_stride] bytes: the linearized response of orientation o, T * T * W * H bytes, then zeros
  spread plane  d_lmc   [lm_stride] bytes: the linearized spread bytes in the same order, then zeros ...
  strip plane   d_lmc   ... or, inside every sub-plane, the grid cut into W / 16 column strips of 16 cells, a strip stored row
                        after row, 16 bytes per row
  bit strips    d_lbits little-endian dwords: index ((sub * 8 + o) * (W / 16) + strip) * H + gy, bit b of the low half
                        "response > 0" of cell strip * 16 + b in grid row gy, bit 16 + b "response == 4"; then zeros
  bit planes    d_blm   16 planes of lm_stride bits: plane o bit j = (LM[o][j] > 0), plane 8 + o bit j = (LM[o][j] == 4), j the
                        flat index of the 8 planes, little-endian (any_geometry_cases.packed)
  tile flags    d_tiles one byte per tile of 32 grid rows x 32 cells (two strips), row-major over ceil(H / 32) x ceil(W / 32)

Worlds are frames (crops of one larger synthetic scene at different offsets, so that shapes run into every border, and one
all-zero frame) or constructed label maps with activity in the last row and column; ROWS says which entry point builds which
world in which form and what sbm_get_level_build must then report, and names the edge the row is there for.  MUTANTS are plain
numpy functions from the maps to WRONG planes, one per mistake a builder can make at a lane, workgroup, frame, row or strip
boundary; a world is a test of a builder only if every mutant that applies to it changes the answer."""
import functools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import any_geometry_cases as AG  # noqa: E402
from coarse_form_cases import oracle_module  # noqa: E402
from shape_based_matching_amd import synth  # noqa: E402
from shape_based_matching_amd.templates import MATCH_DTYPE, from_pyramids  # noqa: E402

WEAK = 30.0
THR = 99.0
CAP = 4096
# sbm_get_level_build: the bit set of current buffers, the forms, the builders
C_PLANES8, C_SPREAD, C_STRIP, C_BIT_STRIPS, C_BIT_PLANES = 1, 2, 4, 8, 16
F_PLANES8, F_SPREAD, F_STRIP, F_BIT_PLANES, F_BIT_STRIPS, F_SPARSE = 0, 1, 2, 3, 4, 5
B_ROWS, B_ANY, B_GENERIC, B_UNFUSED = 1, 2, 3, 4
KNOBS = ("SBM_FULL_LM", "SBM_STRIP_LM", "SBM_LM_ALLTY", "SBM_FUSED_BITS", "SBM_LOCAL_BITS", "SBM_SPARSE_STRIPS", "SBM_SPARSE_GRADIENT")
KNOB_DEFAULTS = {"SBM_FULL_LM": 0, "SBM_STRIP_LM": 1, "SBM_LM_ALLTY": 1, "SBM_FUSED_BITS": 1, "SBM_LOCAL_BITS": -1, "SBM_SPARSE_STRIPS": 1}


# ---- the layouts, restated ------------------------------------------------------------------------------------------------

def grid(rows, cols, T):
    return cols // T, rows // T  # W, H


def rows_from_linear(flat, T, W, H):
    """row-major plane -> ([T * T][H][W], the bytes behind it)"""
    n = T * T * W * H
    return flat[:n].reshape(T * T, H, W), flat[n:]


def rows_from_strips(flat, T, W, H):
    """strip plane -> ([T * T][H][W], the bytes behind it): sub-plane, strip, grid row, 16 cells"""
    n = T * T * W * H
    return flat[:n].reshape(T * T, W // 16, H, 16).transpose(0, 2, 1, 3).reshape(T * T, H, W), flat[n:]


def bits_from_strips(raw, W, H):
    """bit strips (bytes) -> (any [16][8][H][W], exact [16][8][H][W], the bytes behind the strips)"""
    n = 128 * (W // 16) * H
    d = raw[: 4 * n].view("<u4").reshape(16, 8, W // 16, H)
    b = ((d[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)  # [sub][o][strip][gy][bit]
    cells = lambda x: x.transpose(0, 1, 3, 2, 4).reshape(16, 8, H, W)  # noqa: E731
    return cells(b[..., :16]), cells(b[..., 16:]), raw[4 * n:]


def tiles_from_flags(raw, W, H):
    return raw.reshape((H + 31) // 32, (W + 31) // 32)


def cells_of_tiles(flags, W, H):
    """[H][W] bool: the cells of the flagged tiles"""
    return np.kron(flags != 0, np.ones((32, 32), bool))[:H, :W]


# ---- the operation in numpy (the base of the mutants; checked against the oracle on the CPU) -------------------------------

def np_spread(q, T, wide=None, tall=None, below=None, lane=0, group=0, wrap=False):
    """OR over the clipped window of `tall` rows x `wide` columns (both T: spread()).  The variations are the mutants':
    below   rows that lie behind the map's last row (the next frame's first rows) instead of nothing
    lane    no window crosses a multiple of `lane` pixel columns;  group: ... of `group` pixel rows
    wrap    a window that passes the last column goes on in the next row's first columns"""
    rows, cols = q.shape
    wide, tall = (T if wide is None else wide), (T if tall is None else tall)
    src = q if below is None else np.vstack([q, below[: T - 1]])
    r, c = np.arange(rows), np.arange(cols)
    v = np.zeros_like(q)
    for dy in range(tall):
        ok = r + dy < src.shape[0]
        if group:
            ok &= (r + dy) // group == r // group
        v[ok] |= src[(r + dy)[ok]]
    out = np.zeros_like(q)
    if wrap:
        flat = np.concatenate([v.ravel(), np.zeros(T, np.uint8)])
        for dx in range(wide):
            out |= flat[dx: dx + rows * cols].reshape(rows, cols)
        return out
    for dx in range(wide):
        ok = c + dx < cols
        if lane:
            ok &= (c + dx) // lane == c // lane
        out[:, ok] |= v[:, (c + dx)[ok]]
    return out


def linear(sp, T):
    W, H = grid(sp.shape[0], sp.shape[1], T)
    return np.ascontiguousarray(sp[: H * T, : W * T].reshape(H, T, W, T).transpose(1, 3, 0, 2).reshape(T * T, H, W))


def response(sp, drop_next=False):
    """linearized spread bytes [S][H][W] -> (any, exact), each [S][8][H][W] bool"""
    bit = lambda o: ((sp >> (o & 7)) & 1).astype(bool)  # noqa: E731
    exact = np.stack([bit(o) for o in range(8)], axis=1)
    any_ = np.stack([bit(o) | bit(o + 7) | (False if drop_next else bit(o + 1)) for o in range(8)], axis=1)
    return any_, exact


def planes_of(sp_lin):
    return (sp_lin,) + response(sp_lin)


def lma_shape(T):
    """cells and grid rows of a workgroup of the any-stride builder (sbm_lm_any_plan.h: 64 cells, halved until one grid row fits
    40 KiB of LDS; then 8, 4 or 2 grid rows while they fit)"""
    def lds(cells, grows):
        p = (cells * T + T - 1 + 3) & ~3
        return ((grows + 1) * T - 1) * p + grows * T * p + grows * T * T * cells

    cells = 64
    while cells > 8 and lds(cells, 1) > 40 * 1024:
        cells >>= 1
    for g in (8, 4, 2):
        if lds(cells, g) <= 40 * 1024:
            return cells, g
    return cells, 1


def _last_strip_left(sp):
    out = sp.copy()
    out[:, :, -32:-16] = sp[:, :, -16:]
    out[:, :, -16:] = 0
    return out


def _no_last_row(sp):
    out = sp.copy()
    out[:, -1, :] = 0
    return out


# name -> (applies(T, W, H, B, f), planes(qs, f, T)); qs: the batch's maps of one level, in the order they lie in memory
MUTANTS = {
    "a_window_narrow": (lambda T, W, H, B, f: True, lambda qs, f, T: planes_of(linear(np_spread(qs[f], T, wide=T - 1), T))),
    "b_window_short": (lambda T, W, H, B, f: True, lambda qs, f, T: planes_of(linear(np_spread(qs[f], T, tall=T - 1), T))),
    "c_no_halo_4_cells": (lambda T, W, H, B, f: T > 1 and W > 4, lambda qs, f, T: planes_of(linear(np_spread(qs[f], T, lane=4 * T), T))),
    "c_no_halo_any_cells": (lambda T, W, H, B, f: T > 1 and W > lma_shape(T)[0],
                            lambda qs, f, T: planes_of(linear(np_spread(qs[f], T, lane=lma_shape(T)[0] * T), T))),
    "d_no_halo_16_rows": (lambda T, W, H, B, f: T > 1 and H > 16, lambda qs, f, T: planes_of(linear(np_spread(qs[f], T, group=16 * T), T))),
    "d_no_halo_32_rows": (lambda T, W, H, B, f: T > 1 and H > 32, lambda qs, f, T: planes_of(linear(np_spread(qs[f], T, group=32 * T), T))),
    "d_no_halo_any_rows": (lambda T, W, H, B, f: T > 1 and H > lma_shape(T)[1],
                           lambda qs, f, T: planes_of(linear(np_spread(qs[f], T, group=lma_shape(T)[1] * T), T))),
    # (in the last frame the wrong answer is the right one: nothing lies behind it)
    "e_into_next_frame": (lambda T, W, H, B, f: T > 1 and f + 1 < B, lambda qs, f, T: planes_of(linear(np_spread(qs[f], T, below=qs[f + 1]), T))),
    # (the gradient stage leaves a map's first column empty, so a window that wraps by one pixel finds nothing: T - 1 >= 2)
    "f_into_next_row": (lambda T, W, H, B, f: T > 2, lambda qs, f, T: planes_of(linear(np_spread(qs[f], T, wrap=True), T))),
    "g_any_of_two": (lambda T, W, H, B, f: True,
                     lambda qs, f, T: (lambda sp: (sp,) + response(sp, drop_next=True))(linear(np_spread(qs[f], T), T))),
    "g_halves_swapped": (lambda T, W, H, B, f: True, lambda qs, f, T: (lambda p: (p[0], p[2], p[1]))(planes_of(linear(np_spread(qs[f], T), T)))),
    "h_previous_frame": (lambda T, W, H, B, f: B > 1, lambda qs, f, T: planes_of(linear(np_spread(qs[f - 1], T), T))),
    "i_no_last_grid_row": (lambda T, W, H, B, f: True, lambda qs, f, T: planes_of(_no_last_row(linear(np_spread(qs[f], T), T)))),
    "j_last_strip_left": (lambda T, W, H, B, f: W % 16 == 0 and W >= 32, lambda qs, f, T: planes_of(_last_strip_left(linear(np_spread(qs[f], T), T)))),
}
# the mutants that change an all-zero frame: what leaks into it from a neighbour
ZERO_FRAME_MUTANTS = ("e_into_next_frame", "h_previous_frame")


def planes_differ(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


# ---- worlds ---------------------------------------------------------------------------------------------------------------

# image worlds: T, rows, cols, channels; `edges` are the facts the world is here for (facts() recomputes them on the CPU)
IMAGES = {
    # 5 strips (the last tile is half a tile), H0 = 36 (a cut tile row: H % 32 == 4), W1 * H1 = 180: spread plane + pack
    "i48_144x320": dict(T=(4, 8), rows=144, cols=320, ch=3, edges={"strips": [5, 0], "H%32": [4, 9], "WH%256": 180, "tiles": (2, 3)}),
    # exactly one tile row, two whole tiles; W1 = 16, H1 = 8: half a wave's 256 positions
    "i48_128x256": dict(T=(4, 8), rows=128, cols=256, ch=3, edges={"strips": [4, 1], "H%32": [0, 8], "WH%256": 128, "tiles": (1, 2)}),
    # three tile rows, 7 strips; H1 = 17 is odd and W1 = 28 is no multiple of 16
    "i48_272x448": dict(T=(4, 8), rows=272, cols=448, ch=3, edges={"strips": [7, 0], "H%32": [4, 17], "WH%256": 220, "tiles": (3, 4)}),
    # fused bit planes, W1 = 16: a wave's 64 lanes (4 cells each) hold 16 grid rows of one (ty, tx)
    "i48_256x256": dict(T=(4, 8), rows=256, cols=256, ch=3, edges={"strips": [4, 1], "H%32": [0, 16], "WH%256": 0, "tiles": (2, 2)}),
    # fused bit planes, W1 = 64 and H1 = 12: three waves per (ty, tx); H0 = 48, a cut tile row
    "i48_192x1024": dict(T=(4, 8), rows=192, cols=1024, ch=3, edges={"strips": [16, 4], "H%32": [16, 12], "WH%256": 0, "tiles": (2, 8)}),
    # fused bit planes at T = 4 (lanes 0..31 of the transposing wave only); level 0 in strips by per-ty threads at T = 8
    "i84_128x256": dict(T=(8, 4), rows=128, cols=256, ch=3, edges={"strips": [2, 2], "H%32": [16, 16], "WH%256": 0}),
    # whole bit strips at both T = 4 levels of a three-level pyramid
    "i448_256x256": dict(T=(4, 4, 8), rows=256, cols=256, ch=3, edges={"strips": [4, 2, 0], "H%32": [0, 0, 8], "WH%256": 64}),
    # ... and whole bit strips beside a T = 8 strip level of one strip
    "i488_256x256": dict(T=(4, 8, 8), rows=256, cols=256, ch=3, edges={"strips": [4, 1, 0], "H%32": [0, 16, 8], "WH%256": 64}),
    # the strip plane by per-ty threads, T = 8, three strips (W0 % 16 == 0)
    "i88_256x384": dict(T=(8, 8), rows=256, cols=384, ch=3, edges={"strips": [3, 0], "H%32": [0, 16], "WH%256": 128, "W%16": [0, 8]}),
    # the spread plane row-major: W0 = 40 is no multiple of 16
    "i88_256x320": dict(T=(8, 8), rows=256, cols=320, ch=3, edges={"H%32": [0, 16], "WH%256": 64, "W%16": [8, 4]}),
}
# constructed label maps for the stage path: T, per-level (rows, cols)
MAPS = {
    # whole bit strips beside stage-built response planes, the geometry of the sparse rows
    "m48_144x320": dict(T=(4, 8), dims=[(144, 320), (72, 160)], edges={"strips": [5, 0], "H%32": [4, 9]}),
    # odd H: the last grid row is a single-dword store, the pairs before it are 4-byte aligned only
    "m42_132x128": dict(T=(4, 2), dims=[(132, 128), (66, 64)], edges={"strips": [2, 2], "H&1": [1, 1], "H%32": [1, 1]}),
    "m42_140x192": dict(T=(4, 2), dims=[(140, 192), (70, 96)], edges={"strips": [3, 3], "H&1": [1, 1], "H%32": [3, 3]}),
    # the generic builder: W = 34 (byte-wise ends, W % 4 != 0), a stride that is not 4 or 8; the unfused path: T = 16
    "m4_100x136": dict(T=(4,), dims=[(100, 136)], edges={"W%4": [2]}),
    "m5_100x140": dict(T=(5,), dims=[(100, 140)], edges={"W%4": [0]}),
    "m16_96x160": dict(T=(16,), dims=[(96, 160)], edges={"W%4": [2]}),
}


def facts(T, dims):
    WH = [grid(r, c, t) for (r, c), t in zip(dims, T)]
    return {"strips": [w // 16 if w % 16 == 0 else 0 for w, _ in WH], "H%32": [h % 32 for _, h in WH], "H&1": [h & 1 for _, h in WH],
            "WH%256": WH[-1][0] * WH[-1][1] % 256, "W%16": [w % 16 for w, _ in WH], "W%4": [w % 4 for w, _ in WH],
            "tiles": ((WH[0][1] + 31) // 32, (WH[0][0] + 31) // 32), "cols&3": [c & 3 for _, c in dims]}


def image_frames(rows, cols, ch):
    """four crops of one larger scene at different offsets (pairwise different; shapes run into every border) and, third, an
    all-zero frame"""
    scene = (synth.scene_bgr if ch == 3 else synth.scene_gray)(7, rows + 64, cols + 64, n_shapes=60)
    out = []
    for off in ((0, 0), (64, 64), None, (23, 41), (50, 9)):
        out.append(np.zeros_like(scene[:rows, :cols]) if off is None else scene[off[0]: off[0] + rows, off[1]: off[1] + cols])
    return np.ascontiguousarray(np.stack(out))


def constructed_map(seed, rows, cols):
    """synth.onehot_map (its border ring is empty) plus activity in the last row and the last column: the clipped windows"""
    rs = np.random.RandomState(seed)
    q = synth.onehot_map(rs, rows, cols, 60)
    q[-1, :] = rs.randint(0, 2, cols) << 3
    q[:, -1] = rs.randint(0, 2, rows) << 5
    return q


def cut_templates(cuts, box, nf, seed):
    """one template per (maps of one frame, px, py): nf[l] of the set pixels of level l inside the box at (px, py) >> l, as
    synth.templates_from_maps cuts them -- the template scores 100 where it was cut"""
    rs = np.random.RandomState(seed)
    pyramids = []
    for qs, px, py in cuts:
        tp = []
        for l, q in enumerate(qs):
            w = box >> l
            sub = q[(py >> l): (py >> l) + w + 1, (px >> l): (px >> l) + w + 1]
            ys, xs = np.nonzero(sub)
            assert len(ys) >= 4, (l, px, py, len(ys))
            pick = rs.permutation(len(ys))[: nf[l]]
            f = np.stack([xs[pick], ys[pick], np.log2(sub[ys[pick], xs[pick]]).astype(np.int64)], axis=1)
            tp.append({"width": w, "height": w, "tl_x": 0, "tl_y": 0, "pyramid_level": l, "features": f})
        pyramids.append(tp)
    return from_pyramids(pyramids, "cut")


class Expect:
    """one level of one frame, from the oracle alone: sp [T * T][H][W] linearized spread bytes, lm [8][T * T * W * H]"""

    def __init__(self, O, q, T):
        self.T = T
        self.W, self.H = grid(q.shape[0], q.shape[1], T)
        sp = O.spread(q, T)
        rm = O.response_maps(sp)
        self.sp = O.linearize(sp, T).reshape(T * T, self.H, self.W)
        self.lm = np.stack([O.linearize(rm[o], T).reshape(-1) for o in range(8)])

    def bits(self):
        """(any, exact), each [T * T][8][H][W]"""
        lm = self.lm.reshape(8, self.T * self.T, self.H, self.W).transpose(1, 0, 2, 3)
        return lm > 0, lm == 4

    def planes(self):
        return (self.sp,) + self.bits()


class World:
    """frames or maps, the oracle's orientation maps per frame and level, templates cut from them, expectations on request"""

    def __init__(self, O, name):
        self.O, self.name = O, name
        self.frames = None
        if name in IMAGES:
            p = IMAGES[name]
            self.T, self.ch = p["T"], p["ch"]
            self.frames = image_frames(p["rows"], p["cols"], p["ch"])
        elif name in MAPS:
            p = MAPS[name]
            self.T, self.ch = p["T"], 0
            self.maps = [[constructed_map(100 * len(name) + l, r, c) for l, (r, c) in enumerate(p["dims"])]]
        else:
            case = AG.case(O, name)
            self.T, self.ch = case.T, case.ch
            self.frames = case.frames
            self.ts = case.ts
        self.L = len(self.T)
        self.edges = (IMAGES.get(name) or MAPS.get(name) or {}).get("edges", {})
        self._pyr0 = None
        if self.frames is not None:
            self.frames.setflags(write=False)
            self.maps = []
            for f in range(len(self.frames)):
                pyr = O.Pyramid.build(self.frames[f], list(self.T), WEAK)
                self.maps.append([pyr.quantized(l) for l in range(self.L)])
                if f == 0:
                    self._pyr0 = pyr
                else:
                    pyr.free()
        else:
            self._pyr0 = O.Pyramid.from_quantized(self.maps[0], list(self.T))
        self.dims = [m.shape for m in self.maps[0]]
        self.B = len(self.maps)
        if name in IMAGES:
            rows, cols = self.dims[0]
            box, nf = 48, [48, 40, 24][: self.L]
            a = lambda v: v // 8 * 8  # noqa: E731
            # against the bottom right corner (the refinement clamps the candidate there: the last tile row and column), cut
            # from frames 0 and 1; the centre of frame 3
            self.ts = cut_templates([(self.maps[0], a(cols - box - 32), a(rows - box - 32)), (self.maps[1], a(cols - box - 32), a(rows - box - 32)),
                                     (self.maps[3], a((cols - box) // 2), a((rows - box) // 2))], box, nf, 5)
        elif name in MAPS:
            self.ts = cut_templates([(self.maps[0], 16, 16)], 32, [24, 12][: self.L], 5) if self.L > 1 else None
        self._expect = {}

    def expect(self, f, l):
        if (f, l) not in self._expect:
            self._expect[(f, l)] = Expect(self.O, self.maps[f][l], self.T[l])
        return self._expect[(f, l)]

    def lm_of(self, f, l):
        """frame f's [8][lm_stride] linear memories as the oracle's pyramid holds them"""
        if f == 0:
            return self._pyr0.lm(l)
        pyr = self.O.Pyramid.from_quantized(self.maps[f], list(self.T))
        out = pyr.lm(l)
        pyr.free()
        return out

    def geometry(self, l):
        return grid(self.dims[l][0], self.dims[l][1], self.T[l])


@functools.lru_cache(maxsize=None)
def world(name):
    return World(oracle_module(), name)


# ---- rows: entry point x world x form -------------------------------------------------------------------------------------

def w8(split, packed=0, builder=B_ROWS):
    return (C_PLANES8 | (C_BIT_PLANES if packed else 0), F_PLANES8, builder, split if builder == B_ROWS else 0, 0, packed)


def sp(packed=0, builder=B_ROWS):
    return (C_SPREAD | (C_BIT_PLANES if packed else 0), F_SPREAD, builder, 1 if builder == B_ROWS else 0, 0, packed)


def strip(allty):
    return (C_SPREAD | C_STRIP, F_STRIP, B_ROWS, 1, allty, 0)


BITS = (C_BIT_STRIPS, F_BIT_STRIPS, B_ROWS, 1, 1, 0)
SPARSE = (0, F_SPARSE, B_ROWS, 1, 1, 0)
PLANES = (C_BIT_PLANES, F_BIT_PLANES, B_ROWS, 1, 0, 0)
STAGE_BITS = (C_PLANES8 | C_BIT_STRIPS, F_BIT_STRIPS, B_ROWS, 1, 1, 0)  # whole strips beside the stage-built response planes


def row(rid, world_name, entry, frames, want, edge, coarse="auto", bits=None, knobs=None, pick=None, flags=False):
    """entry: "batch" sbm_match_batch_device, "single" sbm_match_device, "stage" set_quantized on every level then
    match_templates, "set" set_quantized alone; want: per level what sbm_get_level_build must report; pick: which of the world's
    frames make the batch (default the first `frames`); flags: the row is there for its tile flags too (check_flags)"""
    pick = list(range(frames)) if pick is None else list(pick)
    assert len(pick) == frames
    return dict(id=rid, world=world_name, entry=entry, frames=frames, want=list(want), edge=edge, coarse=coarse, bits=bits, knobs=knobs or {},
                pick=pick, flags=flags)


def any_rows():
    out = []
    for name, (T, rows, cols, ch, _, _) in AG.GEOS.items():
        fine = [sp(builder=B_ANY)] * (len(T) - 1)
        edge = "k_build_lm_any, every frame and level: cols & 3 = %s" % [(cols >> l) & 3 for l in range(len(T))]
        out.append(row("any_bits_" + name, name, "batch", 5, fine + [sp(1, B_ANY)], edge + "; spread planes, the coarsest packed"))
        out.append(row("any_bytes_" + name, name, "batch", 5, fine + [w8(0, 0, B_ANY)], edge + "; the coarsest level as 8 planes", coarse="block"))
    return out


ROWS = [
    row("sparse5_144x320", "i48_144x320", "batch", 5, [SPARSE, sp(1)], "sparse bit strips; the half tile of strip 5, the cut tile row 32..35; pack from W1 * H1 = 180",
        flags=True),
    # (frames 3 and 4: each has flagged and unflagged tiles; in frames 0 and 1 every tile is flagged)
    row("sparse2_144x320", "i48_144x320", "batch", 2, [SPARSE, sp(1)], "the same in a batch of two", pick=[3, 4], flags=True),
    row("sparse1_144x320", "i48_144x320", "single", 1, [SPARSE, sp(1)], "the same from sbm_match_device", pick=[3], flags=True),
    row("sparse5_128x256", "i48_128x256", "batch", 5, [SPARSE, sp(1)], "one tile row of exactly 32 grid rows, every tile of a frame flagged; W1 * H1 = 128"),
    row("sparse5_272x448", "i48_272x448", "batch", 5, [SPARSE, sp(1)], "three tile rows, four tile columns, 7 strips", flags=True),
    row("whole5_448", "i448_256x256", "batch", 5, [BITS, BITS, sp(1)], "whole bit strips at both T = 4 levels"),
    row("whole5_488", "i488_256x256", "batch", 5, [BITS, strip(0), sp(1)], "whole bit strips; a T = 8 strip level of one strip"),
    row("stage_48_144x320", "m48_144x320", "stage", 1, [STAGE_BITS, w8(4, 2)], "whole bit strips from ensure_local_forms, H0 = 36, 5 strips"),
    row("stage_42_132x128", "m42_132x128", "stage", 1, [STAGE_BITS, w8(0, 2, B_GENERIC)], "odd H0 = 33: the (H & 1) and last-row stores"),
    row("stage_42_140x192", "m42_140x192", "stage", 1, [STAGE_BITS, w8(0, 2, B_GENERIC)], "odd H0 = 35, 3 strips"),
    row("bytes5_144x320", "i48_144x320", "batch", 5, [strip(1), sp(1)], "strip plane, all four ty per thread, 5 strips, H0 = 36", bits=False),
    row("bytes2_144x320", "i48_144x320", "batch", 2, [strip(1), sp(1)], "the same in a batch of two", bits=False),
    row("perty5_88_256x384", "i88_256x384", "batch", 5, [strip(0), sp(1)], "strip plane by per-ty threads, T = 8, three strips"),
    row("rowmajor5_88_256x320", "i88_256x320", "batch", 5, [sp(), sp(1)], "spread plane row-major, W0 = 40"),
    row("fused5_256x256", "i48_256x256", "batch", 5, [SPARSE, PLANES], "fused bit planes, W1 = 16"),
    row("fused2_192x1024", "i48_192x1024", "batch", 2, [SPARSE, PLANES], "fused bit planes, W1 = 64, H1 = 12; H0 = 48"),
    row("fused5_84_128x256", "i84_128x256", "batch", 5, [strip(0), PLANES], "fused bit planes at T = 4: lanes 0..31"),
    row("planes5_144x320", "i48_144x320", "batch", 5, [SPARSE, w8(1)], "8 planes, split 1 (a batch of five)", coarse="block"),
    row("planes2_144x320", "i48_144x320", "batch", 2, [SPARSE, w8(4)], "8 planes, split 4 (a batch of two)", coarse="block"),
    row("planes1_144x320", "i48_144x320", "single", 1, [SPARSE, w8(4)], "8 planes, split 4 (a single frame)", coarse="block"),
    row("planes5_84_128x256", "i84_128x256", "batch", 5, [strip(0), w8(1)], "8 planes at T = 4, split 1", coarse="block"),
    row("planes2_84_128x256", "i84_128x256", "batch", 2, [strip(0), w8(4)], "8 planes at T = 4, split 4", coarse="block"),
    row("generic_4_100x136", "m4_100x136", "set", 1, [w8(0, 0, B_GENERIC)], "k_build_lm, W = 34: byte-wise stores at the row ends"),
    row("generic_5_100x140", "m5_100x140", "set", 1, [w8(0, 0, B_GENERIC)], "k_build_lm, T = 5"),
    row("unfused_16_96x160", "m16_96x160", "set", 1, [w8(0, 0, B_UNFUSED)], "k_spread, k_response, k_linearize: T = 16"),
] + any_rows()

# one fresh process per knob set (the knobs are read once per process): what it runs
CHILD_ROWS = {
    "sparse_strips0": [row("c_whole5_144x320", "i48_144x320", "batch", 5, [BITS, sp(1)], "whole bit strips on {4, 8}: 5 strips, H0 = 36", knobs={"SBM_SPARSE_STRIPS": "0"}),
                       row("c_whole2_272x448", "i48_272x448", "batch", 2, [BITS, sp(1)], "... 7 strips, three tile rows", knobs={"SBM_SPARSE_STRIPS": "0"})],
    "lm_allty0": [row("c_perty5_144x320", "i48_144x320", "batch", 5, [strip(0), sp(1)], "strip plane by per-ty threads at T = 4", knobs={"SBM_LM_ALLTY": "0"}),
                  row("c_perty2_128x256", "i48_128x256", "batch", 2, [strip(0), sp(1)], "... H0 = 32", knobs={"SBM_LM_ALLTY": "0"})],
    "strip_lm0": [row("c_rowmajor5_144x320", "i48_144x320", "batch", 5, [sp(), sp(1)], "spread plane row-major at T = 4", knobs={"SBM_STRIP_LM": "0"}),
                  row("c_rowmajor2_88_256x384", "i88_256x384", "batch", 2, [sp(), sp(1)], "... at T = 8", knobs={"SBM_STRIP_LM": "0"})],
    "full_lm1": [row("c_full5_144x320", "i48_144x320", "batch", 5, [w8(1), w8(1)], "8 planes at every level, split 1", coarse="block", knobs={"SBM_FULL_LM": "1"}),
                 row("c_full2_144x320", "i48_144x320", "batch", 2, [w8(4), sp(1)], "8 planes at level 0, split 4", knobs={"SBM_FULL_LM": "1"}),
                 row("c_full5_any_bgr_4_8", "bgr_4_8", "batch", 5, [w8(0, 0, B_ANY), w8(0, 2, B_ANY)], "k_build_lm_any, 8 planes at every level",
                     knobs={"SBM_FULL_LM": "1"})],
    "fused_bits0": [row("c_pack5_144x320", "i48_144x320", "batch", 5, [SPARSE, w8(1, 2)], "k_pack_bitplanes over five frames", knobs={"SBM_FUSED_BITS": "0"}),
                    row("c_pack2_256x256", "i48_256x256", "batch", 2, [SPARSE, w8(4, 2)], "... over two, W1 * H1 = 256", knobs={"SBM_FUSED_BITS": "0"})],
}
FORMS = {"sparse_strips0": {"SBM_SPARSE_STRIPS": "0"}, "lm_allty0": {"SBM_LM_ALLTY": "0"}, "strip_lm0": {"SBM_STRIP_LM": "0"},
         "full_lm1": {"SBM_FULL_LM": "1"}, "fused_bits0": {"SBM_FUSED_BITS": "0"}}


def one_launch(T, dims):
    """every level takes k_build_lm_rows: T 4 or 8, rows of the map a multiple of 16 columns, W a multiple of 4"""
    return all(t in (4, 8) and c % 16 == 0 and (c // t) % 4 == 0 for t, (_, c) in zip(T, dims))


# ---- the shared check (GPU) -----------------------------------------------------------------------------------------------

def _upload(frames):
    import torch

    return torch.from_numpy(np.array(frames)).to(torch.device("cuda", 0))


def run_entry(ctx, w, r):
    """the row's entry point on its world"""
    import torch

    ctx.set_coarse_mode(r["coarse"])
    ctx.set_refine_bits(r["bits"])
    if r["entry"] in ("stage", "set"):
        for l in range(w.L):
            ctx.set_quantized(l, w.maps[0][l])
        if r["entry"] == "stage":
            ctx.match_templates(THR)
        return
    B = r["frames"]
    dev = torch.device("cuda", 0)
    fr = w.frames[r["pick"]]
    rows, cols = fr.shape[1], fr.shape[2]
    ch = 1 if fr.ndim == 3 else fr.shape[3]
    d_img = _upload(fr)
    d_out = torch.zeros(B * CAP * MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(B * 2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    if r["entry"] == "single":
        ctx.match_device(d_img.data_ptr(), rows, cols, cols * ch, ch, THR, d_out.data_ptr(), CAP, d_cnt.data_ptr())
    else:
        ctx.match_batch_device(d_img.data_ptr(), rows * cols * ch, B, rows, cols, cols * ch, ch, THR, d_out.data_ptr(), CAP, d_cnt.data_ptr())
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy().reshape(B, 2)
    assert (cnt[:, 1] == 0).all() and (cnt[:, 0] <= CAP).all(), cnt


def check_level(ctx, w, l, b, f, build, fail, tag):
    """frame b of the batch (the world's frame f) at level l: every buffer that the record calls current -- and the flagged
    tiles of a sparse level -- decoded and compared with the oracle's planes of that frame's map; everything behind the layout's
    extent zero.  Returns the tile flags."""
    T = w.T[l]
    W, H = w.geometry(l)
    e = w.expect(f, l)
    cur, form = build[0], build[1]
    n = T * T * W * H
    if cur == 0 and form != F_SPARSE:
        fail((tag, l, f, "nothing is current", build))
    if cur & C_PLANES8:
        raw = ctx.level_stored(l, b, 0).reshape(8, -1)
        if not np.array_equal(raw[:, :n], e.lm):
            fail((tag, l, f, "8 planes", np.argwhere(raw[:, :n] != e.lm)[:3].tolist()))
        if raw[:, n:].any():
            fail((tag, l, f, "8 planes: tail", np.argwhere(raw[:, n:])[:3].tolist()))
    if cur & C_SPREAD:
        got, tail = (rows_from_strips if cur & C_STRIP else rows_from_linear)(ctx.level_stored(l, b, 1), T, W, H)
        if not np.array_equal(got, e.sp):
            fail((tag, l, f, "strip plane" if cur & C_STRIP else "spread plane", np.argwhere(got != e.sp)[:3].tolist()))
        if tail.any():
            fail((tag, l, f, "spread plane: tail", np.flatnonzero(tail)[:3].tolist()))
    flags = None
    if cur & C_BIT_STRIPS or form == F_SPARSE:
        any_, exact, tail = bits_from_strips(ctx.level_stored(l, b, 2), W, H)
        want_any, want_exact = e.bits()
        if form == F_SPARSE and not cur & C_BIT_STRIPS:
            # (a fresh context: the cells of the unflagged tiles were never written)
            flags = tiles_from_flags(ctx.level_stored(l, b, 3), W, H)
            if not np.isin(flags, (0, 1)).all():
                fail((tag, l, f, "tile flags", flags.tolist()))
            m = cells_of_tiles(flags, W, H)
            want_any, want_exact = want_any & m, want_exact & m
        if not np.array_equal(any_, want_any):
            fail((tag, l, f, "bit strips: any", np.argwhere(any_ != want_any)[:3].tolist()))
        if not np.array_equal(exact, want_exact):
            fail((tag, l, f, "bit strips: exact", np.argwhere(exact != want_exact)[:3].tolist()))
        if tail.any():
            fail((tag, l, f, "bit strips: tail", np.flatnonzero(tail)[:3].tolist()))
    if cur & C_BIT_PLANES:
        got = ctx.get_coarse_bitplanes(b)
        lm = np.zeros((8, got.shape[1] * 8), np.uint8)  # lm_stride bytes per plane, the tail zero
        lm[:, :n] = e.lm
        if not np.array_equal(got, AG.packed(lm)):
            fail((tag, l, f, "bit planes", np.argwhere(got != AG.packed(lm))[:3].tolist()))
    return flags


def run_row(r, fail):
    """one row on a fresh context.  Returns counts: levels and frames compared, and the tile flags of a sparse level 0."""
    from shape_based_matching_amd import capi

    w = world(r["world"])
    ctx = capi.Context(T=w.T, weak_threshold=WEAK, device_id=0)
    out = {"id": r["id"], "levels": 0, "frames": 0, "flags": None}
    try:
        if w.ts is not None:
            ctx.upload_templates(w.ts)
        run_entry(ctx, w, r)
        frames = list(enumerate(r["pick"]))  # (position in the batch, the world's frame)
        flags = []
        for l in range(w.L):
            build = ctx.level_build(l)
            if build != tuple(r["want"][l]):
                fail((r["id"], l, "sbm_get_level_build", build, tuple(r["want"][l])))
            for b, f in frames:
                fl = check_level(ctx, w, l, b, f, build, fail, r["id"])
                if fl is not None:
                    flags.append(fl)
                out["frames"] += 1
            if ctx.level_build(l) != build:
                fail((r["id"], l, "the accessors changed the record", ctx.level_build(l), build))
            out["levels"] += 1
        if flags:
            out["flags"] = np.stack(flags).astype(int).tolist()
        # the maps the builders read, every frame and level; then what the stage accessor hands out for frame 0
        for l in range(w.L):
            for b, f in frames:
                if not np.array_equal(ctx.get_quantized_frame(l, b), w.maps[f][l]):
                    fail((r["id"], l, f, "orientation map"))
        for l in range(w.L):
            if not np.array_equal(ctx.get_linear_memories(l), w.lm_of(r["pick"][0], l)):
                fail((r["id"], l, "sbm_get_linear_memories"))
    finally:
        ctx.close()
    return out


def check_flags(r, flags):
    """a row that is there for its flags: a flagged tile in the last tile row and in the last tile column, and a frame that has
    flagged tiles and an unflagged one; nothing flagged in the all-zero frame (the world's frame 2)"""
    fl = np.asarray(flags)  # [frames][tile rows][tile columns]
    assert fl[:, -1, :].any(), (r["id"], "no flagged tile in the last tile row", flags)
    assert fl[:, :, -1].any(), (r["id"], "no flagged tile in the last tile column", flags)
    assert any(x.any() and not x.all() for x in fl), (r["id"], "no frame with flagged tiles and an unflagged one", flags)
    for b, f in enumerate(r["pick"]):
        if f == 2:
            assert not fl[b].any(), (r["id"], "the all-zero frame has a flagged tile", flags)


def run_form(form):
    """the child: the rows of one knob set in this (fresh) process; prints one verdict line, or the first difference"""
    for k in KNOBS:  # the knobs are read when the library first looks at them: set before it is loaded
        if k in FORMS[form]:
            os.environ[k] = FORMS[form][k]
        else:
            os.environ.pop(k, None)
    t0 = time.time()

    def fail(what):
        print("DIFFERENCE " + json.dumps([str(v) for v in what]))
        raise SystemExit(3)

    done = [run_row(r, fail) for r in CHILD_ROWS[form]]
    for r, d in zip(CHILD_ROWS[form], done):
        if r["flags"]:
            check_flags(r, d["flags"])
    print("VERDICT " + json.dumps({"form": form, "ok": True, "rows": [d["id"] for d in done], "levels": sum(d["levels"] for d in done),
                                   "frames": sum(d["frames"] for d in done), "seconds": round(time.time() - t0, 2)}))


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--run" or sys.argv[2] not in FORMS:
        raise SystemExit("usage: lm_form_cases.py --run {%s}" % "|".join(FORMS))
    run_form(sys.argv[2])
