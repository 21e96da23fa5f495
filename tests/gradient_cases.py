"""Inputs that sit on the gradient half's edges (line2Dup.cpp:218-450), shared by tests/test_gradient_spec.py (spec vs
oracle, mutation checks) and tests/test_gpu_gradient_spec.py (HIP vs spec).  Deterministic: every case comes from a
fixed seed."""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import gradient_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
from fuzz_gradient import make_image  # noqa: E402

KINDS = ["noise", "low_noise", "rects", "ramp", "checker", "impulses", "half"]
# tile kernel: 16 x 64 output tiles; stream kernel: strips of 240 useful columns
EDGE_COLS = [15, 16, 17, 63, 64, 65, 127, 129, 239, 240, 241]


@dataclass
class Case:
    name: str
    img: np.ndarray
    weak: float = 10.0
    mask: Optional[np.ndarray] = None
    levels: int = 1

    @property
    def shape(self):
        return self.img.shape[:2]


def max_levels(rows: int, cols: int, cap: int = 3) -> int:
    """levels the reference builds before pyrDown would need a side < 2 (cv::pyrDown refuses an empty result)"""
    n = 1
    while n < cap and rows >= 2 and cols >= 2:
        rows, cols = rows // 2, cols // 2
        n += 1
    return n


def kind_image(seed: int, kind: str, rows: int, cols: int, ch: int) -> np.ndarray:
    return make_image(np.random.RandomState(seed), kind, rows, cols, ch)


def border_edges(rows: int, cols: int, ch: int) -> List[Case]:
    """a step edge on each of rows / columns 0..3 and the last four: the replicate borders of the Gaussian and the Sobel,
    the zeroed ring and the vote next to it"""
    out = []
    for k in list(range(4)) + list(range(-4, 0)):
        for axis in (0, 1):
            img = np.full((rows, cols, ch), 40, np.uint8)
            if axis == 0:
                img[k] = 230
            else:
                img[:, k] = 230
            img[rows // 2 :, : cols // 3] = 140  # a corner, so both derivatives are non-zero somewhere
            out.append(Case(f"edge{'rc'[axis]}{k}_{ch}ch", img if ch == 3 else img[:, :, 0], 10.0,
                            levels=max_levels(rows, cols)))
    return out


def colour_ties(rows: int, cols: int, seed: int) -> List[Case]:
    """channels of equal magnitude, with different directions, reaching into the border: the `>=` chain's ties"""
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, (rows, cols)).astype(np.uint8)
    b = np.roll(a, 1, axis=1)
    out = []
    for name, chans in (("opp02", (a, a, 255 - a)), ("opp01", (a, 255 - a, a)), ("opp12", (b, a, 255 - a)),
                        ("tr01", (a, a.T[:rows, :cols] if rows == cols else np.flipud(a), a))):
        out.append(Case(f"tie_{name}_{rows}x{cols}", np.ascontiguousarray(np.stack(chans, axis=2)), 5.0,
                        levels=max_levels(rows, cols)))
    return out


def boundary_ramp_direction(limit: int = 8):
    """(ay, ax) of a linear ramp whose Sobel gradient (8 ax, 8 ay) puts angle*16/360 closest to a half: a bin boundary"""
    best = None
    for ay in range(-limit, limit + 1):
        for ax in range(-limit, limit + 1):
            if ay == 0 or ax == 0:
                continue
            v = float(S.fast_atan2_deg(np.float32(8 * ay), np.float32(8 * ax))) * 16.0 / 360.0
            d = abs(v - np.floor(v) - 0.5)
            if best is None or d < best[0]:
                best = (d, ay, ax)
    return best[1], best[2]


def boundary_ramps(rows: int, cols: int, ch: int) -> List[Case]:
    ay, ax = boundary_ramp_direction()
    yy, xx = np.mgrid[0:rows, 0:cols]
    out = []
    for centre in ((0, 0), (rows - 1, cols - 1), (rows // 2, cols // 2)):  # runs into the border, saturated or not
        v = np.clip(128 + ay * (yy - centre[0]) + ax * (xx - centre[1]), 0, 255).astype(np.uint8)
        img = np.repeat(v[:, :, None], 3, axis=2) if ch == 3 else v
        out.append(Case(f"ramp{ay},{ax}@{centre}_{ch}ch", np.ascontiguousarray(img), 3.0, levels=max_levels(rows, cols)))
    return out


def border_hole_masks(rows: int, cols: int, seed: int) -> List[Case]:
    """masks at odd sizes whose holes touch the border (and one hole inside), over textured frames"""
    out = []
    for ch in (1, 3):
        img = kind_image(seed + ch, "rects", rows, cols, ch)
        for h, holes in enumerate((((0, 0, 3, 5),), ((rows - 2, 0, 2, cols),), ((0, cols - 3, rows, 3), (5, 5, 3, 3)),
                                   ((0, 0, rows, 1), (rows - 1, 0, 1, cols)))):
            m = np.full((rows, cols), 255, np.uint8)
            for r0, c0, hr, hc in holes:
                m[r0 : r0 + hr, c0 : c0 + hc] = 0
            m[1::7, 2::5] = 7  # any non-zero value selects
            out.append(Case(f"mask{h}_{rows}x{cols}_{ch}ch", img, 10.0, m, max_levels(rows, cols)))
    return out


def _voting_magnitudes(img: np.ndarray):
    """(magnitude, row, col) of interior pixels whose 3x3 vote succeeds (so only the threshold decides them)"""
    mag, q, _ = S.quantized_orientations(img, 0.0)
    ys, xs = np.nonzero(q)
    return [(int(mag[y, x]), int(y), int(x)) for y, x in zip(ys, xs)]


def threshold_cases(seed: int) -> List[Case]:
    """weak thresholds whose float32 square equals a magnitude the frame attains at a pixel that votes through:
    one an exact square (weak = |g| of an axis-aligned gradient), one whose float32 square rounds up to the
    integer while the exact square lies below it (float vs double squaring)"""
    out = []
    for ch in (1, 3):
        img = kind_image(seed + ch, "rects", 29, 37, ch)
        mags = _voting_magnitudes(img)
        squares = sorted({m for m, _, _ in mags if int(np.sqrt(m)) ** 2 == m})
        assert squares, "no perfect-square magnitude among the voting pixels"
        out.append(Case(f"thr_square_{ch}ch", img, float(np.sqrt(squares[len(squares) // 2])), levels=2))
        found = None
        for m in sorted({m for m, _, _ in mags}, reverse=True):
            w0 = np.float32(np.sqrt(m))
            cands, up, down = [w0], w0, w0
            for _ in range(6):
                up, down = np.nextafter(up, np.float32(np.inf)), np.nextafter(down, np.float32(-np.inf))
                cands += [up, down]
            for w in cands:
                if float(np.float32(w) * np.float32(w)) == m and float(w) * float(w) < m:
                    found = float(w)
                    break
            if found is not None:
                break
        assert found is not None, "no magnitude whose float32 threshold square rounds onto it from below"
        out.append(Case(f"thr_f32_square_{ch}ch", img, found, levels=2))
    return out


def small_geometries(max_side: int = 9, min_side: int = 1) -> List[Case]:
    out = []
    for r in range(min_side, max_side + 1):
        for c in range(min_side, max_side + 1):
            for ch in (1, 3):
                img = kind_image(1000 * r + 10 * c + ch, "noise", r, c, ch)
                out.append(Case(f"small{r}x{c}_{ch}ch", img, 20.0, levels=max_levels(r, c)))
    return out


def edge_col_cases(rows=(16, 17)) -> List[Case]:
    out = []
    for i, c in enumerate(EDGE_COLS):
        for r in rows:
            for ch in (1, 3):
                kind = KINDS[(i + r + ch) % len(KINDS)]
                out.append(Case(f"cols{c}_{r}_{kind}_{ch}ch", kind_image(i * 31 + r + ch, kind, r, c, ch), 10.0,
                                levels=max_levels(r, c)))
    return out


def kind_cases(rows=33, cols=47) -> List[Case]:
    out = []
    for i, kind in enumerate(KINDS):
        for ch in (1, 3):
            for weak in (0.0, 10.0, 30.5):
                out.append(Case(f"{kind}_{rows}x{cols}_{ch}ch_w{weak}", kind_image(7 * i + ch, kind, rows, cols, ch), weak,
                                levels=3))
    return out


def tiny_pyramids() -> List[Case]:
    """three levels whose level 1 or 2 is 1 to 3 pixels on a side"""
    out = []
    for i, (r, c) in enumerate(((6, 10), (5, 7), (13, 9), (4, 4), (7, 26), (11, 5), (12, 12), (2, 30))):
        for ch in (1, 3):
            out.append(Case(f"tiny{r}x{c}_{ch}ch", kind_image(50 + i, KINDS[i % len(KINDS)], r, c, ch), 5.0,
                            levels=max_levels(r, c)))
    return out


def edge_cases() -> List[Case]:
    """the CPU case set: every geometry and content family of the issue, each with its level count"""
    out = small_geometries()
    out += edge_col_cases()
    out += kind_cases()
    out += tiny_pyramids()
    for ch in (1, 3):
        out += border_edges(21, 19, ch)
        out += boundary_ramps(23, 17, ch)
    out += colour_ties(19, 23, 3) + colour_ties(9, 9, 4)
    out += border_hole_masks(23, 31, 5) + border_hole_masks(17, 9, 6)
    out += threshold_cases(8)
    return out
