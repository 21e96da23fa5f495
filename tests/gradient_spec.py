"""Plain numpy restatement of the match path's pyramid build (line2Dup.cpp:218-450).

Written from the reference's source and OpenCV's documented semantics, independently of oracle/sbm_oracle.c: each
primitive is a whole-array expression, integer work is exact int64 and float work is float32 one rounding at a time.
It is the third party that the oracle and the HIP gradient kernels are held to (tests/test_gradient_spec.py,
tests/test_gpu_gradient_spec.py).

`Spec` carries the rules that a misreading would change, so that the tests can build each plausible misreading as a
variant and show that their case set tells it apart (the mutation checks).
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import List, Optional, Sequence

import numpy as np

F32 = np.float32

GAUSS7 = np.array([8, 28, 56, 72, 56, 28, 8], np.int64)  # getGaussianKernel(7, 0) in 8.8 fixed point
PYR5 = np.array([1, 4, 6, 4, 1], np.int64)


@dataclass(frozen=True)
class Spec:
    gauss_border: str = "edge"  # BORDER_REPLICATE (line2Dup.cpp:320)
    pyr_border: str = "reflect"  # pyrDown's default BORDER_REFLECT_101
    pyr_size_ceil: bool = False  # Size(src.cols / 2, src.rows / 2), integer division (:431)
    tie_lowest_channel: bool = True  # the `>=` chain of :370-387
    thr_strict: bool = True  # mag > threshold (:268)
    vote_first_max: bool = True  # `max_votes < histogram[i]` (:297)
    zero_ring: bool = True  # :227-236
    thr_square_f32: bool = True  # threshold * threshold in float (:328, :399)


SPEC = Spec()


# ---- padding -------------------------------------------------------------------------------------------------------
def _pad(a: np.ndarray, n: int, mode: str) -> np.ndarray:
    """Pads the first two axes by n.  numpy's "reflect" is OpenCV's BORDER_REFLECT_101; where n exceeds the side it
    reflects the whole side again and again, as borderInterpolate does (a 1-pixel side repeats).  Padding one pixel at
    a time would not: it reflects the pad already added."""
    return np.pad(a, [(n, n), (n, n)] + [(0, 0)] * (a.ndim - 2), mode=mode)


# ---- GaussianBlur(7x7, sigma 0, BORDER_REPLICATE) on 8-bit ---------------------------------------------------------
def gaussian7(img: np.ndarray, spec: Spec = SPEC) -> np.ndarray:
    """(sum_j K_j sum_i K_i s + 2^15) >> 16 over a 7x7 window: OpenCV's exact 8.8 horizontal pass and a single rounding
    of the vertical one, written as one 2-D integer sum."""
    s = img.astype(np.int64)
    r, c = s.shape[:2]
    p = _pad(s, 3, spec.gauss_border)
    total = np.zeros(s.shape, np.int64)
    for j in range(7):
        for i in range(7):
            total += GAUSS7[j] * GAUSS7[i] * p[j : j + r, i : i + c]
    return ((total + (1 << 15)) >> 16).astype(np.uint8)


# ---- Sobel 3x3, BORDER_REPLICATE, per channel -----------------------------------------------------------------------
def sobel3(sm: np.ndarray):
    s = sm.astype(np.int64)
    r, c = s.shape[:2]
    p = _pad(s, 1, "edge")
    dx = np.zeros(s.shape, np.int64)
    dy = np.zeros(s.shape, np.int64)
    for j, wj in enumerate((1, 2, 1)):
        dx += wj * (p[j : j + r, 2 : 2 + c] - p[j : j + r, 0:c])
    for i, wi in enumerate((1, 2, 1)):
        dy += wi * (p[2 : 2 + r, i : i + c] - p[0:r, i : i + c])
    return dx, dy


# ---- fastAtan2 (cv::phase, angleInDegrees) -------------------------------------------------------------------------
_DEG = F32(180.0 / np.pi)
ATAN_P = (F32(F32(0.9997878412794807) * _DEG), F32(F32(-0.3258083974640975) * _DEG),
          F32(F32(0.1555786518463281) * _DEG), F32(F32(-0.04432655554792128) * _DEG))
_EPS = F32(np.finfo(np.float64).eps)  # (float)DBL_EPSILON


def fast_atan2_deg(y: np.ndarray, x: np.ndarray) -> np.ndarray:
    """fastAtan2 in degrees, [0, 360): 7th-order polynomial in c = min/(max + eps), folded by 90-, 180-, 360-.
    Unfused: every multiply and add rounds to float32 on its own (the fused form of OpenCV's AVX2 dispatch is
    tests/emu/atan_fma_emu.cpp; test_gradient_spec.py shows it moves no 16-bin index)."""
    y = np.asarray(y, F32)
    x = np.asarray(x, F32)
    ax, ay = np.abs(x), np.abs(y)
    c = (np.minimum(ax, ay) / (np.maximum(ax, ay) + _EPS)).astype(F32)
    c2 = (c * c).astype(F32)
    p1, p3, p5, p7 = ATAN_P
    a = (p7 * c2).astype(F32)
    a = (a + p5).astype(F32)
    a = (a * c2).astype(F32)
    a = (a + p3).astype(F32)
    a = (a * c2).astype(F32)
    a = (a + p1).astype(F32)
    a = (a * c).astype(F32)
    a = np.where(ax >= ay, a, (F32(90.0) - a).astype(F32))
    a = np.where(x < 0, (F32(180.0) - a).astype(F32), a)
    a = np.where(y < 0, (F32(360.0) - a).astype(F32), a)
    return a.astype(F32)


# ---- angle.convertTo(CV_8U, 16.0 / 360.0) ---------------------------------------------------------------------------
SCALE16 = F32(16.0 / 360.0)


def convert_to_u8(angle: np.ndarray) -> np.ndarray:
    v = (angle.astype(F32) * SCALE16).astype(F32)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)  # rint: round half to even, then saturate


def orientation_bins16(dx: np.ndarray, dy: np.ndarray) -> np.ndarray:
    return convert_to_u8(fast_atan2_deg(np.asarray(dy, F32), np.asarray(dx, F32)))


# ---- colour selection / gray magnitude -----------------------------------------------------------------------------
def select_gradient(dx: np.ndarray, dy: np.ndarray, spec: Spec = SPEC):
    """Returns float32 (dx, dy, magnitude) of one level."""
    if dx.ndim == 2:  # gray (:322-330): CV_32F Sobel, magnitude = dx.mul(dx) + dy.mul(dy) in float
        fx, fy = dx.astype(F32), dy.astype(F32)
        return fx, fy, ((fx * fx).astype(F32) + (fy * fy).astype(F32)).astype(F32)
    m = dx * dx + dy * dy  # int (:366-368)
    m0, m1, m2 = m[..., 0], m[..., 1], m[..., 2]
    if spec.tie_lowest_channel:
        pick = np.where((m0 >= m1) & (m0 >= m2), 0, np.where((m1 >= m0) & (m1 >= m2), 1, 2))
    else:
        pick = np.where((m2 >= m1) & (m2 >= m0), 2, np.where((m1 >= m0) & (m1 >= m2), 1, 0))
    take = lambda a: np.take_along_axis(a, pick[..., None], axis=2)[..., 0]  # noqa: E731
    return take(dx).astype(F32), take(dy).astype(F32), take(m).astype(F32)


# ---- hysteresisGradient --------------------------------------------------------------------------------------------
def hysteresis(magnitude: np.ndarray, angle: np.ndarray, weak: float, spec: Spec = SPEC) -> np.ndarray:
    r, c = angle.shape
    q = convert_to_u8(angle)
    if spec.zero_ring:
        q[0, :] = 0
        q[r - 1, :] = 0
        q[:, 0] = 0
        q[:, c - 1] = 0
        q[1 : r - 1, 1 : c - 1] &= 7
    else:  # the misreading: the ring keeps its labels and votes with them
        q &= 7
    out = np.zeros((r, c), np.uint8)
    if r < 3 or c < 3:
        return out
    if spec.thr_square_f32:
        thr = F32(weak) * F32(weak)
        above = magnitude > thr if spec.thr_strict else magnitude >= thr
    else:
        thr = np.float64(F32(weak)) ** 2
        above = magnitude.astype(np.float64) > thr if spec.thr_strict else magnitude.astype(np.float64) >= thr
    hist = np.zeros((8, r - 2, c - 2), np.int64)
    for dr in range(3):
        for dc in range(3):
            lab = q[dr : dr + r - 2, dc : dc + c - 2].astype(np.int64)
            np.add.at(hist, (lab, *np.indices(lab.shape)), 1)
    if spec.vote_first_max:
        idx = np.argmax(hist, axis=0)
    else:
        idx = 7 - np.argmax(hist[::-1], axis=0)
    votes = np.max(hist, axis=0)
    inner = np.where(votes >= 5, (1 << idx).astype(np.uint8), np.uint8(0))
    out[1 : r - 1, 1 : c - 1] = np.where(above[1 : r - 1, 1 : c - 1], inner, 0)
    return out


def quantized_orientations(img: np.ndarray, weak: float, spec: Spec = SPEC):
    """line2Dup.cpp:313-404.  Returns (magnitude f32, quantized one-hot u8, angle f32)."""
    sm = gaussian7(img, spec)
    dx, dy = sobel3(sm)
    fx, fy, mag = select_gradient(dx, dy, spec)
    ang = fast_atan2_deg(fy, fx)
    return mag, hysteresis(mag, ang, weak, spec), ang


# ---- pyrDown / resize(INTER_NEAREST) -------------------------------------------------------------------------------
def pyr_size(rows: int, cols: int, spec: Spec = SPEC):
    if spec.pyr_size_ceil:
        return (rows + 1) // 2, (cols + 1) // 2
    return rows // 2, cols // 2


def pyrdown(img: np.ndarray, spec: Spec = SPEC) -> np.ndarray:
    """[1 4 6 4 1]^2 / 256 at even source positions, (sum + 128) >> 8, source borders by spec.pyr_border."""
    s = img.astype(np.int64)
    dr, dc = pyr_size(s.shape[0], s.shape[1], spec)
    p = _pad(s, 3, spec.pyr_border)
    # output (y, x) reads source rows 2y-2 .. 2y+2 = padded rows 2y+1 .. 2y+5 (3 pixels of pad, for the ceil variant)
    h = 0
    for t, k in enumerate(PYR5):
        h = h + k * p[:, 1 + t : 1 + t + 2 * dc : 2][:, :dc]
    v = 0
    for t, k in enumerate(PYR5):
        v = v + k * h[1 + t : 1 + t + 2 * dr : 2][:dr]
    return ((v + 128) >> 8).astype(np.uint8)


def nearest_index(dst: int, src: int) -> np.ndarray:
    """resizeNN's table: min(floor(x * (1 / (dst / src))), src - 1), in double."""
    ifx = 1.0 / (float(dst) / float(src))
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * ifx).astype(np.int64), src - 1)


def resize_nearest(mask: np.ndarray, rows: int, cols: int) -> np.ndarray:
    return mask[nearest_index(rows, mask.shape[0])][:, nearest_index(cols, mask.shape[1])]


# ---- the match path's pyramid ----------------------------------------------------------------------------------------
@dataclass
class Level:
    src: np.ndarray
    mask: Optional[np.ndarray]
    magnitude: np.ndarray
    angle: np.ndarray  # float degrees (angle_ori)
    quantized: np.ndarray  # ColorGradientPyramid::quantize: one-hot, copyTo through the mask


def build(img: np.ndarray, T_levels: Sequence[int], weak: float = 30.0, mask: Optional[np.ndarray] = None,
          spec: Spec = SPEC) -> List[Level]:
    """ColorGradientPyramid(src, mask) then pyrDown() per further level (:406-450); one Level per entry of T_levels."""
    src = np.ascontiguousarray(img, np.uint8)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    out: List[Level] = []
    for l in range(len(T_levels)):
        if l > 0:
            rows, cols = pyr_size(src.shape[0], src.shape[1], spec)
            src = pyrdown(src, spec)
            if m is not None:
                m = resize_nearest(m, rows, cols)
        mag, q, ang = quantized_orientations(src, weak, spec)
        if m is not None:
            q = np.where(m != 0, q, 0).astype(np.uint8)
        out.append(Level(src, m, mag, ang, q))
    return out


def variant(**kw) -> Spec:
    return replace(SPEC, **kw)
