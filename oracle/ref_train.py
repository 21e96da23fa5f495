"""Runs the reference's own training half (oracle/_ref/ref_train, built by oracle/ref_train.mk) on gradient planes.

TEST INFRASTRUCTURE ONLY.  The binary is the reference's line2Dup.cpp compiled on stand-in headers with
oracle/ref_train_driver.cpp appended: ColorGradientPyramid::extractTemplate per level (selectScatteredFeatures and the
std::stable_sort included), then cropTemplates, in the order of Detector::addTemplate's loop.  It runs as a child process,
one call per template; no gradient arithmetic runs in it -- the planes of every level are the caller's.
"""
from __future__ import annotations

import os
import struct
import subprocess
import tempfile
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
MAGIC = 0x544D4253
LEVEL_FIELDS = ("width", "height", "tl_x", "tl_y", "pyramid_level", "n_features")

LEVEL_DTYPE = np.dtype(
    [("width", "<i4"), ("height", "<i4"), ("tl_x", "<i4"), ("tl_y", "<i4"), ("pyramid_level", "<i4"),
     ("n_features", "<i4"), ("feature_offset", "<i8")]
)
TRAIN_FEATURE_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("label", "<i4"), ("theta", "<f4")])


class Refused(RuntimeError):
    """The reference itself rejected the input (a CV_Assert / CV_Error fired); the message is the reference's."""


class Failed:
    """Detector::addTemplate returned -1: extractTemplate failed at pyramid level ``level``"""

    def __init__(self, level: int):
        self.level = level

    def __repr__(self):
        return f"Failed(level={self.level})"

    def __eq__(self, other):
        return isinstance(other, Failed) and other.level == self.level


def binary() -> str:
    return os.path.join(REF_DIR, "ref_train")


def missing_binaries() -> List[str]:
    return [] if os.access(binary(), os.X_OK) else [binary()]


Planes = Tuple[np.ndarray, np.ndarray, np.ndarray, Optional[np.ndarray]]


def encode(levels: Sequence[Planes], num_features: int, strong: float) -> bytes:
    """The driver's input file: per level (magnitude f32, one-hot angle u8, angle_ori f32, mask u8 or None)."""
    out = [struct.pack("<3if", MAGIC, len(levels), int(num_features), float(np.float32(strong)))]
    for mag, ang, ori, mask in levels:
        rows, cols = mag.shape
        assert ang.shape == (rows, cols) and ori.shape == (rows, cols) and (mask is None or mask.shape == (rows, cols))
        out.append(struct.pack("<3i", rows, cols, 0 if mask is None else 1))
        out.append(np.ascontiguousarray(mag, "<f4").tobytes())
        out.append(np.ascontiguousarray(ang, np.uint8).tobytes())
        out.append(np.ascontiguousarray(ori, "<f4").tobytes())
        if mask is not None:
            out.append(np.ascontiguousarray(mask, np.uint8).tobytes())
    return b"".join(out)


def decode(data: bytes, n_levels: int):
    """(levels, feats) in the oracle's dtypes (feature_offset: level l's features directly behind level l-1's), or
    Failed(level)"""
    (failed,) = struct.unpack_from("<i", data, 0)
    o = 4
    if failed >= 0:
        assert o == len(data)
        return Failed(failed)
    levels = np.zeros(n_levels, LEVEL_DTYPE)
    feats = []
    used = 0
    for l in range(n_levels):
        rec = struct.unpack_from("<6i", data, o)
        o += 24
        for k, v in zip(LEVEL_FIELDS, rec):
            levels[l][k] = v
        levels[l]["feature_offset"] = used
        n = rec[5]
        feats.append(np.frombuffer(data, TRAIN_FEATURE_DTYPE, n, o).copy())
        o += n * TRAIN_FEATURE_DTYPE.itemsize
        used += n
    assert o == len(data)
    return levels, np.concatenate(feats) if feats else np.zeros(0, TRAIN_FEATURE_DTYPE)


def run(levels: Sequence[Planes], num_features: int, strong: float, timeout: float = 600.0):
    """Detector::addTemplate's level loop on the given planes: (levels, feats) or Failed(level)."""
    exe = binary()
    if not os.access(exe, os.X_OK):
        raise FileNotFoundError(f"{exe} is missing: run build() (oracle/ref_train.mk) where the reference tree exists")
    d = tempfile.mkdtemp(prefix="sbm_ref_train_")
    src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    try:
        with open(src, "wb") as f:
            f.write(encode(levels, num_features, strong))
        p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout)
        if p.returncode == 3:
            raise Refused(p.stderr.strip())
        if p.returncode != 0:
            raise RuntimeError(f"ref_train: exit {p.returncode}: {p.stderr}")
        with open(dst, "rb") as f:
            return decode(f.read(), len(levels))
    finally:
        for n in os.listdir(d):
            os.unlink(os.path.join(d, n))
        os.rmdir(d)


def planes_of(oracle, img: np.ndarray, mask: Optional[np.ndarray], n_levels: int, weak: float, nearest) -> List[Planes]:
    """The oracle's gradient planes of the oracle's pyramid images, level by level, with the mask pyramid made by
    ``nearest`` (a function halving a mask, e.g. tests/train_batch_cases.nearest_mask) -- the reference binary's input
    for the image ``oracle.add_template`` would be given."""
    out = []
    cur = np.ascontiguousarray(img, np.uint8)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    for l in range(n_levels):
        if l > 0:
            cur = oracle.pyrdown(cur)
            if m is not None:
                m = nearest(m)
        mag, ang, ori = oracle.quantized_orientations(cur, weak)
        out.append((mag, ang, ori, m))
    return out
