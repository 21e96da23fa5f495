"""Runs the reference's own match half (oracle/_ref/ref_match_<variant>, built by oracle/ref_match.mk) on quantized maps.

TEST INFRASTRUCTURE ONLY.  The binary is the reference's line2Dup.cpp compiled on stand-in headers with
oracle/ref_match_driver.cpp appended; it runs as a child process, one call per query, and the results come back in
the dtypes the tests already use (MATCH_DTYPE records, u8 linear memories, u16 similarity maps).
"""
from __future__ import annotations

import os
import struct
import subprocess
import tempfile
from typing import List, Sequence, Tuple

import numpy as np

from shape_based_matching_amd.templates import MATCH_DTYPE, TemplateSet

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
VARIANTS = ("scalar", "sse42", "avx2")
_CPU_FLAG = {"scalar": None, "sse42": "sse4_2", "avx2": "avx2"}
MAGIC = 0x524D4253


class Refused(RuntimeError):
    """The reference itself rejected the input (a CV_Assert / CV_Error fired); the message is the reference's."""


def binary(variant: str) -> str:
    return os.path.join(REF_DIR, "ref_match_" + variant)


def _cpu_flags() -> set:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("flags"):
                    return set(line.split(":", 1)[1].split())
    except OSError:
        pass
    return set()


def runnable_variants() -> List[str]:
    """The variants this host's CPU can execute (scalar always; SSE4.2 / AVX2 where /proc/cpuinfo lists them)."""
    flags = _cpu_flags()
    return [v for v in VARIANTS if _CPU_FLAG[v] is None or _CPU_FLAG[v] in flags]


def missing_binaries(variants: Sequence[str] = VARIANTS) -> List[str]:
    return [binary(v) for v in variants if not os.access(binary(v), os.X_OK)]


def encode(qs: Sequence[np.ndarray], T: Sequence[int], classes: Sequence[TemplateSet]) -> bytes:
    """The driver's input file: maps per level, then each TemplateSet as one class (all of its templates, in order)."""
    assert len(qs) == len(T)
    out = [struct.pack("<2i", MAGIC, len(T)), np.asarray(T, "<i4").tobytes()]
    for q in qs:
        q = np.ascontiguousarray(q, np.uint8)
        out.append(struct.pack("<2i", *q.shape))
        out.append(q.tobytes())
    out.append(struct.pack("<i", len(classes)))
    for ts in classes:
        assert ts.n_levels == len(T)
        out.append(struct.pack("<i", ts.n_templates))
        for t in range(ts.n_templates):
            for l in range(ts.n_levels):
                lv = ts.levels[t, l]
                f = ts.feats_of(t, l)
                out.append(struct.pack("<6i", int(lv["width"]), int(lv["height"]), int(lv["tl_x"]), int(lv["tl_y"]),
                                       int(lv["pyramid_level"]), len(f)))
                out.append(np.stack([f["x"], f["y"], f["label"]], axis=1).astype("<i4").tobytes())
    return b"".join(out)


def dense_ids(ts: TemplateSet) -> TemplateSet:
    """``ts`` with template_id renumbered 0, 1, .. inside each class, as the reference numbers a class's templates
    (a subset keeps the ids of the full set)"""
    out = ts.subset(range(ts.n_templates))
    for c in np.unique(out.class_idx):
        idx = np.nonzero(out.class_idx == c)[0]
        out.template_id[idx] = np.arange(len(idx), dtype=np.int32)
    return out


def split_classes(ts: TemplateSet) -> List[TemplateSet]:
    """One TemplateSet per class index 0..max, each keeping the template order of ``ts``.  The reference's template_id
    is the index inside its class, so ``ts.template_id`` must count 0, 1, .. within each class."""
    n = int(ts.class_idx.max()) + 1 if ts.n_templates else 0
    out = []
    for c in range(n):
        idx = np.nonzero(ts.class_idx == c)[0]
        assert np.array_equal(ts.template_id[idx], np.arange(len(idx))), "template_id must be the index in its class"
        out.append(ts.subset(idx))
    return out


class Reference:
    """One input (maps + templates) for the reference driver; each query runs the binary once."""

    def __init__(self, qs: Sequence[np.ndarray], T: Sequence[int], ts, variant: str = "avx2", timeout: float = 600.0):
        self.T = list(T)
        self.variant = variant
        self.timeout = timeout
        classes = split_classes(ts) if isinstance(ts, TemplateSet) else list(ts)
        self._dir = tempfile.mkdtemp(prefix="sbm_ref_")
        self._in = os.path.join(self._dir, "in.bin")
        with open(self._in, "wb") as f:
            f.write(encode(qs, T, classes))

    def close(self):
        for n in os.listdir(self._dir):
            os.unlink(os.path.join(self._dir, n))
        os.rmdir(self._dir)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _run(self, *args) -> bytes:
        exe = binary(self.variant)
        if not os.access(exe, os.X_OK):
            raise FileNotFoundError(f"{exe} is missing: run build() (oracle/ref_match.mk) where the reference tree exists")
        out = os.path.join(self._dir, "out.bin")
        p = subprocess.run([exe, self._in, out] + [str(a) for a in args], capture_output=True, text=True,
                           timeout=self.timeout)
        if p.returncode == 3:
            raise Refused(p.stderr.strip())
        if p.returncode != 0:
            raise RuntimeError(f"{os.path.basename(exe)} {' '.join(map(str, args))}: exit {p.returncode}: {p.stderr}")
        with open(out, "rb") as f:
            data = f.read()
        os.unlink(out)
        return data

    def lm(self) -> List[np.ndarray]:
        """Per level, the [8][T*T*W*H] linear memories (orientation-major, then the T*T grid rows)."""
        d = self._run("lm")
        out, o = [], 0
        for _ in self.T:
            T, n = struct.unpack_from("<2i", d, o)
            o += 8
            out.append(np.frombuffer(d, np.uint8, 8 * T * T * n, o).reshape(8, T * T * n).copy())
            o += 8 * T * T * n
        assert o == len(d)
        return out

    def similarity(self, class_idx: int, t: int, level: int = -1) -> Tuple[np.ndarray, int]:
        """(H x W u16 map, 64 or 16 for the similarity_64 / similarity path)"""
        d = self._run("sim", class_idx, t, level)
        H, W, path = struct.unpack_from("<3i", d, 0)
        return np.frombuffer(d, "<u2", H * W, 12).reshape(H, W).copy(), path

    def similarity_local(self, level: int, class_idx: int, t: int, cx: int, cy: int) -> Tuple[np.ndarray, int]:
        d = self._run("local", level, class_idx, t, cx, cy)
        (path,) = struct.unpack_from("<i", d, 0)
        return np.frombuffer(d, "<u2", 256, 4).reshape(16, 16).copy(), path

    def match(self, threshold: float) -> Tuple[np.ndarray, np.ndarray]:
        """(raw matchClass list over every class, list after match()'s std::sort + std::unique), MATCH_DTYPE with
        raw = -1 (the reference keeps no raw score)"""
        d = self._run("match", float(np.float32(threshold)).hex())
        lists, o = [], 0
        for _ in range(2):
            (n,) = struct.unpack_from("<i", d, o)
            o += 4
            rec = np.frombuffer(d, np.dtype([("x", "<i4"), ("y", "<i4"), ("similarity", "<f4"), ("class_idx", "<i4"),
                                             ("template_id", "<i4")]), n, o)
            o += 20 * n
            m = np.zeros(n, MATCH_DTYPE)
            for k in ("x", "y", "similarity", "class_idx", "template_id"):
                m[k] = rec[k]
            m["raw"] = -1
            lists.append(m)
        assert o == len(d)
        return lists[0], lists[1]


def match_key(recs: np.ndarray) -> List[tuple]:
    """sorted (x, y, similarity bits, class_idx, template_id): the raw list as a multiset, raw score left out"""
    r = np.ascontiguousarray(recs, MATCH_DTYPE)
    return sorted(zip(r["x"].tolist(), r["y"].tolist(), r["similarity"].view(np.uint32).tolist(),
                      r["class_idx"].tolist(), r["template_id"].tolist()))


def epilogue_key(recs: np.ndarray) -> List[tuple]:
    """sorted distinct (x, y, similarity bits, class_idx): what survives match()'s std::unique"""
    r = np.ascontiguousarray(recs, MATCH_DTYPE)
    return sorted(set(zip(r["x"].tolist(), r["y"].tolist(), r["similarity"].view(np.uint32).tolist(),
                          r["class_idx"].tolist())))
