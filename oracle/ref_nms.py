"""Runs the reference's own NMS (oracle/_ref/ref_nms, built by oracle/ref_nms.mk) on box lists.

TEST INFRASTRUCTURE ONLY.  The binary is oracle/ref_nms_driver.cpp compiled against the reference's nms.hpp on stand-in
headers: cv_dnn::NMSBoxes with GetMaxScoreIndex's std::stable_sort, NMSFast_'s walk under the adaptive threshold and
jaccardDistance__'s arithmetic.  It runs as a child process; one start takes any number of independent problems, each
of them one NMSBoxes call.
"""
from __future__ import annotations

import os
import struct
import subprocess
import tempfile
from typing import List, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
MAGIC = 0x4E4D4253
BOX_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("score", "<f4")])

# (boxes [[x, y, w, h], ...], scores, score_threshold, nms_threshold, eta, top_k)
Problem = Tuple[Sequence[Sequence[int]], Sequence[float], float, float, float, int]


class Refused(RuntimeError):
    """The reference itself rejected the input (a CV_Assert / CV_Error fired); the message is the reference's."""


def binary() -> str:
    return os.path.join(REF_DIR, "ref_nms")


def reference_tree_present() -> bool:
    """whether oracle/ref_nms.mk would build here: the reference tree it names (SBM_REFERENCE, else its own default) holds nms.hpp"""
    tree = os.environ.get("SBM_REFERENCE")
    if not tree:
        with open(os.path.join(_HERE, "ref_nms.mk")) as f:
            (tree,) = [l.split("?=")[1].strip() for l in f if l.startswith("SBM_REFERENCE")]
    return os.path.exists(os.path.join(tree, "nms.hpp"))


def missing_binaries() -> List[str]:
    return [] if os.access(binary(), os.X_OK) else [binary()]


def encode(problems: Sequence[Problem]) -> bytes:
    out = [struct.pack("<2i", MAGIC, len(problems))]
    for boxes, scores, score_thr, nms_thr, eta, top_k in problems:
        assert len(boxes) == len(scores)
        rec = np.zeros(len(scores), BOX_DTYPE)
        if len(scores):
            b = np.asarray(boxes, np.int64).reshape(-1, 4)
            for k, name in enumerate(("x", "y", "w", "h")):
                rec[name] = b[:, k]
            rec["score"] = np.asarray(scores, np.float32)
        out.append(struct.pack("<i3fi", len(scores), float(np.float32(score_thr)), float(np.float32(nms_thr)), float(np.float32(eta)),
                               int(top_k)))
        out.append(rec.tobytes())
    return b"".join(out)


def decode(data: bytes, n_problems: int) -> List[List[int]]:
    out, o = [], 0
    for _ in range(n_problems):
        (k,) = struct.unpack_from("<i", data, o)
        o += 4
        out.append(np.frombuffer(data, "<i4", k, o).tolist())
        o += 4 * k
    assert o == len(data)
    return out


def run_many(problems: Sequence[Problem], timeout: float = 600.0) -> List[List[int]]:
    """cv_dnn::NMSBoxes of the reference on every problem, in one start of the binary: the kept indices of each"""
    exe = binary()
    if not os.access(exe, os.X_OK):
        raise FileNotFoundError(f"{exe} is missing: run build() (oracle/ref_nms.mk) where the reference tree exists")
    d = tempfile.mkdtemp(prefix="sbm_ref_nms_")
    src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    try:
        with open(src, "wb") as f:
            f.write(encode(problems))
        p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout)
        if p.returncode == 3:
            raise Refused(p.stderr.strip())
        if p.returncode != 0:
            raise RuntimeError(f"ref_nms: exit {p.returncode}: {p.stderr}")
        with open(dst, "rb") as f:
            return decode(f.read(), len(problems))
    finally:
        for n in os.listdir(d):
            os.unlink(os.path.join(d, n))
        os.rmdir(d)


def run(boxes, scores, score_thr, nms_thr, eta=1.0, top_k=0) -> List[int]:
    """cv_dnn::NMSBoxes(boxes, scores, score_thr, nms_thr, indices, eta, top_k) of the reference: indices"""
    return run_many([(boxes, scores, score_thr, nms_thr, eta, top_k)])[0]
