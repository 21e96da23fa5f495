"""CPU (not gpu): the arithmetic of the device NMS stage (shape_based_matching_amd/csrc/sbm_nms_math.h: overlap, adaptive
threshold, in-chunk greedy resolution), host pass compiled here, against test_nms.py::py_nms -- the Python restatement
of include/nms.hpp (cv_dnn::NMSBoxes, the step after Detector::match in test.cpp:491 / test_jabil.cpp:148).  py_nms and the
overlap's bit patterns are pinned to the reference's own nms.hpp (oracle/_ref/ref_nms) by tests/test_reference_nms.py."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_nms import py_nms

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "nms_math_emu.cpp")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("nms_emu") / "libnms_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra",
                           "-I", CSRC, "-o", so, EMU_SRC])
    L = C.CDLL(so)
    L.sbm_emu_nms_overlap.argtypes = [C.c_void_p, C.c_void_p]
    L.sbm_emu_nms_overlap.restype = C.c_float
    L.sbm_emu_nms_walk.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p]
    L.sbm_emu_nms_walk.restype = C.c_int
    return L


def py_overlap(a, b):
    """py_nms's overlap, restated (nms.hpp rectOverlap)"""
    aa, ab = a[2] * a[3], b[2] * b[3]
    if aa + ab <= 0:
        return np.float32(1.0)
    x1, y1 = max(a[0], b[0]), max(a[1], b[1])
    x2, y2 = min(a[0] + a[2], b[0] + b[2]), min(a[1] + a[3], b[1] + b[3])
    inter = 0.0 if (x2 <= x1 or y2 <= y1) else float((x2 - x1) * (y2 - y1))
    return np.float32(1.0) - np.float32(1.0 - inter / (aa + ab - inter))


def emu_overlap(emu, a, b):
    A = np.asarray(a, np.int32)
    B = np.asarray(b, np.int32)
    return np.float32(emu.sbm_emu_nms_overlap(A.ctypes.data, B.ctypes.data))


def bits(v):
    return np.float32(v).view(np.uint32)


def test_overlap_exhaustive_small_boxes(emu):
    """every pair of boxes with x, y in 0..2 and w, h in 0..3: disjoint, touching, nested, identical, zero-area"""
    boxes = list(itertools.product(range(3), range(3), range(4), range(4)))
    for a in boxes:
        for b in boxes:
            assert bits(emu_overlap(emu, a, b)) == bits(py_overlap(a, b)), (a, b)


def test_overlap_random_boxes_and_py_nms_decision(emu):
    rs = np.random.RandomState(11)
    for _ in range(4000):
        a = [int(rs.randint(-50, 400)), int(rs.randint(-50, 400)), int(rs.randint(0, 300)), int(rs.randint(0, 300))]
        if rs.rand() < 0.3:  # near copies: large overlaps, off-by-one edges
            b = [a[0] + int(rs.randint(-3, 4)), a[1] + int(rs.randint(-3, 4)), a[2] + int(rs.randint(-2, 3)), a[3] + int(rs.randint(-2, 3))]
            b[2], b[3] = max(b[2], 0), max(b[3], 0)
        else:
            b = [int(rs.randint(-50, 400)), int(rs.randint(-50, 400)), int(rs.randint(0, 300)), int(rs.randint(0, 300))]
        o = emu_overlap(emu, a, b)
        assert bits(o) == bits(py_overlap(a, b)), (a, b)
        # the bit pattern is the one py_nms decides on: b survives at threshold o, not at the next float below
        assert py_nms([a, b], [2.0, 1.0], 0.0, float(o)) == [0, 1]
        assert py_nms([a, b], [2.0, 1.0], 0.0, float(np.nextafter(o, np.float32(-1)))) == [0], (a, b, o)


def test_touching_nested_identical(emu):
    cases = [((0, 0, 10, 10), (10, 0, 10, 10), 0.0), ((0, 0, 10, 10), (0, 0, 10, 10), 1.0), ((0, 0, 10, 10), (2, 2, 5, 5), 0.25),
             ((0, 0, 0, 0), (5, 5, 0, 0), 1.0), ((0, 0, 0, 7), (0, 0, 4, 4), 0.0)]
    for a, b, want in cases:
        assert emu_overlap(emu, a, b) == np.float32(want), (a, b)


def _walk(emu, boxes, thr, eta):
    b = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
    keep = np.zeros(len(b) + 1, np.int32)
    k = emu.sbm_emu_nms_walk(b.ctypes.data, len(b), C.c_float(thr), C.c_float(eta), keep.ctypes.data)
    return keep[:k].tolist()


@pytest.mark.parametrize("eta", [1.0, 0.9, 0.7])
@pytest.mark.parametrize("thr", [0.0, 0.3, 0.5, 0.7, 1.0, -0.25])
def test_chunked_walk_equals_py_nms(emu, thr, eta):
    """the chunked greedy walk (64-candidate chunks, in-chunk resolution by nms_resolve_chunk) keeps what the
    sequential walk keeps, the adaptive threshold (eta < 1) included, across chunk borders"""
    rs = np.random.RandomState(int(thr * 100) + int(eta * 10) + 100)
    for n, spread in ((1, 100), (5, 100), (63, 50), (64, 50), (65, 50), (200, 80), (300, 400), (700, 150)):
        boxes = np.stack([rs.randint(0, spread, n), rs.randint(0, spread, n), rs.randint(1, 60, n), rs.randint(1, 60, n)], axis=1)
        boxes[::13, 2] = 0  # empty boxes
        scores = np.linspace(100, 1, n).astype(np.float32)  # walk order = index order
        want = py_nms(boxes.tolist(), scores.tolist(), 0.0, thr, eta, 0)
        assert _walk(emu, boxes, thr, eta) == want, (n, spread)
