"""CPU (not gpu): the arithmetic of the verify stage (shape_based_matching_amd/csrc/sbm_verify_math.h: gray, min-max
normalisation, normalised correlation, keep rule), host pass compiled here, against the numpy restatement below of the
"verify rule" of include/sbm.h -- the HCORR stage of the reference's production driver (test_jabil.cpp:152-207: cvtColor,
cv::normalize(NORM_MINMAX, 0, 255, CV_8U), TM_CCORR_NORMED on two images of one size).  The restatement is independent of
the header: np.float32 arithmetic, np.rint, Python integers for the sums, math.sqrt and double division.  The GPU tests
of the stage (test_gpu_verify_stage.py, test_gpu_verify_pipeline.py) take their expected results from it."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "verify_math_emu.cpp")


# ---- the numpy restatement --------------------------------------------------------------------------------------------
def np_gray(img):
    """rule 1: HxWx3 B, G, R -> gray; HxW as it is"""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img.copy()
    v = img.astype(np.int64)
    return ((v[..., 0] * 1868 + v[..., 1] * 9617 + v[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def np_norm_table(lo, hi):
    """rule 2: what each of the 256 gray values becomes in an image with extremes (lo, hi)"""
    if hi == lo:
        return np.zeros(256, np.uint8)
    scale = 255.0 * (1.0 / float(hi - lo))
    shift = 0.0 - float(lo) * scale
    a, b = np.float32(scale), np.float32(shift)
    t = np.arange(256).astype(np.float32) * a
    u = t + b
    assert t.dtype == np.float32 and u.dtype == np.float32
    return np.clip(np.rint(u), 0, 255).astype(np.uint8)


def np_normalise(gray):
    gray = np.asarray(gray, np.uint8)
    if gray.size == 0:
        return gray.copy()
    return np_norm_table(int(gray.min()), int(gray.max()))[gray]


def np_sums(n_roi, n_patch):
    a = [int(v) for v in np.asarray(n_roi).ravel()]
    b = [int(v) for v in np.asarray(n_patch).ravel()]
    return sum(x * y for x, y in zip(a, b)), sum(x * x for x in a), sum(y * y for y in b)


def np_score_from_sums(sab, saa, sbb):
    """rule 3"""
    den = math.sqrt(float(saa) * float(sbb))
    q = 0.0 if den == 0.0 else float(sab) / den
    return np.float32(min(q, 1.0))


def np_score(roi_gray, patch_gray):
    """the score of a gray ROI against a RAW gray patch of the same size"""
    return np_score_from_sums(*np_sums(np_normalise(roi_gray), np_normalise(patch_gray)))


def np_keeps(score, min_corr):
    """rule 4"""
    return float(np.float32(score)) >= float(min_corr)


def np_verify_frame(frame, recs, sizes, patches, min_corr, keep_unverified=False, cap=None, overflow=0, count=None, out_cap=None):
    """One frame of the stage.  frame: HxW or HxWx3 (B, G, R); recs: structured records (x, y, class_idx, template_id);
    sizes: label -> (w0, h0) of the labels that have a patch; patches: label -> raw gray patch.  count / overflow: the
    input pair (count defaults to len(recs)); only min(count, cap) records are read.  Returns (kept indices, their
    scores, every read record's score, {n_kept, flags})."""
    gray = np_gray(frame)
    rows, cols = gray.shape
    count = len(recs) if count is None else count
    cap = len(recs) if cap is None else cap
    n = min(max(count, 0), cap)
    flags = 1 if (overflow != 0 or count > cap) else 0
    kept, kept_scores, all_scores = [], [], []
    for i in range(n):
        r = recs[i]
        label = (int(r["class_idx"]), int(r["template_id"]))
        x, y = int(r["x"]), int(r["y"])
        if label not in patches:
            flags |= 4
            s, keep = np.float32(-1.0), bool(keep_unverified)
        else:
            w0, h0 = sizes[label]
            if x < 0 or y < 0 or x + w0 > cols or y + h0 > rows or w0 * h0 == 0:
                flags |= 8
                s, keep = np.float32(-1.0), bool(keep_unverified)
            else:
                s = np_score(gray[y:y + h0, x:x + w0], patches[label])
                keep = np_keeps(s, min_corr)
        all_scores.append(s)
        if keep:
            kept.append(i)
            kept_scores.append(s)
    n_kept = len(kept)
    if out_cap is not None:
        if n_kept > out_cap:
            flags |= 2
        kept, kept_scores = kept[:out_cap], kept_scores[:out_cap]
    return kept, np.asarray(kept_scores, np.float32), np.asarray(all_scores, np.float32), (n_kept, flags)


def bits(v):
    return np.asarray(v, np.float32).view(np.uint32)


# ---- the header's host pass ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("verify_emu") / "libverify_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra",
                           "-I", CSRC, "-o", so, EMU_SRC])
    L = C.CDLL(so)
    L.sbm_emu_verify_gray.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.sbm_emu_verify_gray.restype = None
    L.sbm_emu_verify_tables.argtypes = [C.c_void_p]
    L.sbm_emu_verify_tables.restype = C.c_int64
    L.sbm_emu_verify_score.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    L.sbm_emu_verify_score.restype = C.c_float
    L.sbm_emu_verify_keeps.argtypes = [C.c_float, C.c_double]
    L.sbm_emu_verify_keeps.restype = C.c_int
    L.sbm_emu_verify_inside.argtypes = [C.c_int] * 6
    L.sbm_emu_verify_inside.restype = C.c_int
    L.sbm_emu_verify_normalise.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p]
    L.sbm_emu_verify_normalise.restype = C.c_uint64
    L.sbm_emu_verify_pair.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.sbm_emu_verify_pair.restype = C.c_float
    return L


def emu_pair(emu, roi, patch):
    roi = np.ascontiguousarray(roi, np.uint8)
    patch = np.ascontiguousarray(patch, np.uint8)
    assert roi.shape == patch.shape
    scratch = np.zeros(max(roi.size, 1), np.uint8)
    return np.float32(emu.sbm_emu_verify_pair(roi.ctypes.data, patch.ctypes.data, roi.shape[1], roi.shape[0], scratch.ctypes.data))


def test_gray_random_and_corner_triples(emu):
    rs = np.random.RandomState(5)
    corners = np.array([[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)], np.uint8)
    px = np.concatenate([rs.randint(0, 256, (100000, 3)).astype(np.uint8), corners])
    out = np.zeros(len(px), np.uint8)
    emu.sbm_emu_verify_gray(px.ctypes.data, len(px), out.ctypes.data)
    assert np.array_equal(out, np_gray(px[None])[0])
    assert out[-8] == 0 and out[-1] == 255  # black and white


def test_normalise_table_every_pair(emu):
    """all 32 640 pairs lo < hi x 256 values, vectorised; the constant image last"""
    lo, hi = np.triu_indices(256, 1)  # row-major: (0,1), (0,2), ..., (254,255)
    assert len(lo) == 32640
    got = np.zeros((len(lo) + 1, 256), np.uint8)
    assert emu.sbm_emu_verify_tables(got.ctypes.data) == len(lo) + 1
    scale = 255.0 * (1.0 / (hi - lo).astype(np.float64))
    shift = 0.0 - lo.astype(np.float64) * scale
    a, b = scale.astype(np.float32), shift.astype(np.float32)
    t = np.arange(256).astype(np.float32)[None, :] * a[:, None]
    u = t + b[:, None]
    assert u.dtype == np.float32
    want = np.clip(np.rint(u), 0, 255).astype(np.uint8)
    assert np.array_equal(got[:-1], want)
    assert not got[-1].any()
    # the vectorised form is np_norm_table's
    for k in (0, 1, 254, 255, 7000, 20000, 32639):
        assert np.array_equal(want[k], np_norm_table(int(lo[k]), int(hi[k])))
    # inside an image's range the ends map to 0 and 255
    assert (want[np.arange(len(lo)), lo] == 0).all() and (want[np.arange(len(lo)), hi] == 255).all()


def test_normalise_image_and_sbb(emu):
    rs = np.random.RandomState(6)
    for h, w, pad in ((1, 1, 0), (5, 3, 2), (33, 65, 7), (40, 40, 0)):
        buf = rs.randint(0, 256, (h, w + pad)).astype(np.uint8)
        out = np.zeros((h, w), np.uint8)
        sbb = emu.sbm_emu_verify_normalise(buf.ctypes.data, w, h, w + pad, out.ctypes.data)
        want = np_normalise(buf[:, :w])
        assert np.array_equal(out, want)
        assert sbb == np_sums(want, want)[2]


def test_scores_random_pairs_bit_for_bit(emu):
    rs = np.random.RandomState(7)
    for k in range(2000):
        h, w = int(rs.randint(1, 41)), int(rs.randint(1, 41))
        roi = rs.randint(0, 256, (h, w)).astype(np.uint8)
        if k % 3 == 0:  # correlated pairs: scores near the threshold and near 1
            patch = np.clip(roi.astype(np.int32) + rs.randint(-40, 41, (h, w)), 0, 255).astype(np.uint8)
        elif k % 3 == 1:  # narrow ranges: few distinct normalised values
            lo = int(rs.randint(0, 250))
            roi = rs.randint(lo, lo + 6, (h, w)).astype(np.uint8)
            patch = rs.randint(0, 256, (h, w)).astype(np.uint8)
        else:
            patch = rs.randint(0, 256, (h, w)).astype(np.uint8)
        assert bits(emu_pair(emu, roi, patch)) == bits(np_score(roi, patch)), (k, h, w)


def test_scores_constructed_cases(emu):
    rs = np.random.RandomState(8)
    patch = rs.randint(0, 256, (9, 13)).astype(np.uint8)
    const = np.full((9, 13), 77, np.uint8)
    assert emu_pair(emu, const, patch) == 0.0 and np_score(const, patch) == 0.0  # constant ROI
    assert emu_pair(emu, patch, const) == 0.0 and np_score(patch, const) == 0.0  # constant patch
    assert emu_pair(emu, patch, patch) == 1.0 and np_score(patch, patch) == 1.0  # identical
    inv = (255 - patch).astype(np.uint8)
    assert bits(emu_pair(emu, inv, patch)) == bits(np_score(inv, patch))  # inverse: a low score, not a negative one
    assert 0.0 <= float(np_score(inv, patch)) < 0.8
    one = np.array([[200]], np.uint8)  # a single pixel is a constant image
    assert emu_pair(emu, one, one) == 0.0 and np_score(one, one) == 0.0


def test_score_from_sums_past_32_bits(emu):
    # 70 000 pixels of 255 against 255: Sab = Saa = Sbb = 255^2 * 70 000 > 2^32
    s = 255 * 255 * 70000
    assert s > 2 ** 32
    assert bits(np.float32(emu.sbm_emu_verify_score(s, s, s))) == bits(np_score_from_sums(s, s, s)) == bits(np.float32(1.0))
    rs = np.random.RandomState(9)
    for _ in range(2000):
        saa, sbb = int(rs.randint(1, 2 ** 62)), int(rs.randint(1, 2 ** 62))
        sab = int(rs.randint(0, int(math.isqrt(saa * sbb)) + 1))
        if rs.rand() < 0.5:
            saa >>= int(rs.randint(0, 50))
            sbb >>= int(rs.randint(0, 50))
            sab = min(sab, math.isqrt(saa * sbb))
        assert bits(np.float32(emu.sbm_emu_verify_score(sab, saa, sbb))) == bits(np_score_from_sums(sab, saa, sbb)), (sab, saa, sbb)
    assert emu.sbm_emu_verify_score(5, 0, 9) == 0.0 and emu.sbm_emu_verify_score(5, 9, 0) == 0.0  # den == 0
    assert emu.sbm_emu_verify_score(10, 3, 3) == 1.0  # q > 1 is 1


def test_keep_rule_and_roi_rule(emu):
    s = np.float32(0.8)  # (float)0.8 is above the double 0.8
    assert emu.sbm_emu_verify_keeps(s, 0.8) == 1 and np_keeps(s, 0.8)
    assert emu.sbm_emu_verify_keeps(s, float(s)) == 1 and np_keeps(s, float(s))
    up = math.nextafter(float(s), 2.0)
    assert emu.sbm_emu_verify_keeps(s, up) == 0 and not np_keeps(s, up)
    below = np.nextafter(np.float32(0.8), np.float32(0))
    assert emu.sbm_emu_verify_keeps(below, 0.8) == 0 and not np_keeps(below, 0.8)
    for x, y, w, h, want in ((0, 0, 128, 96, 1), (-1, 0, 4, 4, 0), (0, -1, 4, 4, 0), (125, 0, 4, 4, 0), (124, 92, 4, 4, 1), (0, 93, 4, 4, 0),
                             (3, 3, 0, 4, 0), (3, 3, 4, 0, 0)):
        assert emu.sbm_emu_verify_inside(x, y, w, h, 96, 128) == want, (x, y, w, h)
