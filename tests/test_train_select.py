"""The scalar pieces of batched template training (csrc/sbm_train_math.h: candidate order, distance predicate, pass control
of the selection, tie resolution, crop arithmetic), walked in the kernels' dataflow on the CPU (tests/emu/train_select_emu.cpp:
64 lanes as loops) against the oracle's add_template -- levels and features bit for bit, None where the oracle fails.
Input per level: the oracle's quantized_orientations of the oracle's pyrdown, the nearest-neighbour mask restated in numpy.
No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import train_batch_cases as TC
from conftest import ROOT

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "train_select_emu.cpp")
INT_MIN = -2 ** 31


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("train_select_emu") / "libtrain_select_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so, EMU_SRC])
    L = C.CDLL(so)
    vp, i32 = C.c_void_p, C.c_int32
    L.sbm_emu_train_image.argtypes = [i32, vp, vp, vp, vp, vp, vp, i32, C.c_float, vp, vp, C.c_int64]
    L.sbm_emu_train_image.restype = i32
    return L


def emu_train(emu, oracle, img, mask, num_features, strong=TC.STRONG, cap=None):
    """(levels, feats) | None | ("capacity",) from the emulation, fed per level by the oracle's gradient stage"""
    planes, masks, rows, cols = [], [], [], []
    cur, m = np.ascontiguousarray(img), None if mask is None else np.ascontiguousarray(mask)
    for l in range(TC.N_LEVELS):
        if l:
            cur = oracle.pyrdown(cur)
            m = None if m is None else TC.nearest_mask(m)
        mag, ang, ori = oracle.quantized_orientations(cur, TC.WEAK)
        planes.append((mag, ang, ori))
        masks.append(m)
        rows.append(cur.shape[0])
        cols.append(cur.shape[1])
    L = TC.N_LEVELS
    ptrs = lambda arrs: (C.c_void_p * L)(*[None if a is None else a.ctypes.data for a in arrs])  # noqa: E731
    cap = sum(r * c for r, c in zip(rows, cols)) if cap is None else cap
    lv = np.zeros((L, 6), np.int32)
    ft = np.zeros((max(cap, 1), 4), np.int32)
    r_, c_ = np.array(rows, np.int32), np.array(cols, np.int32)
    n = emu.sbm_emu_train_image(L, ptrs([p[0] for p in planes]), ptrs([p[1] for p in planes]), ptrs([p[2] for p in planes]),
                                None if mask is None else ptrs(masks), r_.ctypes.data, c_.ctypes.data, num_features, C.c_float(strong),
                                lv.ctypes.data, ft.ctypes.data, cap)
    assert n != INT_MIN + 1, "more candidates than the bound the scratch is sized from"
    if n == INT_MIN:
        return ("capacity",)
    if n < 0:
        return None
    from oracle.oracle import LEVEL_DTYPE, TRAIN_FEATURE_DTYPE
    levels = np.zeros(L, LEVEL_DTYPE)
    for i, k in enumerate(("width", "height", "tl_x", "tl_y", "pyramid_level", "n_features")):
        levels[k] = lv[:, i]
    levels["feature_offset"] = np.concatenate([[0], np.cumsum(lv[:-1, 5])])
    feats = np.zeros(n, TRAIN_FEATURE_DTYPE)
    feats["x"], feats["y"], feats["label"] = ft[:n, 0], ft[:n, 1], ft[:n, 2]
    feats["theta"] = ft[:n, 3].view(np.float32)
    return levels, feats


RECTS = [(96, 96), (64, 64), (50, 70)]
COUNTS = {  # (rows, cols, num_features) -> features at levels 0 / 1, without a mask
    (96, 96, 16): (27, 11), (96, 96, 63): (56, 20), (96, 96, 128): (56, 20),
    (50, 70, 16): (30, 8), (50, 70, 63): (30, 8), (50, 70, 128): (30, 8),
    (64, 64, 16): (32, 8), (64, 64, 63): (32, 8), (64, 64, 128): (32, 8),
}


@pytest.mark.parametrize("rows,cols", RECTS)
@pytest.mark.parametrize("nf", [16, 63, 128])
def test_plateaus(emu, oracle, rows, cols, nf):
    """long plateaus of equal squared magnitude: the tie chain is the normal case; more kept than asked (27 for 16) and the
    exhaustive mode (fewer candidates than asked)"""
    img = TC.rectangle(rows, cols)
    assert TC.s_pairs(oracle.quantized_orientations(img, TC.WEAK)[0]) >= 100
    want = TC.want(oracle, img, None, nf)
    assert want is not None and tuple(int(v) for v in want[0]["n_features"]) == COUNTS[(rows, cols, nf)]
    assert TC.same_template(emu_train(emu, oracle, img, None, nf), want)


@pytest.mark.parametrize("mask_of", [None, lambda r, c: np.full((r, c), 255, np.uint8), TC.left_half, TC.cut_edge], ids=["none", "all", "left", "cut"])
def test_masks(emu, oracle, mask_of):
    img = TC.rectangle(96, 96)
    mask = None if mask_of is None else mask_of(96, 96)
    want = TC.want(oracle, img, mask, 63)
    assert want is not None
    if mask_of is TC.left_half:
        assert tuple(int(v) for v in want[0]["n_features"]) == (28, 9)
    if mask_of is TC.cut_edge:
        assert not TC.same_template(want, TC.want(oracle, img, None, 63)), "the mask cuts nothing"
    assert TC.same_template(emu_train(emu, oracle, img, mask, 63), want)


def test_failures(emu, oracle):
    for img, mask in ((TC.rectangle(50, 70), TC.left_half(50, 70)), (TC.rectangle(64, 64), TC.left_half(64, 64)), (TC.constant(64, 64), None)):
        assert TC.want(oracle, img, mask, 63) is None
        assert emu_train(emu, oracle, img, mask, 63) is None


def test_many_candidates(emu, oracle):
    """uniform noise at strong_threshold 10: more candidates at level 0 than one selection chunk (one wave) holds"""
    img = TC.noise(64, 64, 139)
    assert int(TC.want(oracle, img, None, 100000, strong=10.0)[0]["n_features"][0]) > 64
    for nf in (16, 63, 128, 100000):
        want = TC.want(oracle, img, None, nf, strong=10.0)
        assert want is not None
        assert TC.same_template(emu_train(emu, oracle, img, None, nf, strong=10.0), want)


def test_hundreds_of_candidates(emu, oracle):
    """256 x 256 noise at strong_threshold 10: about a thousand candidates, many selection chunks"""
    img = TC.noise(256, 256, 1)
    for nf in (63, 100000):
        want = TC.want(oracle, img, None, nf, strong=10.0)
        assert want is not None and (nf == 63 or int(want[0]["n_features"][0]) > 512)
        assert TC.same_template(emu_train(emu, oracle, img, None, nf, strong=10.0), want)


def test_reference_roi(emu, oracle, case1):
    img, mask = TC.fixture_roi(case1)
    want = TC.want(oracle, img, mask, 128)
    assert want is not None
    assert TC.same_template(emu_train(emu, oracle, img, mask, 128), want)


def test_capacity(emu, oracle):
    img = TC.rectangle(96, 96)
    total = int(TC.want(oracle, img, None, 63)[0]["n_features"].sum())
    assert emu_train(emu, oracle, img, None, 63, cap=total - 1) == ("capacity",)
    assert TC.same_template(emu_train(emu, oracle, img, None, 63, cap=total), TC.want(oracle, img, None, 63))
