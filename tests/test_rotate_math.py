"""The scalar rule of batched template rotation (csrc/sbm_rotate_math.h), walked in the kernel's two passes on the CPU
(tests/emu/train_rotate_emu.cpp: the workgroup's threads as a loop) against the oracle's add_template_rotate -- level
records and features bit for bit, theta included.  The case1 base at the reference's own 360 angles, hand-made bases on
the rule's edges (train_rotate_cases.py), every status code, and the bound of the wrap loops.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import train_batch_cases as TC
import train_rotate_cases as RC
from conftest import ROOT

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "train_rotate_emu.cpp")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("train_rotate_emu") / "libtrain_rotate_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so, EMU_SRC])
    L = C.CDLL(so)
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    L.sbm_emu_train_rotate.argtypes = [vp, vp, vp, i32, f32, f32, f32, C.c_int64, vp, vp, vp]
    L.sbm_emu_train_rotate.restype = None
    L.sbm_emu_rotate_theta_ok.argtypes = [f32]
    L.sbm_emu_rotate_center_ok.argtypes = [f32]
    L.sbm_emu_rotate_angle.argtypes = [f32, vp, vp]
    L.sbm_emu_rotate_angle.restype = None
    return L


def emu_rotate(emu, base, theta, center, base_status=None, cap=None):
    """(levels, feats[:cap], status pair) of one pair from the emulation"""
    from oracle.oracle import LEVEL_DTYPE, TRAIN_FEATURE_DTYPE

    levels, feats = np.ascontiguousarray(base[0], LEVEL_DTYPE), np.ascontiguousarray(base[1], TRAIN_FEATURE_DTYPE)
    cap = int(levels["n_features"].clip(0).sum()) if cap is None else cap
    out_l = np.full(len(levels), -7, LEVEL_DTYPE)
    out_f = np.zeros(max(cap, 1), TRAIN_FEATURE_DTYPE)
    status = np.full(2, -7, np.int32)
    st = None if base_status is None else np.ascontiguousarray(base_status, np.int32)
    emu.sbm_emu_train_rotate(levels.ctypes.data, feats.ctypes.data if len(feats) else None, None if st is None else st.ctypes.data, len(levels),
                             center[0], center[1], theta, cap, out_l.ctypes.data, out_f.ctypes.data, status.ctypes.data)
    return out_l, out_f[:cap], (int(status[0]), int(status[1]))


def check_pair(emu, oracle, base, theta, center):
    levels, feats, status = emu_rotate(emu, base, theta, center)
    n = int(base[0]["n_features"].sum())
    assert status == (0, n), (theta, center, status)
    assert RC.same_pair((levels, feats), RC.want(oracle, base, theta, center)), (theta, center)


def test_case1_at_the_reference_angles(emu, oracle, case1):
    """test.cpp:303-313: the trained ROI of train.png rotated by 1 .. 360 degrees about the padded image's centre; the
    oracle at these angles is pinned to the reference's own YAML by test_oracle_pins.py"""
    padded, mask = TC.fixture_roi(case1)
    base = TC.want(oracle, padded, mask, 128)
    assert TC.counts(base) == (131, 71)
    for t in range(1, 361):
        check_pair(emu, oracle, base, float(t), (235.0, 235.0))


@pytest.mark.parametrize("case", RC.cpu_cases() + RC.count_cases(), ids=lambda c: c[0])
def test_edges(emu, oracle, case):
    _, base, center, thetas = case
    for theta in thetas:
        check_pair(emu, oracle, base, theta, center)


def test_the_negative_cases_are_negative(oracle):
    """what the cases are there for: an odd negative minimum stays odd (min % 2 == 1 does not fire for it)"""
    want = {c[0]: RC.want(oracle, c[1], c[3][0], c[2])[0] for c in RC.negative_cases()}
    assert (int(want["neg_x_only"][0]["tl_x"]), int(want["neg_x_only"][0]["tl_y"])) == (-7, 34)
    assert (int(want["neg_y_only"][0]["tl_x"]), int(want["neg_y_only"][0]["tl_y"])) == (34, -7)
    assert (int(want["neg_both"][0]["tl_x"]), int(want["neg_both"][0]["tl_y"])) == (-7, -7)
    assert int(want["neg_both"][1]["tl_x"]) == -7 >> 1


def test_the_tie_cases_tie(oracle):
    """a quarter turn about (10.5, 7) puts level-0 x coordinates on k + 0.5 before the rounding"""
    name, base, center, thetas = RC.tie_cases()[0]
    levels, feats = base
    y_abs = feats["y"][: int(levels[0]["n_features"])] + int(levels[0]["tl_y"])
    assert center == (10.5, 7.0) and 90.0 in thetas
    assert np.all(((y_abs - 7.0) + 10.5) % 1 == 0.5)


def test_angle_table_and_domain(emu):
    for theta in RC.ANGLES + [1.0, 45.0, 359.0]:
        cs, sn = C.c_double(0), C.c_double(0)
        emu.sbm_emu_rotate_angle(theta, C.byref(cs), C.byref(sn))
        ang = float(np.float32(-np.float32(theta)) / np.float32(180)) * 3.1415926535897932384626433832795
        assert (cs.value, sn.value) == (np.cos(ang), np.sin(ang)), theta
    ok = [0.0, -0.0, 36000.0, -36000.0, 1e-30]
    bad = [float("inf"), float("-inf"), float("nan"), float(np.nextafter(np.float32(36000), np.float32(1e9))), -36001.0, 1e9]
    assert all(emu.sbm_emu_rotate_theta_ok(t) == 1 for t in ok) and all(emu.sbm_emu_rotate_theta_ok(t) == 0 for t in bad)
    ok = [0.0, 65536.0, -65536.0, 235.0]
    bad = [float("inf"), float("nan"), float(np.nextafter(np.float32(65536), np.float32(1e9))), -1e6]
    assert all(emu.sbm_emu_rotate_center_ok(t) == 1 for t in ok) and all(emu.sbm_emu_rotate_center_ok(t) == 0 for t in bad)


def test_wrap_steps_cover_the_domain(emu):
    """|f.theta - theta| <= 36720 needs at most 102 subtractions of 360; the bound is one above"""
    assert emu.sbm_emu_rotate_wrap_steps() == 103
    for start in (np.float32(36720.0), np.float32(-36720.0)):
        t, steps = start, 0
        while t > 360:
            t, steps = np.float32(t - np.float32(360)), steps + 1
        while t < 0:
            t, steps = np.float32(t + np.float32(360)), steps + 1
        assert steps <= 102


@pytest.mark.parametrize("theta", [float("inf"), float("-inf"), float("nan"), 1e9, -1e9, 720.5, -721.0])
def test_feature_outside_the_domain_is_status_3(emu, theta):
    """a feature theta the wrap loops would spin on (or never leave) ends the pair with {3, 3}; the call returns"""
    levels, feats = RC.random_base((70, 9), 7)
    feats["theta"][68] = theta
    out_l, _, status = emu_rotate(emu, (levels, feats), 10.0, (50.0, 50.0))
    assert status == (3, 3)
    assert not out_l.tobytes().strip(b"\0")


def test_coordinate_outside_the_domain_is_status_3(emu):
    """feature + tl outside 0 .. 32767, by one on either side and where the int sum would overflow"""
    for field, tl, absolute in (("x", "tl_x", 32768), ("y", "tl_y", -1), ("x", "tl_x", None), ("y", "tl_y", None)):
        levels, feats = RC.random_base((5, 300), 8)
        feats[field][304] = 2 ** 31 - 1 if absolute is None else absolute - int(levels[1][tl])  # feature 304: the last of level 1
        assert emu_rotate(emu, (levels, feats), 10.0, (50.0, 50.0))[2] == (3, 3), (field, absolute)
    levels, feats = RC.base_from_points([[(32767, 32767, 1.0), (0, 0, 2.0)]])
    assert emu_rotate(emu, (levels, feats), 10.0, (50.0, 50.0))[2] == (0, 2)


def test_status_codes(emu, oracle):
    base = RC.random_base((20, 6), 9)
    n = 26
    want = RC.want(oracle, base, 30.0, (9.0, 9.0))
    for st in (None, (0, n), (0, 0)):
        levels, feats, status = emu_rotate(emu, base, 30.0, (9.0, 9.0), base_status=st)
        assert status == (0, n) and RC.same_pair((levels, feats), want)
    assert emu_rotate(emu, base, 30.0, (9.0, 9.0), cap=n - 1)[2] == (2, n)
    assert emu_rotate(emu, base, 30.0, (9.0, 9.0), base_status=(1, 1))[2] == (1, 1)
    assert emu_rotate(emu, base, 30.0, (9.0, 9.0), base_status=(1, 0))[2] == (1, 0)
    assert emu_rotate(emu, base, 30.0, (9.0, 9.0), base_status=(2, 99))[2] == (3, 1)
    empty = (base[0].copy(), base[1])
    empty[0]["n_features"] = 0
    assert emu_rotate(emu, empty, 30.0, (9.0, 9.0))[2] == (3, 2)
    for bad in (-1, 8192):
        lv = base[0].copy()
        lv["n_features"][1] = bad
        assert emu_rotate(emu, (lv, base[1]), 30.0, (9.0, 9.0), cap=10000)[2] == (3, 2)
    for st, cap in (((1, 1), n), (None, n - 1), ((2, 5), n)):  # the level records of a pair that is not ok are zeroed
        assert not emu_rotate(emu, base, 30.0, (9.0, 9.0), base_status=st, cap=cap)[0].tobytes().strip(b"\0")
