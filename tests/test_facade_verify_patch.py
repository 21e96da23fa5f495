"""CPU (not gpu): Detector::verifyPatch (shape_based_matching_amd/facade/line2Dup_verify_patch.h), the fiducial patch of a
template as the reference's production driver makes it (test_jabil.cpp:187-191 with rotateScaleImage, utils.cpp:157-187):
resize by sscale unless it is 1, rotate by the integer orientation's quarter turns, crop Rect(tl_x, tl_y, width, height).
tests/emu/verify_patch_driver.cpp is compiled here with facade/cvlite.cpp alone (the helper is header-only: no engine
symbol is needed); the expectation is numpy's (np.rot90, and the 2 x 2 box mean an exact half-size INTER_LINEAR resize is)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FACADE = os.path.join(ROOT, "shape_based_matching_amd", "facade")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("verify_patch") / "driver")
    subprocess.check_call([cxx, "-std=c++14", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I", FACADE, "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "verify_patch_driver.cpp"), os.path.join(FACADE, "cvlite.cpp"), "-lz"])
    return exe


def image(rows, cols, kind):
    r, c = np.mgrid[0:rows, 0:cols]
    return ((2 * c + r) if kind == 0 else ((r * 37 + c * 101 + (r * c) % 13) & 255)).astype(np.uint8)


def patch(driver, rows, cols, kind, sscale, orientation, tl_x, tl_y, w, h):
    out = subprocess.run([driver] + [str(v) for v in (rows, cols, kind, sscale, orientation, tl_x, tl_y, w, h)], capture_output=True, text=True,
                         check=True).stdout.split("\n")
    pr, pc = (int(v) for v in out[0].split())
    if pr == 0 or pc == 0:
        return None
    p = np.array([list(bytes.fromhex(l)) for l in out[1:1 + pr]], np.uint8)
    assert p.shape == (pr, pc)
    return p


ROWS, COLS = 30, 44


def test_identity(driver):
    img = image(ROWS, COLS, 1)
    assert np.array_equal(patch(driver, ROWS, COLS, 1, 1.0, 0.0, 5, 7, 20, 11), img[7:18, 5:25])
    # an orientation that is no quarter turn leaves the image as it is (rotateScaleImage returns)
    assert np.array_equal(patch(driver, ROWS, COLS, 1, 1.0, 45.0, 5, 7, 20, 11), img[7:18, 5:25])
    assert np.array_equal(patch(driver, ROWS, COLS, 1, 1.0, 90.9, 0, 0, 30, 44), np.rot90(img, -1))  # (int)90.9 == 90


@pytest.mark.parametrize("angles, k", [((90, -270), -1), ((180, -180), 2), ((270, -90), 1)])
def test_quarter_turns_both_spellings(driver, angles, k):
    """90 / -270 clockwise, 180 / -180 half a turn, 270 / -90 counter-clockwise (np.rot90 turns counter-clockwise)"""
    img = image(ROWS, COLS, 1)
    turned = np.rot90(img, k)
    for a in angles:
        whole = patch(driver, ROWS, COLS, 1, 1.0, float(a), 0, 0, turned.shape[1], turned.shape[0])
        assert np.array_equal(whole, turned), a
        assert np.array_equal(patch(driver, ROWS, COLS, 1, 1.0, float(a), 3, 4, 9, 13), turned[4:17, 3:12]), a


def test_half_scale_ramp(driver):
    """sscale 0.5 on a 64 x 48 ramp: every output pixel is the rounded mean of its 2 x 2 block (cv::resize INTER_LINEAR at an
    exact half: weights 1/2, 1/2 in both passes)"""
    img = image(48, 64, 0).astype(np.int32)
    half = ((img[0::2, 0::2] + img[0::2, 1::2] + img[1::2, 0::2] + img[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    assert half.shape == (24, 32)
    assert np.array_equal(patch(driver, 48, 64, 0, 0.5, 0.0, 0, 0, 32, 24), half)
    assert np.array_equal(patch(driver, 48, 64, 0, 0.5, 0.0, 10, 3, 7, 5), half[3:8, 10:17])
    # scale, then turn, then crop
    assert np.array_equal(patch(driver, 48, 64, 0, 0.5, 90.0, 2, 1, 20, 30), np.rot90(half, -1)[1:31, 2:22])


def test_crop_at_each_edge_and_one_pixel_outside(driver):
    img = image(ROWS, COLS, 1)
    w, h = 10, 8
    for x, y in ((0, 11), (COLS - w, 11), (17, 0), (17, ROWS - h), (COLS - w, ROWS - h)):
        assert np.array_equal(patch(driver, ROWS, COLS, 1, 1.0, 0.0, x, y, w, h), img[y:y + h, x:x + w]), (x, y)
    for x, y in ((-1, 11), (COLS - w + 1, 11), (17, -1), (17, ROWS - h + 1)):
        assert patch(driver, ROWS, COLS, 1, 1.0, 0.0, x, y, w, h) is None, (x, y)
    # after a quarter turn the image is 30 wide and 44 high: the same crop fits or not by the turned size
    assert patch(driver, ROWS, COLS, 1, 1.0, 90.0, ROWS - w, COLS - h, w, h) is not None
    assert patch(driver, ROWS, COLS, 1, 1.0, 90.0, ROWS - w + 1, 0, w, h) is None
    assert patch(driver, ROWS, COLS, 1, 1.0, 0.0, 0, 0, 0, 5) is None  # an empty template
