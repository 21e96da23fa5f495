"""Detector::addTemplates_rotate against the loop of Detector::addTemplate_rotate, through the facade demo: the `train_rot`
mode (one addTemplates_rotate call, the rotations on the device) writes byte for byte the class YAML and the info file
that the `train` mode (the reference's loop, test.cpp:303-313) writes, and prints the same line."""
import os
import subprocess

import numpy as np
import pytest

import train_batch_cases as TC
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEMO = os.path.join(ROOT, "shape_based_matching_amd", "sbm_facade_demo")


def write_ppm(path, bgr):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (bgr.shape[1], bgr.shape[0]))
        f.write(np.ascontiguousarray(bgr[:, :, ::-1]).tobytes())


def write_pgm(path, g):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (g.shape[1], g.shape[0]))
        f.write(np.ascontiguousarray(g).tobytes())


def both_modes(tmp_path, img, mask, num_features, n_rot, angle_step):
    assert os.path.exists(DEMO), "facade demo not built: run __graft_entry__.build()"
    write_ppm(str(tmp_path / "src.ppm"), img)
    write_pgm(str(tmp_path / "mask.pgm"), mask)
    out = {}
    for mode in ("train", "train_rot"):
        fmt, info = str(tmp_path / (mode + "_%s.yaml")), str(tmp_path / (mode + "_info.yaml"))
        r = subprocess.run([DEMO, mode, str(tmp_path / "src.ppm"), str(tmp_path / "mask.pgm"), str(num_features), str(n_rot), str(angle_step), fmt, "shape",
                            info], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out[mode] = (open(fmt % "shape", "rb").read(), open(info, "rb").read(), r.stdout)
    return out


def test_case1_family_of_360(tmp_path, case1):
    padded, mask = TC.fixture_roi(case1)
    out = both_modes(tmp_path, padded, mask, 128, 360, 1)
    assert out["train"][2] == "trained 361 templates\n"
    assert len(out["train"][0]) > 100000 and len(out["train"][1]) > 1000
    assert out["train_rot"] == out["train"]


def test_rectangle_family_of_5(tmp_path):
    img = TC.rectangle(96, 96)
    out = both_modes(tmp_path, img, np.full((96, 96), 255, np.uint8), 63, 5, 72.5)
    assert out["train"][2].endswith("trained 6 templates\n")  # behind addTemplate's notes on the candidates it found
    assert len(out["train"][0]) > 1000
    assert out["train_rot"] == out["train"]
