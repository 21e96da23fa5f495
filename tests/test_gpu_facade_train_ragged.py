"""The facade over ragged training and the device scale sweep, through the demo binary: `scale_train_batch`
(shapeInfo_producer::addTemplates -> Detector::addTemplatesScaled -> sbm_train_sweep) writes what `scale_train` (the loop of
test.cpp:scale_test("train")) writes, byte for byte; `trainbatch` with a feature count per source (Detector::addTemplates ->
sbm_train_ragged) gives the ids and the YAML of the loop of addTemplate."""
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


def test_scale_train_batch_writes_what_scale_train_writes(tmp_path, golden):
    assert os.path.exists(DEMO), "facade demo not built: run __graft_entry__.build()"
    img = np.load(os.path.join(golden, "case0_circle_bgr.npz"))["bgr"]
    write_ppm(str(tmp_path / "circle.ppm"), img)
    out = {}
    for mode in ("scale_train", "scale_train_batch"):
        fmt, info = str(tmp_path / (mode + "_%s_templ.yaml")), str(tmp_path / (mode + "_info.yaml"))
        r = subprocess.run([DEMO, mode, str(tmp_path / "circle.ppm"), "150", "0.25", "1", "0.25", fmt, "circle", info], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "trained 4 templates of 4 infos" in r.stdout
        out[mode] = (open(fmt % "circle", "rb").read(), open(info, "rb").read())
    assert len(out["scale_train"][0]) > 1000 and len(out["scale_train"][1]) > 20
    assert out["scale_train_batch"][0] == out["scale_train"][0]
    assert out["scale_train_batch"][1] == out["scale_train"][1]


def test_trainbatch_with_a_count_per_source(tmp_path, oracle):
    assert os.path.exists(DEMO)
    items = [(TC.rectangle(96, 96), None, 63), (TC.rectangle(40, 40), None, 8), (TC.rectangle(64, 48), TC.cut_edge(64, 48), 16),
             (TC.rectangle(40, 40), None, 63),  # fails: too few candidates at level 1 for 31 features
             (TC.rectangle(96, 96), TC.left_half(96, 96), 8), (TC.rectangle(64, 48), None, 63)]
    args, want_ids, next_id = [], [], 0
    for k, (img, mask, nf) in enumerate(items):
        write_ppm(str(tmp_path / f"s{k}.ppm"), img)
        args.append(str(tmp_path / f"s{k}.ppm"))
        if mask is None:
            args.append("-")
        else:
            write_pgm(str(tmp_path / f"m{k}.pgm"), mask)
            args.append(str(tmp_path / f"m{k}.pgm"))
        ok = TC.want(oracle, img, mask, nf) is not None
        want_ids.append(next_id if ok else -1)
        next_id += ok
    assert want_ids.count(-1) == 1 and len({i[0].shape for i in items}) == 3
    loop_fmt, batch_fmt = str(tmp_path / "loop_%s.yaml"), str(tmp_path / "batch_%s.yaml")
    counts = "counts=" + ",".join(str(nf) for _, _, nf in items)
    r = subprocess.run([DEMO, "trainbatch", "63", loop_fmt, batch_fmt, "shapes", counts, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines() if l.startswith(("loop", "batch"))}
    assert [int(v) for v in lines["loop"]] == want_ids
    assert [int(v) for v in lines["batch"]] == want_ids
    a, b = open(loop_fmt % "shapes", "rb").read(), open(batch_fmt % "shapes", "rb").read()
    assert len(a) > 1000 and a == b


def test_scale_train_batch_over_rotations(tmp_path):
    """angles 0, 45, 90, 135, 180 at two scales: 0 and 45 are one run (no rotation), 90 and 180 runs of their own, 135 again
    none -- the run splitting, the host rotation per run and the id order of shapeInfo_producer::addTemplates, against the loop
    of addTemplate(src_of(info), mask_of(info)) on an image without a symmetry"""
    img = np.full((160, 200, 3), 20, np.uint8)
    img[30:130, 40:80] = 220
    img[100:130, 40:170] = 220
    write_ppm(str(tmp_path / "ell.ppm"), img)
    out = {}
    for mode in ("scale_train", "scale_train_batch"):
        fmt, info = str(tmp_path / (mode + "_%s_templ.yaml")), str(tmp_path / (mode + "_info.yaml"))
        r = subprocess.run([DEMO, mode, str(tmp_path / "ell.ppm"), "32", "0.5", "1", "0.5", fmt, "ell", info, "0", "180", "45"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        trained = [l for l in r.stdout.splitlines() if l.startswith("trained ")]
        assert trained and trained[0].endswith(" of 10 infos") and int(trained[0].split()[1]) >= 5, r.stdout[-500:]
        out[mode] = (open(fmt % "ell", "rb").read(), open(info, "rb").read())
    assert out["scale_train_batch"] == out["scale_train"]
    # the rotations are in it: upright and lying boxes, at two scales
    from shape_based_matching_amd.templates import read_class_yaml

    lv = read_class_yaml(str(tmp_path / "scale_train_batch_%s_templ.yaml") % "ell").levels[:, 0]
    boxes = {(int(v["width"]), int(v["height"])) for v in lv}
    assert any(w > h for w, h in boxes) and any(h > w for w, h in boxes) and len(boxes) >= 4
