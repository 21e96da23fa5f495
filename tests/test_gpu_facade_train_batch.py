"""Detector::addTemplates against a loop of Detector::addTemplate, through the facade demo's `trainbatch` mode: sources of two
sizes, with and without masks, one failing image; the returned ids equal the loop's and the two writeClasses outputs are
byte-identical."""
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


def test_add_templates_equals_the_loop(tmp_path, oracle):
    assert os.path.exists(DEMO), "facade demo not built: run __graft_entry__.build()"
    items = [(TC.rectangle(96, 96), None), (TC.rectangle(64, 64), TC.cut_edge(64, 64)), (TC.rectangle(96, 96), TC.left_half(96, 96)),
             (TC.rectangle(64, 64), TC.left_half(64, 64)),  # fails
             (TC.noise(64, 64, 5), None), (TC.rectangle(96, 96), TC.cut_edge(96, 96)), (np.ascontiguousarray(TC.rectangle(64, 64)[:, ::-1]), None)]
    args, want_ids, next_id = [], [], 0
    for k, (img, mask) in enumerate(items):
        write_ppm(str(tmp_path / f"s{k}.ppm"), img)
        args.append(str(tmp_path / f"s{k}.ppm"))
        if mask is None:
            args.append("-")
        else:
            write_pgm(str(tmp_path / f"m{k}.pgm"), mask)
            args.append(str(tmp_path / f"m{k}.pgm"))
        ok = TC.want(oracle, img, mask, 63) is not None
        want_ids.append(next_id if ok else -1)
        next_id += ok
    assert want_ids.count(-1) == 1
    loop_fmt, batch_fmt = str(tmp_path / "loop_%s.yaml"), str(tmp_path / "batch_%s.yaml")
    r = subprocess.run([DEMO, "trainbatch", "63", loop_fmt, batch_fmt, "shapes", *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines() if l.startswith(("loop", "batch"))}
    assert [int(v) for v in lines["loop"]] == want_ids
    assert [int(v) for v in lines["batch"]] == want_ids
    a, b = open(loop_fmt % "shapes", "rb").read(), open(batch_fmt % "shapes", "rb").read()
    assert len(a) > 1000 and a == b
