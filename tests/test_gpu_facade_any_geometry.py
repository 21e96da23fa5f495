"""-m gpu: Detector::matchBatch / matchAsync on a frame whose level 1 is not 16-column-aligned (640 x 816: level 1 is
408 columns, 408 % 16 == 8).  The host batch behind them used to run such frames one per sub-batch and now runs whole
sub-batches through the batched any-stride linear-memory builder; either way every frame's list is per-frame match()'s
(checked in the demo) and frame 0's is the oracle's (checked here).  A guard: it passes before and after that change."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from shape_based_matching_amd import synth
from shape_based_matching_amd.templates import write_class_yaml
from test_gpu_facade import write_ppm

pytestmark = pytest.mark.gpu
DEMO = os.path.join(ROOT, "shape_based_matching_amd", "sbm_facade_demo")


def test_facade_batch_on_an_unaligned_level(tmp_path, oracle, case1):
    assert os.path.exists(DEMO), "facade demo not built: run __graft_entry__.build()"
    ts = case1["templates"].subset(range(280, 361, 4))
    ts.class_ids = ["test"]
    ts.template_id = np.arange(ts.n_templates, dtype=np.int32)
    fmt = str(tmp_path / "%s_templ.yaml")
    write_class_yaml(ts, fmt % "test")
    frame = synth.embed(case1["test"], 640, 816, 80, 100)
    img_path = str(tmp_path / "frame.ppm")
    write_ppm(img_path, frame)
    r = subprocess.run([DEMO, "batch", fmt, "test", img_path, "88", "128", "5", "0", "0,0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    head = lines[0].split()
    flags = dict(zip(head[1::2], head[2::2]))
    assert flags["frames"] == "5" and int(flags["matches"]) > 0
    for k in ("batch_same", "async_same", "devices_same", "devices_batch_same", "unknown_class_empty", "async_interleaved_same"):
        assert flags[k] == "1", (k, lines[0])
    got = [(int(a), int(b), int(c), d, int(e)) for a, b, c, d, e in (l.split() for l in lines[1:])]
    pyr = oracle.Pyramid.build(frame, [4, 8], 30.0)
    want = oracle.canonicalize(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, 88.0))
    pyr.free()
    keep = []
    for m in want:
        k = (int(m["x"]), int(m["y"]), int(m["similarity"].view(np.uint32)), "test")
        if keep and keep[-1][:4] == k:
            continue
        keep.append(k + (int(m["template_id"]),))
    assert got == keep and len(got) > 0
