"""-m gpu: the three stages of the reference's production driver (test_jabil.cpp:121-312: MATCH, NMS, HCORR) chained on the
device -- sbm_match_batch_device -> sbm_nms_batch_device -> sbm_verify_batch_device with no host step between --, through
sbm_match_batch_host_verified, and through Detector::matchBatchVerified (the demo's `verify` mode).  The scene is the
case1 setup of tests/test_gpu_nms_device.py, restated here: 640 x 768, 41 templates, 15 shifted copies of the scene and an
empty frame.  Expected: the CPU checker's raw lists -> epilogue + py_nms (nms_form_cases.expected) -> the numpy restatement
of the verify rule (test_verify_math.np_verify_frame).

Patches: a template that matches on frame 0 gets the gray of frame 0 at its top match there (correlation 1 wherever the
object is), except that every second such template's patch is cut 37 columns and 23 rows off that place (correlations
around 0.8, on either side of it); a template that does not match there gets a constant patch (correlation 0).  With
NMSBoxes(0, 0.5), the reference's setting, one match per frame survives NMS and verifies; with the epilogue alone
(-1, 1.0) six do and the stage keeps some and drops some."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from shape_based_matching_amd import synth
from shape_based_matching_amd.templates import MATCH_DTYPE, write_class_yaml
from nms_form_cases import epilogue, expected, rows_of, sizes_of
from test_verify_math import bits, np_gray, np_verify_frame

pytestmark = pytest.mark.gpu
DEMO = os.path.join(ROOT, "shape_based_matching_amd", "sbm_facade_demo")
REC = MATCH_DTYPE.itemsize
ROWS, COLS, B, THR = 640, 768, 16, 80.0
NMS_SETTINGS = ((0.0, 0.5), (-1.0, 1.0))


@pytest.fixture(scope="module")
def scene(oracle, case1):
    ts = case1["templates"].subset(range(280, 361, 2))
    ts.template_id[:] = np.arange(ts.n_templates)  # (a class file numbers its pyramids from 0)
    base = synth.embed(case1["test"], ROWS, COLS, 80, 80)
    frames = [np.roll(base, 8 * k, axis=1) for k in range(B - 1)] + [np.zeros_like(base)]
    raw = []
    for fr in frames:
        pyr = oracle.Pyramid.build(fr, [4, 8], 30.0)
        raw.append(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, THR))
        pyr.free()
    sizes = sizes_of(ts)
    g0, e0 = np_gray(frames[0]), epilogue(raw[0])
    patches, matched = {}, 0
    for lab, (w, h) in sizes.items():
        top = [m for m in e0 if (int(m["class_idx"]), int(m["template_id"])) == lab]
        p = None
        if top:
            off = (37, 23) if matched % 2 else (0, 0)
            x, y = int(top[0]["x"]) + off[0], int(top[0]["y"]) + off[1]
            if x >= 0 and y >= 0 and x + w <= COLS and y + h <= ROWS:
                p = g0[y:y + h, x:x + w].copy()
                matched += 1
        patches[lab] = p if p is not None else np.full((h, w), 128, np.uint8)
    assert matched >= 4 and ts.n_templates == 41
    want = {}
    for prm in NMS_SETTINGS:
        want[prm] = []
        for f in range(B):
            kept = expected(raw[f], sizes, *prm)
            idx, ks, alls, pair = np_verify_frame(frames[f], kept, sizes, patches, 0.8)
            want[prm].append((kept[idx] if idx else np.zeros(0, MATCH_DTYPE), ks, pair, len(kept)))
    # the scene gives both outcomes, before anything runs on the device
    for prm in NMS_SETTINGS:
        assert want[prm][0][2][0] >= 1 and want[prm][B - 1][2] == (0, 0) and all(w[2][1] == 0 for w in want[prm])
    assert any(w[2][0] < w[3] for w in want[(-1.0, 1.0)]) and want[(-1.0, 1.0)][0][2][0] < want[(-1.0, 1.0)][0][3]
    return dict(ts=ts, frames=frames, raw=raw, sizes=sizes, patches=patches, want=want)


def check_frames(got_recs, got_scores, got_counts, want):
    for f, (recs, ks, pair, _) in enumerate(want):
        assert tuple(int(v) for v in got_counts[f]) == pair, (f, got_counts[f], pair)
        assert rows_of(got_recs[f]) == rows_of(recs), f
        assert np.array_equal(bits(got_scores[f]), bits(ks)), (f, got_scores[f], ks)


def test_device_chain_match_nms_verify(ctx_factory, scene):
    import torch

    ctx = ctx_factory()
    ctx.upload_templates(scene["ts"])
    ctx.upload_verify_patches([(c, t, p) for (c, t), p in scene["patches"].items()])
    cap, ncap, out_cap = 1024, 128, 32
    d_imgs = torch.from_numpy(np.stack(scene["frames"])).to("cuda:0")
    d_raw = torch.zeros(B * cap * REC, dtype=torch.uint8, device="cuda:0")
    d_rawc = torch.zeros(B * 2, dtype=torch.int32, device="cuda:0")
    d_nms = torch.zeros(B * ncap * REC, dtype=torch.uint8, device="cuda:0")
    d_nmsc = torch.zeros(B * 2, dtype=torch.int32, device="cuda:0")
    d_out = torch.zeros(B * out_cap * REC, dtype=torch.uint8, device="cuda:0")
    d_sc = torch.zeros(B * out_cap, dtype=torch.float32, device="cuda:0")
    d_oc = torch.zeros(B * 2, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    fs = ROWS * COLS * 3
    for prm in NMS_SETTINGS:
        d_oc.fill_(-1)
        torch.cuda.synchronize()
        # three enqueues on the context's stream, nothing between them
        ctx.match_batch_device(d_imgs.data_ptr(), fs, B, ROWS, COLS, COLS * 3, 3, THR, d_raw.data_ptr(), cap, d_rawc.data_ptr())
        ctx.nms_batch_device(d_raw.data_ptr(), d_rawc.data_ptr(), cap, B, d_nms.data_ptr(), ncap, d_nmsc.data_ptr(), prm[0], prm[1])
        ctx.verify_batch_device(d_imgs.data_ptr(), fs, B, ROWS, COLS, COLS * 3, 3, d_nms.data_ptr(), d_nmsc.data_ptr(), ncap, 0.8,
                                d_out.data_ptr(), d_sc.data_ptr(), out_cap, d_oc.data_ptr())
        torch.cuda.synchronize()
        oc = d_oc.cpu().numpy().reshape(-1, 2)
        out = d_out.cpu().numpy().reshape(B, out_cap * REC)
        sc = d_sc.cpu().numpy().reshape(B, out_cap)
        check_frames([out[f].view(MATCH_DTYPE)[: oc[f, 0]] for f in range(B)], [sc[f, : oc[f, 0]] for f in range(B)], oc, scene["want"][prm])
        assert [int(v) for v in d_nmsc.cpu().numpy().reshape(-1, 2)[:, 0]] == [w[3] for w in scene["want"][prm]]


def test_match_batch_host_verified(ctx_factory, scene):
    ctx = ctx_factory()
    ctx.upload_templates(scene["ts"])
    ctx.upload_verify_patches([(c, t, p) for (c, t), p in scene["patches"].items()])
    for prm in NMS_SETTINGS:
        recs, scores, counts = ctx.match_batch_host_verified(scene["frames"], THR, prm[0], prm[1], 0.8, cap=1024, out_cap=16)
        check_frames(recs, scores, counts, scene["want"][prm])
    # min_corr 0 keeps what NMS kept
    recs, scores, counts = ctx.match_batch_host_verified(scene["frames"], THR, -1.0, 1.0, 0.0, cap=1024, out_cap=16)
    assert [int(c) for c in counts[:, 0]] == [w[3] for w in scene["want"][(-1.0, 1.0)]]


def write_pgm(path, g):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (g.shape[1], g.shape[0]))
        f.write(np.ascontiguousarray(g).tobytes())


def test_facade_match_batch_verified_through_the_demo(tmp_path, scene):
    """Detector::setFiducials + matchBatchVerified: the class file names one fiducial image per template (scale 1,
    orientation 0), in which the template's patch lies at (tl_x, tl_y) -- where Detector::verifyPatch crops it"""
    assert os.path.exists(DEMO)
    ts = scene["ts"]
    t = ts.subset(range(ts.n_templates))
    t.class_ids = ["c1"]
    n = t.n_templates
    srcs = []
    for k in range(n):
        lv = t.levels[k, 0]
        p = scene["patches"][(int(t.class_idx[k]), int(t.template_id[k]))]
        canvas = np.full((int(lv["tl_y"]) + p.shape[0] + 3, int(lv["tl_x"]) + p.shape[1] + 2), 9, np.uint8)
        canvas[int(lv["tl_y"]): int(lv["tl_y"]) + p.shape[0], int(lv["tl_x"]): int(lv["tl_x"]) + p.shape[1]] = p
        path = str(tmp_path / f"fid_{k}.pgm")
        write_pgm(path, canvas)
        srcs.append([path] * t.n_levels)
    t.meta = {"scale": np.ones((n, t.n_levels), np.float32), "orientation": np.zeros((n, t.n_levels), np.float32),
              "tagFieldID": np.zeros((n, t.n_levels), np.int32), "fiducial_src": srcs}
    write_class_yaml(t, str(tmp_path / "c1_templ.yaml"))
    rgb = np.ascontiguousarray(scene["frames"][0][:, :, ::-1])
    with open(str(tmp_path / "test.ppm"), "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(rgb.tobytes())
    prm = (-1.0, 1.0)
    r = subprocess.run([DEMO, "verify", str(tmp_path / "%s_templ.yaml"), "c1", str(tmp_path / "test.ppm"), str(THR), "30", str(B), str(prm[0]),
                        str(prm[1]), "1", "0", "0.8", "0", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got, cur = [], None
    for line in r.stdout.strip().splitlines():
        if line.startswith("frame "):
            cur = []
            got.append(cur)
        elif line.startswith("v "):
            v = line.split()
            cur.append((int(v[1]), int(v[2]), int(v[3]), v[4], int(v[5]), int(v[6])))
    assert len(got) == B
    for f, (recs, ks, pair, _) in enumerate(scene["want"][prm]):
        assert got[f] == [(int(m["x"]), int(m["y"]), int(np.float32(m["similarity"]).view(np.uint32)), "c1", int(m["template_id"]), int(bits(s)))
                          for m, s in zip(recs, ks)], f
