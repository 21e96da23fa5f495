"""-m gpu: the match epilogue + NMS on the device (sbm_nms_batch_device, sbm_match_batch_host_end_nms,
Detector::matchBatchNMS).  The expected list is always computed here: raw lists -> canonical order -> the reference's
adjacent unique on (x, y, similarity, class) -> test_nms.py::py_nms over boxes (x, y, level-0 width, height) -- the
reference callers' loop (test.cpp:470-491, test_jabil.cpp:128-148).  The helpers that compute it live in tests/nms_form_cases.py,
shared with tests/test_gpu_nms_forms.py (the kernel at its edges); tests/test_reference_nms.py pins py_nms to the reference's nms.hpp."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from shape_based_matching_amd import capi, synth
from shape_based_matching_amd.templates import MATCH_DTYPE, TemplateSet, write_class_yaml
from nms_form_cases import epilogue, expected, rows_of, run_nms, sizes_of, synth_list

pytestmark = pytest.mark.gpu
DEMO = os.path.join(ROOT, "shape_based_matching_amd", "sbm_facade_demo")
REC = MATCH_DTYPE.itemsize


def case1_setup(oracle, case1, ch, n=16):
    ts = case1["templates"].subset(range(280, 361, 2))
    base = synth.embed(case1["test"], 640, 768, 80, 80)
    frames = [np.roll(base, 8 * k, axis=1) for k in range(n - 1)] + [np.zeros_like(base)]
    if ch == 1:
        frames = [np.ascontiguousarray(f[:, :, 1]) for f in frames]
    raw = []
    for fr in frames:
        pyr = oracle.Pyramid.build(fr, [4, 8], 30.0)
        raw.append(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, 80.0))
        pyr.free()
    return ts, frames, raw


@pytest.mark.parametrize("ch", [3, 1])
def test_match_batch_device_then_nms(oracle, ctx_factory, case1, ch):
    """16 frames (the scene, shifted copies, an empty frame) through sbm_match_batch_device, then the stage on the
    device lists; nms 1.0 with score -1 is the facade's match() list (the epilogue alone)"""
    import torch

    ts, frames, raw = case1_setup(oracle, case1, ch)
    assert len(raw[0]) > 0 and len(raw[-1]) == 0
    rows, cols = frames[0].shape[:2]
    B, cap = len(frames), 1024
    ctx = ctx_factory()
    ctx.upload_templates(ts)
    d_imgs = torch.from_numpy(np.stack(frames)).to("cuda:0")
    d_out = torch.zeros(B * cap * REC, dtype=torch.uint8, device="cuda:0")
    d_cnt = torch.zeros(B * 2, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    fs = rows * cols * ch
    ctx.match_batch_device(d_imgs.data_ptr(), fs, B, rows, cols, cols * ch, ch, 80.0, d_out.data_ptr(), cap, d_cnt.data_ptr())
    ctx.match_batch_device(d_imgs.data_ptr(), fs, B, rows, cols, cols * ch, ch, 80.0, d_out.data_ptr(), cap, d_cnt.data_ptr())
    sizes = sizes_of(ts)
    for score, thr in ((0.0, 0.5), (-1.0, 1.0)):
        got, oc = run_nms(ctx, d_out.data_ptr(), d_cnt.data_ptr(), cap, B, score, thr, out_cap=cap)
        for f in range(B):
            want = expected(raw[f], sizes, score, thr)
            assert oc[f, 1] == 0, (f, oc[f])
            assert rows_of(got[f]) == rows_of(want), (score, thr, f)
            if thr == 1.0:
                assert rows_of(got[f]) == rows_of(epilogue(raw[f]))
        if thr == 0.5:
            assert 0 < len(got[0]) < len(epilogue(raw[0]))
    # the host-batch sibling: the same kept lists, copied back alone
    host, counts = ctx.match_batch_host_nms(frames, 80.0, 0.0, 0.5, cap=cap, out_cap=64)
    for f in range(B):
        assert counts[f, 1] == 0 and rows_of(host[f]) == rows_of(expected(raw[f], sizes, 0.0, 0.5)), f


def test_facade_match_batch_nms_case2_classes(tmp_path, oracle, case2):
    """Detector::matchBatchNMS through the demo, two classes: every frame's kept list is test_facade_nms_flow_case2's
    expectation (oracle -> canonical -> adjacent unique -> py_nms(0, 0.5)) for that frame"""
    assert os.path.exists(DEMO)
    full = case2["templates"]
    half = full.n_templates // 2
    parts = []
    for k, (name, idx) in enumerate((("a", range(0, half)), ("b", range(half, full.n_templates)))):
        t = full.subset(list(idx))
        t.class_idx[:] = 0
        t.template_id[:] = np.arange(t.n_templates)
        t.class_ids = [name]
        write_class_yaml(t, str(tmp_path / f"{name}_templ.yaml"))
        parts.append(t)
    img = case2["test"]
    rgb = np.ascontiguousarray(img[:, :, ::-1])
    with open(str(tmp_path / "test.ppm"), "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(rgb.tobytes())
    n_frames = 4
    r = subprocess.run([DEMO, "nmsbatch", str(tmp_path / "%s_templ.yaml"), "a,b", str(tmp_path / "test.ppm"), "90", "30", str(n_frames),
                        "0", "0.5", "1", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got, cur = [], None
    for line in r.stdout.strip().splitlines():
        if line.startswith("frame "):
            cur = []
            got.append(cur)
        elif line.startswith("k "):
            v = line.split()
            cur.append((int(v[1]), int(v[2]), int(v[3]), v[4], int(v[5])))
    assert len(got) == n_frames
    frame = np.ascontiguousarray(img[: img.shape[0] // 16 * 16, : img.shape[1] // 16 * 16])
    sizes = {}
    for k, t in enumerate(parts):
        for ti in range(t.n_templates):
            sizes[(k, ti)] = (int(t.levels[ti, 0]["width"]), int(t.levels[ti, 0]["height"]))
    total_kept = 0
    for f in range(n_frames):
        fr = np.ascontiguousarray(np.roll(frame, 8 * f, axis=1))
        pyr = oracle.Pyramid.build(fr, [4, 8], 30.0)
        raw = [pyr.match(t.levels, t.features, np.full(t.n_templates, k, np.int32), t.template_id, 90.0) for k, t in enumerate(parts)]
        pyr.free()
        raw = np.concatenate([np.ascontiguousarray(x, MATCH_DTYPE) for x in raw])
        want = expected(oracle.canonicalize(raw), sizes, 0.0, 0.5)
        assert got[f] == [(int(m["x"]), int(m["y"]), int(np.float32(m["similarity"]).view(np.uint32)), "ab"[int(m["class_idx"])],
                           int(m["template_id"])) for m in want], f
        total_kept += len(want)
    assert total_kept > 0


def synth_templates(case1):
    ts = case1["templates"].subset(range(0, 60))
    ts.class_idx[:] = np.arange(ts.n_templates) % 3
    ts.template_id[:] = np.arange(ts.n_templates) // 3
    return ts


def test_synthetic_lists(ctx_factory, case1):
    """lists written straight into device buffers: ties, duplicates, same (x, y, sim, class) with other template ids,
    n = 0, 1, cap, an overflowed part (flag 0), an unknown label (flag 2), out_cap too small (flag 1), eta, top_k,
    a score threshold cutting the list"""
    import torch

    ts = synth_templates(case1)
    sizes = sizes_of(ts)
    ctx = ctx_factory()
    ctx.upload_templates(ts)
    rs = np.random.RandomState(3)
    cap = 400
    ns = [0, 1, cap, 37, 250, cap, 9, 120]
    lists, counts = [], np.zeros((len(ns), 2), np.int32)
    buf = np.zeros((len(ns), cap), MATCH_DTYPE)
    sims = np.array([90.0, 87.5, 85.0, 82.5, 80.0, 77.5], np.float32)
    for f, n in enumerate(ns):
        l = synth_list(rs, n, sizes, sims, 160 if f != 3 else 2000)
        buf[f, :n] = l
        lists.append(l)
        counts[f] = (n, 0)
    counts[5] = (cap + 17, 0)  # more matches than were stored: flag 0, the stored ones are used
    counts[6, 1] = 1           # the overflow word: flag 0
    buf[7, 5]["class_idx"] = 9  # a label no template carries: flag 2, empty box
    lists[7] = buf[7, : ns[7]].copy()
    d_recs = torch.from_numpy(buf.view(np.uint8).reshape(-1)).to("cuda:0")
    d_cnt = torch.from_numpy(counts.reshape(-1)).to("cuda:0")
    for score, thr, eta, top_k in ((-1.0, 1.0, 1.0, 0), (0.0, 0.5, 1.0, 0), (0.0, 0.5, 0.9, 0), (0.0, 0.8, 0.7, 0), (83.0, 0.5, 1.0, 0),
                                   (0.0, 0.3, 1.0, 1), (0.0, 0.5, 0.9, 20), (81.0, 0.6, 0.7, 20), (0.0, 0.0, 1.0, 0)):
        got, oc = run_nms(ctx, d_recs.data_ptr(), d_cnt.data_ptr(), cap, len(ns), score, thr, eta, top_k)
        for f in range(len(ns)):
            want = expected(lists[f], sizes, score, thr, eta, top_k)
            assert rows_of(got[f]) == rows_of(want), (score, thr, eta, top_k, f)
            assert oc[f, 0] == len(want)
            e = epilogue(lists[f])
            cands = [m for m in e if float(m["similarity"]) > score][: top_k if top_k > 0 else None]
            unknown = any((int(m["class_idx"]), int(m["template_id"])) not in sizes for m in cands)
            assert oc[f, 1] == (1 if f in (5, 6) else 0) | (4 if unknown else 0), (f, oc[f])
        assert oc[7, 1] & 4 or score >= 0
    # out_cap too small: flag 1, the first out_cap kept records stored
    got, oc = run_nms(ctx, d_recs.data_ptr(), d_cnt.data_ptr(), cap, len(ns), -1.0, 1.0, out_cap=5)
    for f in range(len(ns)):
        want = expected(lists[f], sizes, -1.0, 1.0)
        assert oc[f, 0] == len(want) and bool(oc[f, 1] & 2) == (len(want) > 5), f
        assert rows_of(got[f]) == rows_of(want[:5])


def test_global_memory_path_and_parts(ctx_factory, case1):
    """frames whose union of parts exceeds the LDS path (2048 records) take the global-memory sort and walk; the same
    lists split over two parts give the same result"""
    import torch

    ts = synth_templates(case1)
    sizes = sizes_of(ts)
    ctx = ctx_factory()
    ctx.upload_templates(ts)
    rs = np.random.RandomState(8)
    sims = np.linspace(95, 70, 40).astype(np.float32)
    cap = 3000
    ns = [3000, 1500, 2100]
    lists = [synth_list(rs, n, sizes, sims, 900) for n in ns]
    buf = np.zeros((len(ns), cap), MATCH_DTYPE)
    for f, l in enumerate(lists):
        buf[f, : len(l)] = l
    counts = np.array([[n, 0] for n in ns], np.int32)
    d_recs = torch.from_numpy(buf.view(np.uint8).reshape(-1)).to("cuda:0")
    d_cnt = torch.from_numpy(counts.reshape(-1)).to("cuda:0")
    for score, thr, eta in ((0.0, 0.5, 1.0), (75.0, 0.4, 0.9), (-1.0, 1.0, 1.0)):
        got, oc = run_nms(ctx, d_recs.data_ptr(), d_cnt.data_ptr(), cap, len(ns), score, thr, eta)
        for f in range(len(ns)):
            want = expected(lists[f], sizes, score, thr, eta)
            assert oc[f, 1] == 0 and rows_of(got[f]) == rows_of(want), (score, thr, eta, f)
    # two parts of 1600 records per frame (the gathered layout of a sharded step): the union is the list
    pc = 1600
    hdr = (len(ns) * 8 + 15) // 16 * 16  # {n, overflow} per frame, rounded up to 16 bytes
    stride = hdr + len(ns) * pc * REC
    g = np.zeros(2 * stride, np.uint8)
    for p in range(2):
        for f, l in enumerate(lists):
            part = l[p * pc: (p + 1) * pc]
            g[p * stride + 8 * f: p * stride + 8 * f + 8] = np.array([len(part), 0], np.int32).view(np.uint8)
            o = p * stride + hdr + f * pc * REC
            g[o: o + len(part) * REC] = np.ascontiguousarray(part).view(np.uint8)
    d_g = torch.from_numpy(g).to("cuda:0")
    got, oc = run_nms(ctx, d_g.data_ptr() + hdr, d_g.data_ptr(), pc, len(ns), 0.0, 0.5, 0.9, n_parts=2, part_stride=stride)
    for f in range(len(ns)):
        assert oc[f, 1] == 0 and rows_of(got[f]) == rows_of(expected(lists[f], sizes, 0.0, 0.5, 0.9)), f


def test_three_part_merge_of_template_shards(oracle, ctx_factory, case1):
    """three contexts, each an sbm_select_range shard of the templates, write their batch lists into one buffer in the
    gathered layout of sbm_match_batch_device_sharded; the stage over n_parts = 3 equals the whole template set's list
    through the same pipeline"""
    import torch

    ts, frames, raw = case1_setup(oracle, case1, 3, n=4)
    rows, cols = frames[0].shape[:2]
    B, cap = len(frames), 512
    hdr = (B * 8 + 15) // 16 * 16
    shard = hdr + B * cap * REC
    d_g = torch.zeros(3 * shard, dtype=torch.uint8, device="cuda:0")
    d_imgs = torch.from_numpy(np.stack(frames)).to("cuda:0")
    torch.cuda.synchronize()
    n = ts.n_templates
    bounds = [0, n // 3, 2 * n // 3, n]
    ctxs = []
    for p in range(3):
        c = ctx_factory()
        c.upload_templates(ts)
        c.select_range(bounds[p], bounds[p + 1] - bounds[p])
        base = d_g.data_ptr() + p * shard
        c.match_batch_device(d_imgs.data_ptr(), rows * cols * 3, B, rows, cols, cols * 3, 3, 80.0, base + hdr, cap, base)
        ctxs.append(c)
    torch.cuda.synchronize()
    sizes = sizes_of(ts)
    for score, thr in ((0.0, 0.5), (-1.0, 1.0)):
        got, oc = run_nms(ctxs[0], d_g.data_ptr() + hdr, d_g.data_ptr(), cap, B, score, thr, n_parts=3, part_stride=shard, out_cap=cap)
        for f in range(B):
            assert oc[f, 1] == 0 and rows_of(got[f]) == rows_of(expected(raw[f], sizes, score, thr)), (score, f)


def test_captured_match_and_nms_replay(oracle, ctx_factory, case1):
    """sbm_match_batch_device + sbm_nms_batch_device on one caller stream inside torch.cuda.graph, replayed on new
    frames: the kept lists equal the stream-launched calls' and the expectation"""
    import torch

    ts, frames, raw = case1_setup(oracle, case1, 3, n=8)
    rows, cols = frames[0].shape[:2]
    B, cap, out_cap = 4, 1024, 128
    fs = rows * cols * 3
    ctx = ctx_factory()
    ctx.upload_templates(ts)
    d_imgs = torch.from_numpy(np.stack(frames[:B])).to("cuda:0")
    d_out = torch.zeros(B * cap * REC, dtype=torch.uint8, device="cuda:0")
    d_cnt = torch.zeros(B * 2, dtype=torch.int32, device="cuda:0")
    d_kept = torch.zeros(B * out_cap * REC, dtype=torch.uint8, device="cuda:0")
    d_kc = torch.zeros(B * 2, dtype=torch.int32, device="cuda:0")

    def step(stream):
        ctx.match_batch_device(d_imgs.data_ptr(), fs, B, rows, cols, cols * 3, 3, 80.0, d_out.data_ptr(), cap, d_cnt.data_ptr(), stream=stream)
        ctx.nms_batch_device(d_out.data_ptr(), d_cnt.data_ptr(), cap, B, d_kept.data_ptr(), out_cap, d_kc.data_ptr(), 0.0, 0.5, 0.9, 0,
                             stream=stream)

    def read():
        kc = d_kc.cpu().numpy().reshape(-1, 2)
        k = d_kept.cpu().numpy().reshape(B, out_cap * REC)
        return [rows_of(k[f].view(MATCH_DTYPE)[: kc[f, 0]]) for f in range(B)], kc

    sizes = sizes_of(ts)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        step(s.cuda_stream)  # warm-up: tables and buffers are made outside the capture
        step(s.cuda_stream)
    s.synchronize()
    eager = read()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(torch.cuda.current_stream().cuda_stream)
    for first in (4, 0, 2):
        d_imgs.copy_(torch.from_numpy(np.stack(frames[first: first + B])))
        d_kc.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        got, kc = read()
        for f in range(B):
            assert kc[f, 1] == 0 and got[f] == rows_of(expected(raw[first + f], sizes, 0.0, 0.5, 0.9)), (first, f)
        if first == 0:
            assert (got, kc.tolist()) == (eager[0], eager[1].tolist())


def test_label_table_rules(ctx_factory, case1):
    """labels that are not unique within the upload: SBM_ERR_INVALID; a new upload rebuilds the table"""
    import torch

    ts = synth_templates(case1)
    ctx = ctx_factory()
    bad = ts.subset(range(ts.n_templates))
    bad.template_id[1] = bad.template_id[4]
    bad.class_idx[1] = bad.class_idx[4]
    ctx.upload_templates(bad)
    d = torch.zeros(1024, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(capi.SbmError) as e:
        ctx.nms_batch_device(d.data_ptr(), d.data_ptr(), 4, 1, d.data_ptr() + 512, 4, d.data_ptr() + 256, 0.0, 0.5)
    assert e.value.code == -1
    ctx.upload_templates(ts)
    torch.cuda.synchronize()
    ctx.nms_batch_device(d.data_ptr() + 64, d.data_ptr(), 4, 1, d.data_ptr() + 512, 4, d.data_ptr() + 256, 0.0, 0.5)
    torch.cuda.synchronize()
    assert d[256:264].cpu().numpy().view(np.int32).tolist() == [0, 0]
