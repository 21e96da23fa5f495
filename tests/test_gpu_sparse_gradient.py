"""-m gpu: level 0's gradient stage made only where the flagged refinement tiles' strip builders read its map
(BuildPlan::sparse_gradient: the source pass and the sparse pass of csrc/sbm_quantize_stream.h, ensure_level0_map).

A match entry point on a two-level pyramid whose level-0 launch takes the streaming kernel, without mask or bands, runs
    source pass L0 -> gradient L1 -> linear memories L1 -> coarse -> mark tiles -> gradient L0 (flagged items) -> strips -> refinement
and must give the oracle's lists whatever an earlier call left in the map; a later reader of level 0's map gets the whole map of
every frame of the batch, rebuilt from the retained source.  Frames: the case1 image on 512 x 640 and 512 x 512 canvases (4 x 5
and 4 x 4 tiles; 640 columns are two full strips and one of 160, 512 two and a packed one of 32), 3 frames per call, the streaming
kernel forced (it is not chosen below 4 Mpixel per launch) with 18 and with 32 rows per work item.  How many gradient launches a
call made is read from the "k_quantize" timings: 3 for a sparse two-level call, one per level for a whole build."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

from shape_based_matching_amd import capi, synth
from shape_based_matching_amd.synth import templates_from_maps
from shape_based_matching_amd.templates import MATCH_DTYPE, TemplateSet

pytestmark = pytest.mark.gpu
NT = min(16, os.cpu_count() or 1)
ROWS, THR, CAP = 512, 65.0, 8192
SPARSE_ON = os.environ.get("SBM_SPARSE_GRADIENT", "1") != "0" and os.environ.get("SBM_SPARSE_STRIPS", "1") != "0"


def multiset(recs):
    return sorted(np.ascontiguousarray(recs, MATCH_DTYPE).tolist())


def shifted(frame, dy, dx):
    out = np.zeros_like(frame)
    src = frame[max(0, -dy): frame.shape[0] - max(0, dy), max(0, -dx): frame.shape[1] - max(0, dx)]
    out[max(0, dy): max(0, dy) + src.shape[0], max(0, dx): max(0, dx) + src.shape[1]] = src
    return out


def load_templates():
    return TemplateSet.load_npz(os.path.join(GOLDEN, "case1_templates.npz")).subset(range(0, 360, 6))


def make_frames(cols):
    """object at the centre, against the right / bottom border, absent, and the centre frame moved left"""
    img = np.load(os.path.join(GOLDEN, "case1_test_bgr.npz"))["bgr"]
    wide = max(cols, img.shape[1])  # the image is 600 columns wide: the 512-column canvas is cut out of it
    centre = synth.embed(img, ROWS, wide, (ROWS - img.shape[0]) // 2, (wide - img.shape[1]) // 2)
    centre = np.ascontiguousarray(centre[:, (wide - cols) // 2: (wide - cols) // 2 + cols])
    return {"centre": centre, "border": shifted(centre, 30, 36), "absent": synth.scene_bgr(5, ROWS, cols), "left": shifted(centre, 0, -16)}


def batch_lists(ctx, frames, thr=THR, calls=1, mask=None):
    """sbm_match_batch_device (or _masked, one mask per frame) on the stacked frames, `calls` times: the last call's lists"""
    import torch

    dev = torch.device("cuda", 0)
    B = len(frames)
    rows, cols = frames[0].shape[:2]
    ch = 1 if frames[0].ndim == 2 else 3
    d_img = torch.from_numpy(np.stack(frames)).to(dev)
    d_mask = None if mask is None else torch.from_numpy(np.stack([mask] * B)).to(dev)
    d_out = torch.zeros(B * CAP * MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(B * 2, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    out = None
    for _ in range(calls):
        if mask is None:
            ctx.match_batch_device(d_img.data_ptr(), frames[0].size, B, rows, cols, cols * ch, ch, thr, d_out.data_ptr(), CAP, d_cnt.data_ptr(),
                                   stream=st.cuda_stream)
        else:
            ctx.match_batch_device_masked(d_img.data_ptr(), frames[0].size, B, rows, cols, cols * ch, ch, d_mask.data_ptr(), rows * cols, thr,
                                          d_out.data_ptr(), CAP, d_cnt.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        cnt = d_cnt.cpu().numpy().reshape(B, 2)
        recs = d_out.cpu().numpy().view(MATCH_DTYPE).reshape(B, CAP)
        assert (cnt[:, 1] == 0).all() and (cnt[:, 0] <= CAP).all(), cnt
        lists = [multiset(recs[b, : cnt[b, 0]]) for b in range(B)]
        assert out is None or out == lists  # a replay gives what the capture gave
        out = lists
    return out


def gradient_launches(ctx):
    return sum(1 for n, _ in ctx.timings() if n == "k_quantize")


def whole_gradient_child(cols):
    """the child process (SBM_SPARSE_GRADIENT=0): the same frames with level 0's whole gradient in front of the coarse pass"""
    fr = make_frames(int(cols))
    ctx = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0)
    ctx.upload_templates(load_templates())
    ctx.set_quantize_mode("stream", 18)
    ctx.set_profiling(True)
    lists = batch_lists(ctx, [fr["centre"], fr["border"], fr["absent"]], calls=2)
    n = gradient_launches(ctx)
    ctx.close()
    print("LISTS " + json.dumps({"lists": lists, "launches": n}))


@pytest.fixture(scope="module")
def world(oracle):
    """per canvas width: the frames, the oracle's pyramids and lists -- computed once, read by every test"""
    ts = load_templates()
    w = {"ts": ts}
    for cols in (640, 512):
        frames = make_frames(cols)
        want, pyrs = {}, {}
        for name, f in frames.items():
            p = oracle.Pyramid.build(f, [4, 8], 30.0)
            want[name] = multiset(p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, THR, n_threads=NT))
            pyrs[name] = p
        assert len(want["centre"]) > 20 and len(want["border"]) > 20 and want["border"] != want["centre"], cols
        w[cols] = {"frames": frames, "want": want, "pyr": pyrs}
    yield w
    for cols in (640, 512):
        for p in w[cols]["pyr"].values():
            p.free()


@pytest.fixture()
def ctx(world):
    made = []

    def make(hs=18, ts=None, T=(4, 8), **kw):
        c = capi.Context(T=T, weak_threshold=30.0, device_id=0, **kw)
        c.upload_templates(world["ts"] if ts is None else ts)
        c.set_quantize_mode("stream", hs)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


NAMES = ["centre", "border", "absent"]


@pytest.mark.parametrize("cols,hs", [(640, 18), (640, 32), (512, 18), (512, 32)])
def test_placements(world, ctx, cols, hs):
    """object at the centre, at the border and absent, one call; the call made three gradient launches"""
    w = world[cols]
    c = ctx(hs)
    batch_lists(c, [w["frames"][n] for n in NAMES])  # the first call also prepares the template tables
    c.set_profiling(True)
    got = batch_lists(c, [w["frames"][n] for n in NAMES])
    for n, g in zip(NAMES, got):
        assert g == w["want"][n], (cols, hs, n)
    if SPARSE_ON:
        assert gradient_launches(c) == 3
        seq = [n for n, _ in c.timings() if n not in ("k_resize_mask", "k_prep_features")]
        assert seq == ["k_quantize", "k_quantize", "k_build_lm", "k_similarity_coarse", "k_mark_refine_tiles", "k_quantize", "k_build_lm",
                       "k_similarity_local"], seq


@pytest.mark.parametrize("cols", [640, 512])
def test_alternating_batches_on_a_poisoned_map(world, ctx, cols):
    """one context, two batches in turn; between the calls frame 0's map is replaced through the stage setter by a map of
    valid orientation bytes that match nothing right: what a call does not rebuild must not be read"""
    w = world[cols]
    c = ctx(18)
    rs = np.random.RandomState(3)
    poison = (1 << rs.randint(0, 8, (ROWS, cols))).astype(np.uint8)
    batches = [NAMES, ["absent", "left", "centre"]]
    for call in range(4):
        names = batches[call & 1]
        got = batch_lists(c, [w["frames"][n] for n in names])
        for n, g in zip(names, got):
            assert g == w["want"][n], (call, n)
        c.set_quantized(0, poison)


def test_later_readers_get_the_whole_map(world, ctx):
    """after a sparse call the getters and the template loop see every frame's whole level 0, in both orders, and the next
    batch call is sparse again"""
    w = world[640]
    names = ["border", "centre", "absent"]
    fr = [w["frames"][n] for n in names]
    p0 = w["pyr"][names[0]]
    c = ctx(18)
    got = batch_lists(c, fr)
    assert got == [w["want"][n] for n in names]
    for b, name in reversed(list(enumerate(names))):
        for l in range(2):
            assert np.array_equal(c.get_quantized_frame(l, b), w["pyr"][name].quantized(l)), (l, b)
    for l in range(2):
        n = (ROWS >> l) * (640 >> l)
        assert np.array_equal(c.get_linear_memories(l)[:, :n], p0.lm(l)[:, :n]), l
    assert multiset(c.match_templates(THR)) == got[0]
    # the other order: the template loop first, then the planes and the maps
    c2 = ctx(32)
    assert batch_lists(c2, fr) == got
    assert multiset(c2.match_templates(THR)) == got[0]
    assert np.array_equal(c2.get_linear_memories(0)[:, : ROWS * 640], p0.lm(0)[:, : ROWS * 640])
    assert np.array_equal(c2.get_quantized(0), p0.quantized(0))
    assert np.array_equal(c2.get_quantized_frame(0, 2), w["pyr"][names[2]].quantized(0))
    c2.set_profiling(True)
    assert batch_lists(c2, fr) == got
    if SPARSE_ON:
        assert gradient_launches(c2) == 3


def test_graph_replay_and_the_whole_gradient_in_a_child(world, ctx):
    """graph replay at pipeline depth 2: one graph over three calls, the oracle's lists; a child process with
    SBM_SPARSE_GRADIENT=0 gives the same lists from two gradient launches per call"""
    w = world[640]
    fr = [w["frames"][n] for n in NAMES]
    c = ctx(18)
    c.set_pipeline_depth(2)
    c.set_graph_mode(True)
    replayed = batch_lists(c, fr, calls=3)
    assert c.graph_count() == 1
    assert replayed == [w["want"][n] for n in NAMES]
    # a reader between replays: the replayed call is recorded as sparse, so the map is completed for it
    assert np.array_equal(c.get_quantized_frame(0, 1), w["pyr"]["border"].quantized(0))
    assert batch_lists(c, fr, calls=1) == replayed
    env = dict(os.environ, SBM_SPARSE_GRADIENT="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    out = subprocess.run([sys.executable, "-c", "import test_gpu_sparse_gradient as t, sys; t.whole_gradient_child(sys.argv[1])", "640"],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    child = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("LISTS ")][-1][6:])
    assert child["lists"] == [[list(m) for m in l] for l in replayed]
    assert child["launches"] == 2


def test_no_candidates(world, ctx):
    """a threshold no candidate passes: no tile is flagged, every sparse work item returns, empty lists; the next call is right"""
    w = world[512]
    c = ctx(18)
    fr = w["frames"]
    assert batch_lists(c, [fr["absent"], shifted(fr["absent"], 8, 8), fr["absent"]], thr=100.0) == [[], [], []]
    assert batch_lists(c, [fr[n] for n in NAMES]) == [w["want"][n] for n in NAMES]


def test_mask_and_three_levels_take_the_whole_build(world, ctx, oracle):
    """a call with a mask (level 0's is the caller's memory) and a three-level pyramid make one gradient launch per level"""
    w = world[640]
    fr = [w["frames"][n] for n in NAMES]
    mask = np.zeros((ROWS, 640), np.uint8)
    mask[:, 100:] = 255
    c = ctx(18)
    batch_lists(c, fr, mask=mask)
    c.set_profiling(True)
    got = batch_lists(c, fr, mask=mask)
    assert gradient_launches(c) == 2
    ts = world["ts"]
    for f, g in zip(fr, got):
        p = oracle.Pyramid.build(f, [4, 8], 30.0, mask=mask)
        assert g == multiset(p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, THR, n_threads=NT))
        p.free()
    # ... and the same context without the mask is sparse again
    assert batch_lists(c, fr) == [w["want"][n] for n in NAMES]
    if SPARSE_ON:
        assert gradient_launches(c) == 3
    img = synth.scene_bgr(33, 512, 512, n_shapes=120)
    pyr = oracle.Pyramid.build(img, [4, 4, 8], 30.0)
    ts3, nf = templates_from_maps([pyr.quantized(l) for l in range(3)], [80, 40, 20], 128, 6, 5)
    assert nf == [80, 40, 20]
    want = multiset(pyr.match(ts3.levels, ts3.features, ts3.class_idx, ts3.template_id, 50.0, n_threads=NT))
    pyr.free()
    assert len(want) >= 6
    c3 = ctx(18, ts=ts3, T=(4, 4, 8), max_candidates=1 << 20)
    batch_lists(c3, [img, img], thr=50.0)
    c3.set_profiling(True)
    assert batch_lists(c3, [img, img], thr=50.0) == [want, want]
    assert gradient_launches(c3) == 3


def test_overflow_retry(world, ctx):
    """sbm_match with more matches than its pinned result buffer holds: the template loop runs again on the resident pyramid,
    the gradient of the flagged items included (more candidates may flag more tiles)"""
    w = world[640]
    f = w["frames"]["centre"]
    ts = world["ts"]
    want = multiset(w["pyr"]["centre"].match(ts.levels, ts.features, ts.class_idx, ts.template_id, 30.0, n_threads=NT))
    assert len(want) > 4096
    c = ctx(18, max_candidates=1 << 18)
    assert multiset(c.match(f, 30.0)) == want
    assert multiset(c.match(f, THR)) == w["want"]["centre"]
    assert multiset(c.match(f, 30.0)) == want


def test_gray(world, ctx, oracle):
    w = world[512]
    ts = world["ts"]
    fr = [np.ascontiguousarray(w["frames"][n][:, :, 1]) for n in NAMES]
    c = ctx(32)
    batch_lists(c, fr)
    c.set_profiling(True)
    got = batch_lists(c, fr)
    if SPARSE_ON:
        assert gradient_launches(c) == 3
    total = 0
    for b, (f, g) in enumerate(zip(fr, got)):
        p = oracle.Pyramid.build(f, [4, 8], 30.0)
        assert g == multiset(p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, THR, n_threads=NT)), b
        assert np.array_equal(c.get_quantized_frame(0, b), p.quantized(0)), b
        p.free()
        total += len(g)
    assert total > 20
