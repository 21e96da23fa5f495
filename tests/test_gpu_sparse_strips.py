"""-m gpu: level 0's bit strips built only in the tiles the coarse candidates' refinement reads (LM_BIT_STRIPS_SPARSE,
csrc/sbm_refine_tiles.h, k_mark_refine_tiles, the flagged share of k_build_lm_rows).

A match entry point on a two-level pyramid runs coarse pass -> mark tiles -> strips of the flagged tiles -> refinement; the
lists must be the oracle's bit for bit on every launch path, whatever an earlier call left in the unflagged tiles, and the
readers that want level 0 afterwards rebuild it from the orientation map.  Fixture: the case1 image on a 512 x 640 canvas,
4 x 5 tiles at level 0.  The whole-build form (SBM_SPARSE_STRIPS=0, read once per process) runs in one child process.

The reference's templates hold features AT x = width, y = height (cropTemplates), one past the declared box; the `tight`
template set below declares boxes 96 px smaller than its features reach, which moves the clamps so that patches pass the
level's last grid row (the flat overrun into the next strip) and features fall outside the level."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

from shape_based_matching_amd import capi, synth
from shape_based_matching_amd.templates import MATCH_DTYPE, TemplateSet

pytestmark = pytest.mark.gpu
NT = min(16, os.cpu_count() or 1)
ROWS, COLS, THR = 512, 640, 65.0
CAP = 8192


def multiset(recs):
    return sorted(np.ascontiguousarray(recs, MATCH_DTYPE).tolist())


def shifted(frame, dy, dx):
    """the frame moved by (dy, dx); what leaves the canvas is cut, what enters is black"""
    out = np.zeros_like(frame)
    src = frame[max(0, -dy): frame.shape[0] - max(0, dy), max(0, -dx): frame.shape[1] - max(0, dx)]
    out[max(0, dy): max(0, dy) + src.shape[0], max(0, dx): max(0, dx) + src.shape[1]] = src
    return out


def load_templates():
    return TemplateSet.load_npz(os.path.join(GOLDEN, "case1_templates.npz")).subset(range(0, 360, 6))


def tight_templates(ts):
    """the same features in declared boxes 96 px (48 at level 1) smaller"""
    lv = ts.levels.copy()
    for l in range(lv.shape[1]):
        lv["width"][:, l] -= 96 >> l
        lv["height"][:, l] -= 96 >> l
    out = ts.subset(range(ts.n_templates))
    out.levels = lv
    return out


def make_frames(object_box):
    """centre, against the right / bottom border (the object's box ends 2 px before it: the clamps move every candidate
    there), absent, and the centre frame moved left -- a fourth content for the stale-strip test"""
    img = np.load(os.path.join(GOLDEN, "case1_test_bgr.npz"))["bgr"]
    centre = synth.embed(img, ROWS, COLS, (ROWS - img.shape[0]) // 2, (COLS - img.shape[1]) // 2)
    if object_box is None:
        return centre
    x, y, w, h = object_box
    border = shifted(centre, (ROWS - 2 - (y + h)) // 2 * 2, (COLS - 2 - (x + w)) // 2 * 2)
    absent = synth.scene_bgr(5, ROWS, COLS)
    return {"centre": centre, "border": border, "absent": absent, "left": shifted(centre, 0, -16)}


def batch_lists(ctx, frames, thr=THR, calls=1, stream=None):
    """sbm_match_batch_device on the stacked frames, `calls` times with the same arguments: the last call's lists"""
    import torch

    dev = torch.device("cuda", 0)
    B = len(frames)
    d_img = torch.from_numpy(np.stack(frames)).to(dev)
    d_out = torch.zeros(B * CAP * MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(B * 2, dtype=torch.int32, device=dev)
    st = stream or torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    out = None
    for _ in range(calls):
        ctx.match_batch_device(d_img.data_ptr(), frames[0].size, B, ROWS, COLS, COLS * 3, 3, thr, d_out.data_ptr(), CAP, d_cnt.data_ptr(),
                               stream=st.cuda_stream)
        st.synchronize()
        cnt = d_cnt.cpu().numpy().reshape(B, 2)
        recs = d_out.cpu().numpy().view(MATCH_DTYPE).reshape(B, CAP)
        assert (cnt[:, 1] == 0).all() and (cnt[:, 0] <= CAP).all(), cnt
        lists = [multiset(recs[b, : cnt[b, 0]]) for b in range(B)]
        assert out is None or out == lists  # a replay gives what the capture gave
        out = lists
    return out


def whole_build_child(box_json):
    """the child process: the same frames and template sets with the whole-strip build"""
    box = json.loads(box_json)
    fr = make_frames(box)
    ts = load_templates()
    res = {}
    for name, tset in (("plain", ts), ("tight", tight_templates(ts))):
        ctx = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0)
        ctx.upload_templates(tset)
        res[name] = batch_lists(ctx, [fr["centre"], fr["border"], fr["absent"]], calls=2)
        ctx.close()
    print("LISTS " + json.dumps(res))


@pytest.fixture(scope="module")
def world(oracle):
    ts = load_templates()
    centre = make_frames(None)
    pyr = oracle.Pyramid.build(centre, [4, 8], 30.0)
    best = max(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, 90.0, n_threads=NT).tolist(), key=lambda m: m[2])
    pyr.free()
    t = [i for i in range(ts.n_templates) if ts.template_id[i] == best[5] and ts.class_idx[i] == best[4]][0]
    box = [int(best[0]), int(best[1]), int(ts.levels["width"][t, 0]), int(ts.levels["height"][t, 0])]
    frames = make_frames(box)
    assert frames["border"].any()
    want, pyrs = {}, {}
    for name, f in frames.items():
        p = oracle.Pyramid.build(f, [4, 8], 30.0)
        want[name] = multiset(p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, THR, n_threads=NT))
        pyrs[name] = p
    assert len(want["centre"]) > 20 and len(want["border"]) > 20
    yield {"ts": ts, "frames": frames, "want": want, "pyr": pyrs, "box": box}
    for p in pyrs.values():
        p.free()


@pytest.fixture()
def ctx(world):
    made = []

    def make(ts=None, **kw):
        c = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0, **kw)
        c.upload_templates(world["ts"] if ts is None else ts)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


def test_placements(world, ctx):
    """(a) three frames, three placements, one call"""
    names = ["centre", "border", "absent"]
    got = batch_lists(ctx(), [world["frames"][n] for n in names])
    for n, g in zip(names, got):
        assert g == world["want"][n], n


def test_stale_strips(world, ctx):
    """(b) one context, two batches in turn: the tiles a call does not flag hold the other batch's bits"""
    c = ctx()
    batches = [["centre", "border", "absent"], ["absent", "left", "centre"]]
    for call in range(6):
        names = batches[call & 1]
        got = batch_lists(c, [world["frames"][n] for n in names])
        for n, g in zip(names, got):
            assert g == world["want"][n], (call, n)


def test_launch_paths(world, ctx, oracle):
    """(c) several batches in flight and graph replay (captured, then replayed twice), and the whole-strip build in a child
    process: identical lists -- also for templates whose features pass their declared boxes"""
    names = ["centre", "border", "absent"]
    fr = [world["frames"][n] for n in names]
    c = ctx()
    c.set_pipeline_depth(2)
    c.set_graph_mode(True)
    replayed = batch_lists(c, fr, calls=3)
    assert c.graph_count() == 1
    assert replayed == [world["want"][n] for n in names]
    tight = batch_lists(ctx(tight_templates(world["ts"])), fr, calls=2)
    env = dict(os.environ, SBM_SPARSE_STRIPS="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    out = subprocess.run([sys.executable, "-c", "import test_gpu_sparse_strips as t, sys; t.whole_build_child(sys.argv[1])", json.dumps(world["box"])],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    child = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("LISTS ")][-1][6:])
    as_lists = lambda ls: [[list(m) for m in l] for l in ls]  # noqa: E731
    assert child["plain"] == as_lists(replayed)
    assert child["tight"] == as_lists(tight)
    assert sum(len(l) for l in tight) > 0


def test_overflow_retry(world, ctx, oracle):
    """(d) sbm_match with more matches than its pinned result buffer holds (4096): the template loop runs again on the
    resident pyramid -- marks and strips included -- with the device capacity; the candidate capacity does not matter"""
    f = world["frames"]["centre"]
    want = multiset(world["pyr"]["centre"].match(world["ts"].levels, world["ts"].features, world["ts"].class_idx, world["ts"].template_id, 30.0,
                                                 n_threads=NT))
    assert len(want) > 4096
    small, large = ctx(max_candidates=1 << 18), ctx(max_candidates=1 << 20)
    for c in (small, large, small):
        assert multiset(c.match(f, 30.0)) == want
    assert multiset(small.match(f, THR)) == world["want"]["centre"]


def test_later_readers(world, ctx):
    """(e) after a sparse batch call nothing of level 0 is current: the stage getters and the template loop rebuild from the map"""
    names = ["border", "centre", "absent"]
    c = ctx()
    got = batch_lists(c, [world["frames"][n] for n in names])
    p0 = world["pyr"][names[0]]
    for l in range(2):
        lm = c.get_linear_memories(l)
        n = (ROWS >> l) * (COLS >> l)
        assert np.array_equal(lm[:, :n], p0.lm(l)[:, :n]), l
        for b, name in enumerate(names):
            assert np.array_equal(c.get_quantized_frame(l, b), world["pyr"][name].quantized(l)), (l, b)
    assert multiset(c.match_templates(THR)) == got[0] == world["want"][names[0]]
    # ... and in the other order: the template loop first (whole strips of frame 0), then the planes
    c2 = ctx()
    got2 = batch_lists(c2, [world["frames"][n] for n in names])
    assert multiset(c2.match_templates(THR)) == got2[0] == world["want"][names[0]]
    assert np.array_equal(c2.get_linear_memories(0)[:, : ROWS * COLS], p0.lm(0)[:, : ROWS * COLS])
    assert batch_lists(c2, [world["frames"][n] for n in names]) == got


def test_no_candidates(world, ctx):
    """(f) a threshold no candidate passes: no tile is flagged, no strip built, empty lists; the next call is correct"""
    c = ctx()
    fr = world["frames"]
    assert batch_lists(c, [fr["absent"], shifted(fr["absent"], 8, 8), fr["absent"]], thr=100.0) == [[], [], []]
    names = ["centre", "border", "absent"]
    got = batch_lists(c, [fr[n] for n in names])
    assert got == [world["want"][n] for n in names]


def test_the_sparse_build_is_what_runs(world, ctx):
    """the default path of a batch call is the new sequence, not the whole build: by the launches' timing names, the
    linear-memory kernel runs twice with the coarse pass and the mark kernel between, and the refinement last"""
    c = ctx()
    names = ["centre", "border", "absent"]
    fr = [world["frames"][n] for n in names]
    batch_lists(c, fr)  # the first call also prepares the template tables (k_prep_features), once
    c.set_profiling(True)
    assert batch_lists(c, fr) == [world["want"][n] for n in names]
    seq = [n for n, _ in c.timings() if n not in ("k_quantize", "k_resize_mask", "k_prep_features")]
    if os.environ.get("SBM_SPARSE_STRIPS", "1") != "0":
        assert seq == ["k_build_lm", "k_similarity_coarse", "k_mark_refine_tiles", "k_build_lm", "k_similarity_local"], seq
