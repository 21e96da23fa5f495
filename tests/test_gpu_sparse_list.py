"""-m gpu: the sparse level-0 gradient launch runs from the per-frame lists of working items that k_mark_refine_tiles leaves
(csrc/sbm_refine_tiles.h: gradient_rect_list; csrc/sbm_quantize_stream.h: k_quantize_stream_slots; tests/test_sparse_list.py is
the CPU half).

Every match list is compared bit for bit with oracle.Pyramid, and level 0's map is poisoned through the stage setter before the
call.  Geometries: 448 x 576 BGR, 512 x 704 gray (tests/test_gpu_sparse_rects.py) and 512 x 768 BGR (tests/test_gpu_sparse_gradient.py),
stream mode forced.  The threshold is 75: the frames with one object then have between 80 and 256 coarse candidates -- one
workgroup of the mark launch holds such a frame and writes its list --, the frame with two objects has more than 400 and keeps
the sentinel (its waves test their own items, beside frames that carry lists), the scene without the object has none or a few.
(The reference image tiled over these canvases is one crop of it, with no more candidates than `centre`: the two-object frame
takes the place of the frame with more than 256.)  Which case a frame is, the test asserts from the oracle's coarse candidates."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from shape_based_matching_amd import capi
from shape_based_matching_amd.templates import MATCH_DTYPE, from_pyramids
from test_gpu_sparse_geometry import CUT, run_batch
from test_gpu_sparse_gradient import CAP, NT, SPARSE_ON, load_templates, make_frames, multiset
from test_gpu_sparse_rects import frames_of, poison, rects_emu  # noqa: F401  (rects_emu: a fixture)

pytestmark = pytest.mark.gpu
REC = MATCH_DTYPE.itemsize
THR = 75.0
T = 4
LIST_ON = SPARSE_ON and os.environ.get("SBM_SPARSE_RECTS", "1") != "0" and os.environ.get("SBM_SPARSE_LIST", "1") != "0"
SLOTS_ENV = int(os.environ.get("SBM_SPARSE_SLOTS", "0") or 0)
SLOTS_DEFAULT = 1 << 30  # csrc/sbm_capi_ctx.inc: SPARSE_SLOTS_DEFAULT, the items per frame
GEO = dict(CUT, R=(512, 768, 3))


def coarse_candidates(oracle, ts, pyr, thr=THR):
    """the oracle's coarse candidates of one frame: the one-level match of the templates' level-1 records on the pyramid's
    level-1 map, at the call's threshold (tests/test_gpu_sparse_rects.py: cpu_items)"""
    coarse = from_pyramids([[{"width": int(ts.levels[t, 1]["width"]), "height": int(ts.levels[t, 1]["height"]),
                              "features": np.stack([ts.features[k][int(ts.levels[t, 1]["feature_offset"]):][: int(ts.levels[t, 1]["n_features"])]
                                                    for k in ("x", "y", "label")], axis=1)}] for t in range(ts.n_templates)], "c")
    p1 = oracle.Pyramid.from_quantized([pyr.quantized(1)], [8])
    cands = p1.match(coarse.levels, coarse.features, coarse.class_idx, coarse.template_id, thr, n_threads=NT)
    p1.free()
    return cands


def header_items(rects_emu, ts, cands, rows, cols, hs):
    """the working items of one frame over every strip of the grid, by the shared header functions on the coarse candidates"""
    tid = np.asarray(cands["template_id"], np.int64)
    ext = np.zeros((ts.n_templates, 2), np.int32)
    for t in range(ts.n_templates):
        o, n = int(ts.levels[t, 0]["feature_offset"]), int(ts.levels[t, 0]["n_features"])
        ext[t] = (int(ts.features["x"][o: o + n].max()) + 1, int(ts.features["y"][o: o + n].max()) + 1)
    cand = np.ascontiguousarray(np.stack([cands["x"], cands["y"], ts.levels["width"][tid, 0], ts.levels["height"][tid, 0], ext[tid, 0], ext[tid, 1]],
                                         axis=1).astype(np.int32)).reshape(-1, 6)
    W, H = cols // T, rows // T
    flags = np.zeros(((W + 31) // 32) * ((H + 31) // 32), np.uint8)
    rects = np.zeros(((rows + 7) // 8, 2), np.int32)
    assert rects_emu.sbm_emu_mark(len(cand), cand.ctypes.data, rows, cols, T, W, H, flags.ctypes.data, rects.ctypes.data, None) == 0
    return rects_emu.sbm_emu_items(rects.ctypes.data, flags.ctypes.data, rows, cols, hs, T, W, H, None)


def launch_shape(frames, rows, cols, hs, slots=0):
    """(waves per frame, waves launched) of the launch by slots: frames * S and the packed last-strip waves"""
    n_strips, n_rb = (cols + 239) // 240, (rows + hs - 1) // hs
    lanes = (cols - 240 * (n_strips - 1)) // 4 + 4
    per = 64 // lanes
    packed = frames >= 2 and per >= 2
    n_full = n_strips - 1 if packed else n_strips
    S = min(n_full * n_rb, slots or SLOTS_ENV or SLOTS_DEFAULT)
    return S, frames * S + (n_rb * ((frames + per - 1) // per) if packed else 0)


@pytest.fixture(scope="module")
def world(oracle):
    """per geometry the frames, the oracle's pyramids, lists and coarse candidates at THR -- computed once, never changed"""
    ts = load_templates()
    w = {"ts": ts}
    for g, (rows, cols, ch) in GEO.items():
        frames = frames_of(oracle, ts, rows, cols, ch) if g in CUT else make_frames(cols)
        want, pyrs, cands = {}, {}, {}
        for name, f in frames.items():
            p = oracle.Pyramid.build(f, [4, 8], 30.0)
            want[name] = multiset(p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, THR, n_threads=NT))
            pyrs[name] = p
            cands[name] = coarse_candidates(oracle, ts, p)
        w[g] = {"frames": frames, "want": want, "pyr": pyrs, "cands": cands}
        # the cases the threshold is chosen for
        for n in frames:
            k = len(cands[n])
            if n == "absent":
                assert k <= 8 and want[n] == [], (g, n, k)
            elif n == "two":
                assert k > 256 and len(want[n]) > 20, (g, n, k)  # no list: more candidates than one workgroup holds
            else:
                assert 40 <= k <= 256 and len(want[n]) > 10, (g, n, k)  # one workgroup: a list
    yield w
    for g in GEO:
        for p in w[g]["pyr"].values():
            p.free()


@pytest.fixture()
def ctx(world):
    made = []

    def make(hs=24, depth=1, **kw):
        c = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0, **kw)
        c.upload_templates(world["ts"])
        c.set_quantize_mode("stream", hs)
        c.set_pipeline_depth(depth)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


def assert_list_mode(c, frames, rows, cols, hs):
    if not SPARSE_ON:
        return
    S, launched = launch_shape(frames, rows, cols, hs)
    if LIST_ON:
        assert c.sparse_list() == (1, S) and c.sparse_items()[0] == 2 and c.sparse_items()[2] == launched, (c.sparse_list(), c.sparse_items(), S, launched)
    else:
        assert c.sparse_list() == (0, 0)


@pytest.mark.parametrize("geo,hs,depth", [("P", 24, 1), ("P", 32, 4), ("Q", 24, 1), ("Q", 32, 4), ("R", 24, 1), ("R", 18, 4)])
def test_one_object_against_each_border_and_the_counts(world, ctx, rects_emu, geo, hs, depth):
    """every placement in one batch; the profiled launch worked in exactly the items the header gives for the oracle's coarse
    candidates and launched frames * S + packed waves; afterwards the whole map of every frame, the caller's buffer overwritten"""
    rows, cols, _ = GEO[geo]
    e = world[geo]
    names = list(e["frames"])
    c = ctx(hs, depth)
    frames = [e["frames"][n] for n in names]
    run_batch(c, frames)  # the first call also prepares the template tables
    poison(c, rows, cols)
    c.set_profiling(True)
    got, d_img = run_batch(c, frames, thr=THR)
    for n, g in zip(names, got):
        assert g == e["want"][n], (geo, hs, n)
    assert_list_mode(c, len(frames), rows, cols, hs)
    if SPARSE_ON and os.environ.get("SBM_SPARSE_RECTS", "1") != "0":
        want = [header_items(rects_emu, world["ts"], e["cands"][n], rows, cols, hs) for n in names]
        print(geo, hs, dict(zip(names, want)), c.sparse_items(), c.sparse_list())
        assert c.sparse_items()[1] == sum(want) > 0, (c.sparse_items(), want)
    c.set_profiling(False)
    d_img.fill_(0xFF)
    import torch

    torch.cuda.synchronize()
    for b, n in enumerate(names):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][n].quantized(0)), (geo, hs, n)


def test_two_distant_objects_and_a_call_without_candidates(world, ctx):
    """the frame with two objects keeps the sentinel beside frames with lists; then a threshold nothing passes: no list is
    written, no item works; then the batch again"""
    rows, cols, _ = GEO["Q"]
    e = world["Q"]
    c = ctx(32, 4)
    names = ["two", "absent", "centre"]
    run_batch(c, [e["frames"][n] for n in names], thr=THR)
    poison(c, rows, cols)
    got, _ = run_batch(c, [e["frames"][n] for n in names], thr=THR)
    assert got == [e["want"][n] for n in names]
    poison(c, rows, cols)
    c.set_profiling(True)
    got, _ = run_batch(c, [e["frames"][n] for n in names], thr=100.0)
    assert got == [[], [], []]
    if SPARSE_ON:
        assert c.sparse_items()[1] == 0
    assert_list_mode(c, len(names), rows, cols, 32)
    c.set_profiling(False)
    got, _ = run_batch(c, [e["frames"][n] for n in names], thr=THR)
    assert got == [e["want"][n] for n in names]


def test_seven_frames_with_one_on_the_sentinel_then_two_then_seven(world, ctx):
    rows, cols, _ = GEO["P"]
    e = world["P"]
    seven = ["absent", "left", "two", "absent", "right", "top", "centre"]
    two = ["right", "left"]
    c = ctx(24, 1)
    for names in (seven, two, seven):
        poison(c, rows, cols)
        got, _ = run_batch(c, [e["frames"][n] for n in names], thr=THR)
        assert got == [e["want"][n] for n in names], names
        assert_list_mode(c, len(names), rows, cols, 24)
    for b, n in reversed(list(enumerate(seven))):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][n].quantized(0)), (b, n)


def test_one_captured_graph_replayed_on_frames_in_which_the_object_has_moved(world, ctx):
    """graph mode on: the caller's buffers stay, their contents change between the replays -- the lists are device data, so the
    replayed launch follows each call's candidates, from a list to the sentinel and back"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols, ch = GEO["P"]
    e = world["P"]
    c = ctx(32, 4)
    c.set_graph_mode(True)
    calls = [["left", "centre", "absent"], ["two", "bottom", "top"], ["absent", "absent", "left"], ["centre", "right", "two"], ["right", "two", "bottom"]]
    B = 3
    d_img = torch.zeros((B, rows, cols, ch), dtype=torch.uint8, device=dev)
    d_out = torch.zeros(B * CAP * REC, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(B * 2, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    for names in calls:
        d_img.copy_(torch.from_numpy(np.stack([e["frames"][n] for n in names])))
        torch.cuda.synchronize()
        c.match_batch_device(d_img.data_ptr(), rows * cols * ch, B, rows, cols, cols * ch, ch, THR, d_out.data_ptr(), CAP, d_cnt.data_ptr(),
                             stream=st.cuda_stream)
        st.synchronize()
        cnt = d_cnt.cpu().numpy().reshape(B, 2)
        recs = d_out.cpu().numpy().view(MATCH_DTYPE).reshape(B, CAP)
        assert (cnt[:, 1] == 0).all()
        assert [multiset(recs[b, : cnt[b, 0]]) for b in range(B)] == [e["want"][n] for n in names], names
        assert_list_mode(c, B, rows, cols, 32)
    assert c.graph_count() == 1
    d_img.fill_(0xFF)
    torch.cuda.synchronize()
    for b, n in enumerate(calls[-1]):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][n].quantized(0)), n
    assert multiset(c.match_templates(THR)) == e["want"][calls[-1][0]]


def test_every_entry_point_behind_one_context(world, ctx):
    """sbm_match_device, sbm_match, sbm_match_batch_host and sbm_match_batch_device_ptrs"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols, ch = GEO["Q"]
    e = world["Q"]
    c = ctx(24, 1)
    st = torch.cuda.Stream(device=dev)
    d_out = torch.zeros(CAP * REC, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    for n in ("left", "two", "absent", "right"):
        d_img = torch.from_numpy(e["frames"][n]).to(dev)
        torch.cuda.synchronize()
        poison(c, rows, cols)
        c.match_device(d_img.data_ptr(), rows, cols, cols * ch, ch, THR, d_out.data_ptr(), CAP, d_cnt.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        cnt = d_cnt.cpu().numpy()
        assert cnt[1] == 0 and multiset(d_out.cpu().numpy().view(MATCH_DTYPE)[: cnt[0]]) == e["want"][n], n
        d_img.fill_(0xFF)
        torch.cuda.synchronize()
        assert np.array_equal(c.get_quantized_frame(0, 0), e["pyr"][n].quantized(0)), n
    for n in ("bottom", "top"):
        poison(c, rows, cols)
        assert multiset(c.match(e["frames"][n], THR)) == e["want"][n], n
        assert multiset(c.match_templates(THR)) == e["want"][n], n
    names = ["top", "two", "absent", "left"]
    poison(c, rows, cols)
    got = c.match_batch_host([e["frames"][n] for n in names], THR, cap=CAP, sub_batch=4)
    assert [multiset(g) for g in got] == [e["want"][n] for n in names]
    assert_list_mode(c, 4, rows, cols, 24)
    # the frames named by a device table of addresses, in another order than they lie in memory
    names = ["right", "centre", "two", "bottom", "absent"]
    B = len(names)
    d_frames = torch.from_numpy(np.stack([e["frames"][n] for n in reversed(names)])).to(dev)
    ptrs = np.array([d_frames.data_ptr() + (B - 1 - b) * rows * cols * ch for b in range(B)], np.uint64)
    d_ptrs = torch.from_numpy(ptrs.view(np.int64)).to(dev)
    d_outs = torch.zeros(B * CAP * REC, dtype=torch.uint8, device=dev)
    d_cnts = torch.zeros(B * 2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    poison(c, rows, cols)
    c.match_batch_device_ptrs(d_ptrs.data_ptr(), B, rows, cols, cols * ch, ch, THR, d_outs.data_ptr(), CAP, d_cnts.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    cnt = d_cnts.cpu().numpy().reshape(B, 2)
    recs = d_outs.cpu().numpy().view(MATCH_DTYPE).reshape(B, CAP)
    assert (cnt[:, 1] == 0).all()
    assert [multiset(recs[b, : cnt[b, 0]]) for b in range(B)] == [e["want"][n] for n in names]
    assert_list_mode(c, B, rows, cols, 24)


CHILD_NAMES = ["centre", "left", "two", "absent", "right", "top", "bottom"]


def child(geo, npz):
    """the child process (SBM_SPARSE_SLOTS or SBM_SPARSE_LIST set): the batch on the parent's frames, profiled"""
    rows, cols, ch = GEO[geo]
    fr = np.load(npz)
    c = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0)
    c.upload_templates(load_templates())
    c.set_quantize_mode("stream", 32)
    run_batch(c, [fr[n] for n in CHILD_NAMES], thr=THR)
    poison(c, rows, cols)
    c.set_profiling(True)
    lists, _ = run_batch(c, [fr[n] for n in CHILD_NAMES], thr=THR)
    out = {"lists": lists, "items": c.sparse_items(), "list": c.sparse_list()}
    c.close()
    print("LISTS " + json.dumps(out))


@pytest.mark.parametrize("knob,value", [("SBM_SPARSE_SLOTS", "1"), ("SBM_SPARSE_SLOTS", "3"), ("SBM_SPARSE_LIST", "0")])
def test_looping_waves_and_the_launch_without_lists_in_a_child(world, rects_emu, tmp_path, knob, value):
    geo = "P"
    rows, cols, _ = GEO[geo]
    e = world[geo]
    npz = str(tmp_path / "frames.npz")
    np.savez(npz, **{n: e["frames"][n] for n in CHILD_NAMES})
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    env.pop("SBM_SPARSE_SLOTS", None)
    env[knob] = value
    out = subprocess.run([sys.executable, "-c", "import test_gpu_sparse_list as t, sys; t.child(sys.argv[1], sys.argv[2])", geo, npz],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("LISTS ")][-1][6:])
    assert got["lists"] == [[list(m) for m in e["want"][n]] for n in CHILD_NAMES]
    if not (SPARSE_ON and os.environ.get("SBM_SPARSE_RECTS", "1") != "0"):
        return
    working = sum(header_items(rects_emu, world["ts"], e["cands"][n], rows, cols, 32) for n in CHILD_NAMES)
    assert got["items"][0] == 2 and got["items"][1] == working > 0, (got, working)
    n_rb, B = (rows + 31) // 32, len(CHILD_NAMES)
    if knob == "SBM_SPARSE_LIST":
        # the launch without lists: a wave per item of the grid, two strips with a wave per frame and the packed third
        assert got["list"] == [0, 0] and got["items"][2] == 2 * n_rb * B + n_rb * ((B + 1) // 2), got
    elif os.environ.get("SBM_SPARSE_LIST", "1") != "0":
        S, launched = launch_shape(B, rows, cols, 32, slots=int(value))
        assert S == int(value) and got["list"] == [1, S] and got["items"][2] == launched, (got, S, launched)
