"""-m gpu: the sparse level-0 gradient launch takes its work items from the record of need rectangles that k_mark_refine_tiles
keeps beside the tile flags (csrc/sbm_refine_tiles.h: refine_need, gradient_rect_item_needed; tests/test_sparse_rects.py is the
CPU half).

Every list is compared bit for bit with oracle.Pyramid, and level 0's map is poisoned through the stage setter before the call
unless a case says otherwise: what the rect-driven launch does not write must not be read.  Geometries: 448 x 576 BGR and
512 x 704 gray (tests/test_gpu_sparse_geometry.py: cut tiles), the object against each border, two objects in the same rows, no
candidate, batches of 7 and 2 frames.  Under profiling the launch reports its working items (sbm_get_sparse_items): they must be
the items the shared header function gives on the CPU for the oracle's coarse candidates."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from shape_based_matching_amd import capi
from shape_based_matching_amd.templates import MATCH_DTYPE, from_pyramids
from test_gpu_sparse_geometry import CUT, cut_frames, run_batch
from test_gpu_sparse_gradient import CAP, NT, SPARSE_ON, THR, load_templates, multiset, shifted

pytestmark = pytest.mark.gpu
REC = MATCH_DTYPE.itemsize
RECTS_ON = SPARSE_ON and os.environ.get("SBM_SPARSE_RECTS", "1") != "0"
PLACES = ["centre", "left", "right", "top", "bottom", "absent"]
T = 4


def frames_of(oracle, ts, rows, cols, ch):
    """cut_frames (centre, right, bottom, absent) and the object against the left and the top border, and -- where the canvas
    is wide enough -- two objects in the same rows: the left half of `left`, the right half of `right`"""
    fr = cut_frames(oracle, ts, rows, cols, ch)
    pyr = oracle.Pyramid.build(fr["centre"], [4, 8], 30.0)
    best = max(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, 80.0, n_threads=NT).tolist(), key=lambda m: m[2])
    pyr.free()
    fr["left"] = shifted(fr["centre"], 0, -((int(best[0]) - 2) // 2 * 2))
    fr["top"] = shifted(fr["centre"], -((int(best[1]) - 2) // 2 * 2), 0)
    two = fr["left"].copy()
    two[:, cols // 2:] = fr["right"][:, cols // 2:]
    fr["two"] = two
    return fr


@pytest.fixture(scope="module")
def world(oracle):
    ts = load_templates()
    w = {"ts": ts}
    for g, (rows, cols, ch) in CUT.items():
        frames = frames_of(oracle, ts, rows, cols, ch)
        want, pyrs = {}, {}
        for name, f in frames.items():
            p = oracle.Pyramid.build(f, [4, 8], 30.0)
            want[name] = multiset(p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, THR, n_threads=NT))
            pyrs[name] = p
        for n in ("centre", "left", "right", "top", "bottom"):
            assert len(want[n]) > 20, (g, n)
        assert len({json.dumps(want[n]) for n in ("centre", "left", "right", "top", "bottom")}) == 5, g
        w[g] = {"frames": frames, "want": want, "pyr": pyrs}
    yield w
    for g in CUT:
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


@pytest.fixture(scope="module")
def rects_emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("rects_emu") / "librects_emu.so")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "emu"), "-I",
                           os.path.join(ROOT, "shape_based_matching_amd", "csrc"), "-o", so, os.path.join(ROOT, "tests", "emu", "sparse_rects_emu.cpp")])
    L = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    L.sbm_emu_mark.argtypes = [C.c_int64, vp, i, i, i, i, i, vp, vp, vp]
    L.sbm_emu_items.argtypes = [vp, vp, i, i, i, i, i, i, vp]
    return L


def poison(c, rows, cols):
    c.set_quantized(0, (1 << np.random.RandomState(3).randint(0, 8, (rows, cols))).astype(np.uint8))


def cpu_items(oracle, rects_emu, ts, pyr, rows, cols, hs):
    """(rect-driven, tile-driven) working items of one frame, by the shared header functions on the oracle's coarse candidates:
    the one-level match of the templates' level-1 records on the pyramid's level-1 map, at the call's threshold"""
    coarse = from_pyramids([[{"width": int(ts.levels[t, 1]["width"]), "height": int(ts.levels[t, 1]["height"]),
                              "features": np.stack([ts.features[k][int(ts.levels[t, 1]["feature_offset"]):][: int(ts.levels[t, 1]["n_features"])]
                                                    for k in ("x", "y", "label")], axis=1)}] for t in range(ts.n_templates)], "c")
    p1 = oracle.Pyramid.from_quantized([pyr.quantized(1)], [8])
    cands = p1.match(coarse.levels, coarse.features, coarse.class_idx, coarse.template_id, THR, n_threads=NT)
    p1.free()
    tid = np.asarray(cands["template_id"], np.int64)
    ext = np.zeros((ts.n_templates, 2), np.int32)  # the features' own extent at level 0
    for t in range(ts.n_templates):
        o, n = int(ts.levels[t, 0]["feature_offset"]), int(ts.levels[t, 0]["n_features"])
        ext[t] = (int(ts.features["x"][o: o + n].max()) + 1, int(ts.features["y"][o: o + n].max()) + 1)
    cand = np.ascontiguousarray(np.stack([cands["x"], cands["y"], ts.levels["width"][tid, 0], ts.levels["height"][tid, 0], ext[tid, 0], ext[tid, 1]],
                                         axis=1).astype(np.int32)).reshape(-1, 6)
    W, H = cols // T, rows // T
    flags = np.zeros(((W + 31) // 32) * ((H + 31) // 32), np.uint8)
    rects = np.zeros(((rows + 7) // 8, 2), np.int32)
    assert rects_emu.sbm_emu_mark(len(cand), cand.ctypes.data, rows, cols, T, W, H, flags.ctypes.data, rects.ctypes.data, None) == 0
    by_rect = rects_emu.sbm_emu_items(rects.ctypes.data, flags.ctypes.data, rows, cols, hs, T, W, H, None)
    by_tile = rects_emu.sbm_emu_items(None, flags.ctypes.data, rows, cols, hs, T, W, H, None)
    return by_rect, by_tile


@pytest.mark.parametrize("geo,hs,depth", [("P", 24, 1), ("P", 32, 4), ("Q", 24, 1), ("Q", 32, 4)])
def test_borders_and_item_counts(world, ctx, oracle, rects_emu, geo, hs, depth):
    """the object against each border, at the centre and absent, in one batch at pipeline depth 1 and 4 (24 and 32 rows per item);
    the profiled launch worked in exactly the items the header gives for the oracle's coarse candidates"""
    rows, cols, _ = CUT[geo]
    e = world[geo]
    c = ctx(hs, depth)
    frames = [e["frames"][n] for n in PLACES]
    run_batch(c, frames)  # the first call also prepares the template tables
    poison(c, rows, cols)
    c.set_profiling(True)
    got, _ = run_batch(c, frames)
    for n, g in zip(PLACES, got):
        assert g == e["want"][n], (geo, hs, n)
    if not SPARSE_ON:
        return
    sel, working, launched = c.sparse_items()
    assert sel == (2 if RECTS_ON else 1)
    want = [cpu_items(oracle, rects_emu, world["ts"], e["pyr"][n], rows, cols, hs) for n in PLACES]
    for n, (by_rect, by_tile) in zip(PLACES, want):
        print(geo, hs, n, "items by rect", by_rect, "by tile", by_tile)
        assert by_rect <= by_tile
    assert want[0][0] > 0  # (the textured `absent` scene has coarse candidates too: none of them survives the refinement)
    if RECTS_ON:
        # (a wave of the packed last strip counts once for every frame of it that needs the strip)
        assert working == sum(r for r, _ in want) and launched <= len(PLACES) * ((cols + 239) // 240) * ((rows + hs - 1) // hs), (working, launched, want)
        if geo == "Q":  # one object per frame at 512 x 704: fewer items than the tile flags keep
            assert want[0][0] < want[0][1] and working < sum(t for _, t in want), want
    c.set_profiling(False)
    for b, n in enumerate(PLACES):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][n].quantized(0)), (geo, hs, n)


def test_two_objects_in_the_same_rows_and_a_call_without_candidates(world, ctx):
    """the hull of the rows spans both objects (the tile test cuts what lies between); then a threshold nothing passes: an empty
    record, no item works; then the batch again"""
    rows, cols, _ = CUT["Q"]
    e = world["Q"]
    assert len(e["want"]["two"]) > len(e["want"]["left"]) and len(e["want"]["two"]) > len(e["want"]["right"])
    c = ctx(32, 4)
    names = ["two", "absent", "centre"]
    run_batch(c, [e["frames"][n] for n in names])
    poison(c, rows, cols)
    got, _ = run_batch(c, [e["frames"][n] for n in names])
    assert got == [e["want"][n] for n in names]
    poison(c, rows, cols)
    c.set_profiling(True)
    got, _ = run_batch(c, [e["frames"][n] for n in names], thr=100.0)
    assert got == [[], [], []]
    if SPARSE_ON:
        assert c.sparse_items()[1] == 0
    c.set_profiling(False)
    got, _ = run_batch(c, [e["frames"][n] for n in names])
    assert got == [e["want"][n] for n in names]


def test_seven_frames_then_two_on_one_context(world, ctx):
    rows, cols, _ = CUT["P"]
    e = world["P"]
    seven = ["absent", "left", "bottom", "absent", "right", "top", "centre"]
    two = ["right", "left"]
    c = ctx(24, 1)
    for names in (seven, two, seven):
        poison(c, rows, cols)
        got, _ = run_batch(c, [e["frames"][n] for n in names])
        assert got == [e["want"][n] for n in names], names
    for b, n in reversed(list(enumerate(seven))):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][n].quantized(0)), (b, n)


def test_one_captured_graph_replayed_on_frames_in_which_the_object_has_moved(world, ctx):
    """graph mode on: the caller's buffers stay, their contents change between the replays -- the record is device data, so the
    replayed launch follows each call's candidates"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols, ch = CUT["P"]
    e = world["P"]
    c = ctx(32, 4)
    c.set_graph_mode(True)
    calls = [["left", "centre", "absent"], ["right", "bottom", "top"], ["absent", "absent", "left"], ["centre", "right", "bottom"]]
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
    assert c.graph_count() == 1
    if SPARSE_ON:
        assert c.sparse_items()[0] == (2 if RECTS_ON else 1)
    # a reader behind a replay: the whole map of the last call's frames, from the retained copy
    d_img.fill_(0xFF)
    torch.cuda.synchronize()
    for b, n in enumerate(calls[-1]):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][n].quantized(0)), n
    assert multiset(c.match_templates(THR)) == e["want"][calls[-1][0]]


def test_single_frame_and_host_entry_points(world, ctx):
    """sbm_match_device, sbm_match (with its readers behind an overwritten buffer) and sbm_match_batch_host"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols, ch = CUT["Q"]
    e = world["Q"]
    c = ctx(24, 1)
    st = torch.cuda.Stream(device=dev)
    d_out = torch.zeros(CAP * REC, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    for n in ("left", "top", "absent", "right"):
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
        assert multiset(c.match_templates(THR)) == e["want"][n], n
    for n in ("bottom", "two"):
        poison(c, rows, cols)
        assert multiset(c.match(e["frames"][n], THR)) == e["want"][n], n
        assert multiset(c.match_templates(THR)) == e["want"][n], n
    names = ["top", "two", "absent", "left"]
    poison(c, rows, cols)
    got = c.match_batch_host([e["frames"][n] for n in names], THR, cap=CAP, sub_batch=4)
    assert [multiset(g) for g in got] == [e["want"][n] for n in names]
    if SPARSE_ON:
        assert c.sparse_items()[0] == (2 if RECTS_ON else 1)


def test_one_rank_sharded_batch(world, ctx):
    import torch

    dev = torch.device("cuda", 0)
    rows, cols, ch = CUT["P"]
    e = world["P"]
    names = ["top", "left", "absent", "bottom"]
    frames = [e["frames"][n] for n in names]
    c = ctx(32, 4)
    c.comm_init(1, 0, c.comm_unique_id())
    B = len(frames)
    hdr = (8 * B + 15) // 16 * 16
    nbytes = hdr + B * CAP * REC
    d_img = torch.from_numpy(np.stack(frames)).to(dev)
    d_local = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    d_gath = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for call in range(2):
        poison(c, rows, cols)
        c.match_batch_device_sharded(d_img.data_ptr(), rows * cols * ch, B, rows, cols, cols * ch, ch, THR, d_local.data_ptr(), CAP, d_gath.data_ptr(),
                                     stream=st.cuda_stream)
        st.synchronize()
    buf = d_gath.cpu().numpy()
    cnt = buf[: 8 * B].view(np.int32).reshape(B, 2)
    for f, n in enumerate(names):
        assert cnt[f, 1] == 0 and multiset(buf[hdr + f * CAP * REC: hdr + (f + 1) * CAP * REC].view(MATCH_DTYPE)[: cnt[f, 0]]) == e["want"][n], n
    if SPARSE_ON:
        assert c.sparse_items()[0] == (2 if RECTS_ON else 1)


def tile_driven_child(geo):
    """the child process (SBM_SPARSE_RECTS=0): the border batch with the tile-driven selection"""
    from oracle import oracle as O

    O.build()
    O.lib()
    rows, cols, ch = CUT[geo]
    ts = load_templates()
    fr = frames_of(O, ts, rows, cols, ch)
    c = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0)
    c.upload_templates(ts)
    c.set_quantize_mode("stream", 32)
    run_batch(c, [fr[n] for n in PLACES])
    poison(c, rows, cols)
    c.set_profiling(True)
    lists, _ = run_batch(c, [fr[n] for n in PLACES])
    items = c.sparse_items()
    c.close()
    print("LISTS " + json.dumps({"lists": lists, "items": items}))


def test_tile_driven_selection_in_a_child_gives_the_same_lists(world, ctx):
    rows, cols, _ = CUT["Q"]
    e = world["Q"]
    c = ctx(32, 1)
    run_batch(c, [e["frames"][n] for n in PLACES])
    c.set_profiling(True)
    got, _ = run_batch(c, [e["frames"][n] for n in PLACES])
    assert got == [e["want"][n] for n in PLACES]
    mine = c.sparse_items()
    env = dict(os.environ, SBM_SPARSE_RECTS="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    out = subprocess.run([sys.executable, "-c", "import test_gpu_sparse_rects as t, sys; t.tile_driven_child(sys.argv[1])", "Q"],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    child = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("LISTS ")][-1][6:])
    assert child["lists"] == [[list(m) for m in l] for l in got]
    if SPARSE_ON:
        assert child["items"][0] == 1 and child["items"][1] > 0
        if RECTS_ON:
            assert mine[0] == 2 and 0 < mine[1] < child["items"][1], (mine, child["items"])
