"""-m gpu: the sparse level-0 gradient launch on two row grids (csrc/sbm_quantize_stream.h: QSArgs::list_hs; csrc/sbm_capi_ctx.inc:
sparse_list_plan; tests/test_sparse_list_grids.py is the CPU half).

A frame of at most 256 coarse candidates gets a list of its working items from k_mark_refine_tiles, made on the LIST grid; a frame
of more, or of none, has no list and walks the launch's own FIXED grid, as do the packed last-strip waves.  One batch here holds a
frame of each kind: `listed` (the object once, 40 .. 256 candidates), `dense` (two objects, more than 256), `none` (a constant
frame, no candidate at all); which is which is asserted from the oracle's coarse candidates.  512 x 768 x 3 and 448 x 576 x 3,
stream mode with the rows per item set, four batches in flight; the list grid set per context (sbm_set_sparse_list_rows), and by
the rule and the environment in child processes.

Every match list is compared bit for bit with oracle.Pyramid; level 0's map is poisoned through the stage setter before the call
and checked whole afterwards with the caller's buffer overwritten."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from shape_based_matching_amd import capi
from shape_based_matching_amd.templates import MATCH_DTYPE
from test_gpu_sparse_geometry import run_batch
from test_gpu_sparse_gradient import CAP, NT, SPARSE_ON, load_templates, make_frames, multiset, shifted
from test_gpu_sparse_list import THR, coarse_candidates, launch_shape
from test_gpu_sparse_rects import frames_of, poison, rects_emu  # noqa: F401  (rects_emu: a fixture)
from test_sparse_list_grids import throughput_rule

pytestmark = pytest.mark.gpu
REC = MATCH_DTYPE.itemsize
T = 4
GEO = {"R": (512, 768, 3), "P": (448, 576, 3)}
KNOBS_DEFAULT = all(os.environ.get(k, "1") != "0" for k in ("SBM_SPARSE_RECTS", "SBM_SPARSE_LIST")) and not os.environ.get("SBM_SPARSE_SLOTS") \
    and not os.environ.get("SBM_SPARSE_LIST_HS") and not os.environ.get("SBM_QS_HS")
LIST_ON = SPARSE_ON and KNOBS_DEFAULT
N_SIMD = 1024  # MI355X: 256 CUs of 4 SIMDs


def geometry_frames(oracle, ts, geo):
    rows, cols, ch = GEO[geo]
    if geo == "P":
        fr = frames_of(oracle, ts, rows, cols, ch)
        out = {"listed": fr["centre"], "dense": fr["two"], "moved": [fr["left"], fr["right"], fr["top"], fr["bottom"]]}
    else:
        fr = make_frames(cols)
        c = fr["centre"]
        two = np.concatenate([shifted(c, 0, -200)[:, : cols // 2], shifted(c, 0, 200)[:, cols // 2:]], axis=1)
        out = {"listed": c, "dense": np.ascontiguousarray(two), "moved": [fr["border"], fr["left"]]}
    out["none"] = np.zeros((rows, cols, ch), np.uint8)
    return out


@pytest.fixture(scope="module")
def world(oracle):
    """per geometry the frames, the oracle's pyramids, lists and coarse candidates at THR -- computed once, never changed"""
    ts = load_templates()
    w = {"ts": ts}
    for g in GEO:
        fr = geometry_frames(oracle, ts, g)
        frames = {"listed": fr["listed"], "dense": fr["dense"], "none": fr["none"]}
        frames.update({"moved%d" % i: f for i, f in enumerate(fr["moved"])})
        want, pyrs, cands = {}, {}, {}
        for name, f in frames.items():
            p = oracle.Pyramid.build(f, [4, 8], 30.0)
            want[name] = multiset(p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, THR, n_threads=NT))
            pyrs[name] = p
            cands[name] = coarse_candidates(oracle, ts, p)
            f.setflags(write=False)
        for n in frames:  # the three kinds
            k = len(cands[n])
            if n == "none":
                assert k == 0 and want[n] == [], (g, k)
            elif n == "dense":
                assert k > 256 and len(want[n]) > 20, (g, k)
            else:
                assert 40 <= k <= 256 and len(want[n]) > 10, (g, n, k)
        w[g] = {"frames": frames, "want": want, "pyr": pyrs, "cands": cands}
    yield w
    for g in GEO:
        for p in w[g]["pyr"].values():
            p.free()


def item_table(rects_emu, ts, cands, rows, cols, hs):
    """bool (row block, strip): the working items of one frame on the grid of hs rows per item, by the shared header functions on
    the oracle's coarse candidates"""
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
    n_strips, n_rb = (cols + 239) // 240, (rows + hs - 1) // hs
    out = np.zeros((n_rb, n_strips), np.int32)
    rects_emu.sbm_emu_items(rects.ctypes.data, flags.ctypes.data, rows, cols, hs, T, W, H, out.ctypes.data)
    return out >= 0


def expected_working(rects_emu, ts, e, names, rows, cols, hs, list_hs):
    """what the profiled launch counts: a listed frame's items of the LIST grid in the strips that get a wave per frame, a frame
    without a list its items of the FIXED grid there, and every frame's packed last strip on the fixed grid"""
    total = 0
    for n in names:
        k = len(e["cands"][n])
        fixed = item_table(rects_emu, ts, e["cands"][n], rows, cols, hs)
        lst = item_table(rects_emu, ts, e["cands"][n], rows, cols, list_hs)
        total += int(fixed[:, -1].sum())  # (both geometries pack their last strip in a batch of three)
        total += int((lst if 0 < k <= 256 else fixed)[:, :-1].sum())
    return total


@pytest.fixture()
def ctx(world):
    made = []

    def make(hs=32, depth=4, list_rows=-1):
        c = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0)
        c.upload_templates(world["ts"])
        c.set_quantize_mode("stream", hs)
        c.set_pipeline_depth(depth)
        c.set_sparse_list_rows(list_rows)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


NAMES = ["listed", "dense", "none"]


@pytest.mark.parametrize("geo,hs,list_hs", [("R", 32, 18), ("P", 32, 18), ("P", 24, 10), ("R", 32, 16), ("P", 32, 0)])
def test_a_listed_a_dense_and_an_empty_frame_in_one_batch(world, ctx, rects_emu, geo, hs, list_hs):
    """the three kinds of frame in one batch, the list grid set per context (0: the fixed grid); the getters report both grids, the
    profiled launch worked in exactly the items the header gives on each frame's grid; then every frame's whole map"""
    import torch

    rows, cols, _ = GEO[geo]
    e = world[geo]
    c = ctx(hs, 4, list_hs)
    frames = [e["frames"][n] for n in NAMES]
    run_batch(c, frames, thr=THR)  # the first call also prepares the template tables
    poison(c, rows, cols)
    c.set_profiling(True)
    got, d_img = run_batch(c, frames, thr=THR)
    assert got == [e["want"][n] for n in NAMES], (geo, hs, list_hs)
    if LIST_ON:
        S, launched = launch_shape(len(frames), rows, cols, hs)
        grid = list_hs or hs
        print(geo, hs, list_hs, c.sparse_items(), c.sparse_list(), c.sparse_list_rows())
        assert c.sparse_list() == (1, S) and c.sparse_list_rows() == grid  # the waves per frame are the fixed grid's items
        assert c.sparse_items()[0] == 2 and c.sparse_items()[2] == launched, (c.sparse_items(), launched)
        want = expected_working(rects_emu, world["ts"], e, NAMES, rows, cols, hs, grid)
        assert c.sparse_items()[1] == want > 0, (c.sparse_items(), want)
        if grid != hs:  # (the two grids do differ in what works)
            assert want != expected_working(rects_emu, world["ts"], e, NAMES, rows, cols, hs, hs)
    c.set_profiling(False)
    d_img.fill_(0xFF)
    torch.cuda.synchronize()
    for b, n in enumerate(NAMES):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][n].quantized(0)), (geo, hs, list_hs, n)


def test_rows_per_item_set_through_the_api_keep_one_grid(world, ctx):
    """sbm_set_quantize_mode with rows per item and no word on the lists: the lists are on that grid, at any depth"""
    rows, cols, _ = GEO["P"]
    e = world["P"]
    for depth in (1, 4):
        c = ctx(24, depth)
        got, _ = run_batch(c, [e["frames"][n] for n in NAMES], thr=THR)
        assert got == [e["want"][n] for n in NAMES]
        if LIST_ON:
            assert c.sparse_list() == (1, launch_shape(3, rows, cols, 24)[0]) and c.sparse_list_rows() == 24


def test_one_captured_graph_replayed_on_frames_in_which_the_object_moves(world, ctx):
    """graph mode on: the lists are device data, made on the list grid by the replayed mark launch -- a frame goes from a list
    to none and back, and the replayed gradient launch follows"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols, ch = GEO["P"]
    e = world["P"]
    c = ctx(32, 4, 18)
    c.set_graph_mode(True)
    calls = [["listed", "moved0", "none"], ["dense", "moved3", "moved2"], ["none", "none", "moved1"], ["moved2", "listed", "dense"]]
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
        if LIST_ON:
            assert c.sparse_list_rows() == 18
    assert c.graph_count() == 1
    d_img.fill_(0xFF)
    torch.cuda.synchronize()
    for b, n in enumerate(calls[-1]):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][n].quantized(0)), n


def child(geo, npz):
    """the child process (SBM_QS_HS=32 and perhaps SBM_SPARSE_LIST_HS in its environment): stream mode, no rows set through the
    API, four batches in flight; the batch on the parent's frames, profiled"""
    rows, cols, ch = GEO[geo]
    fr = np.load(npz)
    c = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0)
    c.upload_templates(load_templates())
    c.set_quantize_mode("stream")
    c.set_pipeline_depth(4)
    run_batch(c, [fr[n] for n in NAMES], thr=THR)
    poison(c, rows, cols)
    c.set_profiling(True)
    lists, _ = run_batch(c, [fr[n] for n in NAMES], thr=THR)
    out = {"lists": lists, "items": c.sparse_items(), "list": c.sparse_list(), "rows": c.sparse_list_rows()}
    c.close()
    print("LISTS " + json.dumps(out))


@pytest.mark.parametrize("list_env", ["0", None, "18"])
def test_the_rule_and_the_environment_in_a_child(world, rects_emu, tmp_path, list_env):
    """SBM_SPARSE_LIST_HS=0: one grid, the figures of the launch before the lists had a grid of their own; unset: the rule on the
    frames of the call (three frames never give a wave per SIMD: the shortest items); 18: that"""
    geo = "P"
    rows, cols, _ = GEO[geo]
    e = world[geo]
    npz = str(tmp_path / "frames.npz")
    np.savez(npz, **{n: e["frames"][n] for n in NAMES})
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), SBM_QS_HS="32")
    env.pop("SBM_SPARSE_LIST_HS", None)
    if list_env is not None:
        env["SBM_SPARSE_LIST_HS"] = list_env
    out = subprocess.run([sys.executable, "-c", "import test_gpu_sparse_list_grids as t, sys; t.child(sys.argv[1], sys.argv[2])", geo, npz],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("LISTS ")][-1][6:])
    assert got["lists"] == [[list(m) for m in e["want"][n]] for n in NAMES]
    if not LIST_ON:
        return
    grid = {"0": 32, None: min(32, throughput_rule(len(NAMES), rows, N_SIMD)), "18": 18}[list_env]
    assert grid == {"0": 32, None: 4, "18": 18}[list_env]
    S, launched = launch_shape(len(NAMES), rows, cols, 32)
    assert got["list"] == [1, S] and got["rows"] == grid and got["items"][0] == 2 and got["items"][2] == launched, got
    assert got["items"][1] == expected_working(rects_emu, world["ts"], e, NAMES, rows, cols, 32, grid) > 0, got
