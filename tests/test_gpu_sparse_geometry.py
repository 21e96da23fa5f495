"""-m gpu: the sparse level-0 path (source pass -> level-1 gradient -> coarse pass -> mark tiles -> gradient of the flagged work
items -> strips of the flagged tiles -> refinement; tests/test_gpu_sparse_gradient.py) at the geometries, caller layouts, batch
shapes and entry points that file does not reach:

  cut tiles     448 x 576 BGR (3.5 x 4.5 tiles of 128 x 128 pixels; the 96-column last strip packed two frames per wave) and
                512 x 704 gray (4 x 5.5 tiles), the object at the centre, against the right and the bottom border, and absent
  layout        rows padded by 13 and 64 bytes, frames padded by 1000 bytes or interleaved with their inverted copies; the
                caller's buffer overwritten before any reader of level 0 runs (the context's retained copy must serve them)
  pack groups   7 frames of 512 x 512 (5 per wave in the packed last strip) that flag different tiles, then 2, then 7 again
  channels      BGR and gray batches in turn on one context, a reader behind each switch
  entry points  sbm_match_device, sbm_match, sbm_match_batch_host (+ _begin / _end, _end_nms), sbm_nms_batch_device behind a
                sparse batch, the one-rank sbm_match_batch_device_sharded
  whole build   one child process with SBM_SPARSE_GRADIENT=0: the same lists

Everything is compared bit for bit with oracle.Pyramid; the streaming kernel is forced (it is not chosen below 4 Mpixel per
launch).  Where the sparse knobs are on, every test that claims the sparse path proves it by the three "k_quantize" launches
of its profiled call."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from shape_based_matching_amd import capi, synth
from shape_based_matching_amd.templates import MATCH_DTYPE, from_pyramids
from test_gpu_nms_device import expected as nms_expected, rows_of, sizes_of
from test_gpu_sparse_gradient import CAP, NT, SPARSE_ON, THR, gradient_launches, load_templates, multiset, shifted
from test_gpu_sparse_gradient import make_frames as square_frames

sys.path.insert(0, os.path.join(ROOT, "tools"))
from fuzz_sequence import padded_layout  # noqa: E402

pytestmark = pytest.mark.gpu
REC = MATCH_DTYPE.itemsize
CUT = {"P": (448, 576, 3), "Q": (512, 704, 1)}  # (cols / 4) % 32 == 16: the last tile column holds 16 cells; P's last tile row too
PLACES = ["centre", "right", "bottom", "absent"]
SPARSE_SEQ = ["k_quantize", "k_quantize", "k_build_lm", "k_similarity_coarse", "k_mark_refine_tiles", "k_quantize", "k_build_lm",
              "k_similarity_local"]
LAYOUTS = [(0, 0), (13, 0), (64, 0), (0, 1000), (0, -1), (13, -1)]  # (row pad, frame pad; -1: a whole, inverted frame between)


def cut_frames(oracle, ts, rows, cols, ch):
    """the case1 image cut to the canvas, and the frame moved so that the best match's box ends 2 px before the right / the
    bottom border (the refinement clamps move every candidate there)"""
    img = np.load(os.path.join(ROOT, "tests", "golden", "case1_test_bgr.npz"))["bgr"]
    tall, wide = max(rows, img.shape[0]), max(cols, img.shape[1])
    big = synth.embed(img, tall, wide, (tall - img.shape[0]) // 2, (wide - img.shape[1]) // 2)
    centre = np.ascontiguousarray(big[(tall - rows) // 2: (tall - rows) // 2 + rows, (wide - cols) // 2: (wide - cols) // 2 + cols])
    absent = synth.scene_bgr(5, rows, cols)
    if ch == 1:
        centre, absent = np.ascontiguousarray(centre[:, :, 1]), np.ascontiguousarray(absent[:, :, 1])
    pyr = oracle.Pyramid.build(centre, [4, 8], 30.0)
    best = max(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, 80.0, n_threads=NT).tolist(), key=lambda m: m[2])
    pyr.free()
    t = [i for i in range(ts.n_templates) if ts.template_id[i] == best[5] and ts.class_idx[i] == best[4]][0]
    x, y, w, h = int(best[0]), int(best[1]), int(ts.levels["width"][t, 0]), int(ts.levels["height"][t, 0])
    return {"centre": centre, "right": shifted(centre, 0, (cols - 2 - (x + w)) // 2 * 2), "bottom": shifted(centre, (rows - 2 - (y + h)) // 2 * 2, 0),
            "absent": absent}


def entry(oracle, ts, frames):
    want, pyrs = {}, {}
    for name, f in frames.items():
        p = oracle.Pyramid.build(f, [4, 8], 30.0)
        want[name] = multiset(p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, THR, n_threads=NT))
        pyrs[name] = p
    return {"frames": frames, "want": want, "pyr": pyrs}


@pytest.fixture(scope="module")
def world(oracle):
    """per geometry the frames, the oracle's pyramids and lists -- computed once, read by every test, never changed"""
    ts = load_templates()
    w = {"ts": ts}
    for g, (rows, cols, ch) in CUT.items():
        w[g] = entry(oracle, ts, cut_frames(oracle, ts, rows, cols, ch))
        for n in ("centre", "right", "bottom"):  # the oracle's lists are not trivial, and the placements differ
            assert len(w[g]["want"][n]) > 20, (g, n)
        assert w[g]["want"]["right"] != w[g]["want"]["centre"] != w[g]["want"]["bottom"], g
    sq = square_frames(512)
    w["S"] = entry(oracle, ts, sq)
    w["Sg"] = entry(oracle, ts, {n: np.ascontiguousarray(f[:, :, 1]) for n, f in sq.items() if n != "left"})
    for g in ("S", "Sg"):
        assert len(w[g]["want"]["centre"]) > 20 and len(w[g]["want"]["border"]) > 20 and w[g]["want"]["border"] != w[g]["want"]["centre"], g
    yield w
    for g in ("P", "Q", "S", "Sg"):
        for p in w[g]["pyr"].values():
            p.free()


@pytest.fixture()
def ctx(world):
    made = []

    def make(hs=18, **kw):
        c = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0, **kw)
        c.upload_templates(world["ts"])
        c.set_quantize_mode("stream", hs)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


def run_batch(c, frames, row_pad=0, frame_pad=0, thr=THR):
    """sbm_match_batch_device on the frames laid out as a caller might (fuzz_sequence.padded_layout), once: the lists, and the
    caller's device buffer"""
    import torch

    dev = torch.device("cuda", 0)
    B = len(frames)
    rows, cols = frames[0].shape[:2]
    ch = 1 if frames[0].ndim == 2 else 3
    buf, stride, fs = padded_layout(frames, row_pad, frame_pad)
    d_img = torch.from_numpy(buf).to(dev)
    d_out = torch.zeros(B * CAP * REC, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(B * 2, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    c.match_batch_device(d_img.data_ptr(), fs, B, rows, cols, stride, ch, thr, d_out.data_ptr(), CAP, d_cnt.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    cnt = d_cnt.cpu().numpy().reshape(B, 2)
    recs = d_out.cpu().numpy().view(MATCH_DTYPE).reshape(B, CAP)
    assert (cnt[:, 1] == 0).all() and (cnt[:, 0] <= CAP).all(), cnt
    return [multiset(recs[b, : cnt[b, 0]]) for b in range(B)], d_img


def assert_sparse_launches(c, whole_sequence=True):
    """the profiled call ran the sparse path: source pass, level 1, and the gradient of the flagged items behind the marks
    (whole_sequence: a device batch call, whose launches are exactly these)"""
    if SPARSE_ON:
        names = [n for n, _ in c.timings()]  # read once: an accumulating profile is cleared by the read
        assert names.count("k_quantize") == 3, names
        # (k_pack_bitplanes: the coarsest level's planes packed by a launch of their own on grids the fused producer does not take)
        seq = [n for n in names if n not in ("k_resize_mask", "k_prep_features", "k_pack_bitplanes")]
        if whole_sequence:
            assert seq == SPARSE_SEQ, seq
        else:
            assert [n for n in seq if n in ("k_quantize", "k_mark_refine_tiles")] == ["k_quantize", "k_quantize", "k_mark_refine_tiles", "k_quantize"], seq


def assert_level0_readers(c, e, names):
    """every frame's whole level-0 map, frame 0's linear memories and the template loop on frame 0"""
    rows, cols = e["frames"][names[0]].shape[:2]
    for b in reversed(range(len(names))):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][names[b]].quantized(0)), b
    lm, want = c.get_linear_memories(0), e["pyr"][names[0]].lm(0)
    assert np.array_equal(lm[:, : rows * cols], want[:, : rows * cols]) and not lm[:, rows * cols:].any()
    assert multiset(c.match_templates(THR)) == e["want"][names[0]]


# ---- cut tiles ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiles_emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("tiles_emu") / "libtiles_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "shape_based_matching_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "emu", "refine_tiles_emu.cpp")])
    L = C.CDLL(so)
    L.sbm_emu_refine_tiles.argtypes = [C.c_int64, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
    L.sbm_emu_refine_tiles.restype = C.c_int
    return L


def flagged_tiles(oracle, tiles_emu, ts, pyr, rows, cols):
    """the union of the refinement footprints (sbm_refine_tiles.h) of the oracle's coarse candidates: the one-level match of the
    templates' level-1 records on the pyramid's level-1 map, at the call's threshold"""
    coarse = from_pyramids([[{"width": int(ts.levels[t, 1]["width"]), "height": int(ts.levels[t, 1]["height"]),
                              "features": np.stack([ts.features[k][int(ts.levels[t, 1]["feature_offset"]):][: int(ts.levels[t, 1]["n_features"])]
                                                    for k in ("x", "y", "label")], axis=1)}] for t in range(ts.n_templates)], "c")
    p1 = oracle.Pyramid.from_quantized([pyr.quantized(1)], [8])
    cands = p1.match(coarse.levels, coarse.features, coarse.class_idx, coarse.template_id, THR, n_threads=NT)
    p1.free()
    assert len(cands) > 0
    tid = np.asarray(cands["template_id"], np.int64)
    cand = np.ascontiguousarray(np.stack([cands["x"], cands["y"], ts.levels["width"][tid, 0], ts.levels["height"][tid, 0]], axis=1).astype(np.int32))
    origin = np.zeros((len(cand), 4), np.int32)
    mask = np.zeros(len(cand), np.uint64)
    # (the fixture's features reach x = width, y = height: one pixel past the declared box)
    n_tiles = tiles_emu.sbm_emu_refine_tiles(len(cand), cand.ctypes.data, rows, cols, 4, cols // 4, rows // 4, 1, origin.ctypes.data, mask.ctypes.data)
    assert n_tiles == ((cols // 4 + 31) // 32) * ((rows // 4 + 31) // 32)
    return int(np.bitwise_or.reduce(mask))


@pytest.mark.parametrize("geo,hs", [("P", 18), ("P", 32), ("Q", 18), ("Q", 32)])
def test_cut_tiles(world, ctx, oracle, tiles_emu, geo, hs):
    rows, cols, _ = CUT[geo]
    e = world[geo]
    n_cb, n_rb = (cols // 4 + 31) // 32, (rows // 4 + 31) // 32
    assert (cols // 4) % 32 == 16 and ((rows // 4) % 32 == 16) == (geo == "P")
    # not vacuous: the border frames' candidates flag the cut last tile column and the last tile row (cut at 448 rows)
    last_col = sum(1 << (ty * n_cb + n_cb - 1) for ty in range(n_rb))
    last_row = sum(1 << ((n_rb - 1) * n_cb + tx) for tx in range(n_cb))
    assert flagged_tiles(oracle, tiles_emu, world["ts"], e["pyr"]["right"], rows, cols) & last_col
    assert flagged_tiles(oracle, tiles_emu, world["ts"], e["pyr"]["bottom"], rows, cols) & last_row
    c = ctx(hs)
    frames = [e["frames"][n] for n in PLACES]
    run_batch(c, frames)  # the first call also prepares the template tables
    c.set_profiling(True)
    got, _ = run_batch(c, frames)
    for n, g in zip(PLACES, got):
        assert g == e["want"][n], (geo, hs, n)
    assert_sparse_launches(c)
    for b, n in enumerate(PLACES):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][n].quantized(0)), (geo, hs, n)


# ---- the caller's layout --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row_pad,frame_pad", LAYOUTS)
@pytest.mark.parametrize("geo", ["S", "P"])
def test_callers_layout_and_an_overwritten_buffer(world, ctx, geo, row_pad, frame_pad):
    import torch

    e = world[geo]
    names = ["border", "centre", "absent"] if geo == "S" else ["right", "bottom", "absent"]
    frames = [e["frames"][n] for n in names]
    assert sum(len(e["want"][n]) for n in names) > 40
    c = ctx(32 if row_pad == 13 else 18)
    packed, _ = run_batch(c, frames)
    c.set_profiling(True)
    got, d_img = run_batch(c, frames, row_pad, frame_pad)
    assert got == packed == [e["want"][n] for n in names]
    assert_sparse_launches(c)
    c.set_profiling(False)
    d_img.fill_(0xFF)  # the call is synchronised: the buffer is the caller's again
    torch.cuda.synchronize()
    assert_level0_readers(c, e, names)


# ---- pack groups ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hs", [18, 32])
def test_pack_groups_with_other_flags_per_frame(world, ctx, hs):
    """7 frames of 512 columns: the 32-column last strip takes 5 frames per wave, so the first group holds frames that flag
    other tiles (and frames that flag none) and the batch ends in a partial group; then 2 frames, a reader, and 7 again on a
    map the stage setter poisoned"""
    e = world["S"]
    seven = ["absent", "centre", "absent", "absent", "border", "absent", "left"]
    two = ["border", "centre"]
    assert len(e["want"]["left"]) > 20 and e["want"]["left"] != e["want"]["centre"]
    c = ctx(hs)
    run_batch(c, [e["frames"][n] for n in seven])
    c.set_profiling(True)
    got, _ = run_batch(c, [e["frames"][n] for n in seven])
    assert got == [e["want"][n] for n in seven]
    assert_sparse_launches(c)
    for b, n in enumerate(seven):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][n].quantized(0)), (b, n)
    got, _ = run_batch(c, [e["frames"][n] for n in two])
    assert got == [e["want"][n] for n in two]
    assert_sparse_launches(c)
    c.set_profiling(False)
    assert_level0_readers(c, e, two)
    poison = (1 << np.random.RandomState(3).randint(0, 8, (512, 512))).astype(np.uint8)
    c.set_quantized(0, poison)
    c.set_profiling(True)
    got, _ = run_batch(c, [e["frames"][n] for n in seven])
    assert got == [e["want"][n] for n in seven]
    assert_sparse_launches(c)
    for b, n in reversed(list(enumerate(seven))):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][n].quantized(0)), (b, n)


# ---- channels -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", ["S", "Sg"])
def test_channel_count_changes_between_a_sparse_call_and_a_reader(world, ctx, first):
    second = "Sg" if first == "S" else "S"
    names = ["centre", "border", "absent"]
    c = ctx(18)
    for g in (first, second):
        e = world[g]
        got, _ = run_batch(c, [e["frames"][n] for n in names])
        assert got == [e["want"][n] for n in names], g
    assert_level0_readers(c, world[second], names)
    # ... and back, profiled, a reader behind it
    c.set_profiling(True)
    e = world[first]
    got, _ = run_batch(c, [e["frames"][n] for n in names[::-1]])
    assert got == [e["want"][n] for n in names[::-1]]
    assert_sparse_launches(c)
    c.set_profiling(False)
    assert_level0_readers(c, e, names[::-1])
    # a host match of a BGR frame behind whatever the last batch was
    s = world["S"]
    c.set_profiling(True)
    assert multiset(c.match(s["frames"]["border"], THR)) == s["want"]["border"]
    assert_sparse_launches(c, False)
    assert np.array_equal(c.get_quantized(0), s["pyr"]["border"].quantized(0))


# ---- entry points ---------------------------------------------------------------------------------------------------------

def test_single_frame_entry_points(world, ctx):
    """sbm_match_device and sbm_match on a cut geometry: three gradient launches each, the oracle's list, the whole map after"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols, ch = CUT["P"]
    e = world["P"]
    c = ctx(18)
    st = torch.cuda.Stream(device=dev)
    d_out = torch.zeros(CAP * REC, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    c.set_profiling(True)
    for n in ("right", "bottom", "absent", "centre"):
        d_img = torch.from_numpy(e["frames"][n]).to(dev)
        torch.cuda.synchronize()
        c.match_device(d_img.data_ptr(), rows, cols, cols * ch, ch, THR, d_out.data_ptr(), CAP, d_cnt.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        cnt = d_cnt.cpu().numpy()
        assert cnt[1] == 0 and multiset(d_out.cpu().numpy().view(MATCH_DTYPE)[: cnt[0]]) == e["want"][n], n
        assert_sparse_launches(c, False)
        d_img.fill_(0xFF)
        torch.cuda.synchronize()
        assert np.array_equal(c.get_quantized(0), e["pyr"][n].quantized(0)), n
    for n in ("bottom", "right"):
        assert multiset(c.match(e["frames"][n], THR)) == e["want"][n], n
        assert_sparse_launches(c, False)
        assert np.array_equal(c.get_quantized_frame(0, 0), e["pyr"][n].quantized(0)), n
        assert multiset(c.match_templates(THR)) == e["want"][n], n


@pytest.mark.parametrize("split", [False, True])
def test_host_batch(world, ctx, split):
    """sbm_match_batch_host in one call and through _begin / _end: one sub-batch is one sparse call"""
    e = world["Q"]
    frames = [e["frames"][n] for n in PLACES]
    c = ctx(32)
    c.match_batch_host(frames, THR, cap=CAP, sub_batch=4, split=split)
    c.set_profiling(True)
    got = c.match_batch_host(frames, THR, cap=CAP, sub_batch=4, split=split)
    assert [multiset(g) for g in got] == [e["want"][n] for n in PLACES]
    assert_sparse_launches(c, False)
    for b, n in enumerate(PLACES):  # one sub-batch: all four frames are resident
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][n].quantized(0)), n
    # two sub-batches of two frames: two sparse calls
    got = c.match_batch_host(frames, THR, cap=CAP, sub_batch=2, split=split)
    assert [multiset(g) for g in got] == [e["want"][n] for n in PLACES]
    if SPARSE_ON:
        assert gradient_launches(c) == 6


def test_nms_forms_behind_a_sparse_call(world, ctx):
    """sbm_match_batch_host_end_nms, and sbm_nms_batch_device on the lists of a sparse sbm_match_batch_device"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols, ch = CUT["P"]
    e = world["P"]
    ts = world["ts"]
    sizes = sizes_of(ts)
    frames = [e["frames"][n] for n in PLACES]
    raw = [np.array([tuple(m) for m in e["want"][n]], MATCH_DTYPE) for n in PLACES]
    c = ctx(18)
    c.set_profiling(True, accumulate=True)  # (the NMS stage clears the timings of a call that does not accumulate)
    kept, counts = c.match_batch_host_nms(frames, THR, 0.0, 0.5, cap=CAP, out_cap=256, sub_batch=4)
    assert_sparse_launches(c, False)
    for f in range(len(frames)):
        assert counts[f, 1] == 0 and rows_of(kept[f]) == rows_of(nms_expected(raw[f], sizes, 0.0, 0.5)), f
    assert sum(len(k) for k in kept) > 0
    # the device form on the caller's stream, right behind the sparse batch call
    B, out_cap = len(frames), 256
    d_img = torch.from_numpy(np.stack(frames)).to(dev)
    d_out = torch.zeros(B * CAP * REC, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(B * 2, dtype=torch.int32, device=dev)
    d_kept = torch.zeros(B * out_cap * REC, dtype=torch.uint8, device=dev)
    d_kc = torch.full((B * 2,), -1, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    c.set_profiling(True, accumulate=True)  # from here
    c.match_batch_device(d_img.data_ptr(), rows * cols * ch, B, rows, cols, cols * ch, ch, THR, d_out.data_ptr(), CAP, d_cnt.data_ptr(),
                         stream=st.cuda_stream)
    c.nms_batch_device(d_out.data_ptr(), d_cnt.data_ptr(), CAP, B, d_kept.data_ptr(), out_cap, d_kc.data_ptr(), 85.0, 0.3, stream=st.cuda_stream)
    st.synchronize()
    assert_sparse_launches(c, False)
    c.set_profiling(False)
    kc = d_kc.cpu().numpy().reshape(B, 2)
    out = d_kept.cpu().numpy().reshape(B, out_cap * REC)
    for f in range(B):
        assert kc[f, 1] == 0 and rows_of(out[f].view(MATCH_DTYPE)[: kc[f, 0]]) == rows_of(nms_expected(raw[f], sizes, 85.0, 0.3)), f
    assert_level0_readers(c, e, PLACES)


def test_one_rank_sharded_batch(world, ctx):
    """sbm_match_batch_device_sharded on a communicator of one rank: the sparse path, the gathered lists are the oracle's"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols, ch = CUT["Q"]
    e = world["Q"]
    frames = [e["frames"][n] for n in PLACES]
    c = ctx(18)
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
        if call == 1:
            c.set_profiling(True)
        c.match_batch_device_sharded(d_img.data_ptr(), rows * cols * ch, B, rows, cols, cols * ch, ch, THR, d_local.data_ptr(), CAP, d_gath.data_ptr(),
                                     stream=st.cuda_stream)
        st.synchronize()
    assert_sparse_launches(c, False)
    buf = d_gath.cpu().numpy()
    cnt = buf[: 8 * B].view(np.int32).reshape(B, 2)
    for f, n in enumerate(PLACES):
        assert cnt[f, 1] == 0 and multiset(buf[hdr + f * CAP * REC: hdr + (f + 1) * CAP * REC].view(MATCH_DTYPE)[: cnt[f, 0]]) == e["want"][n], n
    c.set_profiling(False)
    for b, n in enumerate(PLACES):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][n].quantized(0)), n


# ---- the whole build ------------------------------------------------------------------------------------------------------

def whole_gradient_child(geo):
    """the child process (SBM_SPARSE_GRADIENT=0): the cut-tile batch with level 0's whole gradient in front of the coarse pass"""
    from oracle import oracle as O

    O.build()
    O.lib()
    rows, cols, ch = CUT[geo]
    ts = load_templates()
    fr = cut_frames(O, ts, rows, cols, ch)
    c = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0)
    c.upload_templates(ts)
    c.set_quantize_mode("stream", 18)
    run_batch(c, [fr[n] for n in PLACES])
    c.set_profiling(True)
    lists, _ = run_batch(c, [fr[n] for n in PLACES])
    n = gradient_launches(c)
    c.close()
    print("LISTS " + json.dumps({"lists": lists, "launches": n}))


def test_whole_gradient_in_a_child_gives_the_same_lists(world, ctx):
    e = world["P"]
    got, _ = run_batch(ctx(18), [e["frames"][n] for n in PLACES])
    assert got == [e["want"][n] for n in PLACES]
    env = dict(os.environ, SBM_SPARSE_GRADIENT="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    out = subprocess.run([sys.executable, "-c", "import test_gpu_sparse_geometry as t, sys; t.whole_gradient_child(sys.argv[1])", "P"],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    child = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("LISTS ")][-1][6:])
    assert child["lists"] == [[list(m) for m in l] for l in got]
    assert child["launches"] == 2
