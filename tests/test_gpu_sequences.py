"""-m gpu: call sequences on ONE context (tools/fuzz_sequence.py) and the regressions the sequences found or were written
for: the form state machine of an sbm_ctx (the per-level ``LevelForms`` record of sbm_level_forms.h), the forms rebuilt
lazily by the template loop, and the caller's stream next to the context's own.  Every list against the oracle."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from shape_based_matching_amd import synth
from shape_based_matching_amd.templates import MATCH_DTYPE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = MATCH_DTYPE.itemsize
SPIN = 20_000_000  # clock cycles of torch.cuda._sleep: a few milliseconds of work queued ahead on the caller's stream


def key(recs):
    return sorted(np.ascontiguousarray(recs, MATCH_DTYPE).tolist())


def test_sequence_fuzz_slice():
    """12 sequences x 25 steps: every pyramid, graph mode and an asynchronous stretch in each"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_sequence

    assert fuzz_sequence.run(12, 5, 25, verbose=False) > 2000


def test_sparse_sequence_fuzz_slice():
    """8 sequences x 30 steps of the sparse profile (tests/test_sequence_generator.py counts what the slice contains): the
    (4, 8) pyramid in stream mode, padded and interleaved caller layouts, cut tile columns, readers behind sparse calls and
    behind overwritten caller buffers"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fuzz_sequence

    from test_sequence_generator import SPARSE_SLICE, sparse_counts

    seed, n, steps = SPARSE_SLICE
    assert fuzz_sequence.run(n, seed, steps, verbose=False, profile="sparse") > 2000
    # the calls drawn as profiled ran under sbm_set_profiling: every sparse-eligible one made the sparse path's three
    # gradient launches (the Runner fails on any other count), and the Runner saw as many as the generator drew
    if fuzz_sequence.LAST_RUN["sparse_on"]:
        assert fuzz_sequence.LAST_RUN["sparse_proven"] == sum(sparse_counts(seed, n, steps)["profiled"].values()) >= 8


def big_frames(case1, n=2):
    img = case1["test"]
    offs = [(300, 500), (1500, 1200), (900, 100)]
    return [synth.embed(img, 2048, 2048, *offs[i]) for i in range(n)]


def oracle_lists(oracle, frames, ts, thr, T=(4, 8)):
    out = []
    for fr in frames:
        p = oracle.Pyramid.build(fr, list(T), 30.0)
        out.append(p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, thr, n_threads=min(16, os.cpu_count() or 1)))
        p.free()
    return out


def test_graph_frame_then_template_loop_same_stream(oracle, ctx_factory, case1):
    """(a) graph mode 1: match_device of a 2048 x 2048 BGR frame on a caller stream, at once followed by
    match_templates_device on the same stream, frames alternating, no host synchronisation.  The single-frame replay leaves
    every level in the 8-plane form, so the template loop rebuilds level 0's bit strips from the orientation map first:
    that launch must wait for the caller's stream, where the map of this frame is still being written."""
    import torch

    dev = torch.device("cuda", 0)
    ts = case1["templates"].subset(range(280, 361, 4))
    frames = big_frames(case1)
    thr = 85.0
    want = oracle_lists(oracle, frames, ts, thr)
    assert len(want[0]) > 0 and key(want[0]) != key(want[1])
    ctx = ctx_factory()
    ctx.upload_templates(ts)
    ctx.set_graph_mode(True)
    s = torch.cuda.Stream(device=dev)
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    cap, n_iter = 4096, 8
    outs = [torch.zeros(cap * REC, dtype=torch.uint8, device=dev) for _ in range(2 * n_iter)]
    cnts = [torch.full((2,), -1, dtype=torch.int32, device=dev) for _ in range(2 * n_iter)]
    torch.cuda.synchronize()
    for it in range(n_iter):
        i = it % 2
        with torch.cuda.stream(s):
            torch.cuda._sleep(SPIN)  # the caller's stream is busy: the frame's launches are still queued when the host returns
        ctx.match_device(d_frames[i].data_ptr(), 2048, 2048, 2048 * 3, 3, thr, outs[2 * it].data_ptr(), cap, cnts[2 * it].data_ptr(),
                         stream=s.cuda_stream)
        ctx.match_templates_device(thr, outs[2 * it + 1].data_ptr(), cap, cnts[2 * it + 1].data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    for it in range(n_iter):
        for j, what in ((0, "match_device"), (1, "match_templates_device")):
            c = cnts[2 * it + j].cpu().numpy()
            got = outs[2 * it + j].cpu().numpy().view(MATCH_DTYPE)[: max(c[0], 0)]
            assert c[1] == 0 and key(got) == key(want[it % 2]), (it, what, int(c[0]), len(want[it % 2]))


@pytest.mark.parametrize("graph", [None, True])
def test_bits_only_batch_then_byte_template_loop(oracle, ctx_factory, case1, graph):
    """(a), second instance: a batch call builds the coarsest level as bit planes only; after set_coarse_mode("bytes") the
    template loop (pipeline depth 2, graph path) rebuilds its response planes from the orientation map -- after the batch
    on the caller's stream, not beside it."""
    import torch

    dev = torch.device("cuda", 0)
    ts = case1["templates"].subset(range(280, 361, 4))
    frames = big_frames(case1, 3)
    thr = 85.0
    want = oracle_lists(oracle, frames, ts, thr)
    ctx = ctx_factory()
    ctx.upload_templates(ts)
    ctx.set_pipeline_depth(2)
    ctx.set_graph_mode(graph)
    s = torch.cuda.Stream(device=dev)
    batches = [torch.from_numpy(np.stack([frames[i], frames[(i + 1) % 3]])).to(dev) for i in range(3)]
    fs = 2048 * 2048 * 3
    cap, n_iter = 4096, 6
    outs = [torch.zeros(3 * cap * REC, dtype=torch.uint8, device=dev) for _ in range(n_iter)]
    cnts = [torch.full((6,), -1, dtype=torch.int32, device=dev) for _ in range(n_iter)]
    torch.cuda.synchronize()
    for it in range(n_iter):
        i = it % 3
        ctx.set_coarse_mode("auto")
        with torch.cuda.stream(s):
            torch.cuda._sleep(SPIN)
        ctx.match_batch_device(batches[i].data_ptr(), fs, 2, 2048, 2048, 2048 * 3, 3, thr, outs[it].data_ptr(), cap, cnts[it].data_ptr() + 8,
                               stream=s.cuda_stream)
        ctx.set_coarse_mode("bytes")
        ctx.match_templates_device(thr, outs[it].data_ptr() + 2 * cap * REC, cap, cnts[it].data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    for it in range(n_iter):
        i = it % 3
        c = cnts[it].cpu().numpy().reshape(3, 2)
        o = outs[it].cpu().numpy().reshape(3, cap * REC)
        for f, w in ((1, want[i]), (2, want[(i + 1) % 3])):
            assert c[f, 1] == 0 and key(o[f - 1].view(MATCH_DTYPE)[: c[f, 0]]) == key(w), (it, "batch frame", f - 1)
        assert c[0, 1] == 0 and key(o[2].view(MATCH_DTYPE)[: c[0, 0]]) == key(want[i]), (it, "template loop", int(c[0, 0]), len(want[i]))


def test_host_entry_points_after_device_call_on_caller_stream(oracle, ctx_factory, case1):
    """a device call on a caller stream, then at once a host-memory entry point or stage read on the same context (found by
    the sequence fuzzer: stall, match_device, match_templates).  The host calls run on the context's own stream and must
    still see this frame's pyramid: sbm_match_templates, sbm_get_quantized, and sbm_match / sbm_build_pyramid /
    sbm_set_quantized, which overwrite the buffers the device call is still using."""
    import torch

    dev = torch.device("cuda", 0)
    ts = case1["templates"].subset(range(280, 361, 4))
    frames = big_frames(case1)
    thr = 85.0
    pyrs = [oracle.Pyramid.build(fr, [4, 8], 30.0) for fr in frames]
    want = [p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, thr, n_threads=min(16, os.cpu_count() or 1)) for p in pyrs]
    assert key(want[0]) != key(want[1])
    ctx = ctx_factory()
    ctx.upload_templates(ts)
    s = torch.cuda.Stream(device=dev)
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    cap = 4096
    out = torch.zeros(cap * REC, dtype=torch.uint8, device=dev)
    cnt = torch.full((2,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def device_call(i):
        with torch.cuda.stream(s):
            torch.cuda._sleep(SPIN)
        ctx.match_device(d_frames[i].data_ptr(), 2048, 2048, 2048 * 3, 3, thr, out.data_ptr(), cap, cnt.data_ptr(), stream=s.cuda_stream)

    for it in range(4):
        i = it % 2
        device_call(i)
        assert key(ctx.match_templates(thr)) == key(want[i]), (it, "match_templates")
        device_call(i)
        assert np.array_equal(ctx.get_quantized(0), pyrs[i].quantized(0)), (it, "get_quantized")
        device_call(i)
        assert key(ctx.match(frames[1 - i], thr)) == key(want[1 - i]), (it, "match")
        s.synchronize()
        c = cnt.cpu().numpy()
        assert c[1] == 0 and key(out.cpu().numpy().view(MATCH_DTYPE)[: c[0]]) == key(want[i]), (it, "match_device beside sbm_match")
        device_call(i)
        for l in range(2):
            ctx.set_quantized(l, pyrs[1 - i].quantized(l))
        s.synchronize()
        c = cnt.cpu().numpy()
        assert c[1] == 0 and key(out.cpu().numpy().view(MATCH_DTYPE)[: c[0]]) == key(want[i]), (it, "match_device beside set_quantized")
        assert key(ctx.match_templates(thr)) == key(want[1 - i]), (it, "template loop on set_quantized maps")
    for p in pyrs:
        p.free()


@pytest.mark.parametrize("graph", [True, False])
def test_empty_selection_match_leaves_no_stale_bit_planes(oracle, ctx_factory, case1, graph):
    """found by the sequence fuzzer: a single-frame match with an empty template selection skips the coarse pass, which
    is where the bit planes of the 8-plane form are packed.  The graph path still marked them current, so the next
    template loop on bit planes read the previous frame's planes."""
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_coarse_bits import packed

    from shape_based_matching_amd import capi

    dev = torch.device("cuda", 0)
    ts = case1["templates"].subset(range(280, 361, 4))
    base = synth.embed(case1["test"], 640, 768, 80, 80)
    frames = [base, np.ascontiguousarray(base[::-1, ::-1])]
    thr = 80.0
    pyrs = [oracle.Pyramid.build(fr, [4, 8], 30.0) for fr in frames]
    want = [p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, thr) for p in pyrs]
    assert len(want[1]) > 0 and key(want[0]) != key(want[1])
    ctx = ctx_factory()
    ctx.upload_templates(ts)
    ctx.set_graph_mode(graph)
    s = torch.cuda.Stream(device=dev)
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    cap = 2048
    out = torch.zeros(cap * REC, dtype=torch.uint8, device=dev)
    cnt = torch.full((2,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for rep in range(2):
        ctx.match_device(d_frames[0].data_ptr(), 640, 768, 768 * 3, 3, thr, out.data_ptr(), cap, cnt.data_ptr(), stream=s.cuda_stream)
        ctx.select_templates([])
        ctx.match_device(d_frames[1].data_ptr(), 640, 768, 768 * 3, 3, thr, out.data_ptr(), cap, cnt.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        assert cnt.cpu().numpy().tolist() == [0, 0]
        try:
            planes = ctx.get_coarse_bitplanes()
        except capi.SbmError as e:
            assert e.code == -4
        else:
            assert np.array_equal(planes, packed(pyrs[1].lm(1))), rep
        ctx.select_range(0, ts.n_templates)
        assert key(ctx.match_templates(thr)) == key(want[1]), rep
    for p in pyrs:
        p.free()


_CHILD = textwrap.dedent("""
    import os, sys
    import numpy as np
    import torch
    sys.path.insert(0, {root!r})
    from oracle import oracle as O
    from shape_based_matching_amd import capi, synth
    from shape_based_matching_amd.templates import MATCH_DTYPE, TemplateSet

    O.build(); O.lib()
    ts = TemplateSet.load_npz(os.path.join({root!r}, "tests", "golden", "case1_templates.npz")).subset(range(280, 361, 2))
    img = np.load(os.path.join({root!r}, "tests", "golden", "case1_test_bgr.npz"))["bgr"]
    frame = synth.embed(img, 640, 768, 80, 80)
    pyr = O.Pyramid.build(frame, [4, 8], 30.0)
    want = pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, 88.0)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    out = torch.full((4096 * MATCH_DTYPE.itemsize,), 0x5a, dtype=torch.uint8, device=dev)
    cnt = torch.full((2,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0)
    ctx.set_graph_mode({graph})
    ctx.upload_templates(ts)
    for l in range(2):
        ctx.set_quantized(l, pyr.quantized(l))
    ctx.match_templates_device(88.0, out.data_ptr(), 4096, cnt.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    c = cnt.cpu().numpy()
    got = out.cpu().numpy().view(MATCH_DTYPE)[: max(int(c[0]), 0)]
    key = lambda r: sorted(np.ascontiguousarray(r, MATCH_DTYPE).tolist())
    assert len(want) > 0
    assert c[1] == 0 and c[0] == len(want) and key(got) == key(want), (c.tolist(), len(want))
    ctx.close()
    print("child ok", len(want))
""")


@pytest.mark.parametrize("graph", [False, True])
def test_first_call_template_loop_in_fresh_process(oracle, graph):
    """(b) the zero-fill path: in a fresh process and a fresh context the FIRST device call is the template loop on a
    pyramid set by set_quantized, on a caller non-blocking stream (the counters' zeroing must be ordered before it)"""
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, graph=graph)], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


BATCH_FORMS = [(None, "auto"), (False, "auto"), (True, "bits"), (None, "bytes"), (True, "block")]  # (set_refine_bits, set_coarse_mode)


@pytest.mark.parametrize("refine_bits,coarse", BATCH_FORMS)
def test_forms_after_batch_graph_replay(oracle, ctx_factory, case1, refine_bits, coarse):
    """(c) pipeline depth 2, automatic graphs: the same batch tuple until it replays, then every stage read and the template
    loop against the oracle -- the flags the replay leaves must describe what the captured launches built"""
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_coarse_bits import packed

    dev = torch.device("cuda", 0)
    ts = case1["templates"].subset(range(280, 361, 3))
    base = synth.embed(case1["test"], 640, 768, 80, 80)
    frames = [np.roll(base, 96, axis=1), base, np.ascontiguousarray(base[::-1])]
    thr = 86.0
    ctx = ctx_factory()
    ctx.upload_templates(ts)
    ctx.set_pipeline_depth(2)
    ctx.set_graph_mode(None)
    ctx.set_refine_bits(refine_bits)
    ctx.set_coarse_mode(coarse)
    s = torch.cuda.Stream(device=dev)
    d_imgs = torch.from_numpy(np.stack(frames)).to(dev)
    cap = 2048
    d_out = torch.zeros(3 * cap * REC, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(6, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for _ in range(4):
        ctx.match_batch_device(d_imgs.data_ptr(), 640 * 768 * 3, 3, 640, 768, 768 * 3, 3, thr, d_out.data_ptr(), cap, d_cnt.data_ptr(),
                               stream=s.cuda_stream)
    s.synchronize()
    # auto mode captures a tuple at its second sighting and launches the graph from then on: calls 2..4 ran as graph launches
    assert ctx.graph_count() >= 1, "the batch tuple was never captured, so no call ran as a graph launch"
    pyr = oracle.Pyramid.build(frames[0], [4, 8], 30.0)
    want = pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, thr)
    cnt = d_cnt.cpu().numpy().reshape(3, 2)
    assert cnt[0, 1] == 0 and key(d_out.cpu().numpy()[: cap * REC].view(MATCH_DTYPE)[: cnt[0, 0]]) == key(want)
    if coarse in ("auto", "bits"):
        assert np.array_equal(ctx.get_coarse_bitplanes(), packed(pyr.lm(1)))
    for l in range(2):
        assert np.array_equal(ctx.get_linear_memories(l), pyr.lm(l)), l
    for t, l, cx, cy in ((0, 0, 300, 200), (5, 0, 401, 333), (9, 1, 150, 100)):
        assert np.array_equal(ctx.similarity_local(l, t, cx, cy), pyr.similarity_local(ts.levels[t, l], ts.features, l, cx, cy)), (t, l)
    one = torch.full((cap * REC,), 0x5a, dtype=torch.uint8, device=dev)
    one_cnt = torch.full((2,), -1, dtype=torch.int32, device=dev)
    for _ in range(3):  # the template loop's own capture replays too
        ctx.match_templates_device(thr, one.data_ptr(), cap, one_cnt.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    c = one_cnt.cpu().numpy()
    assert c[1] == 0 and key(one.cpu().numpy().view(MATCH_DTYPE)[: c[0]]) == key(want)
    assert key(ctx.match_templates(thr)) == key(want)
    pyr.free()


# ---- the record a graph replay leaves (csrc/sbm_call_record.h) ----------------------------------------------------------
RECORD_GEO = (448, 576, 3)  # tests/test_gpu_sparse_list.py's "P": the smallest sparse-eligible two-level T = 4 geometry there
RECORD_THR = 75.0
RECORD_NAMES = ["centre", "right", "absent"]


@pytest.fixture(scope="module")
def record_world(oracle):
    """the frames of RECORD_GEO, their per-frame masks and the oracle's lists without and with them -- computed once, never changed"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_sparse_geometry import cut_frames
    from test_gpu_sparse_gradient import load_templates

    rows, cols, ch = RECORD_GEO
    ts = load_templates()
    fr = cut_frames(oracle, ts, rows, cols, ch)
    frames = np.stack([fr[n] for n in RECORD_NAMES])
    masks = np.zeros((len(frames), rows, cols), np.uint8)
    for b in range(len(frames)):
        masks[b, 100 + 40 * b:, 90:] = 255  # (cuts a part of the object: another list, not an empty one)
    want = {}
    for name, ms in (("plain", [None] * len(frames)), ("masked", masks)):
        want[name] = []
        for f, m in zip(frames, ms):
            p = oracle.Pyramid.build(f, [4, 8], 30.0, mask=m)
            want[name].append(key(p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, RECORD_THR, n_threads=min(16, os.cpu_count() or 1))))
            p.free()
    assert 20 < len(want["plain"][0]) < 4096 and want["plain"][0] != want["plain"][1]
    assert want["masked"][0] not in ([], want["plain"][0]) and want["masked"][1] not in ([], want["plain"][1])
    return {"ts": ts, "frames": frames, "masks": masks, "want": want}


def call_record(ctx, frames):
    """everything the accessors tell of what the last call left and launched; level 0's map of the last frame is read last
    (the read completes a map that a sparse call left in pieces)"""
    from shape_based_matching_amd import capi

    rec = {("level_build", l): ctx.level_build(l) for l in range(2)}
    rec.update({"coarse_form": ctx.coarse_form(), ("refine_form", 0): ctx.refine_form(0), "source_form": ctx.source_form(),
                "sparse_items": ctx.sparse_items(), "sparse_list": ctx.sparse_list()})
    rec["last map"] = ctx.get_quantized_frame(0, frames - 1).tobytes()
    with pytest.raises(capi.SbmError):  # ... and the batch had no more frames than these
        ctx.get_quantized_frame(0, frames)
    return rec


@pytest.mark.parametrize("refine_bits,coarse,variant", [(r, c, "plain") for r, c in BATCH_FORMS] +
                         [(None, "auto", "empty"), (None, "auto", "masked"), (None, "auto", "any")])
def test_replay_leaves_the_record_of_the_plain_call(oracle, ctx_factory, record_world, refine_bits, coarse, variant):
    """The same batch call on two fresh contexts, as plain launches (graph mode 0) and as capture then replay (graph mode 1),
    with a plain call of one frame in between (a batch of one frame is never captured): afterwards both contexts tell the
    same of every level's build and current forms, the coarse, refinement and source forms, the sparse launch's selection,
    items launched and lists, and the last frame's level-0 map -- and the lists are the oracle's.  variant: empty -- no
    template selected; masked -- a mask per frame (level 0 built whole); any -- the (5, 8) pyramid of k_build_lm_any."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import any_geometry_cases as AG
    from test_gpu_batch_any_geometry import Batch
    from test_gpu_sparse_gradient import SPARSE_ON

    if variant == "any":
        case = AG.case(oracle, "bgr_5_8")
        T, ts, frames, thr = case.T, case.ts, case.frames[:3], AG.THRS[0]
        want = [case.want(f, thr) for f in range(3)]
        assert sum(len(w) for w in want) > 0
    else:
        T, ts, frames, thr = (4, 8), record_world["ts"], record_world["frames"], RECORD_THR
        want = [[]] * 3 if variant == "empty" else record_world["want"]["masked" if variant == "masked" else "plain"]
    rows, cols = frames[0].shape[:2]
    recs = []
    for graph in (False, True):
        import torch

        ctx = ctx_factory(T=T)
        ctx.upload_templates(ts)
        if variant != "any":
            ctx.set_quantize_mode("stream", 32)  # (a batch this small takes the tile kernel otherwise: no sparse level 0)
        ctx.set_graph_mode(graph)
        ctx.set_refine_bits(refine_bits)
        ctx.set_coarse_mode(coarse)
        if variant == "empty":
            ctx.select_templates([])
        batch, one = Batch(frames), Batch(frames[:1])
        d_masks = torch.from_numpy(record_world["masks"]).to(torch.device("cuda", 0)) if variant == "masked" else None
        stride = rows * cols if variant == "masked" else None
        batch.run(ctx, thr, d_masks, stride)  # graph mode 1: the capture
        one.run(ctx, thr)                     # plain launches on either context
        got = batch.run(ctx, thr, d_masks, stride)  # graph mode 1: the replay
        assert ctx.graph_count() == (1 if graph else 0), graph
        assert got == want, (graph, [len(g) for g in got])
        recs.append(call_record(ctx, len(frames)))
    plain, replay = recs
    for field in plain:
        assert replay[field] == plain[field], (field, plain[field] if field != "last map" else "", replay[field] if field != "last map" else "")
    assert plain["sparse_items"][1] == -1  # working items are counted under profiling only
    if variant == "plain" and (refine_bits, coarse) == (None, "auto") and SPARSE_ON:
        assert plain["source_form"] != 0 and plain["sparse_items"][0] != 0 and plain["sparse_items"][2] > 0  # the sparse level-0 path ran
    if variant in ("masked", "any"):
        assert plain["source_form"] == 0 and plain["sparse_items"] == (0, -1, 0) and plain["sparse_list"] == (0, 0)
    if variant == "any":
        assert plain["level_build", 0][2] == plain["level_build", 1][2] == 2  # k_build_lm_any made both levels


def test_template_loop_replay_reports_no_source_pass(oracle, ctx_factory, record_world):
    """The template loop has no source pass: the replay of its captured graph leaves source_form as the context has it.  A
    sparse batch (a source pass), the loop captured, a masked batch (level 0 whole: no source pass), the loop replayed."""
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_batch_any_geometry import CAP, Batch
    from test_gpu_sparse_gradient import SPARSE_ON

    dev = torch.device("cuda", 0)
    rows, cols, _ = RECORD_GEO
    w = record_world
    ctx = ctx_factory()
    ctx.upload_templates(w["ts"])
    ctx.set_quantize_mode("stream", 32)
    ctx.set_pipeline_depth(2)
    ctx.set_graph_mode(True)
    batch = Batch(w["frames"])
    d_masks = torch.from_numpy(w["masks"]).to(dev)
    one = torch.zeros(CAP * REC, dtype=torch.uint8, device=dev)
    one_cnt = torch.zeros(2, dtype=torch.int32, device=dev)

    def template_loop():
        ctx.match_templates_device(RECORD_THR, one.data_ptr(), CAP, one_cnt.data_ptr(), stream=batch.stream.cuda_stream)
        batch.stream.synchronize()
        c = one_cnt.cpu().numpy()
        assert c[1] == 0
        return key(one.cpu().numpy().view(MATCH_DTYPE)[: c[0]])

    # (the first call with a mask per frame sizes the levels' mask buffers, which drops every captured graph: have it done)
    assert batch.run(ctx, RECORD_THR, d_masks, rows * cols) == w["want"]["masked"]
    assert batch.run(ctx, RECORD_THR) == w["want"]["plain"]
    if SPARSE_ON:
        assert ctx.source_form() != 0
    assert template_loop() == w["want"]["plain"][0]  # (frame 0 of the batch: what the forms rebuilt on demand cover)
    assert batch.run(ctx, RECORD_THR, d_masks, rows * cols) == w["want"]["masked"]
    assert ctx.source_form() == 0
    n_graphs = ctx.graph_count()
    assert template_loop() == w["want"]["masked"][0]
    assert ctx.graph_count() == n_graphs, "the template loop was captured again instead of replayed"
    assert ctx.source_form() == 0
