"""-m gpu: the retained copy of level 0's source is stored by the last match call enqueued on a context only, and the call's own
sparse gradient launch reads the caller's frames (sbm_get_source_retention).

  geometries  3 frames of 448 x 576 x 3 and of 512 x 704 x 1, two sets of them, A and B; the streaming kernel forced
  one call    synchronise, overwrite the caller's buffer, read every frame's level-0 map: retention {1, 0}
  burst       four calls A B A B on one stream with no host wait between them, behind a bounded delay on that stream, so that the
              host is ahead of the device: every list is right, level 0's maps are the last call's after both buffers were
              overwritten, and of the four calls at least one stored its copy, at least one did not
  replay      the same burst through ONE captured graph (one input buffer that a copy on the stream refills): the decision
              follows the counters, not the capture
  readers     a call on other frames, a match call, the template loop on the device with no host wait, another match call, all
              behind the delay: the loop's list is the second call's, which only the reader's host wait makes so; a sparse call and a masked (whole-build) call behind it with no wait: level 0's map is the second call's
  layouts     rows padded by 13 bytes, and a table of frame pointers, which always stores the copy
  knob        a child process with SBM_RETAIN_ALWAYS=1: four unwaited calls, retention {4, 0}
Everything is compared bit for bit with oracle.Pyramid.  No test waits on anything unbounded."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from shape_based_matching_amd import capi
from shape_based_matching_amd.templates import MATCH_DTYPE
from test_gpu_sparse_geometry import cut_frames, entry
from test_gpu_sparse_gradient import CAP, NT, SPARSE_ON, THR, load_templates, multiset

sys.path.insert(0, os.path.join(ROOT, "tools"))
from fuzz_sequence import padded_layout  # noqa: E402

pytestmark = pytest.mark.gpu
REC = MATCH_DTYPE.itemsize
GEO = {"P": (448, 576, 3), "Q": (512, 704, 1)}
SETS = {"A": ["right", "bottom", "absent"], "B": ["centre", "absent", "right"]}
RETAIN_ALWAYS = os.environ.get("SBM_RETAIN_ALWAYS", "0") not in ("", "0")
SLEEP_CYCLES = 4_000_000  # torch.cuda._sleep: about 20 ms of device time, whichever of the two clocks the build counts
NO_SLEEP = "this torch has no torch.cuda._sleep: nothing holds the device back while the host enqueues, the counts are not asserted"


@pytest.fixture(scope="module")
def world(oracle):
    """per geometry the frames, the oracle's pyramids and lists -- computed once, read by every test, never changed"""
    ts = load_templates()
    w = {"ts": ts}
    for g, (rows, cols, ch) in GEO.items():
        w[g] = entry(oracle, ts, cut_frames(oracle, ts, rows, cols, ch))
        assert len(w[g]["want"]["right"]) > 20 and len(w[g]["want"]["centre"]) > 20 and w[g]["want"]["right"] != w[g]["want"]["centre"], g
    yield w
    for g in GEO:
        for p in w[g]["pyr"].values():
            p.free()


@pytest.fixture()
def ctx(world):
    made = []

    def make(hs=18):
        c = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0)
        c.upload_templates(world["ts"])
        c.set_quantize_mode("stream", hs)  # (the streaming kernel is not chosen below 4 Mpixel per launch)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


class Call:
    """the device buffers of one batch call: the frames in a caller's layout, the lists, the counts"""

    def __init__(self, frames, row_pad=0, frame_pad=0):
        import torch

        self.dev = torch.device("cuda", 0)
        self.B = len(frames)
        self.rows, self.cols = frames[0].shape[:2]
        self.ch = 1 if frames[0].ndim == 2 else 3
        buf, self.stride, self.fs = padded_layout(frames, row_pad, frame_pad)
        self.d_img = torch.from_numpy(buf).to(self.dev)
        self.d_out = torch.zeros(self.B * CAP * REC, dtype=torch.uint8, device=self.dev)
        self.d_cnt = torch.full((self.B * 2,), -1, dtype=torch.int32, device=self.dev)

    def enqueue(self, c, st, d_img=None):
        img = self.d_img if d_img is None else d_img
        c.match_batch_device(img.data_ptr(), self.fs, self.B, self.rows, self.cols, self.stride, self.ch, THR, self.d_out.data_ptr(), CAP,
                             self.d_cnt.data_ptr(), stream=st.cuda_stream)

    def lists(self, d_out=None, d_cnt=None):
        cnt = (self.d_cnt if d_cnt is None else d_cnt).cpu().numpy().reshape(self.B, 2)
        recs = (self.d_out if d_out is None else d_out).cpu().numpy().view(MATCH_DTYPE).reshape(self.B, CAP)
        assert (cnt[:, 1] == 0).all() and (cnt[:, 0] >= 0).all() and (cnt[:, 0] <= CAP).all(), cnt
        return [multiset(recs[b, : cnt[b, 0]]) for b in range(self.B)]


def hold_device(st):
    """a bounded delay on the stream, so that the calls enqueued behind it are all enqueued before the first one runs"""
    import torch

    if not hasattr(torch.cuda, "_sleep"):
        return False
    with torch.cuda.stream(st):
        torch.cuda._sleep(SLEEP_CYCLES)
    return True


def assert_burst_counts(before, after, held, n):
    retained, skipped = after[0] - before[0], after[1] - before[1]
    if not SPARSE_ON:
        return
    assert retained + skipped == n, (before, after)
    if RETAIN_ALWAYS:
        assert (retained, skipped) == (n, 0)
        return
    if not held:
        pytest.skip(NO_SLEEP)
    assert retained >= 1 and skipped >= 1, (before, after)


def want_of(e, names):
    return [e["want"][n] for n in names]


def assert_level0(c, e, names):
    for b in reversed(range(len(names))):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][names[b]].quantized(0)), (b, names[b])


@pytest.mark.parametrize("geo", list(GEO))
def test_one_call_keeps_its_copy(world, ctx, geo):
    import torch

    e = world[geo]
    c = ctx()
    assert c.source_retention() == (0, 0)
    call = Call([e["frames"][n] for n in SETS["A"]])
    st = torch.cuda.Stream(device=call.dev)
    torch.cuda.synchronize()
    call.enqueue(c, st)
    st.synchronize()
    assert call.lists() == want_of(e, SETS["A"])
    call.d_img.fill_(0xFF)  # the call is synchronised: the buffer is the caller's again
    torch.cuda.synchronize()
    assert_level0(c, e, SETS["A"])
    assert c.source_retention() == ((1, 0) if SPARSE_ON else (0, 0))


@pytest.mark.parametrize("geo", list(GEO))
def test_a_burst_of_calls_keeps_the_last_copy(world, ctx, geo):
    import torch

    e = world[geo]
    c = ctx()
    order = ["A", "B", "A", "B"]
    calls = [Call([e["frames"][n] for n in SETS[s]]) for s in order]
    for k in (2, 3):  # two input buffers, A's and B's, each read by two calls
        calls[k].d_img = calls[k - 2].d_img
    st = torch.cuda.Stream(device=calls[0].dev)
    warm = Call([e["frames"][n] for n in SETS["B"]])
    warm.enqueue(c, st)  # the first call also prepares the template tables, with waits of its own
    st.synchronize()
    before = c.source_retention()
    held = hold_device(st)
    for call in calls:
        call.enqueue(c, st)
    st.synchronize()
    for s, call in zip(order, calls):
        assert call.lists() == want_of(e, SETS[s]), s
    calls[0].d_img.fill_(0xFF)
    calls[1].d_img.fill_(0xFF)
    torch.cuda.synchronize()
    after = c.source_retention()
    assert_level0(c, e, SETS["B"])  # the last call's
    assert c.source_retention() == after  # a reader is no call
    assert_burst_counts(before, after, held, 4)


@pytest.mark.parametrize("geo", list(GEO))
def test_a_burst_through_one_replayed_graph_follows_the_counters(world, ctx, geo):
    import torch

    e = world[geo]
    c = ctx()
    c.set_graph_mode(True)
    c.set_pipeline_depth(2)
    order = ["A", "B", "A", "B"]
    src = {s: Call([e["frames"][n] for n in SETS[s]]) for s in SETS}
    call = src["A"]  # the one argument tuple: its input buffer is refilled on the stream, its lists are copied out on the stream
    d_in = torch.empty_like(call.d_img)
    st = torch.cuda.Stream(device=call.dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        d_in.copy_(src["B"].d_img)
    call.enqueue(c, st, d_in)  # captured here
    st.synchronize()
    assert call.lists() == want_of(e, SETS["B"])
    graphs = c.graph_count()
    assert graphs == 1
    before = c.source_retention()
    held = hold_device(st)
    got = []
    for s in order:
        with torch.cuda.stream(st):
            d_in.copy_(src[s].d_img, non_blocking=True)
        call.enqueue(c, st, d_in)
        with torch.cuda.stream(st):
            got.append((call.d_out.clone(), call.d_cnt.clone()))
    st.synchronize()
    assert c.graph_count() == graphs  # one graph, replayed
    for s, (d_out, d_cnt) in zip(order, got):
        assert call.lists(d_out, d_cnt) == want_of(e, SETS[s]), s
    d_in.fill_(0xFF)
    for s in SETS:
        src[s].d_img.fill_(0xFF)
    torch.cuda.synchronize()
    after = c.source_retention()
    assert_level0(c, e, SETS["B"])
    assert_burst_counts(before, after, held, 4)


@pytest.mark.parametrize("geo", list(GEO))
def test_the_template_loop_between_two_calls_reads_the_first_calls_pyramid(world, ctx, geo):
    """Behind the delay: a call x on other frames, the call a, the template loop, a call b -- none waited for by the test.  The
    loop's reader of level 0 (ensure_level0_map) waits for a on the host.  Without that wait the host would have enqueued b
    while the device is still held: x's strip builder would see b enqueued, a's source pass would leave the copy unwritten, and
    the loop would read x's frames out of the copy -- another list (the sets' first frames differ).  With it, a runs as the last
    call enqueued: all three calls keep their copies."""
    import torch

    e = world[geo]
    assert e["want"][SETS["A"][0]] != e["want"][SETS["B"][0]]
    c = ctx()
    x, a, b = (Call([e["frames"][n] for n in SETS[s]]) for s in ("B", "A", "B"))
    st = torch.cuda.Stream(device=a.dev)
    a.enqueue(c, st)  # (prepares the template tables)
    st.synchronize()
    d_out = torch.zeros(CAP * REC, dtype=torch.uint8, device=a.dev)
    d_cnt = torch.full((2,), -1, dtype=torch.int32, device=a.dev)
    before = c.source_retention()
    hold_device(st)  # (the host is ahead of the device while it enqueues)
    x.enqueue(c, st)
    a.enqueue(c, st)
    c.match_templates_device(THR, d_out.data_ptr(), CAP, d_cnt.data_ptr(), stream=st.cuda_stream)  # no host wait of the test's
    b.enqueue(c, st)
    st.synchronize()
    cnt = d_cnt.cpu().numpy()
    assert cnt[1] == 0 and multiset(d_out.cpu().numpy().view(MATCH_DTYPE)[: cnt[0]]) == e["want"][SETS["A"][0]]
    assert x.lists() == want_of(e, SETS["B"]) and a.lists() == want_of(e, SETS["A"]) and b.lists() == want_of(e, SETS["B"])
    for call in (x, a, b):
        call.d_img.fill_(0xFF)
    torch.cuda.synchronize()
    after = c.source_retention()
    assert_level0(c, e, SETS["B"])
    if SPARSE_ON:
        assert (after[0] - before[0], after[1] - before[1]) == (3, 0)  # a was the last call enqueued when it ran, b is, x saw nothing


def test_a_masked_call_behind_a_sparse_call(world, ctx, oracle):
    import torch

    rows, cols, ch = GEO["P"]
    e = world["P"]
    c = ctx()
    a, b = Call([e["frames"][n] for n in SETS["A"]]), Call([e["frames"][n] for n in SETS["B"]])
    mask = np.zeros((rows, cols), np.uint8)
    mask[:, cols // 3:] = 255
    d_mask = torch.from_numpy(mask).to(a.dev)
    pyrs = [oracle.Pyramid.build(e["frames"][n], [4, 8], 30.0, mask=mask) for n in SETS["B"]]
    try:
        ts = world["ts"]
        want = [multiset(p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, THR, n_threads=NT)) for p in pyrs]
        st = torch.cuda.Stream(device=a.dev)
        a.enqueue(c, st)
        st.synchronize()
        before = c.source_retention()
        hold_device(st)
        a.enqueue(c, st)
        c.match_batch_device_masked(b.d_img.data_ptr(), b.fs, b.B, rows, cols, b.stride, ch, d_mask.data_ptr(), 0, THR, b.d_out.data_ptr(), CAP,
                                    b.d_cnt.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        assert a.lists() == want_of(e, SETS["A"]) and b.lists() == want
        assert c.source_form() == 0  # masks: level 0's whole gradient
        a.d_img.fill_(0xFF)
        b.d_img.fill_(0xFF)
        torch.cuda.synchronize()
        for f in reversed(range(b.B)):
            assert np.array_equal(c.get_quantized_frame(0, f), pyrs[f].quantized(0)), f
        after = c.source_retention()
        assert after[0] + after[1] == before[0] + before[1] + (1 if SPARSE_ON else 0)  # the whole-build call counts in neither
    finally:
        for p in pyrs:
            p.free()


def test_a_padded_layout_and_a_table_of_frame_pointers(world, ctx):
    import torch

    rows, cols, ch = GEO["P"]
    e = world["P"]
    c = ctx(32)
    padded = Call([e["frames"][n] for n in SETS["A"]], 13, 0)
    st = torch.cuda.Stream(device=padded.dev)
    padded.enqueue(c, st)
    st.synchronize()
    assert padded.lists() == want_of(e, SETS["A"])
    padded.d_img.fill_(0xFF)
    torch.cuda.synchronize()
    assert_level0(c, e, SETS["A"])
    base = c.source_retention()
    assert base == ((1, 0) if SPARSE_ON else (0, 0))
    # a table of frame pointers: unwaited calls, and every one of them stores its copy
    tab = Call([e["frames"][n] for n in SETS["B"]])
    d_ptrs = torch.tensor([tab.d_img.data_ptr() + f * tab.fs for f in range(tab.B)], dtype=torch.int64, device=tab.dev)
    torch.cuda.synchronize()
    hold_device(st)
    for _ in range(3):
        c.match_batch_device_ptrs(d_ptrs.data_ptr(), tab.B, rows, cols, tab.stride, ch, THR, tab.d_out.data_ptr(), CAP, tab.d_cnt.data_ptr(),
                                  flags=capi.SBM_PTRS_ALIGNED4, stream=st.cuda_stream)
    st.synchronize()
    assert tab.lists() == want_of(e, SETS["B"])
    tab.d_img.fill_(0xFF)
    torch.cuda.synchronize()
    assert_level0(c, e, SETS["B"])
    if SPARSE_ON:
        assert c.source_retention() == (base[0] + 3, base[1])


def knob_child(path):
    """the child process (SBM_RETAIN_ALWAYS=1): four unwaited calls on one stream behind the delay"""
    import torch

    frames = list(np.load(path)["frames"])
    c = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0)
    c.upload_templates(load_templates())
    c.set_quantize_mode("stream", 18)
    calls = [Call(frames) for _ in range(4)]
    st = torch.cuda.Stream(device=calls[0].dev)
    warm = Call(frames)
    warm.enqueue(c, st)
    st.synchronize()
    before = c.source_retention()
    hold_device(st)
    for call in calls:
        call.enqueue(c, st)
    st.synchronize()
    after = c.source_retention()
    lists = calls[-1].lists()
    c.close()
    print("KNOB " + json.dumps({"lists": lists, "retention": [after[0] - before[0], after[1] - before[1]]}))


def test_knob_keeps_every_copy_in_a_child(world, tmp_path):
    e = world["P"]
    path = str(tmp_path / "frames.npz")
    np.savez(path, frames=np.stack([e["frames"][n] for n in SETS["A"]]))
    env = dict(os.environ, SBM_RETAIN_ALWAYS="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    out = subprocess.run([sys.executable, "-c", "import test_gpu_source_retention as t, sys; t.knob_child(sys.argv[1])", path],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    child = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("KNOB ")][-1][5:])
    assert child["lists"] == [[list(m) for m in e["want"][n]] for n in SETS["A"]]
    if SPARSE_ON:
        assert child["retention"] == [4, 0]
