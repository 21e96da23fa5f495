"""-m gpu: the two forms of the sparse level-0 path's source pass -- the line-shaped kernel (sbm_source_lines.h) and the strided
form it falls back to (sbm_quantize_stream.h, QS_SOURCE) -- on the device, each proved by sbm_get_source_form.

  geometries  3 frames of 448 x 576 x 3 (two strips and a 64-column rest), 512 x 704 x 1 (two strips and 192 columns) and
              512 x 768 x 3 (three whole strips); the object against the right border, against the bottom border, absent
  calls       sbm_match_batch_device and sbm_match_device
  layouts     packed and padded on 4-byte boundaries (rows + 64 bytes, frames + 1000): the line form; rows + 13 bytes: the fallback
  checked     against oracle.Pyramid: the match lists, level 1's map (cv::pyrDown of the source pass went into it) and, after the
              caller's buffer was overwritten, every frame's level-0 map (made from the retained copy)
  knob        a child process with SBM_SOURCE_LINES=0: the fallback on the packed layout, the same lists
  replay      captured graphs of both forms on one context: a replay reports the form it was captured with
Every profiled call shows the three "k_quantize" launches of the sparse path, whichever form its first one was."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from shape_based_matching_amd import capi
from shape_based_matching_amd.templates import MATCH_DTYPE
from test_gpu_sparse_geometry import assert_sparse_launches, cut_frames, entry, run_batch
from test_gpu_sparse_gradient import CAP, SPARSE_ON, THR, gradient_launches, load_templates, multiset

pytestmark = pytest.mark.gpu
REC = MATCH_DTYPE.itemsize
GEO = {"P": (448, 576, 3), "Q": (512, 704, 1), "R": (512, 768, 3)}
NAMES = ["right", "bottom", "absent"]
LINES_ON = os.environ.get("SBM_SOURCE_LINES", "1") != "0"
NONE, STRIDED, LINES = 0, 1, 2
# (row pad, frame pad) -> the form the selection rule gives it
LAYOUTS = [((0, 0), LINES), ((64, 1000), LINES), ((13, 0), STRIDED)]


def expected(form):
    return (form if LINES_ON else STRIDED) if SPARSE_ON else NONE


@pytest.fixture(scope="module")
def world(oracle):
    """per geometry the frames, the oracle's pyramids and lists -- computed once, read by every test, never changed"""
    ts = load_templates()
    w = {"ts": ts}
    for g, (rows, cols, ch) in GEO.items():
        fr = cut_frames(oracle, ts, rows, cols, ch)
        w[g] = entry(oracle, ts, {n: fr[n] for n in NAMES})
        assert len(w[g]["want"]["right"]) > 20 and len(w[g]["want"]["bottom"]) > 20 and w[g]["want"]["right"] != w[g]["want"]["bottom"], g
    yield w
    for g in GEO:
        for p in w[g]["pyr"].values():
            p.free()


@pytest.fixture()
def ctx(world):
    made = []

    def make(hs=18, **kw):
        c = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0, **kw)
        c.upload_templates(world["ts"])
        c.set_quantize_mode("stream", hs)  # (the streaming kernel is not chosen below 4 Mpixel per launch)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


@pytest.mark.parametrize("layout,form", LAYOUTS)
@pytest.mark.parametrize("geo", list(GEO))
def test_batch_call(world, ctx, geo, layout, form):
    import torch

    e = world[geo]
    frames = [e["frames"][n] for n in NAMES]
    c = ctx()
    assert c.source_form() == NONE
    run_batch(c, frames, *layout)  # the first call also prepares the template tables
    c.set_profiling(True)
    got, d_img = run_batch(c, frames, *layout)
    assert got == [e["want"][n] for n in NAMES]
    assert c.source_form() == expected(form)
    assert_sparse_launches(c)
    c.set_profiling(False)
    d_img.fill_(0xFF)  # the call is synchronised: the buffer is the caller's again
    torch.cuda.synchronize()
    for b, n in enumerate(NAMES):
        assert np.array_equal(c.get_quantized_frame(1, b), e["pyr"][n].quantized(1)), (geo, layout, n)
    for b, n in reversed(list(enumerate(NAMES))):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][n].quantized(0)), (geo, layout, n)


@pytest.mark.parametrize("geo", list(GEO))
def test_single_frame_call(world, ctx, geo):
    """sbm_match_device from packed rows (the line form) and from rows padded by 13 bytes (the fallback)"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols, ch = GEO[geo]
    e = world[geo]
    c = ctx(32)
    st = torch.cuda.Stream(device=dev)
    d_out = torch.zeros(CAP * REC, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    c.set_profiling(True)
    for n, row_pad, form in (("right", 0, LINES), ("bottom", 13, STRIDED), ("bottom", 0, LINES), ("absent", 64, LINES)):
        stride = cols * ch + row_pad
        buf = np.full((rows, stride), 0xA5, np.uint8)
        buf[:, : cols * ch] = e["frames"][n].reshape(rows, cols * ch)
        d_img = torch.from_numpy(buf).to(dev)
        torch.cuda.synchronize()
        c.match_device(d_img.data_ptr(), rows, cols, stride, ch, THR, d_out.data_ptr(), CAP, d_cnt.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        cnt = d_cnt.cpu().numpy()
        assert cnt[1] == 0 and multiset(d_out.cpu().numpy().view(MATCH_DTYPE)[: cnt[0]]) == e["want"][n], (n, row_pad)
        assert c.source_form() == expected(form), (n, row_pad)
        assert_sparse_launches(c, False)
        d_img.fill_(0xFF)
        torch.cuda.synchronize()
        assert np.array_equal(c.get_quantized(1), e["pyr"][n].quantized(1)), (n, row_pad)
        assert np.array_equal(c.get_quantized(0), e["pyr"][n].quantized(0)), (n, row_pad)


def test_a_replayed_graph_reports_its_own_form(world, ctx):
    e = world["R"]
    frames = [e["frames"][n] for n in NAMES]
    want = [e["want"][n] for n in NAMES]
    import torch

    from fuzz_sequence import padded_layout  # (tools/ is on the path: test_gpu_sparse_geometry put it there)

    dev = torch.device("cuda", 0)
    rows, cols, ch = GEO["R"]
    B = len(frames)
    c = ctx()
    c.set_graph_mode(True)
    # the same buffers in every call, so that the second call of a layout finds the first one's graph
    bufs = {}
    for layout in ((0, 0), (13, 0)):
        buf, stride, fs = padded_layout(frames, *layout)
        bufs[layout] = (torch.from_numpy(buf).to(dev), stride, fs)
    d_out = torch.zeros(B * CAP * REC, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(B * 2, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for layout, form in ((0, 0), LINES), ((13, 0), STRIDED), ((0, 0), LINES), ((13, 0), STRIDED), ((13, 0), STRIDED), ((0, 0), LINES):
        d_img, stride, fs = bufs[layout]
        c.match_batch_device(d_img.data_ptr(), fs, B, rows, cols, stride, ch, THR, d_out.data_ptr(), CAP, d_cnt.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        cnt = d_cnt.cpu().numpy().reshape(B, 2)
        recs = d_out.cpu().numpy().view(MATCH_DTYPE).reshape(B, CAP)
        assert (cnt[:, 1] == 0).all() and [multiset(recs[b, : cnt[b, 0]]) for b in range(B)] == want, layout
        assert c.source_form() == expected(form), layout
    for b, n in enumerate(NAMES):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][n].quantized(0)), n


def knob_child(path):
    """the child process (SBM_SOURCE_LINES=0): the packed batch of the frames in `path` through the strided form"""
    frames = list(np.load(path)["frames"])
    c = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0)
    c.upload_templates(load_templates())
    c.set_quantize_mode("stream", 18)
    run_batch(c, frames)
    c.set_profiling(True)
    lists, _ = run_batch(c, frames)
    form = c.source_form()
    n = gradient_launches(c)
    c.close()
    print("LISTS " + json.dumps({"lists": lists, "launches": n, "form": form}))


def test_knob_forces_the_strided_form_in_a_child(world, tmp_path):
    e = world["R"]
    path = str(tmp_path / "frames.npz")
    np.savez(path, frames=np.stack([e["frames"][n] for n in NAMES]))
    env = dict(os.environ, SBM_SOURCE_LINES="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    out = subprocess.run([sys.executable, "-c", "import test_gpu_source_pass as t, sys; t.knob_child(sys.argv[1])", path],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    child = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("LISTS ")][-1][6:])
    assert child["lists"] == [[list(m) for m in e["want"][n]] for n in NAMES]
    if SPARSE_ON:
        assert child["form"] == STRIDED and child["launches"] == 3
