"""-m gpu: the batched match entry points on pyramids and frame geometries that the one-launch linear-memory builder does
not take -- a stride other than 4 or 8, a level whose width is no multiple of 16 -- which the batched any-stride builder
(k_build_lm_any, csrc/sbm_lm_any.h) serves for strides up to 16.

Reference, frame by frame and bit for bit: oracle.Pyramid.build(frame, T, 30.0[, mask]).match(...) (lists as multisets),
the oracle's orientation maps and linear memories, and the bit planes packed from the latter.  Inputs and expected values:
any_geometry_cases.py, computed once per case."""
import os

import numpy as np
import pytest

import any_geometry_cases as AG
from any_geometry_cases import THRS, multiset, packed
from shape_based_matching_amd import capi
from shape_based_matching_amd.templates import MATCH_DTYPE

pytestmark = pytest.mark.gpu

REC = MATCH_DTYPE.itemsize
CAP = 4096


def dev():
    import torch

    return torch.device("cuda", 0)


class Batch:
    """n frames of a case in HBM in a caller's layout (row_pad bytes behind every row, frame_pad behind every frame, all
    padding 0xA5), result buffers and one stream"""

    def __init__(self, frames, row_pad=0, frame_pad=0):
        import torch

        self.torch = torch
        frames = np.ascontiguousarray(frames)
        self.n, self.rows, self.cols = frames.shape[:3]
        self.ch = 1 if frames.ndim == 3 else 3
        line = self.cols * self.ch
        self.stride = line + row_pad
        self.fs = self.rows * self.stride + frame_pad
        buf = np.full(self.n * self.fs, 0xA5, np.uint8)
        for f in range(self.n):
            buf[f * self.fs: f * self.fs + self.rows * self.stride].reshape(self.rows, self.stride)[:, :line] = frames[f].reshape(self.rows, line)
        self.d_imgs = torch.from_numpy(buf).to(dev())
        self.d_out = torch.zeros(self.n * CAP * REC, dtype=torch.uint8, device=dev())
        self.d_cnt = torch.zeros(self.n * 2, dtype=torch.int32, device=dev())
        self.stream = torch.cuda.Stream(device=dev())
        torch.cuda.synchronize()

    def lists(self):
        self.stream.synchronize()
        cnt = self.d_cnt.cpu().numpy().reshape(-1, 2)
        out = self.d_out.cpu().numpy().reshape(self.n, CAP * REC)
        assert (cnt[:, 1] == 0).all() and (cnt[:, 0] >= 0).all() and (cnt[:, 0] <= CAP).all(), cnt
        return [multiset(out[f].view(MATCH_DTYPE)[: cnt[f, 0]]) for f in range(self.n)]

    def run(self, ctx, thr, d_masks=None, mask_stride=None):
        self.d_cnt.fill_(-1)
        self.torch.cuda.synchronize()
        args = (self.d_imgs.data_ptr(), self.fs, self.n, self.rows, self.cols, self.stride, self.ch)
        if mask_stride is None:
            ctx.match_batch_device(*args, thr, self.d_out.data_ptr(), CAP, self.d_cnt.data_ptr(), stream=self.stream.cuda_stream,
                                   d_mask=d_masks.data_ptr() if d_masks is not None else 0)
        else:
            ctx.match_batch_device_masked(*args, d_masks.data_ptr(), mask_stride, thr, self.d_out.data_ptr(), CAP, self.d_cnt.data_ptr(),
                                          stream=self.stream.cuda_stream)
        return self.lists()


def make_ctx(ctx_factory, case):
    ctx = ctx_factory(T=case.T)
    ctx.upload_templates(case.ts)
    return ctx


# ---- 1. device batch, every geometry ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(AG.GEOS))
def test_device_batch_equals_oracle_per_frame(oracle, ctx_factory, name):
    """5 frames per call at thresholds 60 and 85: frame f's list is the oracle's for frame f alone.  (Refused with "batched
    match needs T in {4, 8} and 16-column-aligned levels" before the any-stride builder.)  On the BGR (4, 8) case also a
    padded caller layout, and threshold -5: every position a candidate, the byte coarse kernels, the coarsest level as 8
    response planes per frame."""
    case = AG.case(oracle, name)
    ctx = make_ctx(ctx_factory, case)
    b = Batch(case.frames)
    for thr in THRS:
        case.check_not_empty(b.n, thr)
        got = b.run(ctx, thr)
        for f in range(b.n):
            assert got[f] == case.want(f, thr), (name, thr, f, len(got[f]), len(case.want(f, thr)))
    assert len({tuple(case.want(f, THRS[0])) for f in range(b.n)}) >= 3, "the frames' lists should differ"
    if name != "bgr_4_8":
        return
    padded = Batch(case.frames, row_pad=13, frame_pad=1000)
    for thr in THRS:
        got = padded.run(ctx, thr)
        for f in range(b.n):
            assert got[f] == case.want(f, thr), ("padded", thr, f)
    one = case.ts.subset([2])
    ctx.upload_templates(one)
    got = b.run(ctx, -5.0)
    for f in range(b.n):
        pyr = case.pyramid(f)
        want = multiset(pyr.match(one.levels, one.features, one.class_idx, one.template_id, -5.0))
        pyr.free()
        assert len(want) > 0 and got[f] == want, (f, len(got[f]), len(want))


# ---- 2. per-frame masks -----------------------------------------------------------------------------------------------
def test_per_frame_masks_and_one_shared_mask(oracle, ctx_factory):
    import torch

    case = AG.case(oracle, "gray_4_8")
    ctx = make_ctx(ctx_factory, case)
    rows, cols, thr, n = case.rows, case.cols, THRS[0], 3
    masks = np.zeros((n, rows, cols), np.uint8)
    masks[0, 20:180, 30:250] = 255
    masks[1, :, : cols // 2 + 17] = 255
    masks[2, 50:, 9:] = 255
    ts = case.ts

    def want(f, m):
        pyr = case.pyramid(f, masks[m])
        out = multiset(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, thr))
        pyr.free()
        return out

    b = Batch(case.frames[:n])
    d_masks = torch.from_numpy(masks).to(dev())
    torch.cuda.synchronize()
    got = b.run(ctx, thr, d_masks, rows * cols)
    wants = [want(f, f) for f in range(n)]
    assert sum(len(w) for w in wants) > 0 and len({tuple(w) for w in wants}) == n
    assert [w != case.want(f, thr) for f, w in enumerate(wants)] == [True] * n, "every mask should change its frame's list"
    for f in range(n):
        assert got[f] == wants[f], f
    got = b.run(ctx, thr, d_masks[1], 0)  # one mask for all frames
    for f in range(n):
        assert got[f] == want(f, 1), f
    got = b.run(ctx, thr, d_masks[2])     # ... through the unmasked entry point's d_mask
    for f in range(n):
        assert got[f] == want(f, 2), f


# ---- 3. what the launch left ------------------------------------------------------------------------------------------
def assert_left_behind(ctx, case, n, thr):
    """maps of every level and frame, bit planes of every frame, frame 0's linear memories whole (zero tail included),
    and the template loop on them"""
    lc = case.L - 1
    pyrs = [case.pyramid(f) for f in range(n)]
    try:
        for f in range(n):
            for l in range(case.L):
                assert np.array_equal(ctx.get_quantized_frame(l, f), pyrs[f].quantized(l)), (f, l)
            assert np.array_equal(ctx.get_coarse_bitplanes(f), packed(pyrs[f].lm(lc))), f
        for l in range(case.L):
            got, want = ctx.get_linear_memories(l), pyrs[0].lm(l)
            assert got.shape == want.shape and np.array_equal(got, want), (l, np.argwhere(got != want)[:5])
        assert multiset(ctx.match_templates(thr)) == case.want(0, thr)
    finally:
        for p in pyrs:
            p.free()


@pytest.mark.parametrize("name", ["bgr_4_8", "bgr_5_8"])
def test_what_a_batch_leaves_resident(oracle, ctx_factory, name):
    case = AG.case(oracle, name)
    ctx = make_ctx(ctx_factory, case)
    b = Batch(case.frames[:4])
    thr = THRS[1]
    got = b.run(ctx, thr)
    assert got == [case.want(f, thr) for f in range(4)]
    assert_left_behind(ctx, case, 4, thr)
    # and the batch again on what the readers rebuilt (frame 0's response planes stand beside the spread planes now)
    assert b.run(ctx, thr) == [case.want(f, thr) for f in range(4)]


# ---- 4. graph replay ----------------------------------------------------------------------------------------------------
def test_graph_modes_give_the_same_lists(oracle, ctx_factory):
    case = AG.case(oracle, "bgr_4_8")
    ctx = make_ctx(ctx_factory, case)
    ctx.set_pipeline_depth(2)
    b = Batch(case.frames[:4])
    thr = THRS[0]
    want = [case.want(f, thr) for f in range(4)]
    for mode in (None, False, True):
        ctx.set_graph_mode(mode)
        for call in range(3):
            assert b.run(ctx, thr) == want, (mode, call)
            if call >= 1 and mode is not False:
                assert ctx.graph_count() >= 1, (mode, call)
        if mode is False:
            assert ctx.graph_count() == 0
    # the last call was a replay: the record of what it left must serve the readers
    assert_left_behind(ctx, case, 4, thr)
    assert b.run(ctx, thr) == want


# ---- 5. host batch ---------------------------------------------------------------------------------------------------------
def test_host_batch_runs_whole_sub_batches(oracle, ctx_factory):
    from test_gpu_nms_device import expected, rows_of, sizes_of

    case = AG.case(oracle, "bgr_4_8")
    ctx = make_ctx(ctx_factory, case)
    thr = THRS[1]
    frames = [case.frames[f] for f in range(4)]
    got = ctx.match_batch_host(frames, thr, cap=CAP, sub_batch=4)
    assert [multiset(g) for g in got] == [case.want(f, thr) for f in range(4)]
    # one sub-batch of four frames: frame 3 is resident (one frame per sub-batch left a single frame, and the read raised)
    assert np.array_equal(ctx.get_quantized_frame(1, 3), case.maps(3)[1])
    masks = [np.zeros((case.rows, case.cols), np.uint8) for _ in range(4)]
    masks[0][:, 40:] = 255
    masks[1] = None
    masks[2][30:190, :] = 255
    masks[3][:, :200] = 255
    got = ctx.match_batch_host_masked(frames, masks, thr, cap=CAP, sub_batch=3)
    ts = case.ts
    for f in range(4):
        pyr = case.pyramid(f, masks[f])
        want = multiset(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, thr))
        pyr.free()
        assert multiset(got[f]) == want, f
    kept, counts = ctx.match_batch_host_nms(frames, thr, 0.0, 0.5, cap=CAP, out_cap=256, sub_batch=4)
    sizes = sizes_of(ts)
    for f in range(4):
        raw = np.array(case.want(f, thr), MATCH_DTYPE)
        assert counts[f, 1] == 0 and rows_of(kept[f]) == rows_of(expected(raw, sizes, 0.0, 0.5)), f


# ---- 6. neighbouring behaviour ----------------------------------------------------------------------------------------------
def lm_launches(ctx):
    return [n for n, _ in ctx.timings() if n.startswith("k_build_lm")]


def test_aligned_geometry_around_an_unaligned_one(oracle, ctx_factory, case1):
    """512 x 768 (every level on the one-launch builder's grid) before and after 208 x 272 in one context: the lists are the
    oracle's, and the aligned batch still makes one k_build_lm launch and no other linear-memory launch"""
    from shape_based_matching_amd import synth

    case = AG.case(oracle, "bgr_4_8")
    ts = case1["templates"].subset(range(300, 361, 6))
    base = synth.embed(case1["test"], 512, 768, 20, 60)
    big = np.stack([base, np.roll(base, 24, axis=1), np.roll(base, 16, axis=0)])
    wants = []
    for fr in big:
        pyr = oracle.Pyramid.build(fr, [4, 8], 30.0)
        wants.append(multiset(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, 85.0)))
        pyr.free()
    assert sum(len(w) for w in wants) > 0
    aligned, unaligned = Batch(big), Batch(case.frames[:3])
    # the launches of the aligned batch in a context that never saw another geometry: one launch of the one-launch builder for
    # the pyramid (and the flagged level-0 strips of the sparse plan behind the coarse pass, under the same name)
    fresh = ctx_factory()
    fresh.upload_templates(ts)
    fresh.set_profiling(True)
    assert aligned.run(fresh, 85.0) == wants
    names = [n for n, _ in fresh.timings()]
    assert 1 <= len(lm_launches(fresh)) <= 2 and set(lm_launches(fresh)) == {"k_build_lm"}, names
    assert names.index("k_build_lm") < names.index("k_similarity_coarse"), names
    ctx = ctx_factory()
    for turn in range(2):
        ctx.upload_templates(ts)
        ctx.set_profiling(True)
        assert aligned.run(ctx, 85.0) == wants, turn
        assert [n for n, _ in ctx.timings()] == names, (turn, ctx.timings())
        ctx.set_profiling(False)
        ctx.upload_templates(case.ts)
        assert unaligned.run(ctx, THRS[0]) == [case.want(f, THRS[0]) for f in range(3)], turn


def test_strides_above_16_and_banded_calls_still_refuse(oracle, ctx_factory):
    import torch

    case = AG.case(oracle, "bgr_4_8")
    ctx = ctx_factory(T=(4, 32))
    ctx.upload_templates(case.ts)
    frames = np.zeros((2, 256, 512, 3), np.uint8)
    b = Batch(frames)
    with pytest.raises(capi.SbmError) as e:
        b.run(ctx, 85.0)
    assert e.value.code == -1 and "T = 32" in str(e.value) and "level 1" in str(e.value), str(e.value)
    one = Batch(frames[:1])  # a single frame through the batch entry point keeps the single-frame path
    assert one.run(ctx, 85.0) == [[]]
    ctx2 = make_ctx(ctx_factory, case)
    b2 = Batch(case.frames[:2])
    hdr = 16
    buf = torch.zeros(hdr + 2 * CAP * REC, dtype=torch.uint8, device=dev())
    torch.cuda.synchronize()
    with pytest.raises(capi.SbmError) as e:
        ctx2.match_batch_device_banded(b2.d_imgs.data_ptr(), b2.fs, 2, b2.rows, b2.cols, b2.stride, b2.ch, 85.0, buf.data_ptr(), CAP, n_bands=2)
    assert e.value.code == -1 and "16-column-aligned" in str(e.value), str(e.value)


# ---- 7. fuzz slice --------------------------------------------------------------------------------------------------------
def test_fuzz_slice_anygeo():
    import sys

    from conftest import ROOT

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_sequence

    n = fuzz_sequence.run(10, 3, steps=12, verbose=False, profile="anygeo")
    assert n > 0 and fuzz_sequence.LAST_RUN["compared"] == n


# ---- 8. one-rank sharded form -----------------------------------------------------------------------------------------------
def test_one_rank_sharded_batch(oracle, ctx_factory):
    import torch

    case = AG.case(oracle, "bgr_5_8")
    ctx = make_ctx(ctx_factory, case)
    ctx.comm_init(1, 0, ctx.comm_unique_id())
    B, thr = 5, THRS[0]
    b = Batch(case.frames)
    hdr = (8 * B + 15) // 16 * 16
    nbytes = hdr + B * CAP * REC
    d_local = torch.zeros(nbytes, dtype=torch.uint8, device=dev())
    d_gath = torch.zeros(nbytes, dtype=torch.uint8, device=dev())
    torch.cuda.synchronize()
    ctx.match_batch_device_sharded(b.d_imgs.data_ptr(), b.fs, B, b.rows, b.cols, b.stride, b.ch, thr, d_local.data_ptr(), CAP, d_gath.data_ptr(),
                                   stream=b.stream.cuda_stream)
    b.stream.synchronize()
    buf = d_gath.cpu().numpy()
    cnt = buf[: 8 * B].view(np.int32).reshape(B, 2)
    for f in range(B):
        assert cnt[f, 1] == 0
        assert multiset(buf[hdr + f * CAP * REC: hdr + (f + 1) * CAP * REC].view(MATCH_DTYPE)[: cnt[f, 0]]) == case.want(f, thr), f
