"""-m gpu: one mask per frame of a batch (sbm_match_batch_device_masked, sbm_match_batch_host*_masked,
sbm_get_quantized_frame), pyramid {4, 8}.

Reference, frame by frame and bit for bit: oracle.Pyramid.build(frame, [4, 8], weak, mask=masks[f]) -- the mask of
Detector::match belongs to the call (line2Dup.cpp:1078); quantize() applies it at every level (:446-450) and pyrDown()
resizes it with INTER_NEAREST from the level above (:439)."""
import numpy as np
import pytest

import frame_mask_cases as FM
from shape_based_matching_amd import capi, synth, templates
from shape_based_matching_amd.templates import MATCH_DTYPE

pytestmark = pytest.mark.gpu

REC = MATCH_DTYPE.itemsize
THR = 80.0
CAP = 1024


def key(recs):
    return sorted(np.ascontiguousarray(recs, MATCH_DTYPE).tolist())


def dev():
    import torch

    return torch.device("cuda", 0)


class Batch:
    """frames and masks in HBM, result buffers, one stream"""

    def __init__(self, frames, mask_buf=None):
        import torch

        self.torch = torch
        frames = np.array(frames, np.uint8, order="C")  # a copy: the shared inputs are read-only
        self.n, self.rows, self.cols = frames.shape[:3]
        self.ch = 1 if frames.ndim == 3 else 3
        self.frame_bytes = self.rows * self.cols * self.ch
        self.d_imgs = torch.from_numpy(frames).to(dev())
        self.d_masks = None if mask_buf is None else torch.from_numpy(np.array(mask_buf, np.uint8, order="C")).to(dev())
        self.d_out = torch.zeros(self.n * CAP * REC, dtype=torch.uint8, device=dev())
        self.d_cnt = torch.zeros(self.n * 2, dtype=torch.int32, device=dev())
        self.stream = torch.cuda.Stream(device=dev())
        torch.cuda.synchronize()

    def set_masks(self, mask_buf):
        """new contents at the same address"""
        self.d_masks.copy_(self.torch.from_numpy(np.array(mask_buf, np.uint8, order="C")))
        self.torch.cuda.synchronize()

    def lists(self, n=None):
        self.stream.synchronize()
        n = self.n if n is None else n
        cnt = self.d_cnt.cpu().numpy().reshape(-1, 2)
        out = self.d_out.cpu().numpy().reshape(self.n, CAP * REC)
        assert (cnt[:n, 1] == 0).all() and (cnt[:n, 0] <= CAP).all(), cnt
        return [out[f].view(MATCH_DTYPE)[: cnt[f, 0]].copy() for f in range(n)]

    def masked(self, ctx, mask_stride, n=None):
        self.d_cnt.fill_(-1)
        self.torch.cuda.synchronize()
        n = self.n if n is None else n
        ctx.match_batch_device_masked(self.d_imgs.data_ptr(), self.frame_bytes, n, self.rows, self.cols, self.cols * self.ch, self.ch,
                                      self.d_masks.data_ptr(), mask_stride, THR, self.d_out.data_ptr(), CAP, self.d_cnt.data_ptr(),
                                      stream=self.stream.cuda_stream)
        return self.lists(n)

    def shared(self, ctx, d_mask):
        self.d_cnt.fill_(-1)
        self.torch.cuda.synchronize()
        ctx.match_batch_device(self.d_imgs.data_ptr(), self.frame_bytes, self.n, self.rows, self.cols, self.cols * self.ch, self.ch, THR,
                               self.d_out.data_ptr(), CAP, self.d_cnt.data_ptr(), stream=self.stream.cuda_stream, d_mask=d_mask)
        return self.lists()


# ---- 1. maps -------------------------------------------------------------------------------------------------------
def tiny_templates():
    """two small templates: the match entry points need some, the maps do not depend on them"""
    f0 = np.array([(2, 2, 0), (6, 5, 3), (10, 9, 5), (12, 3, 1), (4, 12, 7)])
    f1 = np.array([(1, 1, 0), (3, 2, 3), (5, 4, 5)])
    pyr = [{"width": 16, "height": 16, "tl_x": 0, "tl_y": 0, "pyramid_level": 0, "features": f0},
           {"width": 8, "height": 8, "tl_x": 0, "tl_y": 0, "pyramid_level": 1, "features": f1}]
    return templates.from_pyramids([pyr, pyr], "tiny")


MAP_CASES = [(32, 256, 9), (48, 320, 5), (64, 512, 7), (32, 960, 3), (32, 128, 3)]


@pytest.mark.parametrize("ch", [1, 3], ids=["gray", "bgr"])
@pytest.mark.parametrize("rows,cols,n", MAP_CASES)
def test_maps_of_every_frame_and_level(oracle, ctx_factory, rows, cols, n, ch):
    """levels 0 and 1 of every frame through sbm_get_quantized_frame, under every gradient kernel choice: auto and tile
    (k_quantize with the frame's mask stride), stream with the default rows per wave and with 8 (the packed last strip:
    8, 2 and 5 frames per wave at level 0; 8 and 3 at level 1 of the 512- and 128-column cases)"""
    frames = FM.textured_frames(rows + cols + ch, n, rows, cols, ch)
    masks = FM.frame_masks(cols + n, n, rows, cols)
    if n == 3:  # no room for the all-255 frame beside the all-zero one and two telling ones: it takes frame 1's place in a second set
        second = FM.frame_masks(cols + n + 1, n, rows, cols)
        second[1] = 255
        mask_sets = [masks, second]
    else:
        mask_sets = [masks]
    ctx = ctx_factory()
    ctx.upload_templates(tiny_templates())
    for masks in mask_sets:
        want = FM.assert_masks_matter(oracle, frames, masks, [4, 8])
        buf, fs = FM.strided(masks)
        dense, strided = Batch(frames, masks), Batch(frames, buf)
        for mode, rpw in (("auto", 0), ("tile", 0), ("stream", 0), ("stream", 8)):
            ctx.set_quantize_mode(mode, rpw)
            for b, stride in ((dense, rows * cols), (strided, fs)):
                b.masked(ctx, stride)
                for f in range(n):
                    for l in range(2):
                        got = ctx.get_quantized_frame(l, f)
                        assert np.array_equal(got, want[f][l]), (mode, rpw, stride, f, l, np.argwhere(got != want[f][l])[:5])


# ---- 2. - 5. match lists on the case1 image ------------------------------------------------------------------------
ROWS, COLS, B = 640, 768, 7


class Scene:
    """7 frames of the case1 image, shifted as in test_gpu_quantize_stream.py; rectangular masks that contain the object in
    some frames and cut it in others; the oracle's list of (frame f, mask g), computed once per pair and kept"""

    def __init__(self, oracle, case1):
        self.oracle = oracle
        self.ts = case1["templates"].subset(range(300, 361, 6))
        base = synth.embed(case1["test"], ROWS, COLS, 80, 120)
        self.frames = np.stack([np.roll(base, 40 * b, axis=1) for b in range(B)])
        h, w = case1["test"].shape[:2]
        self.masks = np.zeros((B, ROWS, COLS), np.uint8)
        for f in range(B):
            left = 120 + 40 * f
            if f % 3 == 0:    # contains the object
                self.masks[f, 40:min(ROWS, 120 + h), max(0, left - 60):min(COLS, left + w + 60)] = 255
            elif f % 3 == 1:  # cuts it: the upper left part only
                self.masks[f, 0:80 + (2 * h) // 3, 0:min(COLS, left + (2 * w) // 3)] = 200
            else:             # misses it
                self.masks[f, ROWS - 60:, :] = 1
        self.masks.setflags(write=False)
        self.frames.setflags(write=False)
        self.cache = {}

    def want(self, f, g):
        """g: index of a mask, None (no mask)"""
        if (f, g) not in self.cache:
            p = self.oracle.Pyramid.build(self.frames[f], [4, 8], FM.WEAK, mask=None if g is None else self.masks[g])
            self.cache[(f, g)] = key(p.match(self.ts.levels, self.ts.features, self.ts.class_idx, self.ts.template_id, THR))
            p.free()
        return self.cache[(f, g)]


@pytest.fixture(scope="module")
def scene(oracle, case1):
    return Scene(oracle, case1)


def test_match_lists_with_a_mask_stride_of_two(scene, ctx_factory):
    want = [scene.want(f, f) for f in range(B)]
    # on the oracle alone: the masks decide -- one list is empty, two non-empty ones differ
    assert any(len(w) == 0 for w in want)
    assert len({tuple(w) for w in want if w}) >= 2
    ctx = ctx_factory()
    ctx.upload_templates(scene.ts)
    buf, fs = FM.strided(scene.masks)
    for mask_buf, stride in ((scene.masks, ROWS * COLS), (buf, fs)):
        got = Batch(scene.frames, mask_buf).masked(ctx, stride)
        for f in range(B):
            assert key(got[f]) == want[f], (stride, f)


def test_equivalences(scene, ctx_factory):
    import torch

    ctx = ctx_factory()
    ctx.upload_templates(scene.ts)
    b = Batch(scene.frames, scene.masks)
    # stride 0 through the new entry point == the old entry point with that mask
    new = [key(r) for r in b.masked(ctx, 0)]
    old = [key(r) for r in b.shared(ctx, b.d_masks.data_ptr())]
    assert new == old and any(new)
    assert new == [scene.want(f, 0) for f in range(B)]
    # all-255 masks == no mask
    full = Batch(scene.frames, np.full((B, ROWS, COLS), 255, np.uint8))
    assert [key(r) for r in full.masked(ctx, ROWS * COLS)] == [key(r) for r in full.shared(ctx, 0)]
    # n_frames = 1 == sbm_match_device
    one = [key(r) for r in b.masked(ctx, ROWS * COLS, n=1)]
    d_cnt = torch.zeros(2, dtype=torch.int32, device=dev())
    torch.cuda.synchronize()
    ctx.match_device(b.d_imgs.data_ptr(), ROWS, COLS, COLS * 3, 3, THR, b.d_out.data_ptr(), CAP, d_cnt.data_ptr(), stream=b.stream.cuda_stream,
                     d_mask=b.d_masks.data_ptr())
    b.stream.synchronize()
    n = int(d_cnt.cpu()[0])
    single = key(b.d_out.cpu().numpy()[: n * REC].view(MATCH_DTYPE))
    assert one[0] == single == scene.want(0, 0) and single


def test_graph_replay_reads_the_masks_at_replay_time(scene, ctx_factory):
    """pipeline depth 2: the tuple is captured at its second sighting and replayed at its third; the masks' contents change
    in place between the calls and the lists follow them.  The same pointer with stride 0 is another launch (level >= 1
    resizes one mask, not three): a second capture, not a reuse."""
    n = 3
    ctx = ctx_factory()
    ctx.upload_templates(scene.ts)
    ctx.set_pipeline_depth(2)
    b = Batch(scene.frames[:n], scene.masks[:n])
    for call, shift in enumerate((2, 1, 0)):
        b.set_masks(scene.masks[shift:shift + n])
        got = b.masked(ctx, ROWS * COLS)
        for f in range(n):
            assert key(got[f]) == scene.want(f, f + shift), (call, f)
        assert ctx.graph_count() == (0 if call == 0 else 1), call
    assert [scene.want(f, 0) for f in range(n)] != [scene.want(f, f) for f in range(n)] and all(scene.want(f, 0) for f in range(n))
    for call in range(2):  # the buffer now starts with mask 0
        got = b.masked(ctx, 0)
        for f in range(n):
            assert key(got[f]) == scene.want(f, 0), (call, f)
        assert ctx.graph_count() == 1 + call, call


def epilogue(recs):
    """Detector::match's epilogue as sbm_nms_batch_device applies it: canonical order, then std::unique on (x, y, similarity, class)"""
    r = capi.canonicalize(recs)
    keep = [i for i in range(len(r)) if i == 0 or (r[i]["x"], r[i]["y"], r[i]["similarity"], r[i]["class_idx"]) !=
            (r[i - 1]["x"], r[i - 1]["y"], r[i - 1]["similarity"], r[i - 1]["class_idx"])]
    return r[keep].tolist()


def test_host_batch(scene, oracle, ctx_factory):
    """11 frames in sub-batches of 4, 4 and 3, two of them without a mask, from pageable and from pinned memory; the NMS
    ending; then a batch of another geometry on the same context"""
    idx = [(f % B, f % B) for f in range(B)] + [(0, None), (1, None), (2, 2), (3, 3)]
    frames = np.stack([scene.frames[f] for f, _ in idx])
    masks = np.stack([scene.masks[g if g is not None else 0] for _, g in idx])
    mask_list = [masks[i] if g is not None else None for i, (_, g) in enumerate(idx)]
    want = [scene.want(f, g) for f, g in idx]
    assert want[7] != want[0] or want[8] != want[1]  # a missing mask is not frame 0's mask
    ctx = ctx_factory()
    ctx.upload_templates(scene.ts)
    for pinned in (False, True):
        if pinned:
            ctx.pin_host_buffer(frames)
            ctx.pin_host_buffer(masks)
        for split in (False, True):
            got = ctx.match_batch_host_masked(list(frames), mask_list, THR, cap=CAP, sub_batch=4, split=split)
            assert [key(r) for r in got] == want, (pinned, split)
        if pinned:
            ctx.unpin_host_buffer(frames)
            ctx.unpin_host_buffer(masks)
    # _end_nms serves the masked form too: thresholds that keep every record = the epilogue alone
    kept, counts = ctx.match_batch_host_masked(list(frames), mask_list, THR, cap=CAP, sub_batch=4,
                                               nms=capi.SbmNmsParams(-1.0, 1.0, 1.0, 0), out_cap=CAP)
    assert (counts[:, 1] == 0).all()
    for i, (f, g) in enumerate(idx):
        assert kept[i].tolist() == epilogue(np.array(want[i], MATCH_DTYPE)), i
    # another geometry on the same context (sub-batches of 2, 2 and 1): lists, and the maps of the last sub-batch (frame 4)
    r2, c2, n2 = 448, 640, 5
    fr2 = FM.textured_frames(3, n2, r2, c2, 1)
    m2 = FM.frame_masks(4, n2, r2, c2)
    maps = FM.assert_masks_matter(oracle, fr2, m2, [4, 8])
    got = ctx.match_batch_host_masked(list(fr2), [None if f == 3 else m2[f] for f in range(n2)], THR, cap=CAP, sub_batch=2)
    for f in range(n2):
        p = oracle.Pyramid.build(fr2[f], [4, 8], FM.WEAK, mask=None if f == 3 else m2[f])
        assert key(got[f]) == key(p.match(scene.ts.levels, scene.ts.features, scene.ts.class_idx, scene.ts.template_id, THR)), f
        p.free()
    for l in range(2):
        assert np.array_equal(ctx.get_quantized_frame(l, 0), maps[4][l]), l
    with pytest.raises(capi.SbmError):
        ctx.get_quantized_frame(0, 1)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------
def test_refusals(ctx_factory):
    rows, cols, n = 32, 256, 3
    frames = FM.textured_frames(1, n, rows, cols, 1)
    b = Batch(frames, FM.frame_masks(2, n, rows, cols))
    ctx = ctx_factory()
    ctx.upload_templates(tiny_templates())

    def call(d_masks, stride):
        ctx.match_batch_device_masked(b.d_imgs.data_ptr(), b.frame_bytes, n, rows, cols, cols, 1, d_masks, stride, THR, b.d_out.data_ptr(), CAP,
                                      b.d_cnt.data_ptr(), stream=b.stream.cuda_stream)

    for d_masks, stride in ((0, rows * cols), (b.d_masks.data_ptr(), 1), (b.d_masks.data_ptr(), rows * cols - 1), (b.d_masks.data_ptr(), -rows * cols)):
        with pytest.raises(capi.SbmError) as e:
            call(d_masks, stride)
        assert e.value.code == -1, (d_masks, stride)
    call(b.d_masks.data_ptr(), rows * cols)
    b.stream.synchronize()
    ctx.get_quantized_frame(1, n - 1)
    for frame in (n, -1):
        with pytest.raises(capi.SbmError) as e:
            ctx.get_quantized_frame(0, frame)
        assert e.value.code == -1, frame


# ---- 6. facade -----------------------------------------------------------------------------------------------------
def test_facade_batches_with_a_mask_per_frame(tmp_path, oracle, case1):
    """the C++ Detector: matchBatch / matchAsync + wait / matchBatchNMS / setDevices + matchBatch with a vector of masks,
    element f against match(sources[f], thr, ids, masks[f]) in the demo's `maskbatch` mode -- also at a threshold where a
    frame's raw list exceeds the batch's per-frame capacity of 1024 and the frame is matched again alone, under its own mask"""
    import os
    import subprocess

    from conftest import ROOT
    from shape_based_matching_amd.templates import write_class_yaml

    demo = os.path.join(ROOT, "shape_based_matching_amd", "sbm_facade_demo")
    assert os.path.exists(demo), "facade demo not built: run __graft_entry__.build()"
    ts = case1["templates"]
    fmt = str(tmp_path / "%s_templ.yaml")
    write_class_yaml(ts, fmt % "test")
    img = case1["test"]
    img_path = str(tmp_path / "test.ppm")
    with open(img_path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img[:, :, ::-1]).tobytes())
    # a threshold at which the unmasked frame (every fourth frame has no mask) has more raw records than the batch holds
    p = synth.embed(img, img.shape[0] + 200, img.shape[1] + 200, 100, 100)
    frame = np.ascontiguousarray(p[: p.shape[0] // 16 * 16, : p.shape[1] // 16 * 16])
    pyr = oracle.Pyramid.build(frame, [4, 8], 30.0)
    low = None
    for t in (65.0, 60.0):
        if len(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, t, n_threads=min(16, os.cpu_count() or 1))) > 1100:
            low = t
            break
    pyr.free()
    assert low is not None, "no threshold gave more than 1024 raw records"
    for thr, nf, devs in (("88", 6, "0,0"), (str(low), 6, "0,0")):
        r = subprocess.run([demo, "maskbatch", fmt, "test", img_path, thr, "128", str(nf), "100", devs], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        head = r.stdout.strip().splitlines()[0].split()
        flags = dict(zip(head[1::2], head[2::2]))
        assert flags["frames"] == str(nf) and int(flags["matches"]) > 0 and int(flags["masks_matter"]) >= 2, head
        # (the NMS ending is compared at the first threshold only: a frame that is matched again alone goes through the
        # host's NMSBoxes, whose order among equal scores is not match()'s contract)
        for k in ("batch_same", "async_same", "devices_batch_same", "no_masks_same") + (("nms_same",) if thr == "88" else ()):
            assert flags[k] == "1", (k, r.stdout)
