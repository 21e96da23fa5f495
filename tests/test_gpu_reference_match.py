"""-m gpu: the HIP match half against the reference's own match half directly, with no oracle in between.

oracle/_ref/ref_match_<variant> (the reference's line2Dup.cpp compiled on stand-in headers, see
tests/test_reference_match_half.py) is fed with the maps the GPU itself holds: the quantized maps given to
sbm_set_quantized, or the ones sbm_get_quantized returns after the GPU's own gradient stage.  Its matchClass list must
equal the HIP list as a multiset, its linear memories the HIP ones byte for byte.  tests/golden/ref_match_case1.npz,
recorded from the AVX2 build, holds the HIP kernels to the reference even where oracle/_ref could not be built."""
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import ref_match as R
from ref_match_cases import edge_templates, onehot_with_holes, with_classes
from shape_based_matching_amd import capi, synth
from shape_based_matching_amd.templates import MATCH_DTYPE, TemplateSet

pytestmark = pytest.mark.gpu
VARIANT = "avx2" if "avx2" in R.runnable_variants() else "scalar"


def reference(qs, T, ts):
    missing = R.missing_binaries([VARIANT])
    assert not missing, f"{missing} missing: run __graft_entry__.build() where the reference tree is present"
    return R.Reference(qs, T, ts, VARIANT)


@pytest.fixture()
def make_ctx():
    made = []

    def make(T, coarse="auto", refine_bits=None):
        c = capi.Context(T=T, weak_threshold=30.0, device_id=0, max_candidates=1 << 20)
        c.set_coarse_mode(coarse)
        c.set_refine_bits(refine_bits)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


# ---- sbm_set_quantized + sbm_match_templates on the edge templates ----------------------------------------------
_EDGE = {}


def _edge_case(T):
    """random maps of a 2-level pyramid, the edge templates (no negative coordinates: the C ABI refuses those) in two
    classes, and the reference's raw lists at thresholds <= 0, low, and equal to attained scores"""
    if T not in _EDGE:
        rs = np.random.RandomState(sum(T))
        shapes = [(128, 176), (64, 88)]
        qs = [onehot_with_holes(rs, r, c, density=0.3) for r, c in shapes]
        ts, _ = edge_templates(shapes, list(T), seed=11, negative=False)
        ts = with_classes(ts, 2)
        with reference(qs, list(T), ts) as ref:
            thr = [-1.0, 0.0, 10.0, 30.0]
            s = np.unique(ref.match(-1.0)[0]["similarity"])
            s = s[s > 0]
            thr += [float(s[len(s) // 2]), float(s[-1])]
            want = {t: R.match_key(ref.match(t)[0]) for t in thr}
            lms = ref.lm()
        _EDGE[T] = (qs, ts, want, lms)
    return _EDGE[T]


@pytest.mark.parametrize("refine_bits", [True, False])
@pytest.mark.parametrize("coarse", ["bits", "bytes"])
@pytest.mark.parametrize("T", [(4, 8), (8, 4)])
def test_stage_path_edge_templates(make_ctx, T, coarse, refine_bits):
    qs, ts, want, lms = _edge_case(T)
    ctx = make_ctx(T, coarse, refine_bits)
    ctx.upload_templates(ts)
    for l, q in enumerate(qs):
        ctx.set_quantized(l, q)
    total = 0
    for thr, w in want.items():
        if coarse == "bits" and thr < 0:
            continue  # bit planes hold "response > 0" and "== 4": a negative threshold needs the byte kernels
        got = R.match_key(ctx.match_templates(thr))
        assert got == w, (T, coarse, refine_bits, thr, len(got), len(w))
        total += len(w)
    assert total > 100
    if coarse == "bytes" and not refine_bits:
        for l in range(2):
            n = lms[l].shape[1]
            assert np.array_equal(ctx.get_linear_memories(l)[:, :n], lms[l]), (T, l)


# ---- the whole HIP match half on its own maps ---------------------------------------------------------------------
def _frame(name):
    if name == "case1":
        return synth.embed(np.load(os.path.join(GOLDEN, "case1_test_bgr.npz"))["bgr"], 640, 768, 40, 60)
    if name == "case2":
        img = np.load(os.path.join(GOLDEN, "case2_test_bgr.npz"))["bgr"]
        return synth.embed(img, img.shape[0] // 32 * 32 + 32, img.shape[1] // 32 * 32 + 32, 8, 8)
    rows, cols, seed = {"fuzz_a": (480, 832, 5), "fuzz_b": (576, 704, 9), "fuzz_c": (1024, 1088, 13)}[name]
    return synth.scene_bgr(seed, rows, cols, n_shapes=rows * cols // 2000)


def _templates(name, ctx, frame):
    if name in ("case1", "case2"):
        ts = TemplateSet.load_npz(os.path.join(GOLDEN, f"{name}_templates.npz"))
        return R.dense_ids(ts.subset(range(0, ts.n_templates, max(1, ts.n_templates // 90))))
    ctx.build_pyramid(frame)
    qs = [ctx.get_quantized(l) for l in range(2)]
    ts, _ = synth.templates_from_maps(qs, [124, 61], 200, 12, len(name))
    return with_classes(ts, 3)


@pytest.mark.parametrize("name", ["case1", "case2", "fuzz_a", "fuzz_b", "fuzz_c"])
def test_match_and_batch_against_reference_on_own_maps(make_ctx, name):
    import torch

    frame = _frame(name)
    frames = np.stack([frame, np.roll(frame, 24, axis=1)])
    rows, cols = frame.shape[:2]
    ctx = make_ctx((4, 8))
    ts = _templates(name, ctx, frame)
    ctx.upload_templates(ts)
    thresholds = (60.0, 85.0)
    wants = []
    for b in range(len(frames)):
        got = {t: ctx.match(frames[b], t) for t in thresholds}
        qs = [ctx.get_quantized(l) for l in range(2)]
        with reference(qs, [4, 8], ts) as ref:
            want = {t: ref.match(t)[0] for t in thresholds}
            if b == 0:
                lms = ref.lm()
        for t in thresholds:
            assert R.match_key(got[t]) == R.match_key(want[t]), (name, b, t, len(got[t]), len(want[t]))
        wants.append(want)
        if b == 0:
            assert len(want[thresholds[0]]) > 0
    # the batched device entry point on both frames at once
    dev = torch.device("cuda", 0)
    B, cap, rec = len(frames), 1 << 16, MATCH_DTYPE.itemsize
    d_img = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    d_out = torch.zeros(B * cap * rec, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(B * 2, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    for t in thresholds:
        torch.cuda.synchronize()
        ctx.match_batch_device(d_img.data_ptr(), frames[0].size, B, rows, cols, cols * 3, 3, t, d_out.data_ptr(), cap,
                               d_cnt.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        cnt = d_cnt.cpu().numpy().reshape(B, 2)
        recs = d_out.cpu().numpy().view(MATCH_DTYPE).reshape(B, cap)
        for b in range(B):
            assert cnt[b, 1] == 0
            assert R.match_key(recs[b, : cnt[b, 0]]) == R.match_key(wants[b][t]), (name, "batch", b, t)
    # linear memories of frame 0 (a T = 4 and a T = 8 level), built by the byte path
    ctx2 = make_ctx((4, 8), "bytes", False)
    ctx2.upload_templates(ts)
    ctx2.match(frames[0], 85.0)
    for l in range(2):
        n = lms[l].shape[1]
        assert np.array_equal(ctx2.get_linear_memories(l)[:, :n], lms[l]), (name, l)


# ---- the recorded reference outputs -------------------------------------------------------------------------------
def test_hip_against_recorded_reference_golden(make_ctx):
    """tests/golden/ref_match_case1.npz (the AVX2 reference build's lists and one level's linear-memory digest on the
    case1 frame's maps); needs no oracle/_ref"""
    z = np.load(os.path.join(GOLDEN, "ref_match_case1.npz"))
    ts = R.dense_ids(TemplateSet.load_npz(os.path.join(GOLDEN, "case1_templates.npz")).subset(z["template_index"]))
    for coarse, refine_bits in (("auto", None), ("bytes", False)):
        ctx = make_ctx((4, 8), coarse, refine_bits)
        ctx.upload_templates(ts)
        ctx.set_quantized(0, z["q0"])
        ctx.set_quantized(1, z["q1"])
        for k, thr in enumerate(z["thresholds"].tolist()):
            got = ctx.match_templates(thr)
            assert R.match_key(got) == R.match_key(z[f"raw{k}"]), (coarse, thr)
            assert R.epilogue_key(capi.canonicalize(got)) == R.epilogue_key(z[f"epi{k}"]), (coarse, thr)
        assert len(z["raw2"]) > 0
        if coarse == "bytes":
            l = int(z["lm_level"])
            T = ctx.T[l]
            n = T * T * (z[f"q{l}"].shape[0] // T) * (z[f"q{l}"].shape[1] // T)
            lm = np.ascontiguousarray(ctx.get_linear_memories(l)[:, :n])
            assert hashlib.sha256(lm.tobytes()).hexdigest() == str(z["lm_sha256"])
