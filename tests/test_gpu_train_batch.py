"""Batched template training on the device (sbm_train_batch / sbm_train_batch_device) against the oracle's add_template,
bit for bit: levels, features, theta as bits, None where the oracle fails.  BGR inputs, pyramid {4, 8} (two levels)."""
import numpy as np
import pytest

import train_batch_cases as TC

pytestmark = pytest.mark.gpu

NOISE_SEED = 139  # 71 candidates at level 0 (asserted below): more than the selection's workgroup has threads
SELECT_THREADS = 64


def all_set(r, c):
    return np.full((r, c), 255, np.uint8)


def check(got, wants):
    assert len(got) == len(wants)
    for i, (g, w) in enumerate(zip(got, wants)):
        assert TC.same_template(g, w), i


@pytest.mark.parametrize("rows,cols", [(96, 96), (64, 64), (50, 70)])
def test_plateaus(ctx_factory, oracle, rows, cols):
    """rectangles: straight edges are long plateaus of equal squared magnitude, so the row-major tie chain decides nearly
    every maximum; num_features 16 keeps more than asked, 63 and 128 on the small images take every candidate"""
    ctx = ctx_factory()
    img = TC.rectangle(rows, cols)
    assert TC.s_pairs(oracle.quantized_orientations(img, TC.WEAK)[0]) >= 100
    for nf in (16, 63, 128):
        want = TC.want(oracle, img, None, nf)
        assert want is not None
        check(ctx.train_batch([img], None, TC.STRONG, nf), [want])
    assert tuple(int(v) for v in TC.want(oracle, TC.rectangle(96, 96), None, 16)[0]["n_features"]) == (27, 11)


def test_masks(ctx_factory, oracle):
    """no mask, all set, the left half, a mask that cuts one edge -- one batch, a mask per image, one image without"""
    ctx = ctx_factory()
    img = TC.rectangle(96, 96)
    masks = [None, all_set(96, 96), TC.left_half(96, 96), TC.cut_edge(96, 96)]
    wants = [TC.want(oracle, img, m, 63) for m in masks]
    assert all(w is not None for w in wants)
    assert tuple(int(v) for v in wants[2][0]["n_features"]) == (28, 9)
    assert TC.same_template(wants[0], wants[1]) and not TC.same_template(wants[0], wants[3])
    check(ctx.train_batch([img] * 4, masks, TC.STRONG, 63), wants)
    check(ctx.train_batch([img] * 2, None, TC.STRONG, 63), wants[:1] * 2)


class DeviceBatch:
    """a batch in device memory for the device form, on a stream of the caller's"""

    def __init__(self, ctx, imgs, pad_bytes=0):
        import torch

        self.torch, self.ctx = torch, ctx
        self.dev = torch.device("cuda", 0)
        self.n = len(imgs)
        self.rows, self.cols, self.ch = imgs[0].shape
        self.img_stride = self.rows * self.cols * self.ch + pad_bytes
        buf = np.full((self.n, self.img_stride), 0xA5, np.uint8)
        for i, im in enumerate(imgs):
            buf[i, : im.size] = im.reshape(-1)
        self.d_imgs = torch.from_numpy(buf).to(self.dev)
        self.cap = sum(((self.rows >> l) + 2) // 3 * (((self.cols >> l) + 2) // 3) for l in range(TC.N_LEVELS))
        self.stream = torch.cuda.Stream(device=self.dev)

    def run(self, nf, d_masks=None, mask_stride=0, cap=None, strong=TC.STRONG):
        from shape_based_matching_amd.capi import TRAIN_FEATURE_DTYPE
        from shape_based_matching_amd.templates import LEVEL_DTYPE

        torch, cap = self.torch, self.cap if cap is None else cap
        d_lv = torch.zeros(self.n * TC.N_LEVELS * LEVEL_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        d_ft = torch.zeros(max(self.n * cap, 1) * TRAIN_FEATURE_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        d_st = torch.zeros(self.n * 2, dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize()
        self.ctx.train_batch_device(self.d_imgs.data_ptr(), self.img_stride, self.n, self.rows, self.cols, self.cols * self.ch, self.ch, strong, nf,
                                    d_lv.data_ptr(), d_ft.data_ptr(), cap, d_st.data_ptr(), stream=self.stream.cuda_stream,
                                    d_masks=0 if d_masks is None else d_masks.data_ptr(), mask_stride=mask_stride)
        self.stream.synchronize()
        lv = d_lv.cpu().numpy().view(LEVEL_DTYPE).reshape(self.n, TC.N_LEVELS)
        ft = d_ft.cpu().numpy().view(TRAIN_FEATURE_DTYPE)[: self.n * cap].reshape(self.n, cap)
        return lv, ft, d_st.cpu().numpy().reshape(self.n, 2)


def unpack(lv, ft, st):
    return [None if st[i, 0] == 1 else (lv[i], ft[i, : st[i, 1]]) for i in range(len(st))]


def test_device_form_on_a_caller_stream_and_shared_mask(ctx_factory, oracle):
    """img_stride > rows * stride; one mask for all images (mask_stride 0); a mask per image; equal to the host form"""
    import torch

    ctx = ctx_factory()
    imgs = [TC.rectangle(96, 96), np.ascontiguousarray(TC.rectangle(96, 96)[::-1]), TC.noise(96, 96, 3)]
    b = DeviceBatch(ctx, imgs, pad_bytes=1000)
    mask = TC.cut_edge(96, 96)
    wants = [TC.want(oracle, im, mask, 63) for im in imgs]
    lv, ft, st = b.run(63, torch.from_numpy(mask).to(b.dev), 0)
    assert st[:, 0].tolist() == [0 if w is not None else 1 for w in wants]
    check(unpack(lv, ft, st), wants)
    check(ctx.train_batch(imgs, [mask] * 3, TC.STRONG, 63), wants)
    masks = [TC.left_half(96, 96), all_set(96, 96), mask]
    mbuf = np.zeros((3, 96 * 96 + 40), np.uint8)
    for i, m in enumerate(masks):
        mbuf[i, : 96 * 96] = m.reshape(-1)
    lv, ft, st = b.run(63, torch.from_numpy(mbuf).to(b.dev), 96 * 96 + 40)
    check(unpack(lv, ft, st), [TC.want(oracle, im, m, 63) for im, m in zip(imgs, masks)])
    lv, ft, st = b.run(63)
    check(unpack(lv, ft, st), [TC.want(oracle, im, None, 63) for im in imgs])


FAILING = [lambda: (TC.rectangle(64, 64), TC.left_half(64, 64)), lambda: (TC.constant(64, 64), None)]


@pytest.mark.parametrize("n", [1, 3, 9])
def test_failure_and_isolation(ctx_factory, oracle, n):
    """failing images first, in the middle and last: every image's output is its single-image oracle result"""
    ctx = ctx_factory()
    good = [(TC.rectangle(64, 64), None), (TC.noise(64, 64, 5), None), (TC.rectangle(64, 64), TC.cut_edge(64, 64))]
    for where in ("first", "middle", "last"):
        items = [good[i % 3] for i in range(n)]
        bad = {"first": [0], "middle": [n // 2], "last": [n - 1]}[where] + ([1, n - 2] if n == 9 else [])
        for j, k in enumerate(bad):
            items[k] = FAILING[j % 2]()
        imgs, masks = [a for a, _ in items], [m for _, m in items]
        wants = [TC.want(oracle, a, m, 63) for a, m in items]
        assert all(wants[k] is None for k in bad) and (n == 1 or any(w is not None for w in wants))
        lv, ft, st = ctx.train_batch_raw(imgs, masks, TC.STRONG, 63, 600)
        for i, w in enumerate(wants):
            if w is None:
                assert st[i, 0] == 1 and st[i, 1] in (0, 1)
            else:
                assert st[i].tolist() == [0, len(w[1])]
        check(unpack(lv, ft, st), wants)


def test_failing_rectangles_under_their_left_half(ctx_factory, oracle):
    ctx = ctx_factory()
    for r, c in ((50, 70), (64, 64)):
        assert TC.want(oracle, TC.rectangle(r, c), TC.left_half(r, c), 63) is None
        assert ctx.train_batch([TC.rectangle(r, c)], [TC.left_half(r, c)], TC.STRONG, 63) == [None]
    assert TC.want(oracle, TC.constant(64, 64), None, 63) is None
    assert ctx.train_batch([TC.constant(64, 64)], None, TC.STRONG, 63) == [None]


def test_many_candidates(ctx_factory, oracle):
    """uniform noise at strong_threshold 10: more candidates at level 0 than the selection's workgroup has threads (asked of
    the oracle: with more features asked than there are candidates it keeps every candidate)"""
    ctx = ctx_factory()
    img = TC.noise(64, 64, NOISE_SEED)
    everything = TC.want(oracle, img, None, 100000, strong=10.0)
    assert int(everything[0]["n_features"][0]) > SELECT_THREADS
    for nf in (16, 63, 100000):
        check(ctx.train_batch([img], None, 10.0, nf), [TC.want(oracle, img, None, nf, strong=10.0)])


def test_hundreds_of_candidates(ctx_factory, oracle):
    """256 x 256 noise at strong_threshold 10: about a thousand candidates at level 0 -- more than the 256 threads of the sort
    and crop workgroups and more than 512 keys, so every thread of the sort handles several pairs per stage, the selection
    walks many chunks, and with every candidate kept the crop's strided loops run several rounds"""
    ctx = ctx_factory()
    img = TC.noise(256, 256, 1)
    everything = TC.want(oracle, img, None, 100000, strong=10.0)
    assert int(everything[0]["n_features"][0]) > 512 and int(everything[0]["n_features"][1]) > 256
    for nf in (63, 100000):
        check(ctx.train_batch([img], None, 10.0, nf), [TC.want(oracle, img, None, nf, strong=10.0)])


def test_kept_set_beyond_lds(ctx_factory, oracle):
    """544 x 544 noise with every candidate kept: more kept features at level 0 than the selection kernel holds in LDS
    (TRAIN_KEPT_LDS = 4096), so the tail of the kept set is written to and read from global scratch"""
    ctx = ctx_factory()
    img = TC.noise(544, 544, 1)
    want = TC.want(oracle, img, None, 100000, strong=10.0)
    assert int(want[0]["n_features"][0]) > 4096 + 64
    check(ctx.train_batch([img], None, 10.0, 100000), [want])
    # a distance of 2 and more: candidates are tested against a kept set that has outgrown LDS
    for nf in (2500, 4500):
        check(ctx.train_batch([img], None, 10.0, nf), [TC.want(oracle, img, None, nf, strong=10.0)])


def test_reference_roi(ctx_factory, oracle, case1):
    ctx = ctx_factory()
    img, mask = TC.fixture_roi(case1)
    want = TC.want(oracle, img, mask, 128)
    assert want is not None
    check(ctx.train_batch([img], [mask], TC.STRONG, 128), [want])


def test_capacity(ctx_factory, oracle):
    """feat_cap one short of the middle image's total: status 2 with the needed count, the neighbours intact"""
    ctx = ctx_factory()
    imgs = [TC.rectangle(96, 96)] * 3
    masks = [TC.left_half(96, 96), None, TC.cut_edge(96, 96)]
    wants = [TC.want(oracle, im, m, 63) for im, m in zip(imgs, masks)]
    totals = [len(w[1]) for w in wants]
    assert totals[1] > max(totals[0], totals[2]), totals
    lv, ft, st = ctx.train_batch_raw(imgs, masks, TC.STRONG, 63, totals[1] - 1)
    assert st.tolist() == [[0, totals[0]], [2, totals[1]], [0, totals[2]]]
    for i in (0, 2):
        assert TC.same_template((lv[i], ft[i, : st[i, 1]]), wants[i])
    lv, ft, st = ctx.train_batch_raw(imgs, masks, TC.STRONG, 63, totals[1])
    check(unpack(lv, ft, st), wants)


def test_same_bytes_twice(ctx_factory):
    ctx = ctx_factory()
    imgs = [TC.rectangle(50, 70), TC.noise(50, 70, 2), TC.constant(50, 70)]
    masks = [None, TC.left_half(50, 70), None]
    a = ctx.train_batch_raw(imgs, masks, TC.STRONG, 63, 300)
    b = ctx.train_batch_raw(imgs, masks, TC.STRONG, 63, 300)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_argument_errors(ctx_factory):
    import ctypes as C

    import torch

    from shape_based_matching_amd import capi

    ctx = ctx_factory()
    b = DeviceBatch(ctx, [TC.rectangle(64, 64)])
    d_mask = torch.full((64 * 64,), 255, dtype=torch.uint8, device=b.dev)
    for stride in (1, 64 * 64 - 1, -64 * 64):
        with pytest.raises(capi.SbmError) as e:
            b.run(63, d_mask, stride)
        assert e.value.code == -1
    d = torch.zeros(1 << 16, dtype=torch.uint8, device=b.dev)
    p = d.data_ptr()

    def rc(rows=64, cols=64, stride=192, ch=3, n=1, nf=63, imgs=p, lv=p, st=p, cap=0):
        return capi.lib().sbm_train_batch_device(ctx._h, C.c_void_p(imgs), 64 * 64 * 3, n, rows, cols, stride, ch, None, 0, C.c_float(60.0), nf,
                                                 C.c_void_p(lv), None, cap, C.c_void_p(st), None)

    for kw in (dict(rows=32768), dict(cols=32768), dict(n=0), dict(n=-1), dict(ch=2), dict(stride=191), dict(nf=0), dict(nf=1), dict(imgs=None),
               dict(lv=None), dict(st=None), dict(cap=-1), dict(cap=5), dict(rows=5), dict(cols=4)):
        assert rc(**kw) == -1, kw
    lv, ft, st = b.run(63)
    assert st[0, 0] == 0
