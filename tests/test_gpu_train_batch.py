"""Batched template training on the device (sbm_train_batch / sbm_train_batch_device) against the oracle's add_template,
bit for bit: levels, features, theta as bits, None where the oracle fails.  First BGR inputs on a two-level pyramid {4, 8}
with packed rows; then the other configurations a context accepts (one and three levels, gray, padded rows, odd sizes, the
widths at which the tie resolution's segment length changes) and training on a context that is matching.  Where
oracle/_ref/ref_train exists (the reference's own training half, tests/test_reference_train_half.py), the new tests hold
the device output to it as well, without the oracle's training half in between."""
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


# ---- the configurations a context accepts ---------------------------------------------------------------------------------
T_OF = {1: (4,), 2: (4, 8), 3: (4, 8, 8)}
# features per level the oracle keeps at num_features 63 on a three-level pyramid; None: the template fails
RECT_COUNTS = {(48, 200, None): (74, 30, 13), (48, 200, "cut_edge"): (67, 26, 11), (48, 200, "left_half"): (36, 15, 6),
               (97, 131, None): (66, 26, 8), (97, 131, "cut_edge"): (60, 22, 5), (97, 131, "left_half"): None}
MASKS = (None, "cut_edge", "left_half")


def mask_of(name, rows, cols):
    return None if name is None else getattr(TC, name)(rows, cols)


def reference_result(oracle, img, mask, n_levels, nf, strong):
    """what the reference's own training half makes of the oracle's gradient planes, or None where this host has no binary"""
    from oracle import ref_train as RT

    if RT.missing_binaries():
        return None
    return RT.run(RT.planes_of(oracle, img, mask, n_levels, TC.WEAK, TC.nearest_mask), nf, strong)


def check_image(oracle, got, status, img, mask, n_levels, nf, strong=TC.STRONG, counts=None):
    """one image of a device batch against the oracle and, where present, the reference binary; returns the oracle's result"""
    from oracle import ref_train as RT

    want = TC.want(oracle, img, mask, nf, strong, n_levels)
    failed = oracle.add_template_failing_level(img, mask, n_levels, nf, TC.WEAK, strong)
    ref = reference_result(oracle, img, mask, n_levels, nf, strong)
    if isinstance(ref, RT.Failed):
        assert want is None and failed == ref.level
        failed = ref.level  # the level the reference names
    elif ref is not None:
        assert TC.same_template(got, ref)
    if want is None:
        assert got is None and status.tolist() == [1, failed]
    else:
        assert status.tolist() == [0, len(want[1])]
        assert TC.same_template(got, want)
        if counts is not None:
            assert TC.counts(want) == counts
    return want


class DeviceTrain:
    """a batch in device memory with rows of cols * ch + row_pad bytes and images rows * stride + img_pad bytes apart, the
    padding filled with 0xA5; a mask per image where masks are given (None among them: all set)"""

    def __init__(self, ctx, imgs, masks=None, row_pad=0, img_pad=0, stream=None):
        import torch

        from shape_based_matching_amd.capi import TRAIN_FEATURE_DTYPE
        from shape_based_matching_amd.templates import LEVEL_DTYPE

        self.torch, self.ctx, self.L = torch, ctx, ctx.n_levels
        self.dev = torch.device("cuda", 0)
        self.n = n = len(imgs)
        self.rows, self.cols = imgs[0].shape[:2]
        self.ch = 1 if imgs[0].ndim == 2 else 3
        assert all(im.shape == imgs[0].shape for im in imgs)
        self.stride = self.cols * self.ch + row_pad
        self.img_stride = self.rows * self.stride + img_pad
        buf = np.full((n, self.img_stride), 0xA5, np.uint8)
        for i, im in enumerate(imgs):
            buf[i, : self.rows * self.stride].reshape(self.rows, self.stride)[:, : self.cols * self.ch] = im.reshape(self.rows, self.cols * self.ch)
        self.d_imgs = torch.from_numpy(buf).to(self.dev)
        self.d_masks, self.mask_stride = None, 0
        if masks is not None and any(m is not None for m in masks):
            self.mask_stride = self.rows * self.cols + 24
            mbuf = np.full((n, self.mask_stride), 0xA5, np.uint8)
            for i, m in enumerate(masks):
                mbuf[i, : self.rows * self.cols] = 255 if m is None else m.reshape(-1)
            self.d_masks = torch.from_numpy(mbuf).to(self.dev)
        self.cap = sum(((self.rows >> l) + 2) // 3 * (((self.cols >> l) + 2) // 3) for l in range(self.L))
        self.lv_dtype, self.ft_dtype = LEVEL_DTYPE, TRAIN_FEATURE_DTYPE
        self.d_lv = torch.zeros(n * self.L * LEVEL_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        self.d_ft = torch.zeros(n * self.cap * TRAIN_FEATURE_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        self.d_st = torch.full((n * 2,), -7, dtype=torch.int32, device=self.dev)
        self.stream = stream or torch.cuda.Stream(device=self.dev)
        torch.cuda.synchronize()

    def enqueue(self, nf, strong=TC.STRONG):
        self.ctx.train_batch_device(self.d_imgs.data_ptr(), self.img_stride, self.n, self.rows, self.cols, self.stride, self.ch, strong, nf,
                                    self.d_lv.data_ptr(), self.d_ft.data_ptr(), self.cap, self.d_st.data_ptr(), stream=self.stream.cuda_stream,
                                    d_masks=0 if self.d_masks is None else self.d_masks.data_ptr(), mask_stride=self.mask_stride)

    def fetch(self):
        """(templates, status[n, 2], raw bytes of the three outputs) after the stream has drained"""
        self.stream.synchronize()
        lv = self.d_lv.cpu().numpy().view(self.lv_dtype).reshape(self.n, self.L)
        ft = self.d_ft.cpu().numpy().view(self.ft_dtype).reshape(self.n, self.cap)
        st = self.d_st.cpu().numpy().reshape(self.n, 2)
        return unpack(lv, ft, st), st, (lv.tobytes(), ft.tobytes(), st.tobytes())

    def run(self, nf, strong=TC.STRONG):
        self.enqueue(nf, strong)
        return self.fetch()


def shifted_rectangle(rows, cols):
    """the rectangle moved down 3 and right 5: a second content of the same geometry"""
    return np.ascontiguousarray(np.roll(TC.rectangle(rows, cols), (3, 5), axis=(0, 1)))


@pytest.mark.parametrize("rows,cols", [(48, 200), (97, 131)])
@pytest.mark.parametrize("n_levels", [1, 3])
def test_other_pyramids(ctx_factory, oracle, n_levels, rows, cols):
    """T = (4,) and (4, 8, 8): the rectangle and a moved copy under no mask, a mask that cuts an edge and the left half, the six
    images in one call; at three levels 97 x 131 under its left half fails at the last level, next to images that do not"""
    ctx = ctx_factory(T=T_OF[n_levels])
    contents = [TC.rectangle(rows, cols), shifted_rectangle(rows, cols)]
    imgs = [im for im in contents for _ in MASKS]
    masks = [mask_of(m, rows, cols) for _ in contents for m in MASKS]
    got, st, _ = DeviceTrain(ctx, imgs, masks).run(63)
    for i, (im, m) in enumerate(zip(imgs, masks)):
        cnt = RECT_COUNTS[(rows, cols, MASKS[i])] if i < 3 else None
        want = check_image(oracle, got[i], st[i], im, m, n_levels, 63, counts=None if cnt is None else cnt[:n_levels])
        if i < 3 and n_levels == 3:
            assert (want is None) == (cnt is None)
    if n_levels == 3 and (rows, cols) == (97, 131):
        assert st[2].tolist() == [1, 2]
    check(ctx.train_batch(imgs, masks, TC.STRONG, 63), [TC.want(oracle, im, m, 63, TC.STRONG, n_levels) for im, m in zip(imgs, masks)])


@pytest.mark.parametrize("n_levels", [1, 2, 3])
def test_gray(ctx_factory, oracle, n_levels):
    """single-channel images (the green channel of the rectangles) at one, two and three levels"""
    ctx = ctx_factory(T=T_OF[n_levels])
    for rows, cols in ((48, 200), (97, 131)):
        imgs = [TC.gray(TC.rectangle(rows, cols))] * 3
        masks = [mask_of(m, rows, cols) for m in MASKS]
        assert imgs[0].ndim == 2
        got, st, _ = DeviceTrain(ctx, imgs, masks).run(63)
        wants = [check_image(oracle, got[i], st[i], imgs[i], masks[i], n_levels, 63) for i in range(3)]
        assert any(w is not None for w in wants)
        check(ctx.train_batch(imgs, masks, TC.STRONG, 63), wants)


def test_gray_noise(ctx_factory, oracle):
    """gray noise of odd size at strong_threshold 10, one level: 66 features kept of 63 asked, 205 candidates in all"""
    ctx = ctx_factory(T=(4,))
    img = TC.gray(TC.noise(131, 97, 7))
    b = DeviceTrain(ctx, [img])
    for nf, n in ((63, 66), (100000, 205)):
        got, st, _ = b.run(nf, 10.0)
        check_image(oracle, got[0], st[0], img, None, 1, nf, 10.0, counts=(n,))
    check(ctx.train_batch([img], None, 10.0, 63), [TC.want(oracle, img, None, 63, 10.0, 1)])


@pytest.mark.parametrize("gray", [False, True])
def test_padded_rows(ctx_factory, oracle, gray):
    """rows of cols * ch + 13 bytes and images further apart than rows * stride, the padding filled with 0xA5: the packed call's
    output, byte for byte"""
    ctx = ctx_factory()
    imgs = [TC.rectangle(50, 70), TC.noise(50, 70, 2), shifted_rectangle(50, 70)]
    if gray:
        imgs = [TC.gray(im) for im in imgs]
    masks = [TC.cut_edge(50, 70), None, TC.left_half(50, 70)]
    for strong in (TC.STRONG, 10.0):
        packed = DeviceTrain(ctx, imgs, masks).run(63, strong)
        padded = DeviceTrain(ctx, imgs, masks, row_pad=13, img_pad=1000)
        assert padded.stride == 70 * (1 if gray else 3) + 13 and padded.img_stride > 50 * padded.stride
        got, st, raw = padded.run(63, strong)
        assert raw == packed[2]
        wants = [check_image(oracle, got[i], st[i], imgs[i], masks[i], 2, 63, strong) for i in range(3)]
        assert any(w is not None for w in wants)


@pytest.mark.parametrize("rows,cols,n_levels", [(51, 71, 2), (97, 131, 3)])
def test_odd_sizes_with_masks(ctx_factory, oracle, rows, cols, n_levels):
    """odd rows and columns at every level but the last, a mask per image: the nearest-neighbour mask chain from odd sources"""
    ctx = ctx_factory(T=T_OF[n_levels])
    rs = np.random.RandomState(rows)
    imgs = [TC.rectangle(rows, cols), shifted_rectangle(rows, cols), TC.rectangle(rows, cols), TC.rectangle(rows, cols)]
    masks = [(rs.rand(rows, cols) > 0.05).astype(np.uint8) * 255, (rs.rand(rows, cols) > 0.03).astype(np.uint8) * 255, TC.cut_edge(rows, cols), None]
    got, st, _ = DeviceTrain(ctx, imgs, masks).run(63)
    wants = [check_image(oracle, got[i], st[i], imgs[i], masks[i], n_levels, 63) for i in range(4)]
    assert wants[3] is not None and sum(w is not None for w in wants) >= 3
    assert not TC.same_template(wants[0], wants[3])  # the random mask matters
    check(ctx.train_batch(imgs, masks, TC.STRONG, 63), wants)


@pytest.mark.parametrize("cols", sorted(TC.SEGMENT_SEEDS))
def test_resolve_segment_boundaries(ctx_factory, oracle, cols):
    """64, 65, 128 and 129 columns: one, two (with idle lanes), two and three columns per lane of the tie resolution; a
    rectangle, and noise whose candidates reach the last three scanned columns"""
    ctx = ctx_factory(T=(4,))
    rows = TC.SEGMENT_ROWS
    rect, noise = TC.rectangle(rows, cols), TC.noise(rows, cols, TC.SEGMENT_SEEDS[cols])
    assert TC.candidates_in_last_columns(oracle, noise, 10.0) >= 1
    b = DeviceTrain(ctx, [rect, noise])
    for nf in (16, 100000):
        got, st, _ = b.run(nf, 10.0)
        wants = [check_image(oracle, got[i], st[i], im, None, 1, nf, 10.0) for i, im in enumerate((rect, noise))]
        assert all(w is not None for w in wants)
    got, st, _ = b.run(63)
    assert check_image(oracle, got[0], st[0], rect, None, 1, 63) is not None
    check_image(oracle, got[1], st[1], noise, None, 1, 63)


# ---- training on a context that is matching ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def match_world(oracle):
    """three 512 x 640 frames (those of test_gpu_sparse_strips.py), their oracle match lists and the first frame's pyramid"""
    import test_gpu_sparse_strips as S
    from shape_based_matching_amd import synth

    ts = S.load_templates()
    centre = S.make_frames(None)
    frames = [centre, S.shifted(centre, 0, -16), synth.scene_bgr(5, S.ROWS, S.COLS)]
    want, p0 = [], None
    for i, f in enumerate(frames):
        p = oracle.Pyramid.build(f, [4, 8], 30.0)
        want.append(S.multiset(p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, S.THR, n_threads=S.NT)))
        if i == 0:
            p0 = p
        else:
            p.free()
    assert len(want[0]) > 20 and len(want[1]) > 20
    yield {"S": S, "ts": ts, "frames": frames, "want": want, "p0": p0}
    p0.free()


TRAIN_KERNELS = ["k_train_maxima", "k_train_resolve", "k_train_sort", "k_train_select", "k_train_crop"]


@pytest.mark.parametrize("mode", ["plain", "graph", "profiling"])
def test_training_on_a_context_in_use(ctx_factory, oracle, match_world, mode):
    """one {4, 8} context, one caller stream, no host synchronisation between the calls: a batched match of three frames, a
    training batch, the template loop on the resident pyramid, then the first level's linear memories.  Every match list,
    the planes and the templates are the oracle's; a training call adds no graph; its timings name its five kernels once."""
    import torch

    from shape_based_matching_amd.templates import MATCH_DTYPE

    S, w = match_world["S"], match_world
    ctx = ctx_factory()
    ctx.upload_templates(w["ts"])
    if mode == "graph":
        ctx.set_pipeline_depth(2)
        ctx.set_graph_mode(True)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    B, CAP, REC = 3, S.CAP, MATCH_DTYPE.itemsize
    d_img = torch.from_numpy(np.stack(w["frames"])).to(dev)
    d_out = torch.zeros(B * CAP * REC, dtype=torch.uint8, device=dev)
    d_cnt = torch.full((B * 2,), -1, dtype=torch.int32, device=dev)
    d_one = torch.zeros(CAP * REC, dtype=torch.uint8, device=dev)
    d_one_cnt = torch.full((2,), -1, dtype=torch.int32, device=dev)
    imgs = [TC.rectangle(96, 96)] * 3 + [np.ascontiguousarray(TC.rectangle(96, 96)[:, ::-1])]
    masks = [None, TC.left_half(96, 96), TC.cut_edge(96, 96), TC.cut_edge(96, 96)]
    train = DeviceTrain(ctx, imgs, masks, stream=st)
    wants = [TC.want(oracle, im, m, 63) for im, m in zip(imgs, masks)]
    assert all(x is not None for x in wants)
    torch.cuda.synchronize()
    if mode == "profiling":
        ctx.set_profiling(True)
    rounds = 2  # the first round grows the training scratch and, in graph mode, captures; the second is the steady state
    for rnd in range(rounds):
        d_out.zero_(), d_cnt.fill_(-1), d_one.zero_(), d_one_cnt.fill_(-1), train.d_st.fill_(-7), train.d_ft.zero_(), train.d_lv.zero_()
        torch.cuda.synchronize()
        for _ in range(2 if mode == "graph" else 1):
            ctx.match_batch_device(d_img.data_ptr(), w["frames"][0].size, B, S.ROWS, S.COLS, S.COLS * 3, 3, S.THR, d_out.data_ptr(), CAP,
                                   d_cnt.data_ptr(), stream=st.cuda_stream)
        graphs = ctx.graph_count()
        train.enqueue(63)
        assert ctx.graph_count() == graphs
        if mode == "graph":  # the batched match replays its capture; later rounds also hold the template loop's
            assert graphs >= 1
        if mode == "profiling":  # reading a call's timings waits for its kernels: the one host wait of this mode
            names = [n for n, _ in ctx.timings()]
            assert [n for n in names if n.startswith("k_train_")] == TRAIN_KERNELS, names
        ctx.match_templates_device(S.THR, d_one.data_ptr(), CAP, d_one_cnt.data_ptr(), stream=st.cuda_stream)
        lm0 = ctx.get_linear_memories(0)
        got, status, _ = train.fetch()
        cnt = d_cnt.cpu().numpy().reshape(B, 2)
        recs = d_out.cpu().numpy().view(MATCH_DTYPE).reshape(B, CAP)
        assert (cnt[:, 1] == 0).all() and (cnt[:, 0] >= 0).all() and (cnt[:, 0] <= CAP).all(), cnt
        for b in range(B):
            assert S.multiset(recs[b, : cnt[b, 0]]) == w["want"][b], (rnd, b)
        one = d_one_cnt.cpu().numpy()
        assert one[1] == 0 and S.multiset(d_one.cpu().numpy().view(MATCH_DTYPE)[: max(int(one[0]), 0)]) == w["want"][0], rnd
        n0 = S.ROWS * S.COLS
        assert np.array_equal(lm0[:, :n0], w["p0"].lm(0)[:, :n0]), rnd
        for i in range(len(imgs)):
            assert status[i].tolist() == [0, len(wants[i][1])], (rnd, i)
        check(got, wants)
    ref = [reference_result(oracle, im, m, 2, 63, TC.STRONG) for im, m in zip(imgs, masks)]
    if ref[0] is not None:
        check(got, ref)
