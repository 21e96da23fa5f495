"""Ragged batched training (sbm_train_ragged / sbm_train_ragged_device) and the device scale sweep (sbm_train_sweep) against
the oracle's add_template, bit for bit: levels, features, theta as bits, None where the oracle fails, and the failing level.
Images of different sizes, feature counts and masks in one call -- every (image, level) reads its own record of a device
table -- on the two-level pyramid {4, 8} of tests/train_batch_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest

import train_batch_cases as TC

pytestmark = pytest.mark.gpu


def check(got, wants):
    assert len(got) == len(wants)
    for i, (g, w) in enumerate(zip(got, wants)):
        assert TC.same_template(g, w), i


def wants_of(oracle, items, strong=TC.STRONG):
    return [TC.want(oracle, im, m, nf, strong) for im, m, nf in items]


def check_status(oracle, status, items, wants, strong=TC.STRONG):
    """{0, features} where the oracle succeeds, {1, the level addTemplate gives up at} where it does not"""
    for i, ((im, m, nf), w) in enumerate(zip(items, wants)):
        if w is None:
            assert status[i].tolist() == [1, oracle.add_template_failing_level(im, m, TC.N_LEVELS, nf, TC.WEAK, strong)], i
        else:
            assert status[i].tolist() == [0, len(w[1])], i


def run(ctx, items, strong=TC.STRONG):
    got, status = ctx.train_ragged_status([a for a, _, _ in items], [m for _, m, _ in items], strong, [nf for _, _, nf in items])
    return got, status


def plateau(rows, cols):
    """a constant image with a brighter block inside: four straight edges of equal magnitude, a constant border around them"""
    img = TC.constant(rows, cols)
    img[rows // 4: rows - rows // 4, 8: cols - 8] = 200
    return img


def test_one_mixed_call(ctx_factory, oracle):
    """sizes, feature counts, successes and failures mixed; the largest image neither first nor last; then reversed"""
    ctx = ctx_factory()
    items = [(TC.rectangle(64, 48), None, 63), (TC.noise(33, 57, 3), None, 63), (TC.rectangle(33, 57), None, 63), (TC.rectangle(5, 5), None, 63),
             (TC.rectangle(65, 129), None, 63), (TC.rectangle(40, 40), None, 8), (TC.rectangle(96, 96), None, 63), (TC.rectangle(11, 23), None, 63),
             (TC.rectangle(40, 40), None, 63), (TC.noise(65, 129, 3), None, 63), (TC.rectangle(1, 7), None, 63), (TC.rectangle(24, 200), None, 63)]
    sizes = [a.shape[0] * a.shape[1] for a, _, _ in items]
    assert 0 < int(np.argmax(sizes)) < len(items) - 1
    wants = wants_of(oracle, items)
    # what the oracle makes of them: the cases are the ones meant
    assert [None if w is None else list(TC.counts(w)) for w in wants] == [
        [28, 6], None, [20, 6], None, [54, 20], [8, 4], [56, 20], None, None, [64, 21], None, [66, 29]]
    failing = {i: oracle.add_template_failing_level(*items[i][:2], TC.N_LEVELS, items[i][2], TC.WEAK, TC.STRONG) for i in (1, 3, 7, 8, 10)}
    assert failing == {1: 1, 3: 0, 7: 0, 8: 1, 10: 0}  # too few candidates at level 1, at level 0, and levels that are not built
    for order in (list(range(len(items))), list(range(len(items)))[::-1]):
        its, ws = [items[k] for k in order], [wants[k] for k in order]
        got, status = run(ctx, its)
        check(got, ws)
        check_status(oracle, status, its, ws)


def test_per_image_num_features(ctx_factory, oracle):
    """63, 8 and 4 features asked of one geometry in one call: three single calls.  Not 2: halved to one feature at level
    1, where selectScatteredFeatures (line2Dup.cpp:163-212) never returns -- its first candidate is always enough, so it
    clears and widens the distance for ever -- and the device selection follows it step by step."""
    ctx = ctx_factory()
    img = TC.rectangle(96, 96)
    items = [(img, None, 63), (img, None, 8), (img, None, 4)]
    wants = wants_of(oracle, items)
    assert all(w is not None for w in wants) and len({TC.counts(w) for w in wants}) == 3
    got, _ = run(ctx, items)
    check(got, wants)
    for g, (im, _, nf) in zip(got, items):
        check([g], ctx.train_batch([im], None, TC.STRONG, nf))


def test_masks_on_some_images(ctx_factory, oracle):
    ctx = ctx_factory()
    items = [(TC.rectangle(96, 96), TC.left_half(96, 96), 63), (TC.rectangle(64, 48), None, 63), (TC.rectangle(65, 129), TC.cut_edge(65, 129), 63),
             (TC.rectangle(96, 96), None, 63), (TC.rectangle(64, 64), TC.left_half(64, 64), 63), (TC.rectangle(33, 57), TC.cut_edge(33, 57), 16),
             (TC.rectangle(96, 96), TC.cut_edge(96, 96), 63), (TC.rectangle(24, 200), TC.left_half(24, 200), 63)]
    wants = wants_of(oracle, items)
    assert wants[4] is None and sum(w is not None for w in wants) >= 5
    assert not TC.same_template(wants[3], wants[6]) and not TC.same_template(wants[0], wants[3])
    got, status = run(ctx, items)
    check(got, wants)
    check_status(oracle, status, items, wants)


def test_feat_cap_too_small_for_one_image(ctx_factory, oracle):
    """status 2 with the needed count for that image alone; guard records before and after every block keep their fill"""
    from shape_based_matching_amd.capi import TRAIN_FEATURE_DTYPE

    ctx = ctx_factory()
    items = [(TC.rectangle(64, 48), None, 63), (TC.rectangle(96, 96), None, 63), (TC.rectangle(33, 57), None, 63), (TC.noise(33, 57, 3), None, 63)]
    wants = wants_of(oracle, items)
    totals = [None if w is None else len(w[1]) for w in wants]
    assert totals[1] is not None and totals[3] is None
    caps = [totals[0], totals[1] - 1, totals[2], 5]
    guard = 3
    firsts, at = [], guard
    for c in caps:
        firsts.append(at)
        at += c + guard
    fill = np.zeros(at, TRAIN_FEATURE_DTYPE)
    fill["x"], fill["y"], fill["label"], fill["theta"] = -77, -78, -79, np.float32(-80.5)
    feats = fill.copy()
    lv, ft, st, _ = ctx.train_ragged_raw([a for a, _, _ in items], None, TC.STRONG, [63] * 4, caps, firsts, feats)
    assert ft is feats
    assert st.tolist() == [[0, totals[0]], [2, totals[1]], [0, totals[2]], [1, oracle.add_template_failing_level(items[3][0], None, 2, 63, TC.WEAK, TC.STRONG)]]
    inside = np.zeros(at, bool)
    for i in (0, 2):
        inside[firsts[i]: firsts[i] + totals[i]] = True
        assert TC.same_template((lv[i], ft[firsts[i]: firsts[i] + totals[i]]), wants[i])
    assert np.array_equal(ft[~inside], fill[~inside])  # the guards, and the blocks of the two images that are not ok
    assert not lv[1]["n_features"].any() and not lv[3]["n_features"].any()
    # with room for it, the same call is right for every image
    caps[1] = totals[1]
    lv, ft, st, _ = ctx.train_ragged_raw([a for a, _, _ in items], None, TC.STRONG, [63] * 4, caps, firsts, fill.copy())
    assert st[1].tolist() == [0, totals[1]]
    assert TC.same_template((lv[1], ft[firsts[1]: firsts[1] + totals[1]]), wants[1])


def test_equal_geometry_is_train_batch(ctx_factory, oracle):
    ctx = ctx_factory()
    imgs = [TC.rectangle(96, 96), TC.noise(96, 96, 3), TC.checkerboard(96, 96), TC.constant(96, 96)]
    masks = [None, TC.cut_edge(96, 96), None, None]
    batch = ctx.train_batch(imgs, masks, TC.STRONG, 63)
    got, _ = run(ctx, [(a, m, 63) for a, m in zip(imgs, masks)])
    check(got, batch)
    check(got, wants_of(oracle, [(a, m, 63) for a, m in zip(imgs, masks)]))
    assert batch[3] is None and batch[0] is not None


def test_ties_with_a_segment_length_per_image(ctx_factory, oracle):
    """widths 65 and 129 next to 200: the tie resolution's lanes own 2, 3 and 4 columns in one launch"""
    ctx = ctx_factory()
    items = [(TC.checkerboard(48, 65, block=16), None, 16), (plateau(40, 200), None, 63), (TC.checkerboard(64, 129, block=16), None, 16),
             (plateau(24, 65), None, 16), (plateau(32, 129), None, 63), (TC.checkerboard(48, 200, block=16), None, 16), (TC.checkerboard(24, 65), None, 63)]
    for im, _, _ in items:
        assert TC.s_pairs(oracle.quantized_orientations(im, TC.WEAK)[0]) >= 20  # ties to resolve, in every image
    wants = wants_of(oracle, items)
    assert [w is not None for w in wants] == [True] * 6 + [False]
    got, status = run(ctx, items)
    check(got, wants)
    check_status(oracle, status, items, wants)


class DeviceList:
    """a list of images in device memory with the device form's descriptors and outputs"""

    def __init__(self, ctx, imgs, nfs, dev):
        import torch

        from shape_based_matching_amd import capi
        from shape_based_matching_amd.templates import LEVEL_DTYPE

        self.n = len(imgs)
        self.d_imgs = [torch.from_numpy(np.ascontiguousarray(im)).to(dev) for im in imgs]
        self.caps = [ctx._feature_cap(im.shape[0], im.shape[1]) for im in imgs]
        self.firsts = [int(v) for v in np.cumsum([0] + self.caps)[:-1]]
        self.desc = [capi.SbmTrainImage(d.data_ptr(), None, im.shape[0], im.shape[1], im.shape[1] * im.shape[2], nf, f, c)
                     for d, im, nf, f, c in zip(self.d_imgs, imgs, nfs, self.firsts, self.caps)]
        self.d_lv = torch.zeros(self.n * TC.N_LEVELS * LEVEL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_ft = torch.zeros(sum(self.caps) * capi.TRAIN_FEATURE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_st = torch.zeros(self.n * 2, dtype=torch.int32, device=dev)

    def results(self):
        from shape_based_matching_amd import capi
        from shape_based_matching_amd.templates import LEVEL_DTYPE

        lv = self.d_lv.cpu().numpy().view(LEVEL_DTYPE).reshape(self.n, TC.N_LEVELS)
        ft = self.d_ft.cpu().numpy().view(capi.TRAIN_FEATURE_DTYPE)
        st = self.d_st.cpu().numpy().reshape(self.n, 2)
        return [None if st[i, 0] == 1 else (lv[i], ft[self.firsts[i]: self.firsts[i] + st[i, 1]]) for i in range(self.n)]


def test_two_calls_back_to_back_on_one_stream(ctx_factory, oracle):
    """different lists, no synchronisation between the calls: a call's table must not reach the kernels of the call before it.
    A 473 x 600 noise image goes first -- milliseconds in the single-wave kernels -- so the copies of the calls behind it are
    still pending on the stream when the next call wants the pinned slot they read from."""
    import torch

    ctx = ctx_factory()
    dev = torch.device("cuda", 0)
    long_items = [(TC.noise(473, 600, 7), None, 63)]
    a_items = [(TC.rectangle(96, 96), None, 63), (TC.rectangle(33, 57), None, 63), (TC.noise(65, 129, 3), None, 63), (TC.rectangle(5, 5), None, 63)]
    b_items = [(TC.rectangle(24, 200), None, 63), (TC.rectangle(40, 40), None, 8), (TC.rectangle(64, 48), None, 63)]
    # a first call of the larger list, so that neither timed call has to grow the scratch (which waits for the device)
    run(ctx, long_items + a_items + b_items)
    first = DeviceList(ctx, [i[0] for i in long_items], [i[2] for i in long_items], dev)
    a = DeviceList(ctx, [i[0] for i in a_items], [i[2] for i in a_items], dev)
    b = DeviceList(ctx, [i[0] for i in b_items], [i[2] for i in b_items], dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ctx.train_ragged_device(first.desc, 3, TC.STRONG, first.d_lv.data_ptr(), first.d_ft.data_ptr(), first.d_st.data_ptr(), stream=stream.cuda_stream)
    ctx.train_ragged_device(a.desc, 3, TC.STRONG, a.d_lv.data_ptr(), a.d_ft.data_ptr(), a.d_st.data_ptr(), stream=stream.cuda_stream)
    ctx.train_ragged_device(b.desc, 3, TC.STRONG, b.d_lv.data_ptr(), b.d_ft.data_ptr(), b.d_st.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    check(first.results(), wants_of(oracle, long_items))
    check(a.results(), wants_of(oracle, a_items))
    check(b.results(), wants_of(oracle, b_items))


def test_argument_errors_leave_the_context_usable(ctx_factory, oracle):
    from shape_based_matching_amd import capi

    ctx = ctx_factory()
    good_items = [(TC.rectangle(64, 48), None, 63), (TC.rectangle(96, 96), None, 63)]
    good_wants = wants_of(oracle, good_items)
    img = np.ascontiguousarray(TC.rectangle(64, 48))
    levels = np.zeros((70000, TC.N_LEVELS), capi.LEVEL_DTYPE)
    feats = np.zeros(4096, capi.TRAIN_FEATURE_DTYPE)
    status = np.zeros((70000, 2), np.int32)

    def call(descs, n=None, ch=3):
        arr = (capi.SbmTrainImage * max(len(descs), 1))(*descs)
        return capi.lib().sbm_train_ragged(ctx._h, arr, len(descs) if n is None else n, ch, C.c_float(TC.STRONG), capi._p(levels), capi._p(feats),
                                           capi._p(status))

    def d(rows=64, cols=48, stride=None, nf=63, first=0, cap=100, ptr=img.ctypes.data):
        return capi.SbmTrainImage(ptr, None, rows, cols, cols * 3 if stride is None else stride, nf, first, cap)

    bad = {"no image": ([d()], 0), "too many": ([d()], 65536), "channels": ([d()], None, 2), "rows 0": ([d(rows=0)],), "cols over": ([d(cols=32768)],),
           "stride": ([d(), d(stride=143, first=100)],), "features 0": ([d(nf=0)],), "features halved away": ([d(nf=1)],),
           "one feature at level 1": ([d(), d(nf=2, first=100)],), "one feature at level 1, odd": ([d(nf=3)],),
           "negative cap": ([d(cap=-1)],), "overlap": ([d(first=0, cap=100), d(first=99, cap=100)],), "null image": ([d(), d(ptr=None, first=100)],)}
    for name, args in bad.items():
        status[:] = -5
        assert call(*args) == -1, name
        assert capi.lib().sbm_last_error(), name
        assert (status == -5).all(), name  # nothing ran
        got, _ = run(ctx, good_items)
        check(got, good_wants)


@pytest.fixture(scope="module")
def circle(golden):
    return np.load(os.path.join(golden, "case0_circle_bgr.npz"))["bgr"]


SWEEP_SCALES = [float(np.float32(s)) for s in (0.1, 0.13, 0.25, 0.37, 0.5, 1)]


def sweep_wants(oracle, img, mask, scales, nfs):
    wants, items = [], []
    for s, nf in zip(scales, nfs):
        im = oracle.resize_linear(img, s, s)
        m = None if mask is None else np.where(oracle.resize_linear(mask, s, s) > 0, 255, 0).astype(np.uint8)
        items.append((im, m, nf))
        wants.append(TC.want(oracle, im, m, nf))
    return items, wants


@pytest.mark.parametrize("masked", [False, True])
def test_sweep_of_the_circle(ctx_factory, oracle, circle, masked):
    ctx = ctx_factory()
    assert circle.shape == (800, 800, 3)
    mask = None
    if masked:
        yy, xx = np.mgrid[:800, :800]
        mask = np.where((yy - 400) ** 2 + (xx - 400) ** 2 <= 330 ** 2, 255, 0).astype(np.uint8)
    nfs = [int(150 * s) for s in SWEEP_SCALES]
    items, wants = sweep_wants(oracle, circle, mask, SWEEP_SCALES, nfs)
    assert all(w is not None for w in wants)
    if not masked:
        assert [list(TC.counts(w)) for w in wants] == [[18, 7], [20, 11], [40, 24], [56, 27], [78, 39], [169, 96]]
    got, status = ctx.train_sweep_status(circle, mask, SWEEP_SCALES, TC.STRONG, nfs)
    check(got, wants)
    check_status(oracle, status, items, wants)


def test_sweep_of_a_rectangle_with_failures(ctx_factory, oracle):
    from shape_based_matching_amd import capi

    ctx = ctx_factory()
    img = TC.rectangle(96, 96)
    scales = [float(np.float32(s)) for s in (1, 0.5, 0.37, 1.5, 0.11, 0.05)]
    nfs = [8] * len(scales)  # 63 leaves two successes; 8 four, and two scales too small for their pyramid
    for mask in (None, TC.cut_edge(96, 96)):
        items, wants = sweep_wants(oracle, img, mask, scales, nfs)
        if mask is None:
            assert sum(w is not None for w in wants) >= 3 and sum(w is None for w in wants) >= 1
        else:
            assert any(w is not None for w in wants) and any(w is None for w in wants)
        got, status = ctx.train_sweep_status(img, mask, scales, TC.STRONG, nfs)
        check(got, wants)
        check_status(oracle, status, items, wants)
    # fx != fy
    pairs = [(0.5, 1.0), (1.25, 0.75)]
    wants = [TC.want(oracle, oracle.resize_linear(img, fx, fy), None, 63) for fx, fy in pairs]
    check(ctx.train_sweep(img, None, pairs, TC.STRONG, [63, 63]), wants)
    # a scale that resizes to an empty image is an error of the call: 96 * 0.001 rounds to 0
    with pytest.raises(capi.SbmError) as e:
        ctx.train_sweep(img, None, [1.0, 0.001], TC.STRONG, [63, 63])
    assert e.value.code == -1
    check(ctx.train_sweep(img, None, [1.0], TC.STRONG, [63]), [TC.want(oracle, img, None, 63)])
