"""Rotated template families on the device (sbm_train_rotate / sbm_train_rotate_device) against the oracle's
add_template_rotate, bit for bit: level records, features, theta as bits, for every pair of every call.  The case1 family of
the reference (360 angles), the hand-made bases of train_rotate_cases.py at one, two and three pyramid levels, every status
code beside intact neighbours, every argument error, the chain sweep -> rotate on one stream, and two calls back to back."""
import ctypes as C
import os

import numpy as np
import pytest

import train_batch_cases as TC
import train_rotate_cases as RC

pytestmark = pytest.mark.gpu

T_OF = {1: (4,), 2: (4, 8), 3: (4, 8, 16)}
FILL = 0x5A


def check_family(oracle, bases, thetas, centers, levels, feats, status, firsts, caps):
    """every pair of a host-form call against the oracle"""
    for b, base in enumerate(bases):
        n = int(base[0]["n_features"].sum())
        for k, theta in enumerate(thetas):
            assert status[b, k].tolist() == [0, n], (b, k)
            first = firsts[b] + k * caps[b]
            assert RC.same_pair((levels[b, k], feats[first: first + n]), RC.want(oracle, base, theta, centers[b])), (b, k)


def run_family(ctx, oracle, bases, thetas, centers):
    caps = [int(b[0]["n_features"].sum()) for b in bases]
    levels, feats, status, firsts = ctx.train_rotate_raw(bases, thetas, centers, caps)
    check_family(oracle, bases, thetas, centers, levels, feats, status, firsts, caps)


def test_case1_family_equals_the_reference_templates(ctx_factory, oracle, case1):
    """test.cpp:303-313 on the device: the padded ROI of train.png trained by sbm_train_batch, rotated by 1 .. 360 degrees
    about (235, 235) in one call; templates 1 .. 360 of the reference's own YAML, and the oracle bit for bit"""
    ctx = ctx_factory()
    padded, mask = TC.fixture_roi(case1)
    base = ctx.train_batch([padded], [mask], TC.STRONG, 128)[0]
    assert base is not None and TC.same_template(base, TC.want(oracle, padded, mask, 128))
    thetas = [float(t) for t in range(1, 361)]
    got = ctx.train_rotate([base], thetas, [(470 / 2.0, 470 / 2.0)])
    ts = case1["templates"]
    assert ts.n_templates == 361 and len(got) == 360
    for t in range(1, 361):
        levels, feats = got[t - 1]
        for l in range(ts.n_levels):
            lv, ref = levels[l], ts.levels[t, l]
            for key in ("width", "height", "tl_x", "tl_y", "n_features"):
                assert int(lv[key]) == int(ref[key]), (t, l, key)
            assert int(lv["pyramid_level"]) == l
            mine = feats[int(lv["feature_offset"]): int(lv["feature_offset"]) + int(lv["n_features"])]
            rf = ts.feats_of(t, l)
            assert np.array_equal(mine["x"], rf["x"]) and np.array_equal(mine["y"], rf["y"]) and np.array_equal(mine["label"], rf["label"]), (t, l)
        assert RC.same_pair(got[t - 1], RC.want(oracle, base, thetas[t - 1], (235.0, 235.0))), t


@pytest.mark.parametrize("n_levels", [1, 2, 3])
def test_edge_cases_in_one_call_per_pyramid_depth(ctx_factory, oracle, n_levels):
    """every case of train_rotate_cases.py with this many levels as the bases of ONE call, each with its own centre, at the
    union of the cases' angles: negative coordinates and odd negative minima, rounding ties, the orientation wrap at 0, 360
    and beyond +-720, labels one ulp around their boundaries, feature counts at wave and workgroup edges (1 .. 8191), an
    empty level beside a filled one"""
    cases = [c for c in RC.cpu_cases() + RC.count_cases() if len(c[1][0]) == n_levels]
    assert cases
    thetas = sorted({float(t) for c in cases for t in c[3]})
    ctx = ctx_factory(T=T_OF[n_levels])
    run_family(ctx, oracle, [c[1] for c in cases], thetas, [c[2] for c in cases])


@pytest.mark.parametrize("n_bases,n_thetas", [(1, 1), (1, 2), (1, 65), (3, 1), (3, 2), (3, 65)])
def test_bases_and_angles(ctx_factory, oracle, n_bases, n_thetas):
    """bases of different sizes and centres; the angle is the grid's x, the base its y"""
    ctx = ctx_factory()
    bases = [RC.random_base(c, 40 + i) for i, c in enumerate([(257, 65), (3, 1), (64, 300)][:n_bases])]
    centers = [(200.0, 200.0), (-17.5, 1000.25), (0.0, 0.0)][:n_bases]
    thetas = [float(np.float32(t)) for t in np.linspace(-400.0, 400.0, n_thetas)] if n_thetas > 1 else [123.456]
    run_family(ctx, oracle, bases, thetas, centers)


class DeviceFamily:
    """bases in device memory (their level records, features and status pairs), the records of the device form, and its
    outputs pre-filled with FILL"""

    def __init__(self, n_levels, bases, thetas, centers, caps, firsts, dev, base_status=None):
        import torch

        from shape_based_matching_amd import capi

        self.L, self.nb, self.nt = n_levels, len(bases), len(thetas)
        self.thetas, self.caps, self.firsts = list(thetas), list(caps), list(firsts)
        self.keep, self.desc = [], []
        for b, (levels, feats) in enumerate(bases):
            d_lv = torch.from_numpy(np.ascontiguousarray(levels).view(np.uint8).copy()).to(dev)
            d_ft = torch.from_numpy(np.ascontiguousarray(feats if len(feats) else np.zeros(1, capi.TRAIN_FEATURE_DTYPE)).view(np.uint8).copy()).to(dev)
            st = None if base_status is None else base_status[b]
            d_st = None if st is None else torch.from_numpy(np.asarray(st, np.int32)).to(dev)
            self.keep.append((d_lv, d_ft, d_st))
            self.desc.append(capi.SbmRotateBase(d_lv.data_ptr(), d_ft.data_ptr(), None if d_st is None else d_st.data_ptr(), centers[b][0], centers[b][1],
                                                firsts[b], caps[b]))
        self.end = max(f + c * self.nt for f, c in zip(firsts, caps)) + 7  # a few records behind the last block
        pairs = self.nb * self.nt
        self.d_lv = filled(dev, pairs * n_levels * capi.LEVEL_DTYPE.itemsize, np.uint8, FILL)
        self.d_ft = filled(dev, self.end * capi.TRAIN_FEATURE_DTYPE.itemsize, np.uint8, FILL)
        self.d_st = filled(dev, pairs * 2, np.int32, -5)

    def run(self, ctx, stream=0):
        ctx.train_rotate_device(self.desc, self.thetas, self.d_lv.data_ptr(), self.d_ft.data_ptr(), self.d_st.data_ptr(), stream=stream)

    def results(self):
        from shape_based_matching_amd import capi

        lv = self.d_lv.cpu().numpy().view(capi.LEVEL_DTYPE).reshape(self.nb, self.nt, self.L)
        ft = self.d_ft.cpu().numpy().view(capi.TRAIN_FEATURE_DTYPE)
        st = self.d_st.cpu().numpy().reshape(self.nb, self.nt, 2)
        return lv, ft, st


def filled(dev, n, dtype, value):
    """n elements of `value` in device memory, by a copy from the host (no fill kernel of torch's)"""
    import torch

    return torch.from_numpy(np.full(n, value, dtype)).to(dev)


def untouched(records):
    return bool((records.view(np.uint8) == FILL).all())


def test_every_status_beside_intact_neighbours(ctx_factory, oracle):
    """{0, n} | {1, level} | {2, needed} | {3, reason 1, 2, 3}: a pair that is not ok has zeroed level records and, but for the
    base with a feature outside the domain, an untouched feature block; the ok pairs between them are the oracle's; the gaps
    between the blocks and the records behind the last stay as they were"""
    import torch

    ctx = ctx_factory()
    dev = torch.device("cuda", 0)
    ok = [RC.random_base(c, 60 + i) for i, c in enumerate([(70, 9), (300, 1), (5, 5), (64, 64), (1, 0)])]
    small = RC.random_base((130, 31), 70)
    failed, overflowed = RC.random_base((8, 8), 71), RC.random_base((9, 9), 72)
    empty = (RC.random_base((4, 4), 73)[0].copy(), RC.random_base((4, 4), 73)[1])
    empty[0]["n_features"] = 0
    too_many = (RC.random_base((4, 4), 74)[0].copy(), RC.random_base((4, 4), 74)[1])
    too_many[0]["n_features"][1] = 8192
    negative = (too_many[0].copy(), too_many[1])
    negative[0]["n_features"][1] = -1
    outside = []
    for value in (float("inf"), float("nan"), 1e9, -720.5):
        levels, feats = RC.random_base((300, 40), 75)
        feats["theta"][299] = value
        outside.append((levels, feats))
    far = RC.base_from_points([[(3, 3, 1.0), (32767, 5, 2.0)], [(1, 1, 3.0)]])
    far[1]["x"][1] += 1  # x + tl_x = 32768
    outside.append(far)
    bases = [ok[0], small, ok[1], failed, ok[2], overflowed, empty, too_many, negative, ok[3]] + outside + [ok[4]]
    status_in = [None, None, (0, 301), (1, 1), None, (2, 18), None, None, None, (0, 0)] + [None] * len(outside) + [None]
    want = [(0, 79), (2, 161), (0, 301), (1, 1), (0, 10), (3, 1), (3, 2), (3, 2), (3, 2), (0, 128)] + [(3, 3)] * len(outside) + [(0, 1)]
    n = [int(b[0]["n_features"].clip(0, 8191).sum()) for b in bases]
    caps = [c if w[0] != 2 else c - 1 for c, w in zip(n, want)]  # one record too few for the base that is to overflow
    caps[6] = 3  # the empty base has room it does not use
    thetas = [33.0, -200.5]
    firsts, first = [], 5
    for c in caps:
        firsts.append(first)
        first += c * len(thetas) + 3  # gaps between the bases' blocks
    centers = [(100.0 + b, 50.0 - b) for b in range(len(bases))]
    fam = DeviceFamily(2, bases, thetas, centers, caps, firsts, dev, status_in)
    fam.run(ctx)
    torch.cuda.synchronize()
    lv, ft, st = fam.results()
    covered = np.zeros(len(ft), bool)
    for b, base in enumerate(bases):
        for k, theta in enumerate(thetas):
            assert tuple(st[b, k].tolist()) == want[b], (b, k)
            block = slice(firsts[b] + k * caps[b], firsts[b] + (k + 1) * caps[b])
            covered[block] = True
            if want[b][0] == 0:
                assert RC.same_pair((lv[b, k], ft[block][: want[b][1]]), RC.want(oracle, base, theta, centers[b])), (b, k)
                assert untouched(ft[block][want[b][1]:])
            else:
                assert not lv[b, k].tobytes().strip(b"\0"), (b, k)
                if want[b] != (3, 3):
                    assert untouched(ft[block]), (b, k)
    assert untouched(ft[~covered])


def test_argument_errors_enqueue_nothing(ctx_factory, oracle):
    from shape_based_matching_amd import capi

    ctx = ctx_factory()
    base = RC.random_base((20, 6), 9)
    lv, ft = np.ascontiguousarray(base[0]), np.ascontiguousarray(base[1])
    levels = np.zeros((8, 2), capi.LEVEL_DTYPE)
    feats = np.zeros(4096, capi.TRAIN_FEATURE_DTYPE)
    status = np.zeros((8, 2), np.int32)
    many = (capi.SbmRotateBase * 65536)()
    many_thetas = np.zeros(16385, np.float32)

    def d(first=0, cap=26, cx=9.0, cy=9.0, levels_ptr=lv.ctypes.data, feats_ptr=ft.ctypes.data):
        return capi.SbmRotateBase(levels_ptr, feats_ptr, None, cx, cy, first, cap)

    def call(descs, thetas=(10.0, 20.0), n_bases=None, n_thetas=None, out=(levels, feats, status), arr=None, th=None):
        arr = (capi.SbmRotateBase * max(len(descs), 1))(*descs) if arr is None else arr
        th = np.ascontiguousarray(thetas, np.float32) if th is None else th
        return capi.lib().sbm_train_rotate(ctx._h, arr, len(descs) if n_bases is None else n_bases, capi._p(th), len(thetas) if n_thetas is None else n_thetas,
                                           capi._p(out[0]), capi._p(out[1]), capi._p(out[2]))

    inf, nan = float("inf"), float("nan")
    bad = {"no base": dict(descs=[d()], n_bases=0), "no angle": dict(descs=[d()], n_thetas=0), "negative count": dict(descs=[d()], n_bases=-1),
           "too many pairs": dict(descs=[], arr=many, n_bases=65536, th=many_thetas, n_thetas=16385),
           "null levels out": dict(descs=[d()], out=(None, feats, status)), "null feats out": dict(descs=[d()], out=(levels, None, status)),
           "null status out": dict(descs=[d()], out=(levels, feats, None)),
           "null base levels": dict(descs=[d(levels_ptr=None)]), "null base feats": dict(descs=[d(levels_ptr=lv.ctypes.data, feats_ptr=None)]),
           "negative first": dict(descs=[d(first=-1)]), "negative cap": dict(descs=[d(cap=-1)]),
           "overlap by one": dict(descs=[d(first=0), d(first=51)]), "overlap, second first": dict(descs=[d(first=51), d(first=0)]),
           "interleaved": dict(descs=[d(first=0), d(first=26)]), "contained": dict(descs=[d(first=0, cap=100), d(first=120, cap=5)]),
           "theta inf": dict(descs=[d()], thetas=(10.0, inf)), "theta nan": dict(descs=[d()], thetas=(nan, 10.0)),
           "theta beyond": dict(descs=[d()], thetas=(10.0, 36000.01)), "theta below": dict(descs=[d()], thetas=(-36001.0,)),
           "centre nan": dict(descs=[d(cx=nan)]), "centre inf": dict(descs=[d(cy=-inf)]), "centre beyond": dict(descs=[d(), d(first=52, cy=65536.5)])}
    for name, kw in bad.items():
        status[:] = -5
        assert call(**kw) == -1, name
        assert capi.lib().sbm_last_error(), name
        assert (status == -5).all(), name  # nothing ran
    # the null handle and the null tables
    assert capi.lib().sbm_train_rotate(None, (capi.SbmRotateBase * 1)(d()), 1, capi._p(np.zeros(1, np.float32)), 1, capi._p(levels), capi._p(feats),
                                       capi._p(status)) == -1
    assert capi.lib().sbm_train_rotate(ctx._h, None, 1, capi._p(np.zeros(1, np.float32)), 1, capi._p(levels), capi._p(feats), capi._p(status)) == -1
    assert capi.lib().sbm_train_rotate(ctx._h, (capi.SbmRotateBase * 1)(d()), 1, None, 1, capi._p(levels), capi._p(feats), capi._p(status)) == -1
    assert (status == -5).all()
    # adjacent blocks are no overlap, in either order; the context is usable after all of the above
    for descs in ([d(first=0), d(first=52)], [d(first=52), d(first=0)]):
        assert call(descs) == 0
        for b in range(2):
            for k, theta in enumerate((10.0, 20.0)):
                assert status[b * 2 + k].tolist() == [0, 26]
                first = descs[b].out_first + k * 26
                assert RC.same_pair((levels[b * 2 + k], feats[first: first + 26]), RC.want(oracle, base, theta, (9.0, 9.0)))


@pytest.fixture(scope="module")
def circle(golden):
    return np.load(os.path.join(golden, "case0_circle_bgr.npz"))["bgr"]


def test_sweep_then_rotate_without_the_host(ctx_factory, oracle, circle):
    """sbm_train_sweep_device at three scales, then sbm_train_rotate_device at eight angles on the same caller stream with
    the sweep's output buffers as the base records and no synchronisation in between; the middle scale fails its training"""
    import torch

    from shape_based_matching_amd import capi

    ctx = ctx_factory()
    dev = torch.device("cuda", 0)
    scales, nfs = [float(np.float32(s)) for s in (0.25, 0.02, 0.37)], [37, 8, 55]
    L = TC.N_LEVELS
    wants, dims = [], []
    for s, nf in zip(scales, nfs):
        im = oracle.resize_linear(circle, s, s)
        dims.append(im.shape[:2])
        wants.append((TC.want(oracle, im, None, nf), im, nf))
    assert [w[0] is None for w in wants] == [False, True, False]
    failing = oracle.add_template_failing_level(wants[1][1], None, L, nfs[1], TC.WEAK, TC.STRONG)
    thetas = [float(t) for t in (45.0, 90.0, 135.0, 180.0, 225.0, 270.0, 315.0, 360.0)]
    centers = [(c / 2.0, r / 2.0) for r, c in dims]
    # the sweep's outputs
    caps = [ctx._feature_cap(r, c) for r, c in dims]
    firsts = [int(v) for v in np.cumsum([0] + caps)[:-1]]
    desc = (capi.SbmTrainScale * 3)(*[capi.SbmTrainScale(s, s, nf, 0, f, c) for s, nf, f, c in zip(scales, nfs, firsts, caps)])
    lv_size, ft_size = capi.LEVEL_DTYPE.itemsize, capi.TRAIN_FEATURE_DTYPE.itemsize
    d_img = torch.from_numpy(np.ascontiguousarray(circle)).to(dev)
    t_lv, t_ft, t_st = filled(dev, 3 * L * lv_size, np.uint8, 0), filled(dev, sum(caps) * ft_size, np.uint8, 0), filled(dev, 6, np.int32, 0)
    # the rotation's: scale i's eight blocks of caps[i] records
    r_firsts = [int(v) for v in np.cumsum([0] + [c * len(thetas) for c in caps])[:-1]]
    bases = [capi.SbmRotateBase(t_lv.data_ptr() + i * L * lv_size, t_ft.data_ptr() + firsts[i] * ft_size, t_st.data_ptr() + i * 8, centers[i][0], centers[i][1],
                                r_firsts[i], caps[i]) for i in range(3)]
    r_lv = filled(dev, 3 * len(thetas) * L * lv_size, np.uint8, FILL)
    r_ft = filled(dev, sum(caps) * len(thetas) * ft_size, np.uint8, FILL)
    r_st = filled(dev, 3 * len(thetas) * 2, np.int32, -5)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    rows, cols = circle.shape[:2]
    capi._check(capi.lib().sbm_train_sweep_device(ctx._h, C.c_void_p(d_img.data_ptr()), rows, cols, cols * 3, 3, None, desc, 3, C.c_float(TC.STRONG),
                                                  C.c_void_p(t_lv.data_ptr()), C.c_void_p(t_ft.data_ptr()), C.c_void_p(t_st.data_ptr()),
                                                  C.c_void_p(stream.cuda_stream)))
    ctx.train_rotate_device(bases, thetas, r_lv.data_ptr(), r_ft.data_ptr(), r_st.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    lv = r_lv.cpu().numpy().view(capi.LEVEL_DTYPE).reshape(3, len(thetas), L)
    ft = r_ft.cpu().numpy().view(capi.TRAIN_FEATURE_DTYPE)
    st = r_st.cpu().numpy().reshape(3, len(thetas), 2)
    for i in range(3):
        for k, theta in enumerate(thetas):
            if wants[i][0] is None:
                assert st[i, k].tolist() == [1, failing] and not lv[i, k].tobytes().strip(b"\0")
                continue
            n = len(wants[i][0][1])
            assert st[i, k].tolist() == [0, n], (i, k)
            first = r_firsts[i] + k * caps[i]
            assert RC.same_pair((lv[i, k], ft[first: first + n]), RC.want(oracle, wants[i][0], theta, centers[i])), (i, k)


def test_two_calls_back_to_back_on_one_stream(ctx_factory, oracle):
    """different tables, no synchronisation between the calls: the second call's records and angles must not reach the
    first call's kernel.  The first family is the large one, so its kernel is still running when the second is enqueued."""
    import torch

    ctx = ctx_factory()
    dev = torch.device("cuda", 0)

    def family(counts_list, seed, thetas, centers):
        bases = [RC.random_base(c, seed + i, extent=1500) for i, c in enumerate(counts_list)]
        caps = [int(b[0]["n_features"].sum()) for b in bases]
        firsts = [int(v) for v in np.cumsum([0] + [c * len(thetas) for c in caps])[:-1]]
        return bases, DeviceFamily(2, bases, thetas, centers, caps, firsts, dev)

    a_thetas = [float(np.float32(t)) for t in np.linspace(0.5, 359.5, 97)]
    b_thetas = [-77.0, 12.25, 300.0]
    a_centers, b_centers = [(700.0, 650.0), (10.0, 20.0)], [(1.5, 2.5), (400.0, 400.0), (-30.0, 60.0)]
    a_bases, a = family([(8191, 4000), (500, 100)], 80, a_thetas, a_centers)
    b_bases, b = family([(65, 3), (1, 1), (256, 64)], 90, b_thetas, b_centers)
    ctx.train_rotate([a_bases[1]], [1.0], [(0.0, 0.0)])  # the context's stream, pinned slot and scratch exist
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    a.run(ctx, stream.cuda_stream)
    b.run(ctx, stream.cuda_stream)
    stream.synchronize()
    for bases, fam, thetas, centers in ((a_bases, a, a_thetas, a_centers), (b_bases, b, b_thetas, b_centers)):
        lv, ft, st = fam.results()
        levels = lv
        check_family(oracle, bases, thetas, centers, levels, ft, st, fam.firsts, fam.caps)
