"""-m gpu: the verify stage on the device (sbm_verify_batch_device, _ptrs, _planes; k_verify_rois, k_verify_compact) at
its edges: ROI shapes and positions, the LDS budget's border, sums past 32 bits, more records than workgroups, the
unverifiable records, the threshold, the counts' edges, the three frame sources, the patch set's rules and a captured
replay.  Records are written straight into device buffers; every expected score and list comes from the numpy restatement
of the verify rule in tests/test_verify_math.py (np_verify_frame), nothing from the code under test."""
import math

import numpy as np
import pytest

from shape_based_matching_amd import capi
from shape_based_matching_amd.templates import FEATURE_DTYPE, LEVEL_DTYPE, MATCH_DTYPE, TemplateSet
from nms_form_cases import rows_of, synth_list
from test_verify_math import bits, np_gray, np_normalise, np_sums, np_verify_frame

pytestmark = pytest.mark.gpu
REC = MATCH_DTYPE.itemsize
ROWS, COLS = 96, 128
SHAPES = [(1, 1), (3, 5), (63, 7), (64, 64), (65, 33), (127, 2), (2, 90)]


def template_set(sizes):
    """one two-level pyramid per (w0, h0), one feature per level, labels (0, t)"""
    n = len(sizes)
    levels = np.zeros((n, 2), LEVEL_DTYPE)
    feats = np.zeros(2 * n, FEATURE_DTYPE)
    for t, (w, h) in enumerate(sizes):
        for l in range(2):
            levels[t, l] = (max(w >> l, 0), max(h >> l, 0), 0, 0, l, 1, 2 * t + l)
    return TemplateSet(2, levels, feats, np.zeros(n, np.int32), np.arange(n, dtype=np.int32), ["c"])


def recs_of(rows):
    """rows: (x, y, class_idx, template_id)"""
    r = np.zeros(len(rows), MATCH_DTYPE)
    for i, (x, y, c, t) in enumerate(rows):
        r[i] = (x, y, 100.0 - i, 400 - i, c, t)
    return r


class Frames:
    """frames on the device as one of the three sources.  frames: list of HxW or HxWx3 (B, G, R) arrays of one shape."""

    def __init__(self, frames, kind="strided", pad=0, gap=0):
        import torch

        self.kind, self.n = kind, len(frames)
        f0 = np.asarray(frames[0])
        self.rows, self.cols = f0.shape[:2]
        self.ch = 1 if f0.ndim == 2 else 3
        self.keep = []
        if kind == "planes":
            assert self.ch == 3
            self.stride = self.cols + pad
            self.tensors = []
            ptrs = []
            for f in frames:
                rgb = np.zeros((3, self.rows, self.stride), np.uint8)
                rgb[:, :, : self.cols] = np.asarray(f)[:, :, ::-1].transpose(2, 0, 1)  # planes R, G, B
                t = torch.from_numpy(rgb).to("cuda:0")
                self.tensors.append(t)
                plane = self.rows * self.stride
                ptrs += [t.data_ptr() + k * plane for k in (2, 1, 0)]  # listed as B, G, R
            self.table = torch.tensor(ptrs, dtype=torch.int64, device="cuda:0")
            return
        self.stride = self.cols * self.ch + pad
        host = [np.zeros((self.rows, self.stride), np.uint8) for _ in frames]
        for h, f in zip(host, frames):
            h[:, : self.cols * self.ch] = np.asarray(f).reshape(self.rows, -1)
        if kind == "strided":
            self.frame_stride = self.rows * self.stride + gap
            buf = np.full(self.n * self.frame_stride, 0x5A, np.uint8)
            for i, h in enumerate(host):
                buf[i * self.frame_stride: i * self.frame_stride + h.size] = h.reshape(-1)
            self.tensor = torch.from_numpy(buf).to("cuda:0")
        else:  # ptrs: the table lists the frames in reverse allocation order
            self.tensors = [None] * self.n
            for i in reversed(range(self.n)):
                self.tensors[i] = torch.from_numpy(host[i]).to("cuda:0")
            self.table = torch.tensor([t.data_ptr() for t in self.tensors], dtype=torch.int64, device="cuda:0")

    def write(self, frames):
        """overwrite the frames in place (strided, packed rows)"""
        import torch

        assert self.kind == "strided" and self.stride == self.cols * self.ch and self.frame_stride == self.rows * self.stride
        self.tensor.copy_(torch.from_numpy(np.stack([np.asarray(f) for f in frames]).reshape(-1)))

    def verify(self, ctx, d_recs, d_counts, cap, min_corr, d_out, d_scores, out_cap, d_oc, keep_unverified=False, stream=0):
        a = (d_recs, d_counts, cap, min_corr, d_out, d_scores, out_cap, d_oc, keep_unverified, stream)
        if self.kind == "strided":
            ctx.verify_batch_device(self.tensor.data_ptr(), self.frame_stride, self.n, self.rows, self.cols, self.stride, self.ch, *a)
        elif self.kind == "ptrs":
            ctx.verify_batch_device_ptrs(self.table.data_ptr(), self.n, self.rows, self.cols, self.stride, self.ch, *a)
        else:
            ctx.verify_batch_device_planes(self.table.data_ptr(), self.n, self.rows, self.cols, self.stride, *a)


def run_verify(ctx, src, buf, counts, min_corr, keep_unverified=False, out_cap=None):
    """buf: (frames, cap) records; counts: (frames, 2).  Returns per frame (kept records, scores) and the output pairs."""
    import torch

    n, cap = buf.shape
    out_cap = cap if out_cap is None else out_cap
    d_recs = torch.from_numpy(np.ascontiguousarray(buf).view(np.uint8).reshape(-1).copy()).to("cuda:0") if buf.size else \
        torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    d_cnt = torch.from_numpy(np.ascontiguousarray(counts, np.int32).reshape(-1)).to("cuda:0")
    d_out = torch.full((max(n * out_cap * REC, 1),), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_sc = torch.full((max(n * out_cap, 1),), -7.0, dtype=torch.float32, device="cuda:0")
    d_oc = torch.full((n * 2,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    src.verify(ctx, d_recs.data_ptr(), d_cnt.data_ptr(), cap, min_corr, d_out.data_ptr() if out_cap else 0, d_sc.data_ptr() if out_cap else 0, out_cap,
               d_oc.data_ptr(), keep_unverified)
    torch.cuda.synchronize()
    oc = d_oc.cpu().numpy().reshape(-1, 2)
    res = []
    for f in range(n):
        k = min(int(oc[f, 0]), out_cap)
        if out_cap:
            r = d_out.cpu().numpy()[f * out_cap * REC: (f * out_cap + k) * REC].view(MATCH_DTYPE)
            s = d_sc.cpu().numpy()[f * out_cap: f * out_cap + k]
        else:
            r, s = np.zeros(0, MATCH_DTYPE), np.zeros(0, np.float32)
        res.append((r, s))
    return res, oc


def check(ctx, src, frames, lists, sizes, patches, min_corr, keep_unverified=False, cap=None, counts=None, out_cap=None):
    """the stage over `lists` (one record array per frame) against np_verify_frame, bit for bit"""
    cap = max(max(len(l) for l in lists), 1) if cap is None else cap
    buf = np.zeros((len(lists), cap), MATCH_DTYPE)
    for f, l in enumerate(lists):
        buf[f, : min(len(l), cap)] = l[:cap]
    if counts is None:
        counts = np.array([[len(l), 0] for l in lists], np.int32)
    got, oc = run_verify(ctx, src, buf, counts, min_corr, keep_unverified, out_cap)
    wants = []
    for f, l in enumerate(lists):
        kept, ks, alls, pair = np_verify_frame(frames[f], buf[f], sizes, patches, min_corr, keep_unverified, cap=cap, count=int(counts[f, 0]),
                                               overflow=int(counts[f, 1]), out_cap=cap if out_cap is None else out_cap)
        assert tuple(oc[f]) == pair, (f, oc[f], pair)
        assert rows_of(got[f][0]) == rows_of(buf[f][kept]), f
        assert np.array_equal(bits(got[f][1]), bits(ks)), (f, got[f][1], ks)
        wants.append((kept, ks, alls, pair))
    return wants


def corner_rows(sizes, rows, cols):
    out = []
    for t, (w, h) in enumerate(sizes):
        xi = min(((cols - w) // 2) | 1, cols - w)
        for x, y in ((0, 0), (cols - w, 0), (0, rows - h), (cols - w, rows - h), (xi, (rows - h) // 2)):
            out.append((x, y, 0, t))
        assert xi % 2 == 1
    return out


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("ch", [3, 1])
def test_shapes_corners_channels_strides(ctx_factory, ch, pad):
    """seven template sizes, each at the four frame corners and an interior position with odd x; 3 and 1 channels; rows
    tight and padded by 5 bytes; patches cut from the frame (score 1 at their origin), shifted copies and noise"""
    rs = np.random.RandomState(21 + ch + pad)
    shape = (ROWS, COLS, 3) if ch == 3 else (ROWS, COLS)
    frames = [rs.randint(0, 256, shape).astype(np.uint8) for _ in range(2)]
    frames[1] = (frames[1] // 3 + np.arange(COLS, dtype=np.uint8).reshape((1, COLS) + (1,) * (ch == 3))).astype(np.uint8)  # a ramp under noise
    sizes = {(0, t): s for t, s in enumerate(SHAPES)}
    rows = corner_rows(SHAPES, ROWS, COLS)
    g0 = np_gray(frames[0])
    patches = {}
    for t, (w, h) in enumerate(SHAPES):
        x, y = rows[5 * t + (t % 5)][:2]  # one of the five positions scores 1 on frame 0
        p = g0[y:y + h, x:x + w].copy()
        if t in (2, 4):  # near copies: scores between
            p = np.clip(p.astype(np.int32) + rs.randint(-60, 61, p.shape), 0, 255).astype(np.uint8)
        patches[(0, t)] = p
    ctx = ctx_factory()
    ctx.upload_templates(template_set(SHAPES))
    ctx.upload_verify_patches([(0, t, p) for (_, t), p in patches.items()])
    src = Frames(frames, "strided", pad=pad)
    lists = [recs_of(rows), recs_of(rows[::-1])]
    want = check(ctx, src, frames, lists, sizes, patches, 0.0)
    assert all(len(w[0]) == len(rows) and w[3][1] == 0 for w in want)
    ones = [i for i, s in enumerate(want[0][2]) if s == 1.0]
    assert len(ones) >= 4  # the exact cuts (a 1 x 1 image is constant: score 0; two patches are near copies)
    want = check(ctx, src, frames, lists, sizes, patches, 0.8)
    assert 0 < len(want[0][0]) < len(rows)


def test_large_rois_lds_border_and_sums_past_32_bits(ctx_factory):
    """a 300 x 300 template on a 320 x 320 frame, ROI and patch all 255 but one 0 pixel: Sab > 2^32; and the two sizes on
    either side of the kernel's LDS budget (32 768 gray bytes: 181 x 181 inside, 182 x 181 beyond), 3 channels and 1"""
    rs = np.random.RandomState(31)
    big = [(300, 300), (181, 181), (182, 181)]
    sizes = {(0, t): s for t, s in enumerate(big)}
    f1 = np.full((320, 320), 255, np.uint8)
    f1[10, 305] = 0  # inside the ROI at (11, 7) alone
    p0 = np.full((300, 300), 255, np.uint8)
    p0[299, 299] = 0
    assert np_sums(np_normalise(f1[7:307, 11:311]), np_normalise(p0))[0] > 2 ** 32
    f3 = rs.randint(0, 256, (320, 320, 3)).astype(np.uint8)
    g3 = np_gray(f3)
    patches = {(0, 0): p0, (0, 1): np.clip(g3[100:281, 33:214].astype(np.int32) + rs.randint(-80, 81, (181, 181)), 0, 255).astype(np.uint8),
               (0, 2): np.clip(g3[139:320, 137:319].astype(np.int32) + rs.randint(-80, 81, (181, 182)), 0, 255).astype(np.uint8)}
    ctx = ctx_factory()
    ctx.upload_templates(template_set(big))
    ctx.upload_verify_patches([(0, t, p) for (_, t), p in patches.items()])
    lists = [recs_of([(11, 7, 0, 0), (0, 0, 0, 0), (20, 20, 0, 0), (33, 100, 0, 1), (137, 139, 0, 2), (1, 1, 0, 2)])]
    w1 = check(ctx, Frames([f1], "strided"), [f1], lists, sizes, patches, 0.0)
    assert 0.99 < w1[0][2][0] < 1.0 and w1[0][2][1] == 0.0  # one pixel apart; a constant ROI
    w3 = check(ctx, Frames([f3], "strided", pad=5), [f3], lists, sizes, patches, 0.0)
    assert w3[0][2][3] > 0.9 and w3[0][2][4] > 0.9


def test_more_records_than_workgroups(ctx_factory):
    """5000 records in one frame: the launch has 4096 workgroups per frame, the rest are walked by slot"""
    rs = np.random.RandomState(41)
    small = [(3, 5), (1, 1), (8, 2)]
    sizes = {(0, t): s for t, s in enumerate(small)}
    frames = [rs.randint(0, 256, (ROWS, COLS, 3)).astype(np.uint8)]
    patches = {k: rs.randint(0, 256, (h, w)).astype(np.uint8) for k, (w, h) in sizes.items()}
    n = 5000
    lst = synth_list(rs, n, sizes, np.array([90.0, 80.0], np.float32), 90)
    lst["template_id"] %= 3  # (synth_list's ties point at other template ids)
    ctx = ctx_factory()
    ctx.upload_templates(template_set(small))
    ctx.upload_verify_patches([(0, t, p) for (_, t), p in patches.items()])
    want = check(ctx, Frames(frames, "strided"), frames, [lst], sizes, patches, 0.7)
    assert 0 < len(want[0][0]) < n


def test_unverifiable_records(ctx_factory):
    """one record off each edge of the frame, a record whose label has no patch, a label missing from the upload: flag
    bits 3 and 2, score -1, kept or dropped by keep_unverified"""
    rs = np.random.RandomState(51)
    shapes = [(20, 10), (7, 30), (5, 5)]
    sizes = {(0, 0): shapes[0], (0, 1): shapes[1]}  # (0, 2) is uploaded as a template but has no patch
    frames = [rs.randint(0, 256, (ROWS, COLS, 3)).astype(np.uint8) for _ in range(7)]
    patches = {k: rs.randint(0, 256, (h, w)).astype(np.uint8) for k, (w, h) in sizes.items()}
    ctx = ctx_factory()
    ctx.upload_templates(template_set(shapes))
    ctx.upload_verify_patches([(0, t, p) for (_, t), p in patches.items()])
    ok = (10, 10, 0, 0)
    specs = [[ok, (-1, 5, 0, 0), ok], [ok, (5, -1, 0, 1)], [(COLS - 20 + 1, 0, 0, 0), ok], [(0, ROWS - 30 + 1, 0, 1), ok],
             [ok, (3, 3, 0, 2), ok], [ok, (3, 3, 4, 0)], [(COLS - 20, ROWS - 10, 0, 0), (COLS - 7, ROWS - 30, 0, 1)]]
    bit = [8, 8, 8, 8, 4, 4, 0]
    lists = [recs_of(s) for s in specs]
    src = Frames(frames, "strided")
    for keep in (False, True):
        want = check(ctx, src, frames, lists, sizes, patches, 0.0, keep_unverified=keep)
        for f, w in enumerate(want):
            assert w[3][1] == bit[f], f
            n_bad = sum(1 for s in w[2] if s == -1.0)
            assert n_bad == (1 if bit[f] else 0)
            assert len(w[0]) == len(specs[f]) - (0 if keep else n_bad)
    # with both kinds in one frame both bits are set
    both = [recs_of([(3, 3, 0, 2), ok, (-1, 0, 0, 0)])]
    want = check(ctx, Frames(frames[:1], "strided"), frames[:1], both, sizes, patches, 0.0, keep_unverified=True)
    assert want[0][3] == (3, 12)


def test_threshold(ctx_factory):
    """min_corr exactly a record's score keeps it, the next double above drops it; 0 keeps every verifiable record; 0.8
    on a mixed list"""
    rs = np.random.RandomState(61)
    shapes = [(24, 16)]
    sizes = {(0, 0): shapes[0]}
    frame = rs.randint(0, 256, (ROWS, COLS)).astype(np.uint8)
    base = frame[40:56, 50:74].copy()
    patches = {(0, 0): base}
    # ROIs that correlate with the patch to different degrees
    for k, amp in enumerate((0, 30, 60, 90, 140, 250)):
        noisy = np.clip(base.astype(np.int32) + rs.randint(-amp, amp + 1, base.shape), 0, 255).astype(np.uint8)
        frame[4 + 18 * (k // 3): 20 + 18 * (k // 3), 2 + 26 * (k % 3): 26 + 26 * (k % 3)] = noisy
    rows = [(2 + 26 * (k % 3), 4 + 18 * (k // 3), 0, 0) for k in range(6)] + [(50, 40, 0, 0), (-3, 0, 0, 0)]
    lists = [recs_of(rows)]
    ctx = ctx_factory()
    ctx.upload_templates(template_set(shapes))
    ctx.upload_verify_patches([(0, 0, base)])
    src = Frames([frame], "strided")
    w0 = check(ctx, src, [frame], lists, sizes, patches, 0.0)[0]
    assert w0[0] == list(range(7)) and w0[3] == (7, 8)
    scores = w0[2][:7]
    assert scores[0] == 1.0 and scores[6] == 1.0 and len(set(scores.tolist())) >= 5
    for i in (1, 2, 3, 4):
        s = float(scores[i])
        at = check(ctx, src, [frame], lists, sizes, patches, s)[0]
        above = check(ctx, src, [frame], lists, sizes, patches, math.nextafter(s, 2.0))[0]
        assert i in at[0] and i not in above[0]
    w8 = check(ctx, src, [frame], lists, sizes, patches, 0.8)[0]
    assert 2 <= len(w8[0]) < 7
    assert check(ctx, src, [frame], lists, sizes, patches, 0.8, keep_unverified=True)[0][0] == w8[0] + [7]


def test_counts_edges(ctx_factory):
    """16 frames with different counts: 0, cap, more than cap (bit 0), a non-zero second word (bit 0), an out_cap below
    the kept count (bit 1, the prefix stored), out_cap 0; the order is the input's"""
    rs = np.random.RandomState(71)
    shapes = [(6, 4), (9, 9)]
    sizes = {(0, t): s for t, s in enumerate(shapes)}
    frames = [rs.randint(0, 256, (ROWS, COLS, 3)).astype(np.uint8) for _ in range(16)]
    patches = {k: rs.randint(0, 256, (h, w)).astype(np.uint8) for k, (w, h) in sizes.items()}
    cap = 12
    ns = [0, cap, cap, 3, 1, 7, 12, 5, 2, 11, 0, 9, 4, 6, 8, 10]
    lists = []
    for n in ns:
        l = synth_list(rs, n, sizes, np.array([90.0, 85.0], np.float32), 80)
        l["template_id"] %= 2
        lists.append(l)
    counts = np.array([[n, 0] for n in ns], np.int32)
    counts[2, 0] = cap + 5  # more than were stored
    counts[3, 1] = 1        # the overflow word
    counts[4, 0] = -2       # a negative count reads nothing
    ctx = ctx_factory()
    ctx.upload_templates(template_set(shapes))
    ctx.upload_verify_patches([(0, t, p) for (_, t), p in patches.items()])
    src = Frames(frames, "strided")
    full = check(ctx, src, frames, lists, sizes, patches, 0.7, cap=cap, counts=counts)
    assert [w[3][1] for w in full] == [0, 0, 1, 1] + [0] * 12
    assert full[0][3] == (0, 0) and full[4][3] == (0, 0) and max(w[3][0] for w in full) > 3
    small = check(ctx, src, frames, lists, sizes, patches, 0.7, cap=cap, counts=counts, out_cap=3)
    assert any(w[3][1] & 2 for w in small) and any(not w[3][1] & 2 for w in small)
    assert [w[3][0] for w in small] == [w[3][0] for w in full]
    none = check(ctx, src, frames, lists, sizes, patches, 0.7, cap=cap, counts=counts, out_cap=0)
    assert all(bool(w[3][1] & 2) == (w[3][0] > 0) for w in none)


def test_three_sources_agree(ctx_factory):
    """one set of frames, records and patches through the strided form (frames further apart than a frame), the _ptrs form
    (frames listed in reverse allocation order) and the _planes form (an RGB tensor listed as planes 2, 1, 0)"""
    rs = np.random.RandomState(81)
    shapes = [(31, 17), (64, 64), (5, 3)]
    sizes = {(0, t): s for t, s in enumerate(shapes)}
    frames = [rs.randint(0, 256, (ROWS, COLS, 3)).astype(np.uint8) for _ in range(5)]
    patches = {}
    for (k, (w, h)), f in zip(sizes.items(), frames):
        g = np_gray(f)[8:8 + h, 9:9 + w]
        patches[k] = np.clip(g.astype(np.int32) + rs.randint(-50, 51, g.shape), 0, 255).astype(np.uint8)
    lists = []
    for f in range(5):
        rows = [(9, 8, 0, t) for t in range(3)] + [(int(rs.randint(0, COLS - 64)), int(rs.randint(0, ROWS - 64)), 0, int(rs.randint(0, 3))) for _ in range(9)]
        lists.append(recs_of(rows))
    ctx = ctx_factory()
    ctx.upload_templates(template_set(shapes))
    ctx.upload_verify_patches([(0, t, p) for (_, t), p in patches.items()])
    got = {}
    for kind, kw in (("strided", dict(gap=4099, pad=3)), ("ptrs", dict(pad=3)), ("planes", dict(pad=3)), ("planes", dict()), ("ptrs", dict())):
        src = Frames(frames, kind, **kw)
        got[(kind, len(kw))] = check(ctx, src, frames, lists, sizes, patches, 0.8)
    first = next(iter(got.values()))
    assert any(len(w[0]) > 0 for w in first) and any(len(w[0]) < 12 for w in first)
    for v in got.values():
        assert [(w[0], w[1].tolist(), w[3]) for w in v] == [(w[0], w[1].tolist(), w[3]) for w in first]


def test_patch_set_rules(ctx_factory):
    """the stored patch is the normalised one, with its Sbb; every refused upload leaves the old set usable; a new template
    upload makes the stage return SBM_ERR_STATE until patches are uploaded again"""
    rs = np.random.RandomState(91)
    shapes = [(12, 9), (5, 20)]
    sizes = {(0, t): s for t, s in enumerate(shapes)}
    frames = [rs.randint(0, 256, (ROWS, COLS)).astype(np.uint8)]
    patches = {k: rs.randint(30, 200, (h, w)).astype(np.uint8) for k, (w, h) in sizes.items()}
    ts = template_set(shapes)
    ctx = ctx_factory()
    ctx.upload_templates(ts)
    src = Frames(frames, "strided")
    lists = [recs_of([(3, 4, 0, 0), (60, 50, 0, 1), (100, 2, 0, 0)])]
    with pytest.raises(capi.SbmError) as e:  # no set yet
        check(ctx, src, frames, lists, sizes, patches, 0.0)
    assert e.value.code == -4
    wide = np.zeros((9, 40), np.uint8)
    wide[:, :12] = patches[(0, 0)]
    ctx.upload_verify_patches([(0, 1, patches[(0, 1)]), (0, 0, wide[:, :12])])  # any order; a row stride
    for (c, t), p in patches.items():
        stored, sbb = ctx.get_verify_patch(c, t, p.shape[1], p.shape[0])
        want = np_normalise(p)
        assert np.array_equal(stored, want) and sbb == np_sums(want, want)[2]
        assert stored.min() == 0 and stored.max() == 255
    base = check(ctx, src, frames, lists, sizes, patches, 0.0)
    P = capi.SbmVerifyPatch
    good = np.ascontiguousarray(patches[(0, 0)])
    other = np.ascontiguousarray(patches[(0, 1)])
    refusals = [
        ([P(0, 0, 12, 9, 12, 0, good.ctypes.data), P(0, 7, 12, 9, 12, 0, good.ctypes.data)], "patch 1"),   # a label the upload lacks
        ([P(0, 0, 12, 9, 12, 0, good.ctypes.data), P(0, 1, 20, 5, 20, 0, other.ctypes.data)], "patch 1"),  # not the level-0 size
        ([P(0, 0, 12, 9, 12, 0, good.ctypes.data), P(0, 1, 5, 20, 5, 0, other.ctypes.data), P(0, 0, 12, 9, 12, 0, good.ctypes.data)], "patch 2"),
        ([P(0, 0, 12, 9, 11, 0, good.ctypes.data)], "patch 0"),                                            # stride < width
    ]
    for recs, name in refusals:
        with pytest.raises(capi.SbmError) as e:
            ctx.upload_verify_patches_raw(recs)
        assert e.value.code == -1 and name in str(e.value), str(e.value)
        again = check(ctx, src, frames, lists, sizes, patches, 0.0)
        assert [(w[0], w[1].tolist(), w[3]) for w in again] == [(w[0], w[1].tolist(), w[3]) for w in base]
    # a smaller set replaces the old one; an empty one clears it
    ctx.upload_verify_patches([(0, 1, patches[(0, 1)])])
    w = check(ctx, src, frames, lists, sizes, {(0, 1): patches[(0, 1)]}, 0.0, keep_unverified=True)
    assert w[0][3] == (3, 4)
    ctx.upload_verify_patches([])
    assert check(ctx, src, frames, lists, sizes, {}, 0.0)[0][3] == (0, 4)
    # another template upload: the set is gone with the templates it belonged to
    ctx.upload_verify_patches([(0, t, p) for (_, t), p in patches.items()])
    ctx.upload_templates(ts)
    with pytest.raises(capi.SbmError) as e:
        check(ctx, src, frames, lists, sizes, patches, 0.0)
    assert e.value.code == -4
    with pytest.raises(capi.SbmError) as e:
        ctx.get_verify_patch(0, 0, 12, 9)
    assert e.value.code == -4
    ctx.upload_verify_patches([(0, t, p) for (_, t), p in patches.items()])
    again = check(ctx, src, frames, lists, sizes, patches, 0.0)
    assert [(w[0], w[1].tolist(), w[3]) for w in again] == [(w[0], w[1].tolist(), w[3]) for w in base]


def test_captured_stage_follows_the_frames(ctx_factory):
    """the stage twice on one stream inside a torch.cuda.graph capture (a single chain: the second call verifies the
    first's output), the frames overwritten between replays: the results follow the frames"""
    import torch

    rs = np.random.RandomState(101)
    shapes = [(16, 16), (40, 12)]
    sizes = {(0, t): s for t, s in enumerate(shapes)}
    patches = {k: rs.randint(0, 256, (h, w)).astype(np.uint8) for k, (w, h) in sizes.items()}
    B, cap = 3, 10
    sets = []
    for k in range(3):
        fr = [rs.randint(0, 256, (ROWS, COLS, 3)).astype(np.uint8) for _ in range(B)]
        for f in fr[: k + 1]:  # a scoring ROI in some frames, another set of frames each time
            f[20:36, 30:46] = patches[(0, 0)][:, :, None]
        sets.append(fr)
    rows = [(30, 20, 0, 0), (5, 60, 0, 1), (80, 3, 0, 0), (31, 20, 0, 0), (0, 0, 0, 1)]
    lists = [recs_of(rows), recs_of(rows[::-1]), recs_of(rows[1:])]
    buf = np.zeros((B, cap), MATCH_DTYPE)
    for f, l in enumerate(lists):
        buf[f, : len(l)] = l
    counts = np.array([[len(l), 0] for l in lists], np.int32)
    ctx = ctx_factory()
    ctx.upload_templates(template_set(shapes))
    ctx.upload_verify_patches([(0, t, p) for (_, t), p in patches.items()])
    src = Frames(sets[0], "strided")
    d_recs = torch.from_numpy(buf.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    d_cnt = torch.from_numpy(counts.reshape(-1)).to("cuda:0")
    d_mid = torch.zeros(B * cap * REC, dtype=torch.uint8, device="cuda:0")
    d_mids = torch.zeros(B * cap, dtype=torch.float32, device="cuda:0")
    d_midc = torch.zeros(B * 2, dtype=torch.int32, device="cuda:0")
    d_out = torch.zeros(B * cap * REC, dtype=torch.uint8, device="cuda:0")
    d_sc = torch.zeros(B * cap, dtype=torch.float32, device="cuda:0")
    d_oc = torch.zeros(B * 2, dtype=torch.int32, device="cuda:0")

    def step(stream):
        src.verify(ctx, d_recs.data_ptr(), d_cnt.data_ptr(), cap, 0.3, d_mid.data_ptr(), d_mids.data_ptr(), cap, d_midc.data_ptr(), stream=stream)
        src.verify(ctx, d_mid.data_ptr(), d_midc.data_ptr(), cap, 0.8, d_out.data_ptr(), d_sc.data_ptr(), cap, d_oc.data_ptr(), stream=stream)

    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        step(s.cuda_stream)  # warm-up: the scratch is made outside the capture
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(torch.cuda.current_stream().cuda_stream)
    seen = []
    for k in (1, 2, 0):
        src.write(sets[k])
        d_oc.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        oc = d_oc.cpu().numpy().reshape(-1, 2)
        for f in range(B):
            kept, ks, _, pair = np_verify_frame(sets[k][f], buf[f], sizes, patches, 0.8, count=len(lists[f]), cap=cap)  # (0.8 >= 0.3: the chain keeps these)
            assert tuple(oc[f]) == pair, (k, f)
            n = pair[0]
            assert rows_of(d_out.cpu().numpy()[f * cap * REC: (f * cap + n) * REC].view(MATCH_DTYPE)) == rows_of(buf[f][kept])
            assert np.array_equal(bits(d_sc.cpu().numpy()[f * cap: f * cap + n]), bits(ks))
        seen.append(oc[:, 0].tolist())
    assert len({tuple(s) for s in seen}) == 3  # three sets of frames, three results
