"""-m gpu: sbm_match_batch_device_planes -- the batched match on PLANAR frames of three channels, named by a device table of three
plane addresses per frame that the level-0 gradient kernels read when they run (the loop of Detector::match, line2Dup.cpp:1078).

  geometries  3 frames of 448 x 576 x 3 and of 512 x 768 x 3 (the BGR worlds of test_gpu_source_pass.py): the object against the right
              border, against the bottom border, absent; pyramid {4, 8}, the streaming kernel forced (18 rows per item)
  tables      [3, H, W] tensors (torch_frames.plane_table), nine separately allocated planes with a frame listed twice and one in
              (2, 1, 0) order, windows of larger planar noise canvases at odd offsets, tables of mask addresses, a table rewritten
              between the replays of one captured graph
  checked     canonical multisets against oracle.Pyramid for the frames the table presents, and against sbm_match_batch_device_ptrs on
              the interleaved frames; sbm_get_source_form == 1; the three "k_quantize" launches of the sparse path; every frame's maps
              after the caller's planes were overwritten (the retained copy is the interleaved frame)
  other paths the tile kernel, a width that is no multiple of 4, a {2, 4} pyramid, a threshold < 0, sbm_nms_batch_device behind the call
  arguments   every host check answers SBM_ERR_INVALID and leaves the context usable

The gradient stage takes the channel of maximum magnitude, a symmetric choice but for exact ties (which go to the lower channel,
line2Dup.cpp:370-387): on these scenes the ORDER of the planes shows in the maps of the `absent` frame (a few pixels at both levels)
and not in the lists, so the (2, 1, 0) cases compare maps as well, against the oracle on the channel-reversed frame."""
import numpy as np
import pytest

import any_geometry_cases as AG
import frame_mask_cases as FM
from shape_based_matching_amd import capi, torch_frames
from shape_based_matching_amd.templates import MATCH_DTYPE
from test_gpu_frame_ptrs import Call, dev, maps_equal, to_dev
from test_gpu_nms_device import rows_of
from test_gpu_source_pass import GEO, NAMES, STRIDED, ctx, expected, world  # noqa: F401  (ctx, world: fixtures)
from test_gpu_sparse_geometry import assert_sparse_launches
from test_gpu_sparse_gradient import CAP, NT, THR, multiset

pytestmark = pytest.mark.gpu
REC = MATCH_DTYPE.itemsize
SBM_ERR_INVALID = -1
BGR = ["P", "R"]  # the two BGR worlds


def planar(frame):
    """[H, W, 3] -> a [3, H, W] device tensor"""
    return to_dev(np.moveaxis(frame, -1, 0))


def addresses(tensors, orders=None):
    """plane addresses of [3, H, W] device tensors, tensor i's planes in orders[i]"""
    out = []
    for i, t in enumerate(tensors):
        a, stride = torch_frames.plane_addresses(t, orders[i] if orders else (0, 1, 2))
        assert stride == t.shape[2]
        out += a
    return out


class PlaneCall(Call):
    """Call with a plane table: three entries per frame"""

    def __init__(self, n, cap=CAP):
        super().__init__(n, cap)
        self.d_tab = self.torch.zeros(3 * n, dtype=self.torch.int64, device=dev())
        self.torch.cuda.synchronize()

    def run(self, c, ptrs, rows, cols, stride, thr=THR, mask_ptrs=None, flags=0, write=True):
        assert len(ptrs) % 3 == 0
        n = len(ptrs) // 3
        if write:
            self.write(self.d_tab, ptrs)
        if mask_ptrs is not None:
            self.write(self.d_mtab, mask_ptrs)
        self.d_cnt.fill_(-1)
        self.torch.cuda.synchronize()
        c.match_batch_device_planes(self.d_tab.data_ptr(), n, rows, cols, stride, thr, self.d_out.data_ptr(), self.cap, self.d_cnt.data_ptr(),
                                    d_mask_ptrs=self.d_mtab.data_ptr() if mask_ptrs is not None else 0, flags=flags, stream=self.stream.cuda_stream)
        return self.lists(n)


@pytest.fixture(scope="module")
def reversed_absent(world, oracle):  # noqa: F811
    """the oracle on the `absent` frame with its channels reversed, per BGR world: pyramid and list; the maps differ from the
    straight frame's (ties between channels), which is what makes a (2, 1, 0) listing telling"""
    ts = world["ts"]
    out = {}
    for g in BGR:
        f = np.ascontiguousarray(world[g]["frames"]["absent"][..., ::-1])
        p = oracle.Pyramid.build(f, [4, 8], 30.0)
        out[g] = {"pyr": p, "want": multiset(p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, THR, n_threads=NT))}
        straight = world[g]["pyr"]["absent"]
        assert not np.array_equal(p.quantized(0), straight.quantized(0)) and not np.array_equal(p.quantized(1), straight.quantized(1)), g
    yield out
    for g in BGR:
        out[g]["pyr"].free()


def pyramids_equal(c, pyrs):
    """get_quantized_frame(1, b) for every frame, then (0, b) in reverse order, against the oracle's pyramids"""
    for b, p in enumerate(pyrs):
        assert np.array_equal(c.get_quantized_frame(1, b), p.quantized(1)), b
    for b, p in reversed(list(enumerate(pyrs))):
        assert np.array_equal(c.get_quantized_frame(0, b), p.quantized(0)), b


# ---- identity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", BGR)
def test_one_tensor_per_frame_is_the_interleaved_call(world, ctx, geo):  # noqa: F811
    import torch

    rows, cols, ch = GEO[geo]
    e = world[geo]
    frames = [e["frames"][n] for n in NAMES]
    want = [e["want"][n] for n in NAMES]
    c = ctx()
    # sbm_match_batch_device_ptrs on the interleaved frames
    d_inter = [to_dev(f) for f in frames]
    icall = Call(3)
    interleaved = icall.run(c, [t.data_ptr() for t in d_inter], rows, cols, cols * ch, ch, 0)
    # the same pixels as [3, H, W] tensors, the table written by plane_table on the call's stream
    tensors = [planar(f) for f in frames]
    call = PlaneCall(3)
    tab, stride = torch_frames.plane_table(tensors, out=call.d_tab, stream=call.stream)
    assert tab is call.d_tab and stride == cols
    assert call.d_tab.cpu().tolist() == addresses(tensors)
    call.run(c, addresses(tensors), rows, cols, stride, write=False)  # (the first call of its kind on the context)
    c.set_profiling(True)
    got = call.run(c, addresses(tensors), rows, cols, stride, write=False)
    assert got == interleaved == want
    assert c.source_form() == expected(STRIDED)
    assert_sparse_launches(c)
    c.set_profiling(False)
    for t in tensors:  # the call is synchronised: the planes are the caller's again
        t.fill_(0xFF)
    torch.cuda.synchronize()
    maps_equal(c, e, NAMES)  # from the retained copy: the interleaved frame


def test_plane_table_of_a_batch_tensor_in_bgr_order(world, ctx, reversed_absent):  # noqa: F811
    """an RGB [B, 3, H, W] batch presented as the BGR frames it holds: order (2, 1, 0), a new table, no copy of the pixels"""
    rows, cols, ch = GEO["P"]
    e = world["P"]
    rgb = to_dev(np.stack([np.moveaxis(e["frames"][n][..., ::-1], -1, 0) for n in NAMES]))  # [3, 3, H, W], channels R, G, B
    c = ctx()
    call = PlaneCall(3)
    tab, stride = torch_frames.plane_table(rgb, order=(2, 1, 0), stream=call.stream)
    assert tab.dtype == call.torch.int64 and tab.is_cuda and tab.numel() == 9 and stride == cols
    call.d_tab = tab
    assert call.run(c, tab.cpu().tolist(), rows, cols, stride, write=False) == [e["want"][n] for n in NAMES]
    maps_equal(c, e, NAMES)
    # ... and as it lies (R, G, B taken for B, G, R): the reversed frames, whose maps differ where channels tie
    tab, stride = torch_frames.plane_table(rgb, stream=call.stream)
    call.d_tab = tab
    got = call.run(c, tab.cpu().tolist(), rows, cols, stride, write=False)
    assert got[2] == reversed_absent["P"]["want"]
    assert np.array_equal(c.get_quantized_frame(1, 2), reversed_absent["P"]["pyr"].quantized(1))
    assert np.array_equal(c.get_quantized_frame(0, 2), reversed_absent["P"]["pyr"].quantized(0))


# ---- scattered ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", BGR)
def test_nine_separate_planes_one_frame_twice_one_reversed(world, ctx, reversed_absent, geo):  # noqa: F811
    import torch

    rows, cols, ch = GEO[geo]
    e = world[geo]
    # nine allocations; `bottom` is listed twice, `absent` in (2, 1, 0) order: the channel-reversed frame
    planes = {n: [to_dev(e["frames"][n][..., k]) for k in range(3)] for n in NAMES}
    listing = [("bottom", (0, 1, 2)), ("absent", (2, 1, 0)), ("right", (0, 1, 2)), ("bottom", (0, 1, 2))]
    ptrs = [planes[n][k].data_ptr() for n, order in listing for k in order]
    assert len(set(ptrs)) == 9
    rev = reversed_absent[geo]
    want = [e["want"]["bottom"], rev["want"], e["want"]["right"], e["want"]["bottom"]]
    pyrs = [e["pyr"]["bottom"], rev["pyr"], e["pyr"]["right"], e["pyr"]["bottom"]]
    c = ctx()
    call = PlaneCall(4)
    call.run(c, ptrs, rows, cols, cols)
    c.set_profiling(True)
    got = call.run(c, ptrs, rows, cols, cols)
    assert got == want
    assert c.source_form() == expected(STRIDED)
    assert_sparse_launches(c)
    c.set_profiling(False)
    for ps in planes.values():
        for t in ps:
            t.fill_(0xFF)
    torch.cuda.synchronize()
    pyramids_equal(c, pyrs)  # frame 1 is the REVERSED frame's pyramid: the order reached the kernels and the retained copy
    # the three entries of a frame equal: the plane replicated three times
    g = np.ascontiguousarray(e["frames"]["right"][..., 1])
    d_g = to_dev(g)
    got = call.run(c, [d_g.data_ptr()] * 3, rows, cols, cols)
    gray3 = to_dev(np.repeat(g[..., None], 3, axis=-1))
    assert got == Call(1).run(c, [gray3.data_ptr()], rows, cols, cols * 3, 3, 0) and len(got[0]) > 0


# ---- windows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", BGR)
def test_windows_of_larger_planar_canvases(world, ctx, geo):  # noqa: F811
    """one [3, H + 64, W + 96] noise canvas per frame, the frame pasted at another (odd) place in each: the stride is the canvas's W.
    Canvas bytes outside a window must not reach a border pixel (BORDER_REPLICATE, REFLECT_101 are the window's)."""
    rows, cols, ch = GEO[geo]
    e = world[geo]
    want = [e["want"][n] for n in NAMES]
    crows, ccols = rows + 64, cols + 96
    rs = np.random.RandomState(rows + cols + 1)
    places = [(0, 1), (63, 95), (31, 7)]
    canvases, wins = [], []
    for n, (y, x) in zip(NAMES, places):
        cv = rs.randint(0, 256, (3, crows, ccols)).astype(np.uint8)
        cv[:, y:y + rows, x:x + cols] = np.moveaxis(e["frames"][n], -1, 0)
        canvases.append(to_dev(cv))
        wins.append(canvases[-1][:, y:y + rows, x:x + cols])
    ptrs, stride = torch_frames.plane_addresses(wins)
    assert stride == ccols and any(p % 2 for p in ptrs)
    c = ctx()
    call = PlaneCall(3)
    call.run(c, ptrs, rows, cols, stride)
    c.set_profiling(True)
    got = call.run(c, ptrs, rows, cols, stride)
    assert got == want, (geo, places)
    assert c.source_form() == expected(STRIDED)
    assert_sparse_launches(c)
    c.set_profiling(False)
    maps_equal(c, e, NAMES)


# ---- masks ----------------------------------------------------------------------------------------------------------------
def test_tables_of_mask_pointers(world, ctx, oracle):  # noqa: F811
    """three masks with two table entries equal: level 0 is built whole, by the plane form of the whole row loop.  The lists of
    sbm_match_batch_device_ptrs under the same mask table, and the oracle's for (frame f, mask f); level 1's masks are resized
    from the table's"""
    rows, cols, ch = GEO["P"]
    e = world["P"]
    ts = world["ts"]
    frames = [e["frames"][n] for n in NAMES]
    rs = np.random.RandomState(5)
    _, noise, rect5 = FM.rect_mask(rs, rows, cols), FM.noise_mask(rs, rows, cols), FM.rect_mask(rs, rows, cols, n_rects=5)
    masks = [rect5, noise, rect5]  # (the masks of test_gpu_frame_ptrs.py, the first listed twice)
    pyrs = [oracle.Pyramid.build(f, [4, 8], 30.0, mask=m) for f, m in zip(frames, masks)]
    try:
        want = [multiset(p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, THR, n_threads=NT)) for p in pyrs]
        plain = [e["want"][n] for n in NAMES]
        assert want != plain and want[0] and want[1]  # on the oracle alone: the masks decide, and the case is not empty
        c = ctx()
        d_rect, d_noise = to_dev(rect5), to_dev(noise)
        mptrs = [d_rect.data_ptr(), d_noise.data_ptr(), d_rect.data_ptr()]
        d_inter = [to_dev(f) for f in frames]
        ref = Call(3).run(c, [t.data_ptr() for t in d_inter], rows, cols, cols * ch, ch, 0, mask_ptrs=mptrs)
        tensors = [planar(f) for f in frames]
        call = PlaneCall(3)
        got = call.run(c, addresses(tensors), rows, cols, cols, mask_ptrs=mptrs)
        assert got == ref == want
        assert c.source_form() == 0  # masks: level 0's whole gradient
        pyramids_equal(c, pyrs)
    finally:
        for p in pyrs:
            p.free()


# ---- replay ---------------------------------------------------------------------------------------------------------------
def test_one_graph_serves_a_plane_table_that_is_rewritten(world, ctx, reversed_absent):  # noqa: F811
    """the graph's key holds the table's address, not its contents: the caller rewrites the table on the call's stream between
    replays -- the frames moved, the order changed -- and every call's lists are those of the frames the table named at that call.
    The planes are windows of [3, H, 3 W] canvases, so that their stride is the stride of the interleaved frames: a _ptrs call at
    the same table address, with every other argument equal, is another graph and gives the interleaved frames' lists."""
    rows, cols, ch = GEO["R"]
    e = world["R"]
    wide = {}
    for n in NAMES:
        cv = np.full((3, rows, 3 * cols), 0x5A, np.uint8)
        cv[:, :, cols:2 * cols] = np.moveaxis(e["frames"][n], -1, 0)
        wide[n] = to_dev(cv)
    stride = 3 * cols

    def ptrs_of(names, orders):
        wins = [wide[n][:, :, cols:2 * cols] for n in names]
        out = []
        for w, o in zip(wins, orders):
            a, s = torch_frames.plane_addresses(w, o)
            assert s == stride
            out += a
        return out

    c = ctx()
    call = PlaneCall(3)
    straight, rev = (0, 1, 2), (2, 1, 0)
    steps = [(["right", "bottom", "absent"], [straight] * 3), (["absent", "right", "right"], [rev, straight, straight]),
             (["bottom", "absent", "right"], [straight, rev, straight]), (["right", "bottom", "bottom"], [straight] * 3)]

    def step(names, orders):
        got = call.run(c, ptrs_of(names, orders), rows, cols, stride)
        want = [reversed_absent["R"]["want"] if (n == "absent" and o == rev) else e["want"][n] for n, o in zip(names, orders)]
        assert got == want, names
        assert c.source_form() == expected(STRIDED)

    step(*steps[0])  # warm-up: the tables of this threshold, the geometry
    c.set_graph_mode(True)
    step(*steps[0])
    assert c.graph_count() == 1
    for names, orders in steps[1:3]:
        step(names, orders)
        assert c.graph_count() == 1
    # the last rewritten table's maps: frame 1 is `absent` reversed
    pyramids_equal(c, [e["pyr"]["bottom"], reversed_absent["R"]["pyr"], e["pyr"]["right"]])
    step(*steps[3])
    assert c.graph_count() == 1
    maps_equal(c, e, steps[3][0])
    # a _ptrs call at the same table address, stride, channels and flags: not the plane graph
    inter = [to_dev(e["frames"][n]) for n in ("bottom", "right", "absent")]
    call.write(call.d_tab, [t.data_ptr() for t in inter])  # entries 0 .. 2; 3 .. 8 still name planes
    call.d_cnt.fill_(-1)
    call.torch.cuda.synchronize()
    c.match_batch_device_ptrs(call.d_tab.data_ptr(), 3, rows, cols, stride, ch, THR, call.d_out.data_ptr(), call.cap, call.d_cnt.data_ptr(),
                              stream=call.stream.cuda_stream)
    assert call.lists(3) == [e["want"][n] for n in ("bottom", "right", "absent")]
    assert c.graph_count() == 2
    # ... and the plane graph is still there for the plane call
    step(*steps[1])
    assert c.graph_count() == 2


# ---- other gradient paths -------------------------------------------------------------------------------------------------
def test_tile_kernel(world, ctx, reversed_absent):  # noqa: F811
    rows, cols, ch = GEO["P"]
    e = world["P"]
    c = ctx()
    c.set_quantize_mode("tile")
    tensors = {n: planar(e["frames"][n]) for n in NAMES}
    names = ["absent", "bottom", "right"]
    call = PlaneCall(3)
    got = call.run(c, addresses([tensors[n] for n in names], [(2, 1, 0), (0, 1, 2), (0, 1, 2)]), rows, cols, cols)
    assert got == [reversed_absent["P"]["want"], e["want"]["bottom"], e["want"]["right"]]
    assert c.source_form() == 0
    pyramids_equal(c, [reversed_absent["P"]["pyr"], e["pyr"]["bottom"], e["pyr"]["right"]])


@pytest.mark.parametrize("name", ["gray_1", "gray_2_4"])
def test_any_geometry(oracle, ctx_factory, name):
    """a width that is no multiple of 4 (211 columns, one level: the tile kernel's per-byte path) and a {2, 4} pyramid (the batched
    any-stride builder behind it), rows padded by 13 bytes; on the {2, 4} pyramid also one template at threshold -5.  The cases are
    gray: the three entries of a frame name its one plane, which is the gray frame replicated -- the gray frame's own lists and maps
    (every channel ties, the lower one is taken).  Then frames of three DIFFERENT planes against the oracle on the stacked frame."""
    import torch

    case = AG.case(oracle, name)
    c = ctx_factory(T=case.T)
    c.upload_templates(case.ts)
    n = len(case.frames)
    stride = case.cols + 13
    tensors = []
    for f in range(n):
        buf = np.full((case.rows, stride), 0xA5, np.uint8)
        buf[:, :case.cols] = case.frames[f]
        tensors.append(to_dev(buf))
    order = [3, 1, 4, 0, 2]
    ptrs = [tensors[f].data_ptr() for f in order for _ in range(3)]
    call = PlaneCall(n, cap=4096)
    for thr in AG.THRS:
        case.check_not_empty(n, thr)
        got = call.run(c, ptrs, case.rows, case.cols, stride, thr=thr)
        assert got == [case.want(f, thr) for f in order], (name, thr)
    for b, f in enumerate(order):
        for l in range(case.L):
            assert np.array_equal(c.get_quantized_frame(l, b), case.maps(f)[l]), (b, f, l)
    # three different planes per frame
    triples = [(0, 1, 2), (4, 0, 1), (2, 4, 0)]
    ptrs = [tensors[f].data_ptr() for t in triples for f in t]
    got = call.run(c, ptrs, case.rows, case.cols, stride, thr=AG.THRS[0])
    total = 0
    for b, t in enumerate(triples):
        pyr = oracle.Pyramid.build(np.ascontiguousarray(np.stack([case.frames[f] for f in t], -1)), list(case.T), AG.WEAK)
        ts = case.ts
        want = multiset(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, AG.THRS[0]))
        maps = [pyr.quantized(l) for l in range(case.L)]
        pyr.free()
        assert got[b] == want, (name, b, len(got[b]), len(want))
        total += len(want)
        for l in range(case.L):
            assert np.array_equal(c.get_quantized_frame(l, b), maps[l]), (b, l)
    assert total > 0
    if name != "gray_2_4":
        return
    one = case.ts.subset([2])
    c.upload_templates(one)
    ptrs = [tensors[f].data_ptr() for f in order for _ in range(3)]
    got = call.run(c, ptrs, case.rows, case.cols, stride, thr=-5.0)
    for b, f in enumerate(order):
        pyr = case.pyramid(f)
        want = multiset(pyr.match(one.levels, one.features, one.class_idx, one.template_id, -5.0))
        pyr.free()
        assert len(want) > 0 and got[b] == want, (b, f, len(got[b]), len(want))
    torch.cuda.synchronize()


def test_nms_stage_behind_the_call(world, ctx):  # noqa: F811
    """sbm_nms_batch_device on the call's stream right behind it: what the same stage keeps behind the _ptrs call"""
    import torch

    rows, cols, ch = GEO["P"]
    e = world["P"]
    frames = [e["frames"][n] for n in NAMES]
    c = ctx()
    out_cap = 256

    def kept_behind(run, call):
        d_kept = torch.zeros(3 * out_cap * REC, dtype=torch.uint8, device=dev())
        d_kc = torch.full((3 * 2,), -1, dtype=torch.int32, device=dev())
        torch.cuda.synchronize()
        run()
        c.nms_batch_device(call.d_out.data_ptr(), call.d_cnt.data_ptr(), CAP, 3, d_kept.data_ptr(), out_cap, d_kc.data_ptr(), 85.0, 0.3,
                           stream=call.stream.cuda_stream)
        call.stream.synchronize()
        kc = d_kc.cpu().numpy().reshape(3, 2)
        out = d_kept.cpu().numpy().reshape(3, out_cap * REC)
        assert (kc[:, 1] == 0).all() and (kc[:, 0] >= 0).all(), kc
        return [rows_of(out[f].view(MATCH_DTYPE)[: kc[f, 0]]) for f in range(3)]

    d_inter = [to_dev(f) for f in frames]
    icall = Call(3)
    icall.run(c, [t.data_ptr() for t in d_inter], rows, cols, cols * ch, ch, 0)  # (tables written, first call of the geometry)
    ref = kept_behind(lambda: c.match_batch_device_ptrs(icall.d_tab.data_ptr(), 3, rows, cols, cols * ch, ch, THR, icall.d_out.data_ptr(), CAP,
                                                        icall.d_cnt.data_ptr(), stream=icall.stream.cuda_stream), icall)
    tensors = [planar(f) for f in frames]
    call = PlaneCall(3)
    call.run(c, addresses(tensors), rows, cols, cols)
    got = kept_behind(lambda: c.match_batch_device_planes(call.d_tab.data_ptr(), 3, rows, cols, cols, THR, call.d_out.data_ptr(), CAP,
                                                          call.d_cnt.data_ptr(), stream=call.stream.cuda_stream), call)
    assert got == ref and sum(len(k) for k in got) > 0


# ---- arguments ------------------------------------------------------------------------------------------------------------
def test_host_checks_leave_the_context_usable(world, ctx):  # noqa: F811
    rows, cols, ch = GEO["P"]
    e = world["P"]
    tensors = [planar(e["frames"][n]) for n in NAMES]
    ptrs = addresses(tensors)
    want = [e["want"][n] for n in NAMES]
    c = ctx()
    call = PlaneCall(3)
    assert call.run(c, ptrs, rows, cols, cols) == want
    tab, out, cnt = call.d_tab.data_ptr(), call.d_out.data_ptr(), call.d_cnt.data_ptr()
    good = dict(d_plane_ptrs=tab, n_frames=3, rows=rows, cols=cols, stride=cols, threshold=THR, d_out=out, cap=CAP, d_counts=cnt, flags=0,
                stream=call.stream.cuda_stream)
    bad = [dict(d_plane_ptrs=0), dict(n_frames=0), dict(n_frames=-3), dict(flags=1), dict(flags=8), dict(flags=-1), dict(stride=cols - 1),
           dict(stride=0), dict(d_out=0), dict(d_counts=0), dict(rows=rows - 2)]
    # (the last is sbm_match_batch_device's own rule: 446 rows that T = 4 does not divide, line2Dup.cpp:639)
    for change in bad:
        with pytest.raises(capi.SbmError) as err:
            c.match_batch_device_planes(**dict(good, **change))
        assert err.value.code == SBM_ERR_INVALID, change
        assert call.run(c, ptrs, rows, cols, cols) == want, change
    # a stride above 16 with more than one frame, as sbm_match_batch_device refuses it (valid planes of that geometry in the table)
    r2, c2, _ = GEO["R"]
    big = [planar(world["R"]["frames"][n]) for n in NAMES]
    call.write(call.d_tab, addresses(big))
    wide = capi.Context(T=(4, 32), weak_threshold=30.0, device_id=0)
    try:
        wide.upload_templates(world["ts"])
        with pytest.raises(capi.SbmError) as err:
            wide.match_batch_device_planes(tab, 3, r2, c2, c2, THR, out, CAP, cnt, stream=call.stream.cuda_stream)
        assert err.value.code == SBM_ERR_INVALID
    finally:
        wide.close()
    assert call.run(c, ptrs, rows, cols, cols) == want
