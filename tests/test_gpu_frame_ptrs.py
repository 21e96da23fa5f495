"""-m gpu: sbm_match_batch_device_ptrs -- the batched match whose frames (and masks) are named by a device table of addresses that
the level-0 gradient kernels read when they run (the loop of Detector::match, line2Dup.cpp:1078, over frames that lie anywhere).

  geometries  3 frames of 448 x 576 x 3, 512 x 704 x 1 and 512 x 768 x 3 (the worlds of test_gpu_source_pass.py): the object against
              the right border, against the bottom border, absent; pyramid {4, 8}, the streaming kernel forced (18 rows per item)
  tables      the identity over one block, separately allocated tensors with one listed twice, windows of larger noise canvases at
              odd and at aligned offsets, tables of mask addresses, a table rewritten between the replays of one captured graph
  checked     canonical multisets against oracle.Pyramid for the frames in table order, and against sbm_match_batch_device(_masked)
              on a packed copy of the same frames; sbm_get_source_form; the three "k_quantize" launches of the sparse path; every
              frame's maps after the caller's memory was overwritten
  other paths the tile kernel, a width that is no multiple of 4, a {2, 4} pyramid, a partly filled packed group, a threshold < 0
  arguments   every host check answers SBM_ERR_INVALID and leaves the context usable"""
import numpy as np
import pytest

import any_geometry_cases as AG
import frame_mask_cases as FM
from shape_based_matching_amd import capi
from shape_based_matching_amd.templates import MATCH_DTYPE
from test_gpu_source_pass import GEO, LINES, NAMES, STRIDED, ctx, expected, world  # noqa: F401  (ctx, world: fixtures)
from test_gpu_sparse_geometry import assert_sparse_launches, run_batch
from test_gpu_sparse_gradient import CAP, NT, THR, multiset

pytestmark = pytest.mark.gpu
REC = MATCH_DTYPE.itemsize
ALIGNED4 = capi.SBM_PTRS_ALIGNED4
SBM_ERR_INVALID = -1


def dev():
    import torch

    return torch.device("cuda", 0)


def to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


class Call:
    """the result buffers, the two tables and the stream of a table call of up to n frames"""

    def __init__(self, n, cap=CAP):
        import torch

        self.torch, self.n, self.cap = torch, n, cap
        self.d_out = torch.zeros(n * cap * REC, dtype=torch.uint8, device=dev())
        self.d_cnt = torch.zeros(n * 2, dtype=torch.int32, device=dev())
        self.d_tab = torch.zeros(n, dtype=torch.int64, device=dev())
        self.d_mtab = torch.zeros(n, dtype=torch.int64, device=dev())
        self.stream = torch.cuda.Stream(device=dev())
        torch.cuda.synchronize()

    def write(self, tab, ptrs):
        """new addresses into a table on the call's stream, from pinned memory: ordered before the next call's kernels"""
        host = self.torch.tensor(list(ptrs), dtype=self.torch.int64).pin_memory()
        with self.torch.cuda.stream(self.stream):
            tab[: len(ptrs)].copy_(host, non_blocking=True)
        self.stream.synchronize()  # (the pinned source may go)

    def run(self, c, ptrs, rows, cols, stride, ch, flags=0, thr=THR, mask_ptrs=None):
        n = len(ptrs)
        self.write(self.d_tab, ptrs)
        if mask_ptrs is not None:
            self.write(self.d_mtab, mask_ptrs)
        self.d_cnt.fill_(-1)
        self.torch.cuda.synchronize()
        c.match_batch_device_ptrs(self.d_tab.data_ptr(), n, rows, cols, stride, ch, thr, self.d_out.data_ptr(), self.cap, self.d_cnt.data_ptr(),
                                  d_mask_ptrs=self.d_mtab.data_ptr() if mask_ptrs is not None else 0, flags=flags, stream=self.stream.cuda_stream)
        return self.lists(n)

    def lists(self, n):
        self.stream.synchronize()
        cnt = self.d_cnt.cpu().numpy().reshape(-1, 2)
        recs = self.d_out.cpu().numpy().view(MATCH_DTYPE).reshape(self.n, self.cap)
        assert (cnt[:n, 1] == 0).all() and (cnt[:n, 0] >= 0).all() and (cnt[:n, 0] <= self.cap).all(), cnt
        return [multiset(recs[f, : cnt[f, 0]]) for f in range(n)]


def maps_equal(c, e, names):
    for b, n in enumerate(names):
        assert np.array_equal(c.get_quantized_frame(1, b), e["pyr"][n].quantized(1)), (b, n)
    for b, n in reversed(list(enumerate(names))):
        assert np.array_equal(c.get_quantized_frame(0, b), e["pyr"][n].quantized(0)), (b, n)


# ---- 3. identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", list(GEO))
def test_identity_table_is_the_contiguous_call(world, ctx, geo):
    import torch

    rows, cols, ch = GEO[geo]
    e = world[geo]
    frames = [e["frames"][n] for n in NAMES]
    want = [e["want"][n] for n in NAMES]
    c = ctx()
    contiguous, _ = run_batch(c, frames)
    d_block = to_dev(np.stack(frames))
    fs = rows * cols * ch
    ptrs = [d_block.data_ptr() + f * fs for f in range(3)]
    call = Call(3)
    call.run(c, ptrs, rows, cols, cols * ch, ch, ALIGNED4)  # (the first call of its kind on the context)
    c.set_profiling(True)
    got = call.run(c, ptrs, rows, cols, cols * ch, ch, ALIGNED4)
    assert got == contiguous == want
    assert c.source_form() == expected(LINES)
    assert_sparse_launches(c)
    c.set_profiling(False)
    d_block.fill_(0xFF)  # the call is synchronised: the block is the caller's again
    torch.cuda.synchronize()
    maps_equal(c, e, NAMES)
    # the flag cleared: the strided form, the same lists
    d_block.copy_(to_dev(np.stack(frames)))
    torch.cuda.synchronize()
    assert call.run(c, ptrs, rows, cols, cols * ch, ch, 0) == want
    assert c.source_form() == expected(STRIDED)


# ---- 4. scattered ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", list(GEO))
def test_separately_allocated_frames_one_listed_twice(world, ctx, geo):
    import torch

    rows, cols, ch = GEO[geo]
    e = world[geo]
    tensors = [to_dev(e["frames"][n]) for n in NAMES]
    order = (2, 0, 2, 1)
    names = [NAMES[i] for i in order]
    c = ctx()
    call = Call(4)
    ptrs = [tensors[i].data_ptr() for i in order]
    call.run(c, ptrs, rows, cols, cols * ch, ch, ALIGNED4)
    c.set_profiling(True)
    got = call.run(c, ptrs, rows, cols, cols * ch, ch, ALIGNED4)
    assert got == [e["want"][n] for n in names]
    assert c.source_form() == expected(LINES)
    assert_sparse_launches(c)
    c.set_profiling(False)
    for t in tensors:
        t.fill_(0xFF)
    torch.cuda.synchronize()
    maps_equal(c, e, names)


# ---- 5. windows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", list(GEO))
def test_windows_of_larger_canvases(world, ctx, geo):
    """one noise canvas per frame, 64 rows and 96 columns larger than the frame, the frame pasted at another place in each: the
    stride is the canvas row.  Canvas bytes outside a window must not reach a border pixel (BORDER_REPLICATE, REFLECT_101 are the
    window's).  Odd BGR pointers with the flag cleared: the strided form; offsets of 4 pixels with the flag: the line form."""
    rows, cols, ch = GEO[geo]
    e = world[geo]
    want = [e["want"][n] for n in NAMES]
    crows, ccols = rows + 64, cols + 96
    stride = ccols * ch
    rs = np.random.RandomState(rows + cols)
    c = ctx()
    call = Call(3)
    for places, flags, form in (([(0, 1), (63, 95), (31, 7)], 0, STRIDED), ([(0, 4), (64, 96), (31, 8)], ALIGNED4, LINES)):
        canvases = []
        for n, (y, x) in zip(NAMES, places):
            cv = rs.randint(0, 256, (crows, ccols) + ((3,) if ch == 3 else ())).astype(np.uint8)
            cv[y:y + rows, x:x + cols] = e["frames"][n]
            canvases.append(to_dev(cv))
        ptrs = [cv.data_ptr() + y * stride + x * ch for cv, (y, x) in zip(canvases, places)]
        if ch == 3 and not flags:
            assert any(p % 2 for p in ptrs)
        if flags:
            assert all(p % 4 == 0 for p in ptrs) and stride % 4 == 0
        call.run(c, ptrs, rows, cols, stride, ch, flags)
        c.set_profiling(True)
        got = call.run(c, ptrs, rows, cols, stride, ch, flags)
        assert got == want, (geo, places)
        assert c.source_form() == expected(form)
        assert_sparse_launches(c)
        c.set_profiling(False)
        maps_equal(c, e, NAMES)


# ---- 6. masks -------------------------------------------------------------------------------------------------------------
def packed_masked(c, frames, masks, mask_stride):
    """sbm_match_batch_device_masked on packed copies of the frames and masks"""
    import torch

    n, (rows, cols) = len(frames), frames[0].shape[:2]
    ch = 1 if frames[0].ndim == 2 else 3
    d_img, d_masks = to_dev(np.stack(frames)), to_dev(np.stack(masks))
    d_out = torch.zeros(n * CAP * REC, dtype=torch.uint8, device=dev())
    d_cnt = torch.full((n * 2,), -1, dtype=torch.int32, device=dev())
    st = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    c.match_batch_device_masked(d_img.data_ptr(), rows * cols * ch, n, rows, cols, cols * ch, ch, d_masks.data_ptr(), mask_stride, THR, d_out.data_ptr(),
                                CAP, d_cnt.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    cnt = d_cnt.cpu().numpy().reshape(n, 2)
    recs = d_out.cpu().numpy().view(MATCH_DTYPE).reshape(n, CAP)
    assert (cnt[:, 1] == 0).all() and (cnt[:, 0] >= 0).all() and (cnt[:, 0] <= CAP).all(), cnt
    return [multiset(recs[f, : cnt[f, 0]]) for f in range(n)]


def test_tables_of_mask_pointers(world, ctx, oracle):
    """three different masks, then one mask listed three times: the lists of sbm_match_batch_device_masked on packed copies
    (mask_stride = rows * cols, and 0), and the oracle's for (frame f, mask f)"""
    rows, cols, ch = GEO["P"]
    e = world["P"]
    ts = world["ts"]
    frames = [e["frames"][n] for n in NAMES]
    rs = np.random.RandomState(5)
    rect3, noise, rect5 = FM.rect_mask(rs, rows, cols), FM.noise_mask(rs, rows, cols), FM.rect_mask(rs, rows, cols, n_rects=5)
    masks = [rect5, noise, rect3]

    def oracle_lists(ms):
        out = []
        for f, m in zip(frames, ms):
            p = oracle.Pyramid.build(f, [4, 8], 30.0, mask=m)
            out.append(multiset(p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, THR, n_threads=NT)))
            p.free()
        return out

    want3, want1 = oracle_lists(masks), oracle_lists([masks[0]] * 3)
    plain = [e["want"][n] for n in NAMES]
    # on the oracle alone: the masks decide, and neither case is empty
    assert want3 != plain and want1 != plain and want3 != want1 and want3[0] and want3[1] and want1[0] and want1[1]
    c = ctx()
    ref3, ref1 = packed_masked(c, frames, masks, rows * cols), packed_masked(c, frames, masks, 0)
    d_frames = [to_dev(f) for f in frames]
    d_masks = [to_dev(m) for m in masks]
    call = Call(3)
    ptrs = [t.data_ptr() for t in d_frames]
    for mptrs, want, ref in (([m.data_ptr() for m in d_masks], want3, ref3), ([d_masks[0].data_ptr()] * 3, want1, ref1)):
        got = call.run(c, ptrs, rows, cols, cols * ch, ch, ALIGNED4, mask_ptrs=mptrs)
        assert got == ref == want
        assert c.source_form() == 0  # masks: level 0's whole gradient
    # level 1's masks are resized from the table's: every frame's maps under its own mask
    call.run(c, ptrs, rows, cols, cols * ch, ch, 0, mask_ptrs=[m.data_ptr() for m in d_masks])
    for f in range(3):
        p = oracle.Pyramid.build(frames[f], [4, 8], 30.0, mask=masks[f])
        for l in (1, 0):
            assert np.array_equal(c.get_quantized_frame(l, f), p.quantized(l)), (f, l)
        p.free()


# ---- 7. other gradient paths ----------------------------------------------------------------------------------------------
def test_tile_kernel(world, ctx):
    rows, cols, ch = GEO["P"]
    e = world["P"]
    c = ctx()
    c.set_quantize_mode("tile")
    tensors = [to_dev(e["frames"][n]) for n in NAMES]
    call = Call(3)
    got = call.run(c, [t.data_ptr() for t in reversed(tensors)], rows, cols, cols * ch, ch, ALIGNED4)
    assert got == [e["want"][n] for n in reversed(NAMES)]
    assert c.source_form() == 0
    maps_equal(c, e, NAMES[::-1])


@pytest.mark.parametrize("name", ["gray_1", "gray_2_4"])
def test_any_geometry(oracle, ctx_factory, name):
    """a width that is no multiple of 4 (211 columns, one level) and a {2, 4} pyramid: the tile kernel's table form and the batched
    any-stride builder behind it; rows padded by 13 bytes; on the {2, 4} pyramid also one template at threshold -5"""
    import torch

    case = AG.case(oracle, name)
    c = ctx_factory(T=case.T)
    c.upload_templates(case.ts)
    n = len(case.frames)
    line = case.cols * case.ch
    stride = line + 13
    tensors = []
    for f in range(n):
        buf = np.full((case.rows, stride), 0xA5, np.uint8)
        buf[:, :line] = case.frames[f].reshape(case.rows, line)
        tensors.append(to_dev(buf))
    order = [3, 1, 4, 0, 2]
    ptrs = [tensors[f].data_ptr() for f in order]
    call = Call(n, cap=4096)
    for thr in AG.THRS:
        case.check_not_empty(n, thr)
        got = call.run(c, ptrs, case.rows, case.cols, stride, case.ch, 0, thr=thr)
        assert got == [case.want(f, thr) for f in order], (name, thr)
    for b, f in enumerate(order):
        for l in range(case.L):
            assert np.array_equal(c.get_quantized_frame(l, b), case.maps(f)[l]), (b, f, l)
    if name != "gray_2_4":
        return
    one = case.ts.subset([2])
    c.upload_templates(one)
    got = call.run(c, ptrs, case.rows, case.cols, stride, case.ch, 0, thr=-5.0)
    for b, f in enumerate(order):
        pyr = case.pyramid(f)
        want = multiset(pyr.match(one.levels, one.features, one.class_idx, one.template_id, -5.0))
        pyr.free()
        assert len(want) > 0 and got[b] == want, (b, f, len(got[b]), len(want))
    torch.cuda.synchronize()


def test_five_frames_where_the_contiguous_call_packs(world, ctx):
    """576 columns: the 96-column last strip takes two frames per wave in the contiguous form, so five frames end in a partly
    filled group there; the table form gives every frame a wave of its own -- the same lists and maps"""
    rows, cols, ch = GEO["P"]
    e = world["P"]
    names = ["right", "absent", "bottom", "right", "bottom"]
    frames = [e["frames"][n] for n in names]
    c = ctx()
    contiguous, _ = run_batch(c, frames)
    tensors = {n: to_dev(e["frames"][n]) for n in NAMES}
    call = Call(5)
    c.set_profiling(True)
    got = call.run(c, [tensors[n].data_ptr() for n in names], rows, cols, cols * ch, ch, ALIGNED4)
    assert got == contiguous == [e["want"][n] for n in names]
    assert_sparse_launches(c)
    c.set_profiling(False)
    maps_equal(c, e, names)
    # the whole gradient through the table at the same geometry (a mask table of all-255 masks forces it)
    full = to_dev(np.full((rows, cols), 255, np.uint8))
    got = call.run(c, [tensors[n].data_ptr() for n in names], rows, cols, cols * ch, ch, 0, mask_ptrs=[full.data_ptr()] * 5)
    assert got == contiguous and c.source_form() == 0
    maps_equal(c, e, names)


# ---- 8. replay ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["always", "auto"])
def test_one_graph_serves_a_table_that_is_rewritten(world, ctx, mode):
    """the graph's key holds the table's address, not its contents: the caller rewrites the table on the call's stream between
    replays and every call's lists are those of the frames the table named at that call"""
    rows, cols, ch = GEO["R"]
    e = world["R"]
    tensors = {n: to_dev(e["frames"][n]) for n in NAMES}
    c = ctx()
    call = Call(3)
    orders = [["right", "bottom", "absent"], ["absent", "right", "right"], ["bottom", "absent", "right"], ["right", "bottom", "bottom"]]

    def step(names):
        got = call.run(c, [tensors[n].data_ptr() for n in names], rows, cols, cols * ch, ch, ALIGNED4)
        assert got == [e["want"][n] for n in names], names
        assert c.source_form() == expected(LINES)

    step(orders[0])  # warm-up: the tables of this threshold, the geometry
    if mode == "always":
        c.set_graph_mode(True)
        step(orders[0])
        captured = c.graph_count()
        assert captured == 1
        for names in orders[1:]:
            step(names)
            assert c.graph_count() == captured
    else:
        c.set_pipeline_depth(2)  # drops what was captured; the default graph mode replays once a tuple repeats
        assert c.graph_count() == 0
        step(orders[1])  # first sighting of the tuple: plain launches
        assert c.graph_count() == 0
        step(orders[2])  # second sighting: captured
        assert c.graph_count() == 1
        step(orders[3])  # rewritten contents: a replay
        assert c.graph_count() == 1
    maps_equal(c, e, orders[3])
    # another flag value is another tuple
    got = call.run(c, [tensors[n].data_ptr() for n in orders[0]], rows, cols, cols * ch, ch, 0)
    assert got == [e["want"][n] for n in orders[0]] and c.source_form() == expected(STRIDED)


# ---- 9. arguments ---------------------------------------------------------------------------------------------------------
def test_host_checks_leave_the_context_usable(world, ctx):
    rows, cols, ch = GEO["P"]
    e = world["P"]
    tensors = [to_dev(e["frames"][n]) for n in NAMES]
    ptrs = [t.data_ptr() for t in tensors]
    want = [e["want"][n] for n in NAMES]
    c = ctx()
    call = Call(3)
    assert call.run(c, ptrs, rows, cols, cols * ch, ch, ALIGNED4) == want
    tab, out, cnt = call.d_tab.data_ptr(), call.d_out.data_ptr(), call.d_cnt.data_ptr()
    good = dict(d_frame_ptrs=tab, n_frames=3, rows=rows, cols=cols, stride=cols * ch, channels=ch, threshold=THR, d_out=out, cap=CAP, d_counts=cnt,
                flags=ALIGNED4, stream=call.stream.cuda_stream)
    bad = [dict(d_frame_ptrs=0), dict(n_frames=0), dict(n_frames=-3), dict(flags=2), dict(flags=ALIGNED4 | 8), dict(flags=-1),
           dict(stride=cols * ch - 1), dict(stride=cols), dict(d_out=0), dict(d_counts=0), dict(channels=2), dict(rows=rows - 2)]
    # (the last two are sbm_match_batch_device's own rules: the channel count, and 446 rows that T = 4 does not divide, line2Dup.cpp:639)
    for change in bad:
        with pytest.raises(capi.SbmError) as err:
            c.match_batch_device_ptrs(**dict(good, **change))
        assert err.value.code == SBM_ERR_INVALID, change
        assert call.run(c, ptrs, rows, cols, cols * ch, ch, ALIGNED4) == want, change
    # a stride above 16 with more than one frame, as sbm_match_batch_device refuses it (valid frames of that geometry in the table)
    r2, c2, ch2 = GEO["R"]
    big = [to_dev(world["R"]["frames"][n]) for n in NAMES]
    call.write(call.d_tab, [t.data_ptr() for t in big])
    wide = capi.Context(T=(4, 32), weak_threshold=30.0, device_id=0)
    try:
        wide.upload_templates(world["ts"])
        with pytest.raises(capi.SbmError) as err:
            wide.match_batch_device_ptrs(tab, 3, r2, c2, c2 * ch2, ch2, THR, out, CAP, cnt, stream=call.stream.cuda_stream)
        assert err.value.code == SBM_ERR_INVALID
    finally:
        wide.close()
