"""GPU: the HIP gradient half (k_quantize tile kernel, k_quantize_stream, k_pyrdown, k_resize_mask) against the numpy
restatement tests/gradient_spec.py, bit for bit, at the geometries and contents of tests/gradient_cases.py -- through
the stage entry points, build_pyramid in every quantize mode and the batched device path."""
import numpy as np
import pytest

import gradient_cases as G
import gradient_spec as S
from shape_based_matching_amd import capi, synth
from shape_based_matching_amd.templates import MATCH_DTYPE

pytestmark = pytest.mark.gpu

MODES = [("tile", 0), ("stream", 0), ("stream", 8), ("stream", 32), ("stream", 64), ("auto", 0)]


def _stage_cases():
    """level-0 inputs for the stage entry points: every geometry from 3 x 3 (the smallest the entry point accepts) to
    9 x 9, columns on both sides of the tile and strip edges, every content family"""
    cs = [c for c in G.small_geometries(9, 3)] + G.edge_col_cases((16, 17, 19)) + G.kind_cases()
    for ch in (1, 3):
        cs += G.border_edges(21, 19, ch) + G.boundary_ramps(23, 17, ch) + G.border_edges(17, 66, ch)
    cs += G.colour_ties(19, 23, 3) + G.colour_ties(9, 9, 4) + G.threshold_cases(8)
    return cs


STAGE_CASES = _stage_cases()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _eq(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("mode,hs", [("tile", 0), ("stream", 0), ("auto", 0)])
def test_quantized_orientations_equal_spec(ctx_factory, mode, hs):
    ctx = ctx_factory(T=(4,))
    ctx.set_quantize_mode(mode, hs)
    for case in STAGE_CASES:
        mag, q, ang = S.quantized_orientations(case.img, case.weak)
        g_mag, g_q, g_ang = ctx.quantized_orientations(case.img, case.weak, want_float=True)
        _eq(g_q, q, (case.name, "quantized"))
        _eq(g_mag, mag, (case.name, "magnitude"))
        _eq(g_ang, ang, (case.name, "angle"))


def test_quantized_orientations_refuses_below_3x3(ctx_factory):
    ctx = ctx_factory(T=(4,))
    for shape in ((2, 3), (3, 2), (2, 9), (9, 2)):
        for ch in (1, 3):
            img = np.zeros(shape if ch == 1 else shape + (3,), np.uint8)
            with pytest.raises(capi.SbmError):
                ctx.quantized_orientations(img, 10.0)


def test_float_angle_follows_unfused_phase(ctx_factory):
    """a frame whose gradients include pairs where OpenCV's fused (AVX2) `phase` gives another float angle: the HIP
    angle output equals the unfused spec there too (test_gradient_spec::test_fused_phase_moves_angles_but_no_bin)"""
    rs = np.random.RandomState(11)
    img = rs.randint(0, 256, (64, 96)).astype(np.uint8)
    ctx = ctx_factory(T=(4,))
    _, _, g_ang = ctx.quantized_orientations(img, 0.0)
    _eq(g_ang, S.quantized_orientations(img, 0.0)[2], "angle")


def test_pyrdown_chain_equals_spec(ctx_factory):
    """sbm_pyrdown (from 2 x 2, its smallest input) chained down to levels of 1 to 3 pixels on a side"""
    ctx = ctx_factory(T=(4,))
    cases = G.small_geometries(9, 2) + G.tiny_pyramids() + G.edge_col_cases((16, 17))
    for case in cases:
        src = case.img
        while src.shape[0] >= 2 and src.shape[1] >= 2:
            want = S.pyrdown(src)
            got = ctx.pyrdown(src)
            _eq(got, want, (case.name, src.shape))
            src = want
    for shape in ((1, 5), (5, 1), (1, 1)):
        with pytest.raises(capi.SbmError):
            ctx.pyrdown(np.zeros(shape, np.uint8))


def _pyramid_cases():
    """(T, case): geometries build_pyramid accepts (every level a multiple of T with rows*cols % 16 == 0), from the
    smallest ones to tile / strip edges, with levels of 1 to 3 pixels on a side"""
    out = []
    small = [(r, c) for r in range(1, 10) for c in range(1, 17) if (r * c) % 16 == 0] + [(16, 1), (16, 3)]
    for i, (r, c) in enumerate(small):
        for ch in (1, 3):
            out.append(((1,), G.Case(f"p{r}x{c}_{ch}ch", G.kind_image(300 + i, G.KINDS[i % 7], r, c, ch), 10.0)))
    for (r, c), T in (((8, 32), (1, 1, 1)), ((4, 64), (1, 1, 1)), ((12, 64), (1, 1, 1)), ((64, 12), (1, 1, 1)),
                      ((64, 4), (1, 1, 1)), ((16, 240), (4, 4)), ((16, 64), (4, 4)), ((32, 1024), (4, 8)),
                      ((48, 240), (4, 4, 4)), ((64, 496), (4, 8)), ((17 * 16, 48), (4, 8))):
        for ch in (1, 3):
            for k, kind in enumerate(G.KINDS):
                out.append((T, G.Case(f"p{r}x{c}_{kind}_{ch}ch", G.kind_image(r * c + k + ch, kind, r, c, ch), 10.0,
                                      levels=len(T))))
    for ch in (1, 3):
        for case in G.border_edges(32, 48, ch):
            out.append(((4, 8), G.Case(case.name, case.img, case.weak, levels=2)))
    for r, c, T in ((32, 48, (4, 8)), (32, 40, (1, 1, 1)), (16, 240, (4, 4))):
        for case in G.border_hole_masks(r, c, 9):
            out.append((T, G.Case(case.name, case.img, case.weak, case.mask, len(T))))
    for case in G.colour_ties(32, 48, 5):
        out.append(((4, 8), G.Case(case.name, case.img, case.weak, levels=2)))
    return out


PYR_CASES = _pyramid_cases()


@pytest.mark.parametrize("mode,hs", MODES)
def test_build_pyramid_equals_spec(ctx_factory, mode, hs):
    ctxs = {}
    for T, case in PYR_CASES:
        key = (T, case.weak)
        if key not in ctxs:
            ctxs[key] = ctx_factory(T=T, weak=case.weak)
            ctxs[key].set_quantize_mode(mode, hs)
        ctx = ctxs[key]
        ctx.build_pyramid(case.img, case.mask)
        for l, lv in enumerate(S.build(case.img, T, case.weak, case.mask)):
            assert ctx.level_dims(l) == lv.src.shape[:2], (case.name, T, l)
            _eq(ctx.get_quantized(l), lv.quantized, (case.name, T, l, mode, hs))


def test_build_pyramid_refuses_unfit_geometry(ctx_factory):
    """just below the smallest accepted sizes: rows*cols % 16 (computeResponseMaps) and multiples of T (linearize)"""
    for T, shape in (((1,), (3, 5)), ((1,), (1, 15)), ((1,), (15, 1)), ((4,), (4, 3)), ((4,), (3, 4)), ((1, 1), (2, 8))):
        ctx = ctx_factory(T=T)
        with pytest.raises(capi.SbmError):
            ctx.build_pyramid(np.zeros(shape, np.uint8))


@pytest.mark.parametrize("mode", ["tile", "stream", "auto"])
def test_match_batch_device_on_spec_maps(ctx_factory, mode):
    """a batch of mixed content through sbm_match_batch_device: each frame's match list equals the oracle's matchClass
    run on the SPEC's quantized maps, so the batched gradient kernels are held to the spec"""
    import torch

    from oracle import oracle as O

    rows, cols, B, thr = 192, 256, 8, 60.0
    dev = torch.device("cuda", 0)
    frames = [G.kind_image(700 + f, G.KINDS[f % 7], rows, cols, 3) for f in range(B)]
    frames[0] = synth.scene_bgr(7, rows, cols, n_shapes=30)  # the templates are cut from this frame's maps
    frames[4] = np.roll(frames[0], 8, axis=1)
    mask = np.full((rows, cols), 255, np.uint8)
    mask[:, :3] = 0
    mask[rows - 5 :, 40:90] = 0
    spec_maps = {m: [[lv.quantized for lv in S.build(f, (4, 8), 30.0, mask if m else None)] for f in frames]
                 for m in (False, True)}
    ts, got = synth.templates_from_maps(spec_maps[False][0], [40, 20], 32, 6, 3)
    assert got == [40, 20]
    ctx = ctx_factory(T=(4, 8), weak=30.0)
    ctx.upload_templates(ts)
    ctx.set_quantize_mode(mode)
    cap, rec = 4096, MATCH_DTYPE.itemsize
    d_imgs = torch.from_numpy(np.stack(frames)).to(dev)
    d_mask = torch.from_numpy(mask).to(dev)
    d_out = torch.zeros(B * cap * rec, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(B * 2, dtype=torch.int32, device=dev)
    key = lambda r: sorted(np.ascontiguousarray(r, MATCH_DTYPE).tolist())  # noqa: E731
    total = 0
    for use_mask in (False, True):
        d_cnt.fill_(-1)
        torch.cuda.synchronize()
        ctx.match_batch_device(d_imgs.data_ptr(), frames[0].size, B, rows, cols, cols * 3, 3, thr, d_out.data_ptr(), cap,
                               d_cnt.data_ptr(), d_mask=d_mask.data_ptr() if use_mask else 0)
        torch.cuda.synchronize()
        cnt = d_cnt.cpu().numpy().reshape(-1, 2)
        out = d_out.cpu().numpy().reshape(B, cap * rec)
        for f in range(B):
            p = O.Pyramid.from_quantized(spec_maps[use_mask][f], [4, 8])
            want = p.match(ts.levels, ts.features, ts.class_idx, ts.template_id, thr)
            p.free()
            assert cnt[f, 1] == 0 and cnt[f, 0] == len(want), (use_mask, f, cnt[f].tolist(), len(want))
            assert key(out[f].view(MATCH_DTYPE)[: cnt[f, 0]]) == key(want), (use_mask, f)
            total += len(want)
    assert total > 0
