"""CPU: the gradient half's third restatement (tests/gradient_spec.py, numpy from line2Dup.cpp:218-450 and OpenCV's
documented semantics) against the C oracle, bit for bit; the mutation checks that show the case set reaches every rule
a misreading would change; and the fused-multiply-add question of OpenCV's AVX2 `phase`."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import gradient_cases as G
import gradient_spec as S
from conftest import ROOT
from test_oracle_pins import _case1_training_input

CASES = G.edge_cases()


def oracle_resize_nearest(O, m: np.ndarray, rows: int, cols: int) -> np.ndarray:
    L = O.lib()
    L.sbo_resize_nearest_u8.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.sbo_resize_nearest_u8.restype = None
    m = np.ascontiguousarray(m, np.uint8)
    out = np.empty((rows, cols), np.uint8)
    L.sbo_resize_nearest_u8(m.ctypes.data, m.shape[0], m.shape[1], out.ctypes.data, rows, cols)
    return out


def oracle_levels(O, case: G.Case):
    """the oracle's primitives chained as ColorGradientPyramid does: (src, mask, magnitude, quantized, angle) per level"""
    src, m, out = np.ascontiguousarray(case.img), case.mask, []
    for l in range(case.levels):
        if l > 0:
            src = O.pyrdown(src)
            if m is not None:
                m = oracle_resize_nearest(O, m, src.shape[0], src.shape[1])
        mag, q, ang = O.quantized_orientations(src, case.weak)
        if m is not None:
            q = np.where(m != 0, q, 0).astype(np.uint8)
        out.append((src, m, mag, q, ang))
    return out


def same_level(a: S.Level, b: S.Level) -> bool:
    return (a.src.shape == b.src.shape and np.array_equal(a.src, b.src) and np.array_equal(a.magnitude, b.magnitude)
            and np.array_equal(a.angle.view(np.uint32), b.angle.view(np.uint32)) and np.array_equal(a.quantized, b.quantized))


def spec_levels(case: G.Case, spec: S.Spec = S.SPEC):
    return S.build(case.img, [4] * case.levels, case.weak, case.mask, spec)


def first_difference(got, want, what):
    if got.shape != want.shape:
        return f"{what}: shape {got.shape} != {want.shape}"
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    bad = np.argwhere(got != want)
    return None if len(bad) == 0 else f"{what}: {len(bad)} differ, first {bad[:4].tolist()}"


# ---- spec == oracle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_spec_equals_oracle(oracle, case):
    mine = spec_levels(case)
    theirs = oracle_levels(oracle, case)
    assert len(mine) == case.levels
    for l, (lv, (src, m, mag, q, ang)) in enumerate(zip(mine, theirs)):
        for what, a, b in (("src", lv.src, src), ("magnitude", lv.magnitude, mag), ("angle", lv.angle, ang),
                           ("quantized", lv.quantized, q)):
            d = first_difference(a, b, what)
            assert d is None, (case.name, l, d)
        if m is not None:
            assert np.array_equal(lv.mask, m), (case.name, l)


def _masked_frame():
    m = np.pad(np.full((58, 90), 255, np.uint8), 3)
    m[0, 20:40] = 255  # the selected region reaches the border row there
    return G.Case("masked64x96", G.kind_image(3, "rects", 64, 96, 3), 10.0, m, 3)


PYR_CASES = [c for c in CASES if c.shape[0] % 16 == 0 and c.shape[1] % 16 == 0 and c.shape[0] * c.shape[1] % 256 == 0]
PYR_CASES += [_masked_frame()]


@pytest.mark.parametrize("case", PYR_CASES, ids=[c.name for c in PYR_CASES])
def test_spec_equals_oracle_pyramid(oracle, case):
    """the oracle's own pyramid build (sbo_pyramid_build, mask included) where the geometry suits T = 4 at every level"""
    n = min(case.levels, 3)
    p = oracle.Pyramid.build(case.img, [4] * n, case.weak, mask=case.mask)
    try:
        for l, lv in enumerate(S.build(case.img, [4] * n, case.weak, case.mask)):
            assert np.array_equal(p.quantized(l), lv.quantized), (case.name, l)
    finally:
        p.free()


def test_case1_training_chain(oracle, case1):
    """the padded case1 training input (test.cpp:266-279, Detector(128, {4, 8}), weak 30): the spec's two levels equal
    the oracle's, whose addTemplate on the same input reproduces the reference's test_templ.yaml
    (test_oracle_pins::test_case1_*) -- so the spec is tied to the reference's recorded output"""
    padded, mask = _case1_training_input(case1)
    case = G.Case("case1_train", padded, 30.0, mask, 2)
    test_spec_equals_oracle(oracle, case)
    lv = spec_levels(case)
    assert [l.src.shape[:2] for l in lv] == [(470, 470), (235, 235)]
    assert all(np.count_nonzero(l.quantized) > 1000 for l in lv)


# ---- the primitives' own checks ------------------------------------------------------------------------------------
ALL_G = np.arange(-1020, 1021)


def test_fast_atan2_accuracy_bound():
    """every integer gradient pair with |g| <= 1020 is within OpenCV's documented ~0.3 degrees of atan2"""
    gx, gy = np.meshgrid(ALL_G, ALL_G)
    got = S.fast_atan2_deg(gy.astype(np.float32), gx.astype(np.float32)).astype(np.float64)
    want = np.degrees(np.arctan2(gy, gx)) % 360.0
    err = np.abs(got - want)
    err = np.minimum(err, 360.0 - err)
    err[(gx == 0) & (gy == 0)] = 0.0
    assert 0.009 < err.max() < 0.0096, err.max()  # measured: 0.00955 degrees, far inside the documented 0.3
    assert got.min() >= 0.0 and got.max() < 360.0


def test_orientation_bins_equal_oracle_exhaustive(oracle):
    gx, gy = np.meshgrid(ALL_G, ALL_G)
    want = oracle.orientation_bins(gx.astype(np.int16), gy.astype(np.int16))
    assert np.array_equal(S.orientation_bins16(gx, gy), want)


def test_convert_to_rounds_half_to_even():
    a = np.array([0.0, 11.25, 33.75, 56.25, 348.75, 359.99, 360.0, 22.5 * 2.5], np.float32)
    v = (a * S.SCALE16).astype(np.float32)
    got = S.convert_to_u8(a)
    assert got.tolist() == np.rint(v).astype(int).tolist()
    assert S.convert_to_u8(np.array([360.0], np.float32))[0] == 16  # & 7 -> 0 afterwards: label 0 again


@pytest.mark.parametrize("sw", [2, 3, 5, 7, 8191, 8192])
def test_resize_nearest_index_rule(oracle, sw):
    dw = sw // 2
    rule = S.nearest_index(dw, sw)
    assert np.array_equal(rule, (np.arange(dw) * sw) // dw)
    m = (np.arange(sw) % 251).astype(np.uint8)[None, :].repeat(2, 0)
    assert np.array_equal(oracle_resize_nearest(oracle, m, 1, dw), S.resize_nearest(m, 1, dw))


@pytest.mark.parametrize("rows,cols", [(51, 71), (97, 131), (33, 47)])
def test_mask_pyramid_on_odd_sizes(oracle, rows, cols):
    """three levels of the mask pyramid from an odd-sized mask, every level from the one before: the oracle's nearest
    resize, the spec's and train_batch_cases.nearest_mask (which the training tests feed the reference binary) agree"""
    import train_batch_cases as TC

    m = (np.random.RandomState(rows * cols).randint(0, 10, (rows, cols)) > 0).astype(np.uint8) * 255
    for _ in range(3):
        dr, dc = m.shape[0] // 2, m.shape[1] // 2
        want = S.resize_nearest(m, dr, dc)
        assert 0 < np.count_nonzero(want) < want.size
        assert np.array_equal(oracle_resize_nearest(oracle, m, dr, dc), want)
        assert np.array_equal(TC.nearest_mask(m), want)
        m = want


def test_resize_nearest_index_rule_all_widths():
    """min(floor(x * (1 / (dw / sw))), sw - 1) == floor(x * sw / dw) for every sw <= 8192 at dw = sw / 2: the spec may
    use either form"""
    for sw in range(2, 8193):
        dw = sw // 2
        x = np.arange(dw)
        ifx = 1.0 / (dw / sw)
        assert np.array_equal(np.minimum(np.floor(x * ifx).astype(np.int64), sw - 1), (x * sw) // dw), sw


def test_pyrdown_reflect101_tiny_sides(oracle):
    """borderInterpolate(BORDER_REFLECT_101) on 2- and 3-pixel sides reflects the whole side again (numpy pads the
    same way); a one-pixel-at-a-time pad would not"""
    rs = np.random.RandomState(2)
    for r, c in itertools.product((2, 3, 4, 5), (2, 3, 4, 5)):
        img = rs.randint(0, 256, (r, c)).astype(np.uint8)
        assert np.array_equal(S.pyrdown(img), oracle.pyrdown(img)), (r, c)


# ---- mutation checks -------------------------------------------------------------------------------------------------
def _differs(spec: S.Spec, case: G.Case) -> bool:
    a, b = spec_levels(case), spec_levels(case, spec)
    return len(a) != len(b) or not all(same_level(x, y) for x, y in zip(a, b))


MUTATIONS = {
    "gauss_reflect101": S.variant(gauss_border="reflect"),
    "pyrdown_replicate": S.variant(pyr_border="edge"),
    "pyrdown_ceil_size": S.variant(pyr_size_ceil=True),
    "tie_highest_channel": S.variant(tie_lowest_channel=False),
    "threshold_ge": S.variant(thr_strict=False),
    "ring_not_zeroed": S.variant(zero_ring=False),
    "threshold_square_f64": S.variant(thr_square_f32=False),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_case_set_tells_mutation_apart(name):
    spec = MUTATIONS[name]
    hits = [c.name for c in CASES if _differs(spec, c)]
    assert hits, f"no case distinguishes the misreading {name}: the case set never reaches that rule"


def test_vote_tie_rule_is_unreachable():
    """The `last maximum wins` misreading cannot be told apart by any input: 9 votes over 8 labels with a winner of
    >= 5 votes (:306) is a strict majority, so the maximum is unique whenever it is used.  Shown over every way of
    splitting 9 votes, and on the case set."""
    for cut in itertools.combinations(range(16), 7):  # stars and bars: every histogram of 9 votes over 8 labels
        h = np.diff((-1,) + cut + (16,)) - 1
        if h.max() >= 5:
            assert np.count_nonzero(h == h.max()) == 1
    spec = S.variant(vote_first_max=False)
    assert not any(_differs(spec, c) for c in CASES[::7])


# ---- the FMA question ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def atan_emu():
    d = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["make", "-s", "-C", d])
    L = C.CDLL(os.path.join(d, "libsbm_atan_emu.so"))
    L.sbm_emu_fast_atan2.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.sbm_emu_fast_atan2.restype = None

    def run(y, x, fused):
        y = np.ascontiguousarray(y, np.float32)
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty(y.shape, np.float32)
        L.sbm_emu_fast_atan2(y.ctypes.data, x.ctypes.data, y.size, int(fused), out.ctypes.data)
        return out

    return run


def fma_moved_pairs(atan_emu):
    gx, gy = np.meshgrid(ALL_G.astype(np.float32), ALL_G.astype(np.float32))
    plain, fused = atan_emu(gy, gx, False), atan_emu(gy, gx, True)
    return gx, gy, plain, fused


def test_fused_phase_moves_angles_but_no_bin(atan_emu, oracle):
    """OpenCV's AVX2 `phase` fuses the polynomial's multiply-adds.  Over all 2041^2 integer gradient pairs the fused
    float angle differs from the unfused one for 81,369 pairs, and the 16-bin index (convertTo(CV_8U, 16/360)) for none:
    the quantized maps do not depend on which dispatch the reference ran.  The float angle (angle_ori, the training
    path's theta) does; the project follows the unfused evaluation."""
    gx, gy, plain, fused = fma_moved_pairs(atan_emu)
    assert np.array_equal(plain.view(np.uint32), S.fast_atan2_deg(gy, gx).view(np.uint32))  # the C helper is the spec
    moved = plain.view(np.uint32) != fused.view(np.uint32)
    assert int(moved.sum()) == 81369
    assert np.array_equal(S.convert_to_u8(plain), S.convert_to_u8(fused))
    assert np.abs(plain.astype(np.float64) - fused.astype(np.float64)).max() < 1e-4


def test_oracle_float_angle_is_unfused(atan_emu, oracle):
    """the oracle's angle output follows the unfused evaluation on pixels where fusing would move it"""
    gx, gy, plain, fused = fma_moved_pairs(atan_emu)
    moved = plain.view(np.uint32) != fused.view(np.uint32)
    ys, xs = np.nonzero(moved)
    sel = np.random.RandomState(0).choice(len(ys), 4096, replace=False)
    for i in sel[:256]:
        y, x = float(gy[ys[i], xs[i]]), float(gx[ys[i], xs[i]])
        assert np.float32(oracle.fast_atan2_deg(y, x)).view(np.uint32) == plain[ys[i], xs[i]].view(np.uint32)
