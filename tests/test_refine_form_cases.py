"""The inputs of tests/test_gpu_refine_forms.py do what they claim, checked without a GPU: the numpy reference of
refine_form_cases.py equals the oracle's two-level match bit for bit at every (world, group, threshold); the saturated regions
saturate; every feature count is realised; every equality threshold has a candidate exactly on it; every patch corner is some
candidate's unique maximum; the candidates arrive at all 16 window columns and rows; the thin templates' features lie in their
classes; the ties tie; the clamps clamp at every border.

These are conditions on the generator: where a seed does not meet one, the seed changes."""
import os

import numpy as np
import pytest

import refine_form_cases as RF
from coarse_form_cases import as_rows, first_difference, score_of

NT = min(16, os.cpu_count() or 1)


@pytest.fixture(scope="module", params=list(RF.WORLDS))
def w(request, oracle):
    return RF.world(request.param)


def oracle_pyramid(oracle, w, img=None):
    if w.img is None:
        return oracle.Pyramid.from_quantized(w.maps, list(w.T))
    return oracle.Pyramid.build(w.img if img is None else img, list(w.T), RF.WEAK_I)


def kinds(w, *ks):
    return [t for t, s in enumerate(w.specs) if s["kind"] in ks]


def test_numpy_reference_equals_the_oracle_at_every_case(w, oracle):
    pyr = oracle_pyramid(oracle, w)
    n = 0
    for g in RF.GROUPS:
        ts = w.ts.subset(w.groups[g])
        for thr, name, _, _ in w.thresholds[g]:
            want = as_rows(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, thr, n_threads=NT))
            assert first_difference(want, w.reference(w.groups[g], thr)) is None, (w.name, g, name, thr)
            n += 1
    pyr.free()
    assert n == len(w.cases()) and n >= 6 * 5


def test_the_saturated_region_saturates(w):
    """every saturated and thin template has a candidate whose patch holds 4 nf in at least 200 of the 256 cells (M: in all of
    them, and 3 nf in all of them over the neighbour region): there the byte accumulators and the slot counters run full"""
    for t in kinds(w, "sat", "thin"):
        nf = int(w.nf[t])
        full = [int((c[4] == 4 * nf).sum()) for c in w.candidates(t, RF.HIGH)]
        assert full and max(full) >= (256 if w.img is None else 200), (w.name, t, nf, full)
        if w.img is None:
            near = [int((c[4] == 3 * nf).sum()) for c in w.candidates(t, RF.HIGH)]
            assert max(near) == 256, (t, nf)
            # the whole-patch tie resolves to cell (0, 0)
            rows = w.reference([t], RF.HIGH)
            windows = {((c[2] * w.T[0] + RF.offset_of(w.T[0])), (c[3] * w.T[0] + RF.offset_of(w.T[0]))) for c in w.candidates(t, RF.HIGH)
                       if (c[4] == 4 * nf).all()}
            assert windows <= {(int(r[0]), int(r[1])) for r in rows if r[3] == 4 * nf} and len(windows) >= 3


def test_every_count_is_realised(w):
    for kind in ("sat", "planted"):
        assert [int(w.nf[t]) for t in kinds(w, kind)] == RF.COUNTS
        assert [int(w.ts.levels[t, 0]["n_features"]) for t in kinds(w, kind)] == RF.COUNTS
    for edge in (8, 9, 16, 17, 32, 33, 64, 65, 252, 253, 1024, 2044, 2045, 8191):  # window tails, counter widths, the largest
        assert edge in RF.COUNTS
    assert [int(w.nf[t]) for t in kinds(w, "thin")] == RF.THIN_COUNTS * 3
    # every planted count template is found at the cell it was cut for (two in three have a share of their labels spoiled, so
    # that the world has scores below 100: those only score high there)
    for t in kinds(w, "planted"):
        cell, nf = w.specs[t]["cell"], int(w.nf[t])
        gx, gy = RF.window_of_home(w.p["p_home"], w.specs[t]["w"], w.specs[t]["h"], w.rows, w.cols, w.T)
        local = w.patch(t, gx, gy)
        if w.specs[t]["spoil"] == 0 or nf < 8:
            assert local[cell] == local.max() == 4 * nf, (w.name, nf, cell)
        else:
            assert 0.7 * 4 * nf <= local[cell] <= 4 * nf, (w.name, nf, cell)


def test_thin_templates_lie_in_their_classes(w):
    T0 = w.T[0]
    seen = []
    for t in kinds(w, "thin"):
        cls = set(((w.feats0[t][:, 0] // T0) & 15).tolist())
        assert cls == set(w.specs[t]["classes"]), (w.name, t)
        seen.append(sorted(cls))
    assert [5] in seen and [0, 15] in seen and [3, 7, 11, 15] in seen
    # ... while the other saturated templates of 64 features or more spread over all 16
    for t in kinds(w, "sat"):
        if w.nf[t] >= 128:
            assert len(set(((w.feats0[t][:, 0] // T0) & 15).tolist())) == 16


def test_equality_thresholds_sit_on_scores(w):
    for g in RF.GROUPS:
        ths = w.thresholds[g]
        assert [t[1] for t in ths[:2]] == ["low", "high"]
        eq = [t for t in ths if t[1].startswith("eq_")]
        assert len(eq) >= 1 and len(ths) == 2 + 3 * len(eq), (w.name, g)
        for i, (thr, name, t, raw) in enumerate(eq):
            nf = int(w.nf[t])
            thr32 = np.float32(thr)
            assert float(thr32) == thr and score_of(raw, nf) == thr32 and 0 < raw < 4 * nf
            below, above = ths[2 + 3 * i + 1][0], ths[2 + 3 * i + 2][0]
            assert np.float32(below) < thr32 < np.float32(above) and np.nextafter(np.float32(below), np.float32(200)) == thr32
            tid = int(w.ts.template_id[t])
            on = lambda rows: int(((rows[:, 5] == tid) & (rows[:, 3] == raw)).sum())  # noqa: E731
            at, lo, hi = w.reference([t], thr), w.reference([t], below), w.reference([t], above)
            # a candidate with exactly that score: kept at the threshold and one ulp below it, dropped one ulp above
            assert on(lo) >= on(at) >= 1 and on(hi) == 0, (w.name, g, name)
            assert (at[:, 2] == int(thr32.view(np.uint32))).sum() >= 1


def test_every_patch_corner_is_a_unique_maximum(w):
    got = set()
    for t in kinds(w, "corner"):
        gx, gy = RF.window_of_home(w.p["p_home"], w.specs[t]["w"], w.specs[t]["h"], w.rows, w.cols, w.T)
        local = w.patch(t, gx, gy)
        cell = w.specs[t]["cell"]
        assert local[cell] == local.max() and int((local == local.max()).sum()) == 1, (w.name, cell)
        rows = w.reference([t], RF.LOW)
        off = RF.offset_of(w.T[0])
        assert ((rows[:, 0] == (gx + cell[1]) * w.T[0] + off) & (rows[:, 1] == (gy + cell[0]) * w.T[0] + off) & (rows[:, 3] == local.max())).any()
        got.add(cell)
    assert got == set(RF.CORNERS)


def test_two_equal_maxima_take_the_first(oracle):
    w = RF.world("M")
    for name, (dr, dc) in (("tie_row", (0, 6)), ("tie_col", (6, 0))):
        t, = kinds(w, name)
        gx, gy = RF.window_of_home(w.p["p_home"], w.specs[t]["w"], w.specs[t]["h"], w.rows, w.cols, w.T)
        local, (r, c) = w.patch(t, gx, gy), RF.TIE_CELL[name]
        assert local[r, c] == local[r + dr, c + dc] == local.max() == 4 * RF.TIE_NF and int((local == local.max()).sum()) == 2
        rows = w.reference([t], RF.HIGH)
        off = RF.offset_of(w.T[0])
        assert [(int(v[0]), int(v[1])) for v in rows if v[3] == 4 * RF.TIE_NF] == [((gx + c) * w.T[0] + off, (gy + r) * w.T[0] + off)]


def test_all_16_window_columns_and_rows_occur(w):
    cols, rows = set(), set()
    for t in kinds(w, "sweep"):
        home = [c for c in w.candidates(t, RF.HIGH) if (c[2], c[3]) == w.specs[t]["window"]]
        assert home, (w.name, t)  # the clamped candidate of the sweep's home
        local = home[0][4]
        here = local[RF.SWEEP_CELL, RF.SWEEP_CELL]  # (the odd copies have a tenth of their labels spoiled)
        assert here == local.max() == 4 * RF.SWEEP_NF if kinds(w, "sweep").index(t) % 2 == 0 else 0.8 * 4 * RF.SWEEP_NF <= here < 4 * RF.SWEEP_NF
        cols.add(home[0][2] & 15)
        rows.add(home[0][3] & 15)
    assert cols == set(range(16)) and rows == set(range(16)), (w.name, sorted(cols), sorted(rows))
    # the candidate's pixel position takes every residue of the stride
    xs = {refine_x % w.T[0] for t in kinds(w, "sweep") for refine_x, _, gx, gy, _, _ in w.candidates(t, RF.HIGH) if (gx, gy) == w.specs[t]["window"]}
    assert xs == set(range(w.T[0]))
    # every template of the world fits its level (the ones that do not are test_gpu_match's)
    for s in w.specs:
        assert w.cols - s["w"] - 8 * w.T[0] >= 8 * w.T[0] and w.rows - s["h"] - 8 * w.T[0] >= 8 * w.T[0]


def test_features_outside_and_the_clamps(w):
    t, = kinds(w, "outside")
    f = w.feats0[t]
    out = (f[:, 0] >= w.cols) | (f[:, 1] >= w.rows)
    assert out.sum() == 5 and (f[:, 0] >= w.cols).sum() == 3 and (f[:, 1] >= w.rows).sum() == 3 and not out[:20].any() and not out[25:].any()
    gx, gy = RF.window_of_home(w.p["p_home"], w.specs[t]["w"], w.specs[t]["h"], w.rows, w.cols, w.T)
    assert w.patch(t, gx, gy).max() == 4 * (len(f) - 5)  # they count in nf and score nothing
    T0 = w.T[0]
    border = 8 * T0
    # left and top: the saturated templates' candidates; right and bottom: the clamp templates', at their own maxima
    xs = {(c[0], c[1]) for t in kinds(w, "sat")[:3] for c in w.candidates(t, RF.HIGH)}
    assert any(x == border for x, _ in xs) and any(y == border for _, y in xs)
    for kind, axis in (("clamp_right", 0), ("clamp_bottom", 1)):
        t, = kinds(w, kind)
        lim = (w.cols - w.specs[t]["w"] - border, w.rows - w.specs[t]["h"] - border)[axis]
        hit = [c for c in w.candidates(t, RF.HIGH) if c[axis] == lim]
        assert hit and lim >= border and any(c[4][w.specs[t]["cell"]] == c[4].max() == 4 * w.nf[t] for c in hit), (w.name, kind)


def test_the_host_rule_reaches_every_form():
    E = RF.expected_form
    assert E("M", "templates", True) == (4, 1, 0, 0, 0, 2048) and E("M", "templates", False) == (1, 16, 0, 0, 0, 512)
    assert E("M", "templates", None, depth=2) == (4, 1, 0, 0, 0, 512) and E("M", "templates", False, depth=2) == (1, 16, 0, 0, 0, 128)
    assert E("I48", "match", True) == (4, 1, 0, 0, 1, 2048) and E("I48", "match", False) == (3, 16, 0, 0, 0, 512)
    assert E("I88", "match", True) == E("I88", "match", False) == (3, 16, 0, 1, 0, 512)
    assert E("I17", "match", True) == (1, 16, 0, 0, 0, 512) and E("I17", "match", False, 4, order="list") == (2, 4, 2, 0, 0, 512)
    assert E("I48", "match", False, 8, order="list") == (3, 4, 2, 0, 0, 512) and E("I48", "match", True, 8, order="slots") == (4, 1, 0, 0, 1, 2048)
    K = RF.FORMS
    assert E("I48", "match", False, 8, K["waves16"]) == (3, 16, 0, 0, 0, 512) and E("I48", "match", False, 1, K["waves4"]) == (3, 4, 0, 0, 0, 512)
    assert E("I48", "match", None, 1, K["grid3"]) == (4, 1, 0, 0, 1, 3) and E("I48", "match", False, 1, K["grid3"]) == (3, 16, 0, 0, 0, 3)
    assert E("I48", "match", True, 1, K["strip_lm0"]) == (2, 16, 0, 0, 0, 512) and E("I48", "match", True, 1, K["full_lm1"]) == (1, 16, 0, 0, 0, 512)
    assert E("I48", "match", True, 1, K["lm_allty0"]) == (3, 16, 0, 0, 0, 512) and E("I48", "match", True, 1, K["sparse_strips0"]) == (4, 1, 0, 0, 0, 2048)
    assert E("I48", "match", None, 1, K["local_bits0"]) == (3, 16, 0, 0, 0, 512) and E("I48", "match", True, 1, K["local_bits0"]) == (4, 1, 0, 0, 1, 2048)
    # every kind, LW, order, t8 and sparse value is in some record that test_gpu_refine_forms.py asserts
    seen = {f[2:] for form in K for f in RF.expected_child_forms(form)}
    for i, vals in enumerate([{1, 2, 3, 4}, {1, 4, 16}, {0, 2}, {0, 1}, {0, 1}]):
        assert {f[i] for f in seen} == vals, (i, vals)


def test_batched_slices(oracle):
    for name, B in RF.BATCH.items():
        w = RF.world(name)
        frames, per, thrs = RF.batch_slice(name)
        idx = RF.batch_templates(w)
        assert frames.shape == (B, w.rows, w.cols) and not frames[B - 2].any() and frames[B - 1].any() and len(thrs) == 2
        assert len(idx) >= 40 and max(w.nf[idx]) <= 300
        ts = w.ts.subset(idx)
        for b in (0, 1, B - 2):  # numpy on the frame's own planes == the oracle's match of that frame
            pyr = oracle_pyramid(oracle, w, frames[b])
            for thr in thrs:
                want = as_rows(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, thr, n_threads=NT))
                assert first_difference(want, w.reference(idx, thr, per[b][0], per[b][1])) is None, (name, b, thr)
                assert (len(want) > 0) == (b != B - 2)
            pyr.free()


def test_three_level_threshold_sits_on_the_intermediate_score(oracle):
    maps, ts, thr, at, above, home = RF.three_level_case()
    nf1, nf0 = RF.THREE_NF[1], RF.THREE_NF[0]
    thr32 = np.float32(thr)
    # the threshold is a level-1 score (a raw of 40 features) below 100, and no score of 60 or of 20 features ...
    assert any(score_of(raw, nf1) == thr32 for raw in range(4 * (nf1 - RF.THREE_SPOILED), 4 * nf1))
    assert not any(score_of(raw, n) == thr32 for n in (nf0, RF.THREE_NF[2]) for raw in range(4 * n + 1))
    # ... the record's own score is far above it, and one ulp above the threshold the record is gone: dropped at level 1
    assert score_of(int(home[3]), nf0) > np.float32(95.0) and home[5] == 0
    present = lambda rows: bool((rows[:, [0, 1, 3, 5]] == home[[0, 1, 3, 5]]).all(axis=1).any())  # noqa: E731
    assert present(at) and not present(above) and len(at) == len(above) + 1
