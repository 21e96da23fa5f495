"""The inputs of tests/test_gpu_coarse_forms.py do what they claim, checked without a GPU: the numpy reference of
coarse_form_cases.py equals the oracle's one-level match bit for bit at every (geometry, group, threshold); every feature count
and position count the coarse kernels branch on is present; every median / percentile threshold has positions exactly on it,
above it and below it; 100 yields nothing, 0 neither nothing nor everything, 90 the planted templates' home positions.

These are conditions on the generator: where a seed does not meet one, the seed changes."""
import os

import numpy as np
import pytest

import coarse_form_cases as CF

NT = min(16, os.cpu_count() or 1)


@pytest.fixture(scope="module", params=list(CF.GEOS))
def w(request, oracle):
    return CF.world(request.param)


def test_numpy_reference_equals_the_oracle_at_every_case(w, oracle):
    pyr = oracle.Pyramid.from_quantized([w.q], [w.T])
    n = 0
    for g in CF.GROUPS:
        ts = w.ts.subset(w.groups[g])
        for thr, name, _, _ in w.thresholds[g]:
            want = CF.as_rows(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, thr, n_threads=NT))
            assert CF.first_difference(want, w.reference(w.groups[g], thr)) is None, (w.geo, g, name, thr)
            n += 1
    pyr.free()
    assert n == len(w.cases()) == 5 * 9


def test_every_feature_count_and_position_count_is_present(w):
    kinds = [s[3] for s in w.specs]
    counts = [int(w.nf[t]) for t, k in enumerate(kinds) if k == "count"]
    assert counts == CF.COUNTS == sorted(set(CF.COUNTS))
    for edge in (8, 16, 32, 52, 53, 63, 64, 65, 127, 128, 1023, 1024, 1056, 4095, 8191):  # batch, chunk, widening, P boundaries
        assert edge in counts
    assert (w.W, w.H) == {"T4": (68, 64), "T5": (68, 48)}[w.geo]
    npos = [int(w.npos[t]) for t, k in enumerate(kinds) if k == "npos"]
    assert npos == [n for n, _ in CF.NPOS[w.geo]]
    if w.geo == "T4":
        assert set(npos) == {2015, 2016, 2017, 4032, 4033, 1}
        boxes = {(int(w.npos[t]), (s[2] - 1) // 4 + 1, (s[1] - 1) // 4 + 1) for t, s in enumerate(w.specs) if s[3] == "npos"}
        assert boxes == {(2015, 35, 26), (2016, 35, 25), (2017, 35, 24), (4032, 5, 49), (4033, 5, 48), (1, 64, 68)}  # (npos, hf, wf)
    # the boxes are spread over small, middle and large feature counts
    nf_of = sorted(int(w.nf[t]) for t, k in enumerate(kinds) if k == "npos")
    assert nf_of[0] < 64 and any(128 <= v < 1024 for v in nf_of) and nf_of[-1] >= 1024
    # the count templates reach every work item: the last one-dword item (positions >= 4032 of T4) too
    assert int(w.npos.max()) > 2 * CF.CB_POS if w.geo == "T4" else int(w.npos.max()) == w.W * w.H
    tall = kinds.index("tall")
    assert w.npos[tall] <= 0 and len(w.raw[tall]) == 0
    assert len(w.reference([tall], 0.0)) == 0  # it contributes nothing
    out = kinds.index("outside")
    f = np.array(w.feats(out))
    outside = (f[:, 0] >= w.W * w.T) | (f[:, 1] >= w.H * w.T)
    assert outside.sum() == CF.OUTSIDE_OUT and (f[:, 0] >= w.W * w.T).any() and (f[:, 1] >= w.H * w.T).any()
    assert w.raw[out].max() <= 4 * (CF.OUTSIDE_NF - CF.OUTSIDE_OUT) and w.raw[out].max() > 0


def test_groups_hold_what_their_launch_form_needs(w):
    mx = {g: int(w.nf[w.groups[g]].max()) for g in CF.GROUPS}
    assert mx == {"le63": 63, "le127": 127, "mid": 1023, "big": 8191, "all": 8191}
    for g in ("mid", "big"):
        assert sorted(int(v) for v in w.nf[w.groups[g]] if v < 128) == list(CF.SMALL_IN_LARGE_GROUPS)
    assert min(w.nf[w.groups["mid"]][len(CF.SMALL_IN_LARGE_GROUPS):]) == 128 and min(w.nf[w.groups["big"]][len(CF.SMALL_IN_LARGE_GROUPS):]) == 1024
    # nothing can overflow: every position of every template fits the candidate list
    assert int(np.maximum(w.npos, 0).sum()) <= CF.MAX_CANDIDATES
    # the forms the host rule gives these groups in one process without knobs (a whole MI355X: 1024 SIMDs), and under each forced form
    P = {"le63": 7, "le127": 7, "mid": 10, "big": 13, "all": 13}
    for g in CF.GROUPS:
        assert CF.group_form(w, g, 1, 1024, {}) == (4, P[g], 0, 0)
        assert CF.group_form(w, g, 1, 1024, CF.FORMS["block"]) == (4, P[g], 0, 0)
        for dw in (1, 2):
            for wide in (0, 1):
                form = CF.FORMS["wave_dw%d_%s" % (dw, "wide" if wide else "narrow")]
                assert CF.group_form(w, g, 1, 1024, form) == (3, P[g], 1 if P[g] == 13 else wide, dw)


def test_thresholds_sit_on_scores(w):
    for g in CF.GROUPS:
        ths = w.thresholds[g]
        assert [t[1] for t in ths[:3]] == ["zero", "hundred", "ninety"] and len(ths) == 9
        picked = w.threshold_templates(g)
        assert w.nf[picked[0]] == min(w.nf[t] for t in w.groups[g] if w.npos[t] > 0) and w.nf[picked[2]] == w.nf[w.groups[g]].max()
        assert w.nf[picked[0]] <= w.nf[picked[1]] <= w.nf[picked[2]] and len(set(picked)) == 3
        for thr, name, t, raw in ths[3:]:
            thr32, nf = np.float32(thr), int(w.nf[t])
            assert float(thr32) == thr and CF.score_of(raw, nf) == thr32
            sc = CF.score_of(w.raw[t], nf)
            on = int((sc == thr32).sum())
            assert on >= 1 and on == int((w.raw[t] == raw).sum()), (w.geo, g, name)
            # ... which the strict comparison drops, while raw + 1 stays
            ref = w.reference([t], thr)
            assert len(ref) == int((w.raw[t] > raw).sum()) and (len(ref) == 0 or ref[:, 3].min() > raw)
            # A raw of 4 nf (every feature an exact hit) has nothing above it and a raw of 0 nothing below it, whatever the
            # seed: a one-feature template's scores are 0, 75 and 100 and a fifth of its positions score 100.  Everywhere else
            # the threshold has positions strictly above and below it.
            if raw < 4 * nf:
                assert (sc > thr32).any(), (w.geo, g, name)
            else:
                assert nf == 1 and thr == 100.0
            assert raw > 0 and (sc < thr32).any(), (w.geo, g, name)


def test_fixed_thresholds(w):
    for g in CF.GROUPS:
        idx = w.groups[g]
        total = int(np.maximum(w.npos[idx], 0).sum())
        assert len(w.reference(idx, 100.0)) == 0
        zero = w.reference(idx, 0.0)
        assert 0 < len(zero) < total
        assert len(zero) == sum(int((w.raw[t] > 0).sum()) for t in idx)  # rmin = 1: every position with a hit
        ninety = w.reference(idx, 90.0)
        planted = [t for t in idx if t in w.planted]
        assert planted, g
        off = w.T // 2 + (w.T % 2 - 1)
        for t in planted:  # the home position of every planted template of the group
            j = w.planted[t]
            home = ninety[(ninety[:, 5] == t) & (ninety[:, 0] == (j % w.W) * w.T + off) & (ninety[:, 1] == (j // w.W) * w.T + off)]
            assert len(home) == 1 and home[0, 3] > 0.9 * 4 * w.nf[t], (w.geo, g, t)
        # beyond them only what the reference says: templates of few features, or of many in a box of a few pixels, reach 90 by
        # chance -- no count template of 64 features or more does
        others = ninety[~np.isin(ninety[:, 5], planted)]
        by_chance = sorted(set(int(t) for t in others[:, 5]))
        assert all(w.nf[t] < 64 or w.specs[t][3] != "count" for t in by_chance), (w.geo, g, [int(w.nf[t]) for t in by_chance])
        assert len(ninety) < total // 20  # most positions, and with them most work items, die early


def test_batched_slice_and_two_level_inputs(oracle):
    w = CF.world("T4")
    frames, raws, thrs = CF.batch_slice()
    assert frames.shape == (3, 256, 272) and not frames[2].any()
    assert CF.batch_case_count() == 2 * 4 * 3
    for g in CF.BATCH_GROUPS:
        assert thrs[g][0] == 0.0 and thrs[g][3] == 0.0 and thrs[g][1] > 0 and thrs[g][2] > 0  # the all-zero frame's median score is 0
        for b in range(2):  # numpy on the frame's own level == the oracle's match of that frame, at the frame's own threshold
            pyr = oracle.Pyramid.build(frames[b], [4], 30.0)
            ts = w.ts.subset(w.groups[g])
            for thr in (0.0, thrs[g][1 + b]):
                want = CF.as_rows(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, thr, n_threads=NT))
                assert CF.first_difference(want, w.reference(w.groups[g], thr, raws[b])) is None, (g, b, thr)
                assert len(want) > 0 or thr > 0
            pyr.free()
        assert all(len(w.reference(w.groups[g], t, raws[2])) == 0 for t in thrs[g])
    for nf in CF.TWO_LEVEL:
        maps, ts = CF.two_level_inputs(nf)
        pyr = oracle.Pyramid.from_quantized(maps, [4, 8])
        assert len(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, 90.0, n_threads=NT)) > 0
        pyr.free()
        assert int(ts.levels["n_features"][0, 1]) == nf[1]
