"""The CPU oracle's training half against the reference's own.

oracle/_ref/ref_train is the reference's line2Dup.cpp compiled on stand-in headers (oracle/ref_cv/) with
oracle/ref_train_driver.cpp appended (build() makes it by oracle/ref_train.mk where the reference tree exists): its
ColorGradientPyramid::extractTemplate per level -- the magnitude_valid scan, std::stable_sort, selectScatteredFeatures --
and cropTemplates, in the order of Detector::addTemplate's loop.  Fed with the oracle's own gradient planes of the oracle's
pyramid images, and with the mask pyramid made by train_batch_cases.nearest_mask, its templates must equal
oracle.add_template's bit for bit: level records, features, theta as bits, and on failure the failing level.  The inputs
are those the device tests (tests/test_gpu_train_batch.py) hold the HIP training kernels to the oracle on, and plateaus
beyond them.  tests/golden/ref_train_cases.npz, recorded from the binary, holds the oracle to the reference even where
oracle/_ref could not be built."""
import os

import numpy as np
import pytest

import train_batch_cases as TC
from conftest import GOLDEN
from oracle import ref_train as RT


def test_the_binary_this_host_runs():
    """one variant (the training half uses no MIPP); it must exist wherever this suite runs next to a built tree"""
    assert not RT.missing_binaries(), "run __graft_entry__.build() where the reference tree is present"


@pytest.fixture(scope="module")
def ref_train():
    missing = RT.missing_binaries()
    assert not missing, f"{missing} missing: run __graft_entry__.build() where the reference tree is present"
    return RT


def same(ref_result, oracle_result, oracle_failed_level):
    """the binary's result equals the oracle's: the template, or the level at which addTemplate gives up"""
    if isinstance(ref_result, RT.Failed):
        return oracle_result is None and ref_result.level == oracle_failed_level
    return oracle_result is not None and TC.same_template(ref_result, oracle_result)


def n_candidates(oracle, img, mask, strong):
    """level-0 candidates: with far more features asked than there are candidates every candidate is kept (the first sweep,
    at distance 1, keeps every distinct position and does not reach num_features)"""
    res = oracle.add_template(img, mask, 1, 100000, TC.WEAK, strong)
    return 0 if res is None else int(res[0]["n_features"][0])


class Case:
    def __init__(self, name, make, n_levels, nfs, strong=TC.STRONG, min_pairs=0, min_cands=0, fails_at=None, counts=None):
        self.name, self.make, self.n_levels, self.nfs, self.strong = name, make, n_levels, nfs, strong
        self.min_pairs, self.min_cands, self.fails_at, self.counts = min_pairs, min_cands, fails_at, counts


def _cases():
    out = []
    R, N = TC.rectangle, TC.noise
    # ---- the inputs of tests/test_gpu_train_batch.py as it was: two levels, BGR
    for r, c in ((96, 96), (64, 64), (50, 70)):
        out.append(Case(f"rect{r}x{c}", lambda r=r, c=c: (R(r, c), None), 2, (16, 63, 128), min_pairs=100))
    out.append(Case("rect96-all_set", lambda: (R(96, 96), np.full((96, 96), 255, np.uint8)), 2, (63,), min_pairs=100, counts={63: (56, 20)}))
    out.append(Case("rect96-left_half", lambda: (R(96, 96), TC.left_half(96, 96)), 2, (63,), min_pairs=50, counts={63: (28, 9)}))
    out.append(Case("rect96-cut_edge", lambda: (R(96, 96), TC.cut_edge(96, 96)), 2, (63,), min_pairs=100, counts={63: (49, 17)}))
    out.append(Case("rect96-flipped-cut_edge", lambda: (np.ascontiguousarray(R(96, 96)[::-1]), TC.cut_edge(96, 96)), 2, (63,), min_pairs=100))
    out.append(Case("noise96-cut_edge", lambda: (N(96, 96, 3), TC.cut_edge(96, 96)), 2, (63,)))
    out.append(Case("noise64-5", lambda: (N(64, 64, 5), None), 2, (63,)))
    out.append(Case("rect64-cut_edge", lambda: (R(64, 64), TC.cut_edge(64, 64)), 2, (63,), min_pairs=50))
    out.append(Case("FAILING-rect64-left_half", lambda: (R(64, 64), TC.left_half(64, 64)), 2, (63,), fails_at=1))
    out.append(Case("FAILING-constant64", lambda: (TC.constant(64, 64), None), 2, (63,), fails_at=0))
    out.append(Case("FAILING-rect50x70-left_half", lambda: (R(50, 70), TC.left_half(50, 70)), 2, (63,), fails_at=1))
    out.append(Case("noise64-139-strong10", lambda: (N(64, 64, 139), None), 2, (16, 63, 100000), strong=10.0, min_cands=65))
    out.append(Case("noise256-strong10", lambda: (N(256, 256, 1), None), 2, (16, 63, 100000), strong=10.0, min_cands=513))
    out.append(Case("noise544-strong10", lambda: (N(544, 544, 1), None), 2, (2500, 4500, 100000), strong=10.0, min_cands=4096 + 65))
    # ---- the configurations tests/test_gpu_train_batch.py adds: one and three levels, gray, odd sizes, the widths at which
    #      the tie resolution's segment length changes
    want3 = {(48, 200, None): (74, 30, 13), (48, 200, "cut_edge"): (67, 26, 11), (48, 200, "left_half"): (36, 15, 6),
             (97, 131, None): (66, 26, 8), (97, 131, "cut_edge"): (60, 22, 5), (97, 131, "left_half"): None}
    for (r, c, mk), cnt in want3.items():
        mask = (lambda r=r, c=c, mk=mk: None if mk is None else getattr(TC, mk)(r, c))
        for L in (1, 2, 3):
            fails = 2 if (cnt is None and L == 3) else None
            counts = None if cnt is None else {63: cnt[:L]}
            out.append(Case(f"rect{r}x{c}-{mk}-L{L}", lambda r=r, c=c, mask=mask: (R(r, c), mask()), L, (63,), min_pairs=50, fails_at=fails, counts=counts))
            out.append(Case(f"gray-rect{r}x{c}-{mk}-L{L}", lambda r=r, c=c, mask=mask: (TC.gray(R(r, c)), mask()), L, (63,), min_pairs=50, fails_at=fails))
    out.append(Case("gray-noise131x97-strong10", lambda: (TC.gray(N(131, 97, 7)), None), 1, (63, 100000), strong=10.0, min_cands=65,
                    counts={63: (66,), 100000: (205,)}))
    rs = np.random.RandomState(51)
    odd = {(51, 71): (rs.rand(51, 71) > 0.05).astype(np.uint8) * 255, (97, 131): (rs.rand(97, 131) > 0.03).astype(np.uint8) * 255}
    out.append(Case("odd51x71-random_mask-L2", lambda: (R(51, 71), odd[(51, 71)]), 2, (63,), min_pairs=10))
    out.append(Case("odd97x131-random_mask-L3", lambda: (R(97, 131), odd[(97, 131)]), 3, (63,), min_pairs=10))
    out.append(Case("odd51x71-noise-left_half-L2", lambda: (N(51, 71, 11), TC.left_half(51, 71)), 2, (63,), strong=10.0, min_cands=5))
    for w, seed in TC.SEGMENT_SEEDS.items():
        out.append(Case(f"segment-rect-w{w}", lambda w=w: (R(TC.SEGMENT_ROWS, w), None), 1, (63,), min_pairs=50))
        out.append(Case(f"segment-noise-w{w}", lambda w=w, seed=seed: (N(TC.SEGMENT_ROWS, w, seed), None), 1, (16, 100000), strong=10.0, min_cands=5))
    # ---- plateaus the rectangles lack
    out.append(Case("checkerboard96-L1", lambda: (TC.checkerboard(96, 96), None), 1, (16, 63, 100000), min_pairs=100,
                    counts={16: (16,), 63: (90,), 100000: (264,)}))
    # its second level (blocks of 4 x 4 under the 7 x 7 Gaussian) has nothing above the threshold
    out.append(Case("FAILING-checkerboard96-L2", lambda: (TC.checkerboard(96, 96), None), 2, (16, 63), fails_at=1))
    out.append(Case("checkerboard50x70-L2", lambda: (TC.checkerboard(50, 70), None), 2, (16, 63, 100000), min_pairs=100))
    out.append(Case("checkerboard96-blocks16-L2", lambda: (TC.checkerboard(96, 96, 16), None), 2, (16, 63, 100000), min_pairs=100))
    out.append(Case("checkerboard50x70-cut_edge", lambda: (TC.checkerboard(50, 70), TC.cut_edge(50, 70)), 2, (63,), min_pairs=100))
    return out


CASES = _cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_add_template_equals_the_reference(oracle, ref_train, case):
    img, mask = case.make()
    mag = oracle.quantized_orientations(img, TC.WEAK)[0]
    if case.fails_at is None:  # not degenerate: ties for the scan to resolve, or candidates for the selection to thin
        if case.min_pairs:
            assert TC.s_pairs(mag, case.strong, mask) >= case.min_pairs
        assert n_candidates(oracle, img, mask, case.strong) >= max(case.min_cands, 5)
    planes = RT.planes_of(oracle, img, mask, case.n_levels, TC.WEAK, TC.nearest_mask)
    for nf in case.nfs:
        want = TC.want(oracle, img, mask, nf, case.strong, case.n_levels)
        failed = oracle.add_template_failing_level(img, mask, case.n_levels, nf, TC.WEAK, case.strong)
        assert (want is None) == (case.fails_at is not None) and failed == (-1 if case.fails_at is None else case.fails_at)
        if case.counts and nf in case.counts:
            assert TC.counts(want) == case.counts[nf]
        got = ref_train.run(planes, nf, case.strong)
        assert same(got, want, failed), (case.name, nf, got if isinstance(got, RT.Failed) else TC.counts(got))


def test_segment_noise_reaches_the_last_columns(oracle):
    """the seeds of train_batch_cases.SEGMENT_SEEDS put candidates into the last three scanned columns"""
    for w, seed in TC.SEGMENT_SEEDS.items():
        assert TC.candidates_in_last_columns(oracle, TC.noise(TC.SEGMENT_ROWS, w, seed), 10.0) >= 1, w


def test_reference_roi(oracle, ref_train, case1):
    img, mask = TC.fixture_roi(case1)
    want = TC.want(oracle, img, mask, 128)
    assert want is not None and min(TC.counts(want)) >= 64
    got = ref_train.run(RT.planes_of(oracle, img, mask, TC.N_LEVELS, TC.WEAK, TC.nearest_mask), 128, TC.STRONG)
    assert same(got, want, -1)


# ---- planes no image produces: small-integer magnitudes, ties everywhere ------------------------------------------
def _tie_planes(seed, rows, cols, values, step, masked):
    rs = np.random.RandomState(seed)
    mag = rs.randint(0, values, (rows, cols)).astype(np.float32) * np.float32(step)
    ang = (1 << rs.randint(0, 8, (rows, cols))).astype(np.uint8)
    ang[rs.rand(rows, cols) < 0.2] = 0  # maxima without a quantized orientation: they suppress, but are no candidates
    ori = (rs.rand(rows, cols) * 360.0).astype(np.float32)
    mask = (rs.rand(rows, cols) > 0.1).astype(np.uint8) * 255 if masked else None
    return mag, ang, ori, mask


TIE_PLANES = [(3, 33, 47, 3, 4000.0, True, 60.0), (4, 48, 80, 6, 1000.0, False, 30.0), (5, 64, 129, 2, 4000.0, True, 60.0),
              (6, 40, 64, 3, 4000.0, False, 60.0)]


@pytest.mark.parametrize("seed,rows,cols,values,step,masked,strong", TIE_PLANES)
def test_tie_fields_handed_in_as_planes(oracle, ref_train, seed, rows, cols, values, step, masked, strong):
    """the magnitude plane handed in directly: a handful of values, so that nearly every maximum is decided by the row-major
    order of the magnitude_valid scan, under a random 90 % mask that takes pixels out of the scan altogether"""
    p = _tie_planes(seed, rows, cols, values, step, masked)
    assert TC.s_pairs(p[0], strong, p[3]) >= 100
    for nf in (8, 63, 100000):
        want = oracle.add_template_planes([p], nf, strong)
        assert not isinstance(want, int) and TC.counts(want)[0] >= 5
        assert same(ref_train.run([p], nf, strong), want, -1), nf
    # two levels of such planes: the halving of num_features and cropTemplates over both
    q = _tie_planes(seed + 100, rows // 2, cols // 2, values, step, masked)
    want = oracle.add_template_planes([p, q], 63, strong)
    assert same(ref_train.run([p, q], 63, strong), want, -1)
    # a second level with nothing above the threshold: the failure is reported at level 1 by both
    empty = (np.zeros_like(q[0]), q[1], q[2], q[3])
    assert oracle.add_template_planes([p, empty], 63, strong) == 1
    assert ref_train.run([p, empty], 63, strong) == RT.Failed(1)


# ---- the recorded output of the binary ---------------------------------------------------------------------------------
def test_recorded_reference_output(oracle):
    """tests/golden/ref_train_cases.npz (tools/make_fixtures.py --ref-train): the oracle equals what the binary gave when it was
    recorded, and the binary, where this host has it, still gives it"""
    z = np.load(os.path.join(GOLDEN, "ref_train_cases.npz"))
    cases = TC.recorded_cases()
    assert sorted(k[: -len("_failed")] for k in z.files if k.endswith("_failed")) == sorted(cases)
    seen_failure = False
    for name, (img, mask) in cases.items():
        want = TC.want(oracle, img, mask, 63)
        failed = oracle.add_template_failing_level(img, mask, TC.N_LEVELS, 63, TC.WEAK, TC.STRONG)
        assert int(z[name + "_failed"]) == failed
        results = [want if want is not None else RT.Failed(failed)]
        if not RT.missing_binaries():
            results.append(RT.run(RT.planes_of(oracle, img, mask, TC.N_LEVELS, TC.WEAK, TC.nearest_mask), 63, TC.STRONG))
        for res in results:
            packed = TC.pack_recorded(name, res, RT)
            for k, v in packed.items():
                assert z[k].dtype == np.int32 and np.array_equal(z[k], v), (name, k)
        seen_failure = seen_failure or failed >= 0
    assert seen_failure and len(z["none_feats"]) == 76
