"""The CPU oracle against the reference's own match half (rows a-4, a-6 .. a-10 of DESIGN.md section 2).

oracle/_ref/ref_match_{scalar,sse42,avx2} are the reference's line2Dup.cpp compiled on stand-in headers
(oracle/ref_cv/) with oracle/ref_match_driver.cpp appended, one binary per code path MIPP selects on x86 (build() makes
them by oracle/ref_match.mk where the reference tree exists).  Fed with the oracle's own quantized maps, they give the
reference's spread -> computeResponseMaps -> linearize linear memories, similarity / similarity_64 maps,
similarityLocal / similarityLocal_64 patches and matchClass lists, which must equal the oracle's bit for bit.  Each test
runs for every variant this CPU can execute.  The oracle is what the HIP kernels are held to (bit for bit) by the GPU
suite, and tests/test_gpu_reference_match.py also holds them to these binaries directly."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import ref_match as R
from ref_match_cases import edge_templates, onehot_with_holes, with_classes, zero_fill_similarity
from shape_based_matching_amd import synth
from shape_based_matching_amd.templates import TemplateSet

VARIANTS = R.runnable_variants()
COUNTS = {}  # variant -> compared quantity -> count, reported at the end of the module


def count(variant, what, n):
    COUNTS.setdefault(variant, {}).setdefault(what, 0)
    COUNTS[variant][what] += int(n)


@pytest.fixture(scope="module", autouse=True)
def report(request):
    yield
    tr = request.config.pluginmanager.getplugin("terminalreporter")
    for v in VARIANTS:
        line = f"reference match half [{v}]: " + ", ".join(f"{n} {k}" for k, n in sorted(COUNTS.get(v, {}).items()))
        if tr is not None:
            tr.write_line(line)
        else:
            print(line)


@pytest.fixture(scope="module", params=VARIANTS)
def variant(request):
    missing = R.missing_binaries([request.param])
    assert not missing, f"{missing} missing: run __graft_entry__.build() where the reference tree is present"
    return request.param


def test_the_variants_this_host_runs():
    """the scalar path always; the SIMD paths wherever the CPU has them (every x86-64 host this project builds on has
    SSE4.2; AVX2 is what the reference's -march=native selects on a current one)"""
    assert VARIANTS[0] == "scalar"
    assert not R.missing_binaries(VARIANTS), "run __graft_entry__.build() where the reference tree is present"


# ---- inputs -----------------------------------------------------------------------------------------------------
def _frames():
    c1 = np.load(os.path.join(GOLDEN, "case1_test_bgr.npz"))["bgr"]
    c2 = np.load(os.path.join(GOLDEN, "case2_test_bgr.npz"))["bgr"]
    return {
        "case1": synth.embed(c1, 640, 768, 40, 60),
        "case2": synth.embed(c2, c2.shape[0] // 32 * 32 + 32, c2.shape[1] // 32 * 32 + 32, 8, 8),
        "scene": synth.scene_bgr(21, 512, 704, n_shapes=200),
    }


@pytest.fixture(scope="module")
def frames():
    return _frames()


@pytest.fixture(scope="module")
def case1_set():
    return TemplateSet.load_npz(os.path.join(GOLDEN, "case1_templates.npz"))


# ---- linear memories --------------------------------------------------------------------------------------------
# (rows, cols, T): multiples of T, not of 16 or 64; some with rows * cols % 32 != 0, which the AVX2 path of
# computeResponseMaps refuses (CV_Assert((src.rows * src.cols) % mipp::N<uint8_t>() == 0))
LM_GEOMETRIES = [(36, 52, 4), (44, 60, 4), (100, 116, 4), (40, 88, 8), (24, 104, 8), (72, 136, 8), (20, 28, 4)]


@pytest.mark.parametrize("rows,cols,T", LM_GEOMETRIES)
def test_linear_memories_random_maps(oracle, variant, rows, cols, T):
    q = onehot_with_holes(np.random.RandomState(rows * cols + T), rows, cols)
    pyr = oracle.Pyramid.from_quantized([q], [T])
    with R.Reference([q], [T], [], variant) as ref:
        try:
            got = ref.lm()[0]
        except R.Refused as e:
            # the reference's own refusal is a result: only the AVX2 build refuses, only where rows * cols % 32 != 0
            assert variant == "avx2" and (rows * cols) % 32 != 0, str(e)
            assert "mipp::N<uint8_t>()" in str(e), str(e)
            count(variant, "refused geometries", 1)
            return
    assert (rows * cols) % (32 if variant == "avx2" else 16) == 0
    n = got.shape[1]
    want = pyr.lm(0)
    assert np.array_equal(want[:, :n], got)
    assert not want[:, n:].any(), "the oracle's zero tail"
    count(variant, "lm bytes", got.size)


@pytest.mark.parametrize("name,T", [("case1", (4, 8)), ("case2", (4, 8)), ("scene", (8, 4)), ("case1", (4, 8, 8))])
def test_linear_memories_of_frames(oracle, variant, frames, name, T):
    pyr = oracle.Pyramid.build(frames[name], list(T), 30.0)
    qs = [pyr.quantized(l) for l in range(len(T))]
    with R.Reference(qs, T, [], variant) as ref:
        got = ref.lm()
    for l, g in enumerate(got):
        assert np.array_equal(pyr.lm(l)[:, : g.shape[1]], g), (name, l)
        count(variant, "lm bytes", g.size)


# ---- similarity maps and local patches on edge templates -------------------------------------------------------
# single-level pyramids: the coarse map is the one of the given T, and every feature-count path runs on it
EDGE_FRAMES = [(96, 136, 4), (136, 152, 8)]  # W x H = 34 x 24 and 19 x 17 cells; rows * cols % 32 == 0


def _edge_input(rows, cols, T):
    rs = np.random.RandomState(rows + cols)
    q = onehot_with_holes(rs, rows, cols, density=0.4)
    ts, names = edge_templates([(rows, cols)], [T], seed=T)
    return q, ts, names


@pytest.mark.parametrize("rows,cols,T", EDGE_FRAMES)
def test_similarity_maps_on_edge_templates(oracle, variant, rows, cols, T):
    q, ts, names = _edge_input(rows, cols, T)
    pyr = oracle.Pyramid.from_quantized([q], [T])
    lm = pyr.lm(0)
    zero_fill_differs = []
    with R.Reference([q], [T], ts, variant) as ref:
        for t, name in enumerate(names):
            got, path = ref.similarity(0, t)
            nf = int(ts.levels[t, 0]["n_features"])
            assert path == (64 if nf < 64 else 16), name
            want = pyr.similarity(ts.levels[t, 0], ts.features, 0)
            assert np.array_equal(want, got), (name, np.argwhere(want != got)[:5])
            zf = zero_fill_similarity(lm, rows, cols, T, ts.feats_of(t, 0), int(ts.levels[t, 0]["width"]),
                                      int(ts.levels[t, 0]["height"]))
            if not np.array_equal(zf, got):
                zero_fill_differs.append(name)
            count(variant, "similarity positions", got.size)
    # the pin has teeth: reading on into the next linear-memory row changes these maps, so a model that
    # stops at the row end, as a misreading of the overrun would, cannot pass this comparison
    assert zero_fill_differs, "no edge template reaches past a linear-memory row: the overrun case is not exercised"
    assert "nf8191" in zero_fill_differs or "nf1021" in zero_fill_differs, zero_fill_differs


def _centres(rows, cols, T, width, height):
    """patch centres: matchClass's clamp of a few raw positions (x = min(max(x, 8T), max_x), which lands below the
    border when max_x < 8T, negative for templates as wide as the frame), plus unclamped corners"""
    border = 8 * T
    max_x, max_y = cols - width - border, rows - height - border
    out = {(min(max(x, border), max_x), min(max(y, border), max_y)) for x in (1, cols // 2 + 1, cols - 1)
           for y in (1, rows // 2 + 1, rows - 1)}
    out |= {(0, 0), (cols - 1, rows - 1), (T * 8 + 3, 5), (-T - 1, rows // 2), (cols // 3, -2 * T + 1)}
    return sorted(out)


@pytest.mark.parametrize("rows,cols,T", EDGE_FRAMES)
def test_similarity_local_patches_on_edge_templates(oracle, variant, rows, cols, T):
    q, ts, names = _edge_input(rows, cols, T)
    pyr = oracle.Pyramid.from_quantized([q], [T])
    below_border = 0
    with R.Reference([q], [T], ts, variant) as ref:
        for t, name in enumerate(names):
            lv = ts.levels[t, 0]
            for cx, cy in _centres(rows, cols, T, int(lv["width"]), int(lv["height"])):
                got, path = ref.similarity_local(0, 0, t, cx, cy)
                want = pyr.similarity_local(lv, ts.features, 0, cx, cy)
                assert np.array_equal(want, got), (name, cx, cy, np.argwhere(want != got)[:5])
                below_border += cx < 8 * T
                count(variant, "patch cells", got.size)
    assert below_border > 0


# ---- matchClass lists -------------------------------------------------------------------------------------------
def _compare_match(oracle, pyr, ts, qs, T, thresholds, variant, min_matches=1):
    """raw list as a multiset; the epilogue as distinct (x, y, similarity, class) tuples, and in order where the
    reference's sort key (similarity desc, template_id asc) has no ties"""
    seen = 0
    with R.Reference(qs, T, ts, variant) as ref:
        for thr in thresholds:
            raw, epi = ref.match(thr)
            want = pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, float(np.float32(thr)))
            assert R.match_key(raw) == R.match_key(want), (thr, len(raw), len(want))
            canon = oracle.canonicalize(want)
            assert R.epilogue_key(epi) == R.epilogue_key(canon), thr
            key = list(zip(-epi["similarity"].astype(np.float64), epi["template_id"].tolist()))
            assert key == sorted(key), "the reference's epilogue is sorted by (similarity desc, template_id asc)"
            uniq = {k for k in key if key.count(k) == 1} if len(key) < 3000 else set()
            ckey = list(zip(-canon["similarity"].astype(np.float64), canon["template_id"].tolist()))
            assert [k for k in key if k in uniq] == [k for k in ckey if k in uniq]
            count(variant, "matches", len(raw))
            seen += len(raw)
    assert seen >= min_matches
    return seen


def _attainable(raw_list, k=2):
    """thresholds equal to scores the list holds ((raw * 100.f) / (4 * nf) as float32): where '>' (coarse scan) and
    '<' (refinement filter) decide"""
    s = np.unique(raw_list["similarity"])
    return [float(s[0]), float(s[len(s) // 2])][:k] if len(s) else []


@pytest.mark.parametrize("shift", ["plain", "shifted", "tiled"])
def test_match_case1(oracle, variant, case1_set, shift):
    ts = R.dense_ids(case1_set.subset(range(0, 361, 3) if shift == "plain" else range(0, 361, 9)))
    img = np.load(os.path.join(GOLDEN, "case1_test_bgr.npz"))["bgr"]
    if shift == "plain":
        frame = synth.embed(img, 640, 768, 40, 60)
    elif shift == "shifted":
        frame = synth.embed(img, 512, 672, 3, 61)
    else:
        frame = np.tile(synth.embed(img[:, :320], 480, 320, 0, 0), (1, 3, 1))
    pyr = oracle.Pyramid.build(frame, [4, 8], 30.0)
    qs = [pyr.quantized(0), pyr.quantized(1)]
    thr = [50.0, 75.0, 90.0]
    with R.Reference(qs, [4, 8], ts, variant) as ref:
        thr += _attainable(ref.match(70.0)[0])
    _compare_match(oracle, pyr, ts, qs, [4, 8], thr, variant, min_matches=100)


def test_match_case2(oracle, variant, frames):
    ts = TemplateSet.load_npz(os.path.join(GOLDEN, "case2_templates.npz"))
    ts = R.dense_ids(ts.subset(range(0, ts.n_templates, max(1, ts.n_templates // 60))))
    pyr = oracle.Pyramid.build(frames["case2"], [4, 8], 30.0)
    qs = [pyr.quantized(0), pyr.quantized(1)]
    _compare_match(oracle, pyr, ts, qs, [4, 8], [60.0, 80.0, 90.0], variant, min_matches=10)


@pytest.mark.parametrize("T,nf,box", [((4, 8), [100, 40], 200), ((8, 4), [63, 64], 160), ((4, 8, 8), [160, 80, 40], 256),
                                      ((4, 4, 8), [1021, 125, 65], 320)])
def test_match_templates_cut_from_the_frame(oracle, variant, frames, T, nf, box):
    """templates cut out of the frame's own maps (each scores 100 where it was cut), 2- and 3-level pyramids with
    mixed T, dealt into three classes"""
    pyr = oracle.Pyramid.build(frames["scene"], list(T), 30.0)
    qs = [pyr.quantized(l) for l in range(len(T))]
    ts, _ = synth.templates_from_maps(qs, nf, box, 9, 3 + nf[0])
    ts = with_classes(ts, 3)
    n = _compare_match(oracle, pyr, ts, qs, T, [80.0, 95.0, 100.0], variant, min_matches=9)
    assert n > 0


@pytest.mark.parametrize("T", [(4, 8), (8, 4)])
def test_match_edge_templates_and_thresholds_at_or_below_zero(oracle, variant, T):
    """the edge templates in a 2-level pyramid of random maps: thresholds <= 0 make every coarse position a candidate
    (also where the patch holds no response and the refinement keeps best_c = best_r = -1), patch centres are clamped
    below the border for the templates as wide / high as the level, thresholds equal to attained scores"""
    rs = np.random.RandomState(sum(T))
    shapes = [(128, 176), (64, 88)]
    qs = [onehot_with_holes(rs, r, c, density=0.3) for r, c in shapes]
    ts, names = edge_templates(shapes, list(T), seed=11)
    ts = with_classes(ts.subset([i for i, n in enumerate(names) if n not in ("nf8191", "nf1020", "nf1021")]), 2)
    pyr = oracle.Pyramid.from_quantized(qs, list(T))
    thr = [-1.0, 0.0, 10.0, 30.0]
    with R.Reference(qs, list(T), ts, variant) as ref:
        thr += _attainable(ref.match(20.0)[0])
    _compare_match(oracle, pyr, ts, qs, list(T), thr, variant, min_matches=1000)


def test_variants_agree_with_each_other(variant, frames, case1_set):
    """every variant gives the scalar build's linear memories and the same raw list in the same (serial) order"""
    from oracle import oracle as O

    pyr = O.Pyramid.build(frames["case1"], [4, 8], 30.0)
    qs = [pyr.quantized(0), pyr.quantized(1)]
    ts = R.dense_ids(case1_set.subset(range(0, 361, 6)))
    outs = {}
    for v in ("scalar", variant):
        with R.Reference(qs, [4, 8], ts, v) as ref:
            outs[v] = (ref.lm(), ref.match(60.0))
    (lm_a, (raw_a, epi_a)), (lm_b, (raw_b, epi_b)) = outs["scalar"], outs[variant]
    assert all(np.array_equal(a, b) for a, b in zip(lm_a, lm_b))
    assert raw_a.tobytes() == raw_b.tobytes()
    assert R.epilogue_key(epi_a) == R.epilogue_key(epi_b)


# ---- the recorded reference outputs -----------------------------------------------------------------------------
def test_binary_reproduces_the_recorded_golden(variant):
    """tests/golden/ref_match_case1.npz was written by tools/make_fixtures.py --ref from the AVX2 build; the build here
    (any variant) must still give it"""
    import hashlib

    z = np.load(os.path.join(GOLDEN, "ref_match_case1.npz"))
    qs = [z["q0"], z["q1"]]
    ts = R.dense_ids(TemplateSet.load_npz(os.path.join(GOLDEN, "case1_templates.npz")).subset(z["template_index"]))
    with R.Reference(qs, [4, 8], ts, variant) as ref:
        lm = ref.lm()
        assert hashlib.sha256(lm[int(z["lm_level"])].tobytes()).hexdigest() == str(z["lm_sha256"])
        for k, thr in enumerate(z["thresholds"].tolist()):
            raw, epi = ref.match(thr)
            assert raw.tobytes() == z[f"raw{k}"].tobytes(), thr
            assert R.epilogue_key(epi) == R.epilogue_key(z[f"epi{k}"]), thr
            count(variant, "matches", len(raw))
