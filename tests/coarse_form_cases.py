"""Deterministic inputs for the coarse pass at its feature-count and position-count edges, their plain numpy reference, and
the child worker of tests/test_gpu_coarse_forms.py (``python tests/coarse_form_cases.py --run FORM``).

One-level pyramids on one-hot maps installed with set_quantized: the coarse pass then emits the match list itself
(k_emit_coarse), so the list IS the score map above the threshold and a raw score that is off by one shows.

  geometries   T4: T = (4,), 256 x 272 -> W = 68, H = 64, 4352 positions (one-dword items 2016 + 2016 + 320, two-dword
               items 4032 + 320);  T5: T = (5,), 240 x 340 -> W = 68, H = 48, 3264 positions
  maps         synth.onehot_map at 110 per mille, four templates planted at multiples of T
  templates    one per feature count of COUNTS (batch, 64-offset chunk, widening and counter-plane boundaries), boxes that
               put npos on a work-item boundary (NPOS), one taller than the level (npos <= 0), one with features outside it
  groups       what one launch holds (P and the batch schedule follow the largest count): GROUPS
  thresholds   0, 100, 90 and, for the group's smallest, middle and largest template, the float32 score of its median and
               of its 90th-percentile raw: positions with exactly that raw have score == threshold and must be dropped

Reference: raw[j] = sum over the template's in-level features of LM[label][offset_f + j], j < npos, in int64, on the oracle's
response planes; score = (raw * 100.f) / (4 * nf) in float32; a record where score > thr."""
import functools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from shape_based_matching_amd import synth  # noqa: E402
from shape_based_matching_amd.templates import MATCH_DTYPE, from_pyramids  # noqa: E402

SEED = 5
DENSITY = 110
GEOS = {"T4": (4, 256, 272), "T5": (5, 240, 340)}  # T, rows, cols
COUNTS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 52, 53, 60, 61, 63, 64, 65, 127,
          128, 129, 191, 192, 193, 1023,
          1024, 1025, 1055, 1056, 1057, 4095, 8191]
BOXES = [(16, 16), (60, 44), (100, 100)]  # pixels; the count templates take them in turn
PLANTED = [63, 127, 193, 1056]  # counts of the templates written into the map (boxes of 100 x 100 pixels)
# (npos, features): boxes that put the position count on a work-item boundary (2016 positions per one-dword item, 4032 per
# two-dword item), on a single position and, for T5 (3264 positions), on the whole level and one less
NPOS = {"T4": [(2015, 12), (2016, 1100), (2017, 200), (4032, 24), (4033, 300), (1, 6), (2016, 90)],
        "T5": [(2015, 12), (2016, 1100), (2017, 200), (3264, 24), (3263, 300), (1, 6), (2016, 90)]}
TALL_NF, OUTSIDE_NF, OUTSIDE_OUT = 20, 50, 5
SMALL_IN_LARGE_GROUPS = (8, 33, 60)
GROUPS = ["le63", "le127", "mid", "big", "all"]

FORMS = {  # the process-wide knobs of each forced form (read once per process)
    "block": {"SBM_BITS_BLOCK": "1"},
    "wave_dw1_wide": {"SBM_BITS_BLOCK": "0", "SBM_BITS_DW": "1", "SBM_BITS_WIDE": "1"},
    "wave_dw1_narrow": {"SBM_BITS_BLOCK": "0", "SBM_BITS_DW": "1", "SBM_BITS_WIDE": "0"},
    "wave_dw2_wide": {"SBM_BITS_BLOCK": "0", "SBM_BITS_DW": "2", "SBM_BITS_WIDE": "1"},
    "wave_dw2_narrow": {"SBM_BITS_BLOCK": "0", "SBM_BITS_DW": "2", "SBM_BITS_WIDE": "0"},
}
KNOBS = ("SBM_BITS_BLOCK", "SBM_BITS_DW", "SBM_BITS_WIDE")
BATCH_FORMS = ("block", "wave_dw2_wide", "wave_dw2_narrow")  # the children that also run the batched slice
CB_POS = 2016  # positions per one-dword work item of the bit-plane kernels
MAX_CANDIDATES = 1 << 18  # >= templates x positions of either geometry: nothing overflows at threshold 0


def oracle_module():
    from oracle import oracle as O

    O.build()
    O.lib()
    return O


def box_for_npos(npos, T, W, H):
    """(width, height) in pixels of a template scored at exactly npos positions: npos = (H - hf) W + (W - wf) + 1"""
    hf, wf = H - (npos - 1) // W, W - (npos - 1) % W
    assert 1 <= hf <= H and 1 <= wf <= W and (H - hf) * W + (W - wf) + 1 == npos
    return wf * T - 1, hf * T - 1


def template_npos(width, height, T, W, H):
    wf, hf = (width - 1) // T + 1, (height - 1) // T + 1
    return (H - hf) * W + (W - wf) + 1


def score_of(raw, nf):
    """the reference's expression, in float32"""
    return (np.asarray(raw).astype(np.float32) * np.float32(100.0)) / np.float32(4 * nf)


def raw_scores(lm, T, W, H, rows, cols, width, height, feats):
    """int64 raw score of every position j < npos of one template on the response planes lm [8][stride]"""
    npos = template_npos(width, height, T, W, H)
    if npos <= 0:
        return np.zeros(0, np.int64)
    raw = np.zeros(npos, np.int64)
    for x, y, label in feats:
        if x < 0 or y < 0 or x >= cols or y >= rows:
            continue
        off = ((y % T) * T + x % T) * W * H + (y // T) * W + x // T
        assert off + npos <= lm.shape[1]
        raw += lm[label, off: off + npos]
    return raw


def as_rows(recs):
    """match records -> int64 rows (x, y, similarity bits, raw, class, template id), sorted: equal arrays <=> equal multisets"""
    r = np.ascontiguousarray(recs, MATCH_DTYPE)
    a = np.stack([r["x"].astype(np.int64), r["y"].astype(np.int64), r["similarity"].view(np.uint32).astype(np.int64),
                  r["raw"].astype(np.int64), r["class_idx"].astype(np.int64), r["template_id"].astype(np.int64)], axis=1)
    return a[np.lexsort(a.T[::-1])] if len(a) else a.reshape(0, 6)


def first_difference(want, got):
    """None, or (template id, (x, y), want row or None, got row or None) of the first record the sorted lists disagree on"""
    if want.shape == got.shape and np.array_equal(want, got):
        return None
    w, g = [tuple(r) for r in want.tolist()], [tuple(r) for r in got.tolist()]
    i = 0
    while i < len(w) and i < len(g) and w[i] == g[i]:
        i += 1
    wr, gr = (w[i] if i < len(w) else None), (g[i] if i < len(g) else None)
    if wr is not None and gr is not None:  # the smaller one is missing from the other list
        wr, gr = (wr, None) if wr < gr else (None, gr)
    r = wr if wr is not None else gr
    return int(r[5]), (int(r[0]), int(r[1])), wr, gr


class World:
    """one geometry: the map, the templates, every template's raw scores and the thresholds of every group"""

    def __init__(self, geo, O=None):
        O = O or oracle_module()
        self.geo = geo
        self.T, self.rows, self.cols = GEOS[geo]
        T, rows, cols = self.T, self.rows, self.cols
        self.W, self.H = cols // T, rows // T
        W, H = self.W, self.H
        rs = np.random.RandomState([SEED, T])
        q = synth.onehot_map(rs, rows, cols, DENSITY)
        specs = []  # (nf, width, height, kind)
        for i, nf in enumerate(COUNTS):
            specs.append((nf,) + ((100, 100) if nf in PLANTED else BOXES[i % 3]) + ("count",))
        for npos, nf in NPOS[geo]:
            specs.append((nf,) + box_for_npos(npos, T, W, H) + ("npos",))
        specs.append((TALL_NF, 40, rows + T, "tall"))
        specs.append((OUTSIDE_NF, 60, 44, "outside"))
        pyramids, self.planted = [], {}
        spots = [(2 * T, 2 * T), (2 * T, cols // 2 // T * T), (rows // 2 // T * T, 2 * T), (rows // 2 // T * T, cols // 2 // T * T)]
        for t, (nf, w, h, kind) in enumerate(specs):
            f = np.stack([rs.randint(0, w, nf), rs.randint(0, min(h, rows), nf), rs.randint(0, 8, nf)], axis=1)
            if kind == "outside":  # a few features right of and below the level: the coarse pass reads the zero tail for them
                f[:OUTSIDE_OUT, 0] = cols + np.arange(OUTSIDE_OUT)
                f[1:OUTSIDE_OUT:2, 0] = 7
                f[1:OUTSIDE_OUT:2, 1] = rows + np.arange(1, OUTSIDE_OUT, 2)
            if kind == "count" and nf in PLANTED:
                py, px = spots[len(self.planted)]
                q[py + f[:, 1], px + f[:, 0]] = (1 << f[:, 2]).astype(np.uint8)
                self.planted[t] = (py // T) * W + px // T
            pyramids.append([{"width": w, "height": h, "features": f}])
        q[0, :] = q[-1, :] = 0
        q[:, 0] = q[:, -1] = 0
        self.q = q
        self.specs = specs
        self.ts = from_pyramids(pyramids, "forms")
        self.nf = np.array([s[0] for s in specs])
        self.npos = np.array([template_npos(s[1], s[2], T, W, H) for s in specs])
        pyr = O.Pyramid.from_quantized([q], [T])
        self.lm = pyr.lm(0)
        pyr.free()
        self.raw = self.raws_on(self.lm)
        self.groups = self._groups()
        self.thresholds = {g: self._thresholds(g) for g in GROUPS}

    def feats(self, t):
        f = self.ts.feats_of(t, 0)
        return np.stack([f["x"], f["y"], f["label"]], axis=1).tolist()

    def raws_on(self, lm):
        return [raw_scores(lm, self.T, self.W, self.H, self.rows, self.cols, s[1], s[2], self.feats(t)) for t, s in enumerate(self.specs)]

    def _groups(self):
        nf, n = self.nf, len(self.specs)
        small = [t for t in range(n) if self.specs[t][3] == "count" and nf[t] in SMALL_IN_LARGE_GROUPS]
        return {"le63": [t for t in range(n) if nf[t] <= 63],
                "le127": [t for t in range(n) if nf[t] <= 127],
                "mid": small + [t for t in range(n) if 128 <= nf[t] <= 1023],
                "big": small + [t for t in range(n) if nf[t] >= 1024],
                "all": list(range(n))}

    def threshold_templates(self, g):
        """the smallest, the middle and the largest feature count among the group's templates that have a position"""
        idx = sorted((t for t in self.groups[g] if self.npos[t] > 0), key=lambda t: (self.nf[t], t))
        return [idx[0], idx[len(idx) // 2], idx[-1]]

    def _thresholds(self, g):
        """[(threshold, name, template or None, raw or None)]"""
        out = [(0.0, "zero", None, None), (100.0, "hundred", None, None), (90.0, "ninety", None, None)]
        for t in self.threshold_templates(g):
            s = np.sort(self.raw[t])
            for name, k in (("median", len(s) // 2), ("p90", (len(s) * 9) // 10)):
                out.append((float(score_of(s[k], self.nf[t])), "%s_of_%d" % (name, self.nf[t]), t, int(s[k])))
        return out

    def reference(self, templates, thr, raws=None):
        """the match list of `templates` above thr as sorted int64 rows (as_rows)"""
        raws = self.raw if raws is None else raws
        off = self.T // 2 + (self.T % 2 - 1)
        thr = np.float32(thr)
        rows = []
        for t in templates:
            raw = raws[t]
            sc = score_of(raw, self.nf[t])
            j = np.nonzero(sc > thr)[0]
            if len(j) == 0:
                continue
            rows.append(np.stack([(j % self.W) * self.T + off, (j // self.W) * self.T + off, sc[j].view(np.uint32).astype(np.int64), raw[j],
                                  np.full(len(j), int(self.ts.class_idx[t]), np.int64), np.full(len(j), int(self.ts.template_id[t]), np.int64)], axis=1))
        if not rows:
            return np.zeros((0, 6), np.int64)
        a = np.concatenate(rows).astype(np.int64)
        return a[np.lexsort(a.T[::-1])]

    def cases(self):
        return [(g, thr, name) for g in GROUPS for thr, name, _, _ in self.thresholds[g]]


@functools.lru_cache(maxsize=None)
def world(geo):
    return World(geo)


def expected_form(W, H, max_nf, max_npos, n_active, frames, n_simd, knobs):
    """the host rule of enqueue_coarse for a bit-plane launch, restated: (kind, P, wide, dw).  knobs: the SBM_BITS_* settings"""
    chunks = lambda per: max(1, (min(max(max_npos, 0), W * H) + per - 1) // per)  # noqa: E731
    dw = int(knobs["SBM_BITS_DW"]) if "SBM_BITS_DW" in knobs else (2 if max_nf < 1024 and chunks(CB_POS) * n_active * frames > n_simd * 8 else 1)
    items = chunks(dw * CB_POS) * n_active * frames
    block = int(knobs["SBM_BITS_BLOCK"]) != 0 if "SBM_BITS_BLOCK" in knobs else items <= 2048
    P = 7 if max_nf < 128 else (10 if max_nf < 1024 else 13)
    if block:
        return (4, P, 0, 0)
    wide = P == 13 or (int(knobs["SBM_BITS_WIDE"]) != 0 if "SBM_BITS_WIDE" in knobs else max_nf >= 64)
    return (3, P, int(wide), dw)


def group_form(w, g, frames, n_simd, knobs):
    idx = w.groups[g]
    return expected_form(w.W, w.H, int(w.nf[idx].max()), int(w.npos[idx].max()), len(idx), frames, n_simd, knobs)


# ---- the batched slice: three gray frames of the T4 geometry through sbm_match_batch_device ------------------------------

BATCH_GROUPS = ("le127", "mid")


@functools.lru_cache(maxsize=None)
def batch_slice():
    """frames [3][256][272], per frame the raw scores of every T4 template on the oracle's level of that frame, and per group the
    thresholds: 0 and the score of the median raw of the group's largest template on each frame"""
    O = oracle_module()
    w = world("T4")
    rs = np.random.RandomState([SEED, 77])
    frames = np.stack([rs.randint(0, 256, (w.rows, w.cols)).astype(np.uint8), synth.scene_gray(SEED, w.rows, w.cols), np.zeros((w.rows, w.cols), np.uint8)])
    raws = []
    for f in frames:
        pyr = O.Pyramid.build(f, [w.T], 30.0)
        raws.append(w.raws_on(pyr.lm(0)))
        pyr.free()
    thrs = {}
    for g in BATCH_GROUPS:
        t = w.threshold_templates(g)[2]
        thrs[g] = [0.0] + [float(score_of(np.sort(r[t])[len(r[t]) // 2], w.nf[t])) for r in raws]
    return frames, raws, thrs


def run_batch_slice(ctx, knobs, n_simd, tag, fail):
    """every (group, threshold) of the slice on ctx (T4 templates uploaded): each frame's list against numpy; returns (cases, records)"""
    import torch

    w = world("T4")
    frames, raws, thrs = batch_slice()
    dev = torch.device("cuda", 0)
    B, cap, rec = len(frames), MAX_CANDIDATES, MATCH_DTYPE.itemsize
    d_img = torch.from_numpy(frames).to(dev)
    d_out = torch.zeros(B * cap * rec, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(B * 2, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    n_cases = n_recs = 0
    for g in BATCH_GROUPS:
        ctx.select_templates(w.groups[g])
        for thr in thrs[g]:
            torch.cuda.synchronize()
            ctx.match_batch_device(d_img.data_ptr(), frames[0].size, B, w.rows, w.cols, w.cols, 1, thr, d_out.data_ptr(), cap, d_cnt.data_ptr(),
                                   stream=st.cuda_stream)
            st.synchronize()
            form = ctx.coarse_form()
            want_form = group_form(w, g, B, n_simd, knobs)
            if form != want_form:
                fail((tag, "batch", g, thr, "coarse_form", None, want_form, form))
            cnt = d_cnt.cpu().numpy().reshape(B, 2)
            if cnt[:, 1].any() or (cnt[:, 0] > cap).any():
                fail((tag, "batch", g, thr, "overflow", None, 0, cnt.tolist()))
            out = d_out.cpu().numpy().view(MATCH_DTYPE).reshape(B, cap)
            for b in range(B):
                want, got = w.reference(w.groups[g], thr, raws[b]), as_rows(out[b, : cnt[b, 0]])
                d = first_difference(want, got)
                if d:
                    fail((tag, "batch frame %d" % b, g, thr) + d)
                n_cases += 1
                n_recs += len(want)
    return n_cases, n_recs


def batch_case_count():
    return sum(len(t) for t in batch_slice()[2].values()) * 3


# ---- one two-level case per feature-count pair: cand_fill_next and the refinement behind a forced form --------------------

TWO_LEVEL = [(63, 31), (260, 130)]


def two_level_inputs(nf):
    return synth.stage_b(23, 512, 512, (4, 8), 24, list(nf), plant_every=6)


# ---- the worker ----------------------------------------------------------------------------------------------------------

def run_form(form):
    """one forced form in this (fresh) process: every case of both geometries in mode "bits", the batched slice where the
    form has one, the two-level cases; prints one JSON line of counts, or raises SystemExit with the first difference"""
    knobs = FORMS[form]
    for k in KNOBS:  # the knobs are read when the library first looks at them: set before it is loaded
        if k in knobs:
            os.environ[k] = knobs[k]
        else:
            os.environ.pop(k, None)
    t0 = time.time()
    from shape_based_matching_amd import capi

    O = oracle_module()

    def fail(what):
        print("DIFFERENCE " + json.dumps([str(v) for v in what]))
        raise SystemExit(3)

    import torch

    n_simd = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    counts = {"form": form, "cases": 0, "records": 0, "batch_cases": 0, "batch_records": 0, "two_level": 0, "forms": []}
    seen = set()
    for geo in GEOS:
        w = world(geo)
        ctx = capi.Context(T=(w.T,), weak_threshold=30.0, device_id=0, max_candidates=MAX_CANDIDATES)
        ctx.upload_templates(w.ts)
        ctx.set_quantized(0, w.q)
        ctx.set_coarse_mode("bits")
        for g in GROUPS:
            ctx.select_templates(w.groups[g])
            want_form = group_form(w, g, 1, n_simd, knobs)
            for thr, name, _, _ in w.thresholds[g]:
                got = as_rows(ctx.match_templates(thr))
                form_ran = ctx.coarse_form()
                if form_ran != want_form:
                    fail((form, geo, g, thr, "coarse_form", None, want_form, form_ran))
                want = w.reference(w.groups[g], thr)
                d = first_difference(want, got)
                if d:
                    fail((form, geo, g, thr) + d)
                counts["cases"] += 1
                counts["records"] += len(want)
            seen.add(want_form)
        if geo == "T4" and form in BATCH_FORMS:
            ctx.set_coarse_mode("auto")
            counts["batch_cases"], counts["batch_records"] = run_batch_slice(ctx, knobs, n_simd, form, fail)
        ctx.close()
    for nf in TWO_LEVEL:
        maps, ts = two_level_inputs(nf)
        ctx = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0, max_candidates=1 << 20)
        ctx.upload_templates(ts)
        for l in range(2):
            ctx.set_quantized(l, maps[l])
        ctx.set_coarse_mode("bits")
        got = as_rows(ctx.match_templates(90.0))
        form_ran = ctx.coarse_form()
        want_form = expected_form(512 // 16, 512 // 16, nf[1], template_npos(130, 130, 8, 32, 32), ts.n_templates, 1, n_simd, knobs)
        if form_ran != want_form:
            fail((form, "two-level", nf, 90.0, "coarse_form", None, want_form, form_ran))
        pyr = O.Pyramid.from_quantized(maps, [4, 8])
        want = as_rows(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, 90.0, n_threads=min(16, os.cpu_count() or 1)))
        pyr.free()
        if len(want) == 0:
            fail((form, "two-level", nf, 90.0, "empty reference", None, None, None))
        d = first_difference(want, got)
        if d:
            fail((form, "two-level", nf, 90.0) + d)
        seen.add(want_form)
        counts["two_level"] += 1
        ctx.close()
    counts["forms"] = sorted(seen)
    counts["seconds"] = round(time.time() - t0, 2)
    print("COUNTS " + json.dumps(counts))


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--run" or sys.argv[2] not in FORMS:
        raise SystemExit("usage: coarse_form_cases.py --run {%s}" % "|".join(FORMS))
    run_form(sys.argv[2])
