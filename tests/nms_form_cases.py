"""Cases for the epilogue + NMS stage (k_nms_frames, sbm_nms_kernels.h) at the edges of its four steps, shared by
tests/test_reference_nms.py (CPU: the reference's nms.hpp, py_nms, include/nms.hpp and the chunked walk agree on every
case, and every case reaches its edge) and tests/test_gpu_nms_forms.py (the kernel through sbm_nms_batch_device).

The kernel runs one workgroup of 1024 threads per frame: gather of every part's records (each list clamped to cap), bitonic
sort of record indices padded to a power of two (the index breaks exact ties), adjacent unique + score filter + top_k in
tiles of 1024 positions by ballot ranks, then the greedy walk in chunks of 64 candidates, the kept list sliced over the 16
waves.  Up to NMS_LDS_MAX = 2048 records a frame lives in LDS, beyond that in global scratch, which the HOST allocates by
n_parts * cap > 2048 while the KERNEL decides by the frame's own n.

A Case is one frame: the records each part's buffer holds, the {count, overflow} words, cap, the parameters, out_cap, the
flags word it must produce, the edge it exists for and a predicate, evaluated on the expectation side only, that the
case reaches that edge.  A Launch is a list of cases with the same cap, parts and parameters: the frames of one call.
The expectation of a case is always expected() -- epilogue() then test_nms.py::py_nms, the restatement the reference
binary pins; for the all-disjoint cases (every box kept, whatever the walk does) it is the epilogue list itself, and
test_reference_nms.py holds py_nms to that on the smallest of them.

Every buffer is filled with decoy records (similarity 127, above every case's) wherever a part holds no record of its own:
a kernel that reads past a count, or a part whose count word says -1, shows up at the head of the kept list."""
import collections
import functools
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from shape_based_matching_amd.templates import MATCH_DTYPE  # noqa: E402
from test_nms import py_nms  # noqa: E402

REC = MATCH_DTYPE.itemsize
NMS_LDS_MAX, NMS_TILE, NMS_CHUNK, NMS_WAVES = 2048, 1024, 64, 16  # sbm_nms_kernels.h
SENTINEL_BYTE = 0xA5


# ---- the expectation (moved here from test_gpu_nms_device.py, unchanged) ---------------------------------------------------

def epilogue(recs):
    """sort by (similarity desc, template_id, class_idx, y, x), then drop a record equal to its predecessor in
    (x, y, similarity, class_idx) (Match::operator== under std::unique)"""
    r = np.ascontiguousarray(recs, MATCH_DTYPE)
    order = sorted(range(len(r)), key=lambda i: (-float(r[i]["similarity"]), int(r[i]["template_id"]), int(r[i]["class_idx"]),
                                                  int(r[i]["y"]), int(r[i]["x"])))
    out = []
    for i in order:
        m = r[i]
        if out and (int(out[-1]["x"]), int(out[-1]["y"]), float(out[-1]["similarity"]), int(out[-1]["class_idx"])) == \
                (int(m["x"]), int(m["y"]), float(m["similarity"]), int(m["class_idx"])):
            continue
        out.append(m)
    return np.array(out, MATCH_DTYPE) if out else np.zeros(0, MATCH_DTYPE)


def boxes_of(e, sizes):
    return [[int(m["x"]), int(m["y"])] + list(sizes.get((int(m["class_idx"]), int(m["template_id"])), (0, 0))) for m in e]


def expected(recs, sizes, score_thr, nms_thr, eta=1.0, top_k=0):
    """sizes: {(class_idx, template_id): (w0, h0)}; an unknown label has an empty box"""
    e = epilogue(recs)
    boxes = [[int(m["x"]), int(m["y"])] + list(sizes.get((int(m["class_idx"]), int(m["template_id"])), (0, 0))) for m in e]
    keep = py_nms(boxes, [float(m["similarity"]) for m in e], score_thr, nms_thr, eta, top_k)
    return e[keep] if keep else np.zeros(0, MATCH_DTYPE)


def sizes_of(ts):
    return {(int(ts.class_idx[t]), int(ts.template_id[t])): (int(ts.levels[t, 0]["width"]), int(ts.levels[t, 0]["height"]))
            for t in range(ts.n_templates)}


def rows_of(a):
    return np.ascontiguousarray(a, MATCH_DTYPE).tolist()


def synth_list(rs, n, sizes, sims, spread):
    labels = list(sizes)
    r = np.zeros(n, MATCH_DTYPE)
    r["x"] = rs.randint(0, spread, n)
    r["y"] = rs.randint(0, spread, n)
    r["similarity"] = rs.choice(sims, n)  # ties
    lab = [labels[i] for i in rs.randint(0, len(labels), n)]
    r["class_idx"] = [l[0] for l in lab]
    r["template_id"] = [l[1] for l in lab]
    r["raw"] = (r["similarity"] * 4).astype(np.int32)
    if n >= 8:
        r[1] = r[0]  # an exact duplicate
        r[3] = r[2]
        r[3]["template_id"] = (int(r[2]["template_id"]) + 1) % 20  # same (x, y, sim, class), other template: adjacent ...
        r[n - 1] = r[4]
        r[n - 1]["template_id"] = (int(r[4]["template_id"]) + 7) % 20  # ... and, with other templates between, not adjacent
    return r


def run_nms(ctx, d_recs, d_counts, cap, n_frames, score, thr, eta=1.0, top_k=0, out_cap=None, n_parts=1, part_stride=0, stream=0):
    import torch

    out_cap = cap * n_parts if out_cap is None else out_cap
    d_out = torch.zeros(max(n_frames * out_cap * REC, 1), dtype=torch.uint8, device="cuda:0")
    d_oc = torch.full((n_frames * 2,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.nms_batch_device(d_recs, d_counts, cap, n_frames, d_out.data_ptr(), out_cap, d_oc.data_ptr(), score, thr, eta, top_k,
                         n_parts=n_parts, part_stride=part_stride, stream=stream)
    torch.cuda.synchronize()
    oc = d_oc.cpu().numpy().reshape(-1, 2)
    out = d_out.cpu().numpy()[: n_frames * out_cap * REC].reshape(n_frames, out_cap * REC) if out_cap else None
    return [(out[f].view(MATCH_DTYPE)[: min(oc[f, 0], out_cap)] if out_cap else np.zeros(0, MATCH_DTYPE)) for f in range(n_frames)], oc


# ---- the label table ---------------------------------------------------------------------------------------------------------
# classes 0..2, template ids 0..19; the level-0 size depends on the template id alone.  (80, 40) against (40, 40) at one origin is
# IoU 1600 / 3200 = 0.5 exactly; (0, 0) and (0, 7) are empty boxes.
SIZE_OF_TID = {**{t: (40, 40) for t in range(20)}, 10: (80, 40), 11: (33, 57), 12: (1, 1), 13: (0, 0), 14: (0, 7)}
SIZES = {(c, t): SIZE_OF_TID[t] for c in range(3) for t in range(20)}
SOLID_TIDS = [t for t in range(20) if SIZE_OF_TID[t][0] * SIZE_OF_TID[t][1] > 0]
UNKNOWN = (9, 3)  # a label no template carries
CELL_W, CELL_H = 90, 60  # a grid cell holds any box of the table


def label_table(case1_templates):
    """a copy of 60 case1 templates as classes 0..2 x template ids 0..19 with the level-0 width / height of SIZES
    (sbm_upload_templates does not validate them; no match runs on the context that gets this table)"""
    ts = case1_templates.subset(range(0, 60))
    ts.class_idx[:] = np.arange(ts.n_templates) % 3
    ts.template_id[:] = np.arange(ts.n_templates) // 3
    for t in range(ts.n_templates):
        w, h = SIZES[(int(ts.class_idx[t]), int(ts.template_id[t]))]
        ts.levels[t, 0]["width"], ts.levels[t, 0]["height"] = w, h
    return ts


# ---- cases and launches ------------------------------------------------------------------------------------------------------
P = collections.namedtuple("P", "score thr eta top_k")
P.__new__.__defaults__ = (1.0, 0)
DECOY = (0, 0, 127.0, -7, 0, 0)  # (x, y, similarity, raw, class_idx, template_id)


class Case:
    def __init__(self, name, edge, parts, cap, params, check, flags=0, counts=None, out_cap=None, disjoint=False):
        self.name, self.edge, self.cap, self.params, self.check, self.flags = name, edge, int(cap), params, check, flags
        self.parts = [np.ascontiguousarray(p, MATCH_DTYPE) for p in (parts if isinstance(parts, (list, tuple)) else [parts])]
        self.counts = [(len(p), 0) for p in self.parts] if counts is None else [tuple(c) for c in counts]
        self.out_cap = len(self.parts) * self.cap if out_cap is None else int(out_cap)
        self.disjoint = disjoint
        assert len(self.counts) == len(self.parts) and all(len(p) <= self.cap for p in self.parts)
        assert not disjoint or (params.top_k == 0 and params.thr >= 0 and params.score < 0)

    @property
    def n_parts(self):
        return len(self.parts)

    def used(self):
        """the records the stage gathers: every part's first clamp(count, 0, cap), in part order"""
        got = [p[: min(max(c, 0), self.cap)] for p, (c, _) in zip(self.parts, self.counts)]
        assert all(len(g) == min(max(c, 0), self.cap) for g, (c, _) in zip(got, self.counts)), "a buffer shorter than its count"
        return np.concatenate(got) if got else np.zeros(0, MATCH_DTYPE)

    def at(self, name=None, **kw):
        """the same lists under another cap, parameters or out_cap"""
        a = dict(cap=self.cap, params=self.params, check=self.check, flags=self.flags, counts=self.counts, disjoint=self.disjoint)
        a.update(kw)
        return Case(name or self.name, self.edge, self.parts, **a)

    def __repr__(self):
        return f"Case({self.name})"


class Launch:
    def __init__(self, name, cases):
        c0 = cases[0]
        assert all((c.cap, c.n_parts, c.params, c.out_cap) == (c0.cap, c0.n_parts, c0.params, c0.out_cap) for c in cases), name
        self.name, self.cases = name, list(cases)
        self.cap, self.n_parts, self.params, self.out_cap = c0.cap, c0.n_parts, c0.params, c0.out_cap

    def buffer(self, order=None):
        """(bytes, header, part_stride): the gathered layout of a sharded step -- per part the {count, overflow} pairs of every
        frame, rounded up to 16 bytes, then n_frames * cap records; parts part_stride apart, which is more than one part's
        records, a multiple of 8 (the pairs are read as int32) and not of 16.  Frame k of the call is cases[order[k]]."""
        order = list(range(len(self.cases))) if order is None else list(order)
        nf = len(order)
        hdr = (8 * nf + 15) // 16 * 16
        stride = hdr + nf * self.cap * REC + 8
        stride += 8 if stride % 16 == 0 else 0
        assert stride % 8 == 0 and stride % 16 != 0 and stride > nf * self.cap * REC
        buf = np.zeros(self.n_parts * stride, np.uint8)
        decoys = np.array([DECOY] * self.cap, MATCH_DTYPE).view(np.uint8) if self.cap else np.zeros(0, np.uint8)
        for p in range(self.n_parts):
            for k, ci in enumerate(order):
                c = self.cases[ci]
                o = p * stride + hdr + k * self.cap * REC
                buf[o: o + self.cap * REC] = decoys
                buf[o: o + len(c.parts[p]) * REC] = c.parts[p].view(np.uint8)
                buf[p * stride + 8 * k: p * stride + 8 * k + 8] = np.array(c.counts[p], np.int32).view(np.uint8)
        return buf, hdr, stride


_EPI, _WANT = {}, {}


def _key(u):
    return hashlib.sha1(u.tobytes()).digest()


def epi(case):
    u = case.used()
    k = _key(u)
    if k not in _EPI:
        _EPI[k] = epilogue(u)
    return _EPI[k]


def want(case, params=None):
    """the kept records of a case (under other parameters where given), computed once per process"""
    params = case.params if params is None else params
    k = (_key(case.used()), tuple(params), case.disjoint and params == case.params)
    if k not in _WANT:
        _WANT[k] = epi(case) if k[2] else expected(case.used(), SIZES, *params)
    return _WANT[k]


def candidates(case):
    """the epilogue list after the score filter and top_k: what enters the walk"""
    e = epi(case)
    c = e[[i for i in range(len(e)) if float(e[i]["similarity"]) > case.params.score]]
    return c[: case.params.top_k] if 0 < case.params.top_k < len(c) else c


def problem(case):
    """the case as an NMSBoxes call: the boxes and scores of the epilogue list, and the parameters"""
    e = epi(case)
    return (boxes_of(e, SIZES), [float(m["similarity"]) for m in e]) + tuple(case.params)


def flags_of(case):
    """the flags word from the expectation side: 1 a raw list overflowed, 2 out_cap too small, 4 an unknown label in the walk"""
    f = 1 if any(c > case.cap or o != 0 for c, o in case.counts) else 0
    f |= 2 if len(want(case)) > case.out_cap else 0
    f |= 4 if any((int(m["class_idx"]), int(m["template_id"])) not in SIZES for m in candidates(case)) else 0
    return f


def all_disjoint(case):
    """every box non-empty and inside a grid cell of its own: no two overlap, every record is kept"""
    e = epi(case)
    b = np.array(boxes_of(e, SIZES), np.int64).reshape(-1, 4)
    cells = set(zip((b[:, 0] // CELL_W).tolist(), (b[:, 1] // CELL_H).tolist()))
    return bool(len(e) == len(case.used()) and len(cells) == len(b) and (b[:, 2] > 0).all() and (b[:, 3] > 0).all()
                and (b[:, 0] % CELL_W + b[:, 2] <= CELL_W).all() and (b[:, 1] % CELL_H + b[:, 3] <= CELL_H).all())


# ---- record lists --------------------------------------------------------------------------------------------------------------

def sim(i):
    """strictly decreasing, exact in float32 up to i = 4160; the midpoint of two neighbours is exact too"""
    return np.float32(100.0 - i / 64.0)


def recs(rows):
    """rows of (x, y, similarity, class_idx, template_id); raw is the position in the list, so that two records equal in every
    compared field can still be told apart"""
    r = np.zeros(len(rows), MATCH_DTYPE)
    for k, (x, y, s, c, t) in enumerate(rows):
        r[k] = (x, y, s, k, c, t)
    return r


def reraw(r):
    r = r.copy()
    r["raw"] = np.arange(len(r))
    return r


def shuffled(r, seed):
    return reraw(r[np.random.RandomState(seed).permutation(len(r))])


def ranked(n, seed, spread, tids=SOLID_TIDS):
    """n records, record i with similarity sim(i) (its position after the sort), random positions and labels"""
    rs = np.random.RandomState(seed)
    return recs([(int(rs.randint(-20, spread)), int(rs.randint(-20, spread)), sim(i), int(rs.randint(0, 3)), int(tids[rs.randint(0, len(tids))]))
                 for i in range(n)])


def gridded(n, seed=None, first=0, rank0=0):
    """n records in grid cells of their own (all disjoint), record i with similarity sim(rank0 + i); shuffled when seeded"""
    r = recs([(((first + i) % 64) * CELL_W + (i % 7), ((first + i) // 64) * CELL_H + (i % 3), sim(rank0 + i), i % 3, SOLID_TIDS[i % len(SOLID_TIDS)])
              for i in range(n)])
    return r if seed is None else shuffled(r, seed)


def n_candidates_is(m):
    return lambda c: len(candidates(c)) == m


# ---- 1. record counts ------------------------------------------------------------------------------------------------------------
COUNTS_N = [0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097]
OVERLAP = P(0.0, 0.5)


@functools.lru_cache(None)
def count_list(n):
    """n records with distinct similarities and random overlapping boxes, gathered order shuffled.  From 1000 records on, three
    quarters of them, the best one included, lie within 3 pixels of one position far from the rest: the first kept box
    suppresses them, so that the Python walk stays short while the sort, the compaction and the walk still see all n"""
    if n < 1000:
        return shuffled(ranked(n, 1000 + n, 300), n)
    r = ranked(n, 1000 + n, 200 if n > 2000 else 250, tids=[0, 1, 2, 10, 11])
    rs = np.random.RandomState(n)
    pile = rs.rand(n) < 0.75
    pile[0] = True
    r["x"][pile] = 5000 + rs.randint(-3, 4, int(pile.sum()))
    r["y"][pile] = 5000 + rs.randint(-3, 4, int(pile.sum()))
    r["template_id"][pile] = rs.randint(0, 3, int(pile.sum()))
    return shuffled(r, n)


def _count_check(n):
    def check(c):
        u = c.used()
        return len(u) == n and len(set(u["similarity"].tolist())) == n and len(epi(c)) == n and (n < 65 or 0 < len(want(c)) < n)
    return check


def group_counts():
    big = Launch("counts-cap4097", [Case(f"n{n}", "n records gathered, LDS and scratch frames in one launch", count_list(n), 4097, OVERLAP,
                                         _count_check(n)) for n in COUNTS_N])
    edge = "host: N = n_parts * cap > NMS_LDS_MAX allocates scratch; kernel: n <= NMS_LDS_MAX takes LDS"
    return [big,
            Launch("counts-cap2048-n2048", [Case("cap2048-n2048", edge, count_list(2048), 2048, OVERLAP, _count_check(2048))]),
            Launch("counts-cap2049-n2049", [Case("cap2049-n2049", edge, count_list(2049), 2049, OVERLAP, _count_check(2049))]),
            Launch("counts-cap2049-n2048", [Case("cap2049-n2048", edge, count_list(2048), 2049, OVERLAP, _count_check(2048))])]


# ---- 2. candidate counts ---------------------------------------------------------------------------------------------------------
CANDIDATES_M = [0, 1, 63, 64, 65, 128, 129, 1024, 1025]


@functools.lru_cache(None)
def list1100():
    return shuffled(ranked(1100, 77, 250), 78)


def group_candidates():
    out = []
    for m in CANDIDATES_M:
        between = float(np.float32((float(sim(m - 1)) + float(sim(m))) / 2)) if m else 101.0
        out.append(Launch(f"candidates-m{m}", [Case(f"m{m}-between", "m candidates after unique and score: threshold between two similarities",
                                                    list1100(), 1100, P(between, 0.5), n_candidates_is(m))]))
        # the threshold equal to record m's similarity: `>` leaves that record out
        out.append(Launch(f"candidates-m{m}-equal", [Case(f"m{m}-equal", "score_threshold equal to a held similarity: > leaves it out",
                                                          list1100(), 1100, P(float(sim(m)), 0.5),
                                                          lambda c, m=m: len(candidates(c)) == m and float(sim(m)) in epi(c)["similarity"].tolist())]))
    return out


# ---- 3. top_k ----------------------------------------------------------------------------------------------------------------------
TOP_K = [1, 63, 64, 65, 1023, 1024, 1025, 1099, 1100, 1101]


def _with_unknown(r, rank):
    """the record of similarity sim(rank) gets a label no template carries"""
    r = r.copy()
    (i,) = np.nonzero(r["similarity"] == sim(rank))[0]
    r[i]["class_idx"], r[i]["template_id"] = UNKNOWN
    return r


def _unknown_at(c, rank, inside):
    cand = candidates(c)
    pos = [k for k, m in enumerate(epi(c)) if (int(m["class_idx"]), int(m["template_id"])) == UNKNOWN]
    return len(cand) == min(c.params.top_k, 1100) and pos == [rank] and (rank < len(cand)) == inside


def group_top_k():
    out = []
    for k in TOP_K:
        cases = []
        if k < 1100:  # at candidate position top_k: cut, flag 4 stays clear
            cases.append(Case(f"topk{k}-unknown-cut", "top_k: the unknown label at candidate position top_k is cut", _with_unknown(list1100(), k),
                              1100, P(0.0, 0.5, 1.0, k), lambda c, k=k: _unknown_at(c, k, False), flags=0))
        else:
            cases.append(Case(f"topk{k}-plain", "top_k at or beyond the candidate count cuts nothing", list1100(), 1100, P(0.0, 0.5, 1.0, k),
                              n_candidates_is(1100), flags=0))
        last = min(k, 1100) - 1  # at position top_k - 1: the last candidate, kept as an empty box, flag 4
        cases.append(Case(f"topk{k}-unknown-last", "top_k: the unknown label at candidate position top_k - 1 walks as an empty box",
                          _with_unknown(list1100(), last), 1100, P(0.0, 0.5, 1.0, k),
                          lambda c, last=last: _unknown_at(c, last, True) and UNKNOWN in [(int(m["class_idx"]), int(m["template_id"])) for m in want(c)],
                          flags=4))
        out.append(Launch(f"topk{k}", cases))
    return out


# ---- 4. the unique step ------------------------------------------------------------------------------------------------------------
RUN_TIDS = (3, 10, 11)  # (40, 40), (80, 40), (33, 57): the wrong survivor of a run has another box too


def _with_run(r, first, length):
    """records first .. first + length - 1 (by rank) become equal in (x, y, similarity, class) with template ids RUN_TIDS: after
    the sort they lie at those positions in that order, and only the first survives"""
    r = r.copy()
    for j in range(length):
        r[first + j] = r[first]
        r[first + j]["template_id"] = RUN_TIDS[j]
    return r


def _runs_at(runs, n):
    def check(c):
        u, e = c.used(), epi(c)
        order = sorted(range(len(u)), key=lambda i: (-float(u[i]["similarity"]), int(u[i]["template_id"])))
        ok = len(u) == n and len(e) == n - sum(length - 1 for _, length in runs)
        for first, length in runs:
            same = [u[order[first + j]] for j in range(length)]
            ok = ok and all((int(s["x"]), int(s["y"]), float(s["similarity"]), int(s["class_idx"])) ==
                            (int(same[0]["x"]), int(same[0]["y"]), float(same[0]["similarity"]), int(same[0]["class_idx"])) for s in same)
            ok = ok and [int(s["template_id"]) for s in same] == list(RUN_TIDS[:length])
            ok = ok and sum(1 for m in e if float(m["similarity"]) == float(same[0]["similarity"])) == 1
        return ok
    return check


def bitonic_order(r, tie_break=True):
    """the kernel's sort network over record indices padded with sentinels to a power of two; without the index tie-break it is
    what an unstable sort may make of equal records"""
    n = len(r)
    size = 1
    while size < n:
        size <<= 1
    keys = [(-float(m["similarity"]), int(m["template_id"]), int(m["class_idx"]), int(m["y"]), int(m["x"])) for m in r]
    idx = list(range(n)) + [None] * (size - n)

    def before(a, b):
        if b is None:
            return a is not None
        if a is None:
            return False
        if keys[a] != keys[b]:
            return keys[a] < keys[b]
        return a < b if tie_break else False

    k = 2
    while k <= size:
        j = k >> 1
        while j > 0:
            for t in range(size >> 1):
                i = 2 * j * (t // j) + (t % j)
                a, b = idx[i], idx[i + j]
                if before(b, a) if (i & k) == 0 else before(a, b):
                    idx[i], idx[i + j] = b, a
            j >>= 1
        k <<= 1
    return idx[:n]


def _unique_raws(r, order):
    out, last = [], None
    for i in order:
        k = (int(r[i]["x"]), int(r[i]["y"]), float(r[i]["similarity"]), int(r[i]["class_idx"]))
        if k != last:
            out.append(int(r[i]["raw"]))
        last = k
    return out


def _tie_break_decides(c):
    """the survivors are the earlier records in gathered order, the network with the tie-break finds them, and the same network
    without it keeps another record of at least one pair"""
    u = c.used()
    stable = _unique_raws(u, bitonic_order(u, True))
    first = {}
    for m in u:
        k = (int(m["x"]), int(m["y"]), float(m["similarity"]), int(m["class_idx"]), int(m["template_id"]))
        first.setdefault(k, int(m["raw"]))
    return (stable == [int(m["raw"]) for m in epi(c)] and set(stable) == set(first.values()) and len(first) < len(u)
            and _unique_raws(u, bitonic_order(u, False)) != stable)


def _with_duplicates(r, pairs):
    """record b becomes record a in every field but raw, for (a, b) in pairs, a < b in gathered order"""
    r = r.copy()
    for a, b in pairs:
        raw = int(r[b]["raw"])
        r[b] = r[a]
        r[b]["raw"] = raw
    return r


def dup_pairs(n):
    """24 disjoint pairs of gathered positions (a, b), a < b"""
    p = np.random.RandomState(n).permutation(n)[:48].reshape(-1, 2)
    return [(int(min(a, b)), int(max(a, b))) for a, b in p]


def group_unique():
    n = 1100
    base = ranked(n, 41, 450)
    two = [(0, 2), (63, 2), (1023, 2), (n - 2, 2)]
    three = [(0, 3), (62, 3), (1022, 3), (n - 3, 3)]
    r2, r3 = base, base
    for first, length in two:
        r2 = _with_run(r2, first, length)
    for first, length in three:
        r3 = _with_run(r3, first, length)
    # not adjacent: ranks 500 and 502 equal in (x, y, similarity, class) with template ids 2 and 7, rank 501 of the same similarity
    # with template id 5 elsewhere: it sorts between them, both survive
    apart = base.copy()
    apart[500]["template_id"] = 2
    apart[502] = apart[500]
    apart[502]["template_id"] = 7
    apart[501]["similarity"] = apart[500]["similarity"]
    apart[501]["template_id"] = 5
    apart[501]["x"] = int(apart[500]["x"]) + 300
    apart = reraw(apart)
    runs = Launch("unique-runs", [
        Case("runs-of-2", "runs of 2 at sorted positions 0|1, 63|64, 1023|1024 and ending at n - 1", shuffled(r2, 5), n, OVERLAP, _runs_at(two, n)),
        Case("runs-of-3", "runs of 3 at sorted positions 0..2, 62..64, 1022..1024 and ending at n - 1", shuffled(r3, 6), n, OVERLAP, _runs_at(three, n)),
        Case("not-adjacent", "equal in the compared fields but apart after the sort: both survive", shuffled(apart, 7), n, OVERLAP,
             lambda c: len(epi(c)) == n and sorted(int(m["template_id"]) for m in epi(c) if float(m["similarity"]) == float(sim(500))) == [2, 5, 7])])
    ties = []
    for m in (65, 1025):  # one more than a power of two: the network runs over sentinels too
        r = _with_duplicates(shuffled(ranked(m, 90 + m, 300), m), dup_pairs(m))
        ties.append(Case(f"duplicates-n{m}", "exact duplicates differing in raw, inside one part, n = 2^k + 1: the index tie-break",
                         r, 1025, P(-1.0, 1.0), _tie_break_decides))
    r = _with_duplicates(shuffled(ranked(65, 33, 300), 34), [(0, 64), (3, 50), (10, 45), (19, 46), (7, 8)])
    parts3 = [r[:20], r[20:45], r[45:]]
    across = Case("duplicates-across-parts", "exact duplicates in part 0 and part 2: the earlier in gathered order survives",
                  parts3, 25, P(-1.0, 1.0), lambda c: _tie_break_decides(c) and c.n_parts == 3)
    return [runs, Launch("unique-duplicates", ties), Launch("unique-duplicates-parts", [across])]


# ---- 5. sort keys ------------------------------------------------------------------------------------------------------------------
SORT_KEYS = ("template_id", "class_idx", "y", "x")


def sort_key_list():
    """four pairs, each tied in similarity and differing in exactly one later key; gathered with the later record first, so that
    the index order is the wrong one"""
    rows = [(10, 20, 90.0, 1, 5), (10, 20, 90.0, 1, 4),          # template_id alone: a run, the lower id survives the unique step
            (300, 20, 89.0, 2, 4), (300, 20, 89.0, 0, 4),        # class_idx alone: one position, the lower class suppresses the other
            (600, 3, 88.0, 1, 4), (600, -7, 88.0, 1, 4),         # y alone, one of them negative: overlap 0.6
            (-2, 300, 87.0, 1, 4), (-12, 300, 87.0, 1, 4),       # x alone, both negative: overlap 0.6
            (900, 900, 86.0, 0, 0)]
    return recs(rows)


def _each_key_decides(c):
    u = c.used()
    decided = set()
    for a in range(len(u)):
        for b in range(a + 1, len(u)):
            if float(u[a]["similarity"]) == float(u[b]["similarity"]):
                diff = [k for k in SORT_KEYS if int(u[a][k]) != int(u[b][k])]
                if len(diff) == 1:
                    decided.add(diff[0])
    neg = (u["x"] < 0).any() and (u["y"] < 0).any()
    return decided == set(SORT_KEYS) and bool(neg) and [int(m["raw"]) for m in epi(c)] == [1, 3, 2, 5, 4, 7, 6, 8]


def group_sort_keys():
    edge = "records tied in similarity, ordered by exactly one later key (template_id, class_idx, y, x; negative values)"
    return [Launch("sortkeys-thr0.5", [Case("sortkeys-suppressing", edge, sort_key_list(), 16, OVERLAP,
                                            lambda c: _each_key_decides(c) and [int(m["raw"]) for m in want(c)] == [1, 3, 5, 7, 8])]),
            Launch("sortkeys-thr1", [Case("sortkeys-order", edge, sort_key_list(), 16, P(0.0, 1.0), _each_key_decides)])]


# ---- 6. the order of the walk ------------------------------------------------------------------------------------------------------
def chain(n=130, rank0=0, y=0):
    """boxes (25 i, y) of 40 x 40, decreasing similarity: neighbours overlap by 15 * 40 / (3200 - 600) = 15 / 65, nothing else does"""
    return recs([(25 * i, y, sim(rank0 + i), i % 3, i % 10) for i in range(n)])


def _kept_raws(c):
    return [int(m["raw"]) for m in want(c)]


def group_walk():
    ch = chain()
    ahead = reraw(np.concatenate([gridded(64, first=64), chain(130, 64)]))  # 64 disjoint boxes (grid rows 1.., y >= 60) sort before the chain
    same = recs([(70, 70, sim(i), i % 3, i % 10) for i in range(200)])  # one position, 40 x 40 each: every overlap is 1
    apart = gridded(130)
    return [
        Launch("walk-chain-thr0.2", [
            Case("chain130-thr0.2", "a chain across chunks: every other box survives (overlap 15/65 > 0.2)", shuffled(ch, 1), 200, P(0.0, 0.2),
                 lambda c: [float(m["similarity"]) for m in want(c)] == [float(sim(i)) for i in range(0, 130, 2)]),
            Case("chain130-behind-64", "the chain behind 64 disjoint boxes: its decisions cross the chunk borders at the other parity",
                 shuffled(ahead, 2), 200, P(0.0, 0.2),
                 lambda c: [float(m["similarity"]) for m in want(c)] == [float(sim(i)) for i in list(range(64)) + list(range(64, 194, 2))])]),
        Launch("walk-chain-thr0.25", [Case("chain130-thr0.25", "the same chain under a threshold above 15/65: all survive", shuffled(ch, 1), 200,
                                           P(0.0, 0.25), lambda c: len(want(c)) == 130)]),
        Launch("walk-one-position-thr0.5", [Case("same200-thr0.5", "200 boxes at one position: chunks 1.. are suppressed through the earlier-chunk path alone",
                                                 shuffled(same, 3), 200, OVERLAP, lambda c: _kept_raws(c) == [int(epi(c)[0]["raw"])] and len(epi(c)) == 200)]),
        Launch("walk-one-position-thr1", [Case("same200-thr1", "overlap 1 is not greater than threshold 1: all 200 survive", shuffled(same, 3), 200,
                                               P(0.0, 1.0), lambda c: len(want(c)) == 200)]),
        Launch("walk-negative-thr", [Case("disjoint130-thr-0.25", "overlap 0 is greater than a negative threshold: only the first survives",
                                          shuffled(apart, 4), 200, P(0.0, -0.25), lambda c: all_disjoint(c) and len(want(c)) == 1)])]


# ---- 7. overlap equal to the threshold ---------------------------------------------------------------------------------------------
BELOW_HALF = float(np.nextafter(np.float32(0.5), np.float32(0)))


def group_equal_overlap():
    pair = recs([(5, 5, 90.0, 0, 0), (5, 5, 80.0, 1, 10)])          # (40, 40) and (80, 40) at one origin: overlap exactly 0.5
    empties = recs([(5, 5, 90.0, 0, 13), (400, 9, 80.0, 1, 14)])    # (0, 0) and (0, 7): two empty boxes have overlap 1
    mixed = recs([(5, 5, 90.0, 0, 0), (5, 5, 80.0, 1, 13), (45, 5, 70.0, 2, 0), (-7, -7, 60.0, 0, 12)])  # solid, empty inside it, touching, corner
    n_kept = lambda n: (lambda c: len(want(c)) == n)  # noqa: E731
    return [
        Launch("equal-thr0.5", [Case("half-at-0.5", "overlap == threshold is kept (<=)", pair, 4, OVERLAP, n_kept(2)),
                                Case("empties-at-0.5", "two empty boxes overlap by 1: the second is dropped", empties, 4, OVERLAP, n_kept(1))]),
        Launch("equal-thr-below-0.5", [Case("half-below-0.5", "the next float below the overlap drops the box", pair, 4, P(0.0, BELOW_HALF), n_kept(1))]),
        Launch("equal-thr1", [Case("empties-at-1", "overlap 1 at threshold 1 is kept", empties, 4, P(0.0, 1.0), n_kept(2))]),
        Launch("equal-thr0", [Case("zero-at-0", "an empty box against a solid one, touching boxes, a negative corner: overlap 0 is kept at 0", mixed, 4,
                                   P(0.0, 0.0), n_kept(4))])]


# ---- 8. the adaptive threshold -----------------------------------------------------------------------------------------------------
def thresholds(thr, eta, n):
    """the threshold before kept box 0, 1, ... n - 1 (nms.hpp: multiplied after a kept box while eta < 1 and it is > 0.5)"""
    t, out = np.float32(thr), []
    for _ in range(n):
        out.append(float(t))
        if eta < 1 and t > 0.5:
            t = np.float32(t * np.float32(eta))
    return out


@functools.lru_cache(None)
def adaptive_list(n):
    return shuffled(ranked(n, 600 + n, 700, tids=[0, 1, 2, 10, 11]), 601)


def _passes_half_late(c):
    """the threshold passes 0.5 after the 183rd kept box, which lies beyond walk position 128"""
    t = thresholds(c.params.thr, c.params.eta, 200)
    w, e = want(c), epi(c)
    pos = {int(m["raw"]): k for k, m in enumerate(e)}
    return t[182] > 0.5 >= t[183] and len(w) > 183 and pos[int(w[182]["raw"])] > 2 * NMS_CHUNK


def group_adaptive():
    early = shuffled(ranked(60, 8, 60, tids=[0, 1, 2]), 9)
    slow = P(0.0, 0.6, 0.999)

    def differs(c):
        return rows_of(want(c)) != rows_of(want(c, P(0.0, 0.6))) and rows_of(want(c)) != rows_of(want(c, P(0.0, 0.5))) and _passes_half_late(c)

    return [
        Launch("adaptive-early", [Case("eta0.8-thr0.9", "0.9 -> 0.72 -> 0.576 -> 0.4608: the threshold stops falling after three kept boxes, inside chunk 0",
                                       early, 64, P(0.0, 0.9, 0.8),
                                       lambda c: thresholds(0.9, 0.8, 6)[3] <= 0.5 < thresholds(0.9, 0.8, 6)[2] and len(want(c)) >= 4
                                       and rows_of(want(c)) != rows_of(want(c, P(0.0, 0.9))) and rows_of(want(c)) != rows_of(want(c, P(0.0, 0.9, 0.5))))]),
        Launch("adaptive-late", [Case("eta0.999-n1500", "the threshold crosses 0.5 in a later chunk than the first", adaptive_list(1500), 1500, slow, differs)]),
        Launch("adaptive-late-scratch", [Case("eta0.999-n2049", "the same on the scratch path", adaptive_list(2049), 2049, slow,
                                              lambda c: _passes_half_late(c) and len(c.used()) > NMS_LDS_MAX)])]


# ---- 9. the kept list and the outputs ----------------------------------------------------------------------------------------------
KEEP_ALL = P(-1.0, 1.0)
OUT_CAPS = [(2049, 0), (2048, 2), (5, 2), (0, 2)]  # (out_cap, flags)


@functools.lru_cache(None)
def disjoint_list(n):
    return gridded(n, seed=n)


def group_outputs():
    edge = "2049 disjoint boxes, all kept: the kept list lives in scratch and is sliced over the 16 waves 129 times; out_cap against it"
    out = []
    for oc, flags in OUT_CAPS:
        # n = 0 rides along: its {0, 0} pair must be written too
        out.append(Launch(f"outputs-outcap{oc}", [
            Case(f"kept2049-outcap{oc}", edge, disjoint_list(2049), 2049, KEEP_ALL, lambda c: all_disjoint(c) and len(want(c)) == 2049 > NMS_WAVES * NMS_CHUNK,
                 flags=flags, out_cap=oc, disjoint=True),
            Case(f"kept0-outcap{oc}", "n = 0: the count pair is still written", np.zeros(0, MATCH_DTYPE), 2049, KEEP_ALL, lambda c: len(want(c)) == 0,
                 out_cap=oc, disjoint=True)]))
    return out


def smallest_disjoint_case():
    return Case("kept130", "py_nms keeps every box of an all-disjoint list", disjoint_list(130), 130, KEEP_ALL, all_disjoint, disjoint=True)


# ---- 10. parts ---------------------------------------------------------------------------------------------------------------------
def group_parts():
    cap = 700
    r = shuffled(ranked(2100, 55, 700), 56)
    a = shuffled(ranked(707, 57, 400), 58)
    b = shuffled(ranked(703, 59, 400), 60)
    s = shuffled(ranked(18, 61, 120), 62)
    none = np.zeros(0, MATCH_DTYPE)
    used_n = lambda n: (lambda c: len(c.used()) == n and len(want(c)) > 0)  # noqa: E731
    cases = [
        Case("parts-0-cap-7", "an empty part beside a full one", [none, a[:700], a[700:]], cap, OVERLAP, used_n(707)),
        Case("parts-overflowed", "count = cap + 5: flag 1, the first cap records are used", [b[:700], b[700:], none], cap, OVERLAP, used_n(703),
             flags=1, counts=[(cap + 5, 0), (3, 0), (0, 0)]),
        Case("parts-negative-count", "a negative count is read as 0: the records behind it are not gathered", [s[:10], s[10:14], s[14:]], cap, OVERLAP,
             used_n(8), counts=[(-1, 0), (4, 0), (4, 0)]),
        Case("parts-overflow-word", "the overflow word set in part 1 only: flag 1", [s[:5], s[5:11], s[11:]], cap, OVERLAP, used_n(18), flags=1,
             counts=[(5, 0), (6, 1), (7, 0)]),
        Case("parts-union-2100", "3 x 700: every part below 2048, their union above it", [r[:700], r[700:1400], r[1400:]], cap, OVERLAP,
             lambda c: len(c.used()) == 2100 > NMS_LDS_MAX >= cap)]
    return [Launch("parts-3x700", cases)]


# ---- 11. launches ------------------------------------------------------------------------------------------------------------------
def small_cases():
    """the small lists of the groups above under one cap and one set of parameters"""
    src = [c for l in group_counts()[:1] for c in l.cases if len(c.used()) <= 65]
    src += [l.cases[0] for l in group_sort_keys()[:1] + group_walk() + group_equal_overlap()] + [group_unique()[1].cases[0], group_adaptive()[0].cases[0]]
    return [c.at(name=f"small-{c.name}", cap=200, params=OVERLAP, flags=0, check=lambda c: len(c.used()) <= 200) for c in src]


def group_launches():
    small = small_cases()
    return [Launch("launch-70-frames", [small[k % len(small)].at(name=f"{small[k % len(small)].name}-frame{k}") for k in range(70)])]


def scratch_growth():
    """(first, second): the second call's n_parts * cap makes the scratch grow; the first is repeated after it"""
    small = small_cases()
    first = Launch("growth-first", [Case("growth-n2049", "a scratch frame before and after the scratch grows", count_list(2049), 2049, OVERLAP,
                                         _count_check(2049))] + [c.at(cap=2049) for c in small[:3]])
    return first, group_counts()[0]


GROUPS = collections.OrderedDict([
    ("counts", group_counts), ("candidates", group_candidates), ("top_k", group_top_k), ("unique", group_unique), ("sort_keys", group_sort_keys),
    ("walk", group_walk), ("equal_overlap", group_equal_overlap), ("adaptive", group_adaptive), ("outputs", group_outputs), ("parts", group_parts),
    ("launches", group_launches)])


@functools.lru_cache(None)
def launches(group):
    return GROUPS[group]()


def all_cases():
    """(group, launch, case) of every case; names are unique"""
    out = [(g, l, c) for g in GROUPS for l in launches(g) for c in l.cases]
    names = [c.name for _, _, c in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return out


TIE_SEEDS = [(1, 1.0, 0), (2, 0.9, 0), (3, 1.0, 20), (4, 0.8, 50)]  # test_nms.py::test_nms_boxes


def tie_problems():
    """{key: NMSBoxes problem}: the lists of test_nms.py::test_nms_boxes (40 score values over 300 boxes, some of them empty:
    the stable sort decides) under its thresholds, top_k and eta, and lists of 0 and 1 boxes"""
    out = collections.OrderedDict()
    for seed, eta, top_k in TIE_SEEDS:
        rs = np.random.RandomState(seed)
        n = 300
        boxes = np.stack([rs.randint(0, 400, n), rs.randint(0, 400, n), rs.randint(1, 120, n), rs.randint(1, 120, n)], axis=1).astype(np.int32)
        boxes[::17, 2] = 0
        scores = (rs.randint(0, 40, n) * 2.5).astype(np.float32)
        for thr in (0.5, 0.3, 0.7):
            for m in (n, 0, 1):
                out[f"ties|seed{seed}|n{m}|{thr!r}|{eta!r}|{top_k}"] = (boxes[:m].tolist(), scores[:m].tolist(), 10.0, thr, eta, top_k)
    return out


def recorded_key(case):
    """the key of a case in tests/golden/ref_nms_cases.npz: its name and its parameters"""
    return f"{case.name}|{case.params.score!r}|{case.params.thr!r}|{case.params.eta!r}|{case.params.top_k}"


def pack_recorded(kept):
    """{key: kept indices} as three arrays: the keys, the concatenated indices and each key's offset into them"""
    keys = list(kept)
    return {"keys": np.array(keys), "offsets": np.cumsum([0] + [len(kept[k]) for k in keys]).astype("<i4"),
            "kept": np.concatenate([np.asarray(kept[k], "<u2") for k in keys] + [np.zeros(0, "<u2")])}


def load_recorded(path):
    z = np.load(path)
    assert z["kept"].dtype == np.dtype("<u2")
    return {str(k): z["kept"][a:b].astype(np.int64).tolist() for k, a, b in zip(z["keys"], z["offsets"][:-1], z["offsets"][1:])}
