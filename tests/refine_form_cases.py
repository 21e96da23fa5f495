"""Deterministic inputs for the refinement pass (similarityLocal) at its counter, accumulator, class-run and patch edges, their
plain numpy reference, and the child worker of tests/test_gpu_refine_forms.py (``python tests/refine_form_cases.py --run FORM``).

Two-level pyramids, small.  A world is one geometry: its two orientation maps, the oracle's response planes of them, a list of
templates written as explicit feature lists, launch groups and thresholds.

  worlds       M    T = (4, 8), 256 x 320 (W = 80): constructed label maps installed with set_quantized -- the 8 response planes
                    (set_refine_bits(False)) or whole bit strips built by ensure_local_forms (set_refine_bits(True))
               I48  T = (4, 8), 256 x 320: a synthetic image through the match entry points -- spread strips | sparse bit strips
               I88  T = (8, 8), 320 x 512 (W = 64): spread strips, the T = 8 instantiation
               I17  T = (4, 8), 256 x 272 (W = 68; level 1 is 136 wide, off the one-launch builder's grid): a single frame keeps the
                    8 response planes, a batch takes the spread plane row-major
  regions      saturated: one constant orientation over the template box and the 16 patch cells beyond it, so every feature of
               that label scores 4 at all 256 patch cells (M: a constant label; I: a sawtooth intensity ramp, whose gradient
               direction is constant -- the weak threshold is WEAK_I so that the ramp passes);  neighbour (M only): the same
               with the adjacent orientation, every feature scores 3;  texture: M a field of one random label per 8 x 8 pixels, I
               random shapes -- "planted" templates are cut out of it, so they score 4 nf where they were cut
  templates    COUNTS twice (saturated label | planted); thin ones whose features sit in one, two (15 and 0) or four (3, 7, 11, 15)
               of the (x / T) & 15 classes; a sweep of 16 copies of one template whose declared boxes clamp the candidate to 16
               consecutive window columns and rows; a unique best cell in each patch corner; two equal maxima in a row and in a
               column (M); features outside the level; boxes that clamp at every border
  thresholds   per group a low and a high one and, for up to three refined candidates, their float32 score and one ulp either side

A note on the window column.  With T = (4, 8) an unclamped candidate arrives at x = 2 (8 c + 3) + 1 = 16 c + 7, window column
4 c - 7: only X15 = 1, 5, 9, 13 occur however a template is shifted.  The other columns are reached through the clamp
x <= cols - width - 8 T, which is what the sweep's declared boxes are for (each copy is cut where its clamped window puts it).

Reference (line2Dup.cpp, matchClass :1160-1297): coarse scores as coarse_form_cases.raw_scores, a candidate where
(raw * 100.f) / (4 nf) > thr; x = 2 x + 1, clamped to [8 T, cols - width - 8 T], lower bound first; window origin
(x / T - 8, y / T - 8); local[r][c] = sum over in-image features of LM[label][index(fx + ox, fy + oy) + r W + c], flat in the
sub-plane, int64; first maximum in row-major order with strict > from 0; the position (x / T - 8 + c) T + T / 2 + (T % 2 - 1);
dropped where the float32 score < thr (MatchPredicate :1153-1158), so a score equal to the threshold stays."""
import functools
import json
import os
import pickle
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from coarse_form_cases import as_rows, first_difference, oracle_module, raw_scores, score_of  # noqa: E402
from shape_based_matching_amd import synth  # noqa: E402
from shape_based_matching_amd.templates import MATCH_DTYPE, from_pyramids  # noqa: E402

SEED = 11
WEAK_I = 10.0  # the ramp's Sobel response is 24 (level 0) and 48 (level 1)
RAMP_SLOPE = 3
COUNTS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 72, 73, 127, 128, 129, 252, 253, 256, 257, 1023, 1024, 1025, 2044, 2045,
          2048, 2049, 4095, 8191]
THIN_COUNTS = [64, 65, 256, 257, 1100]
THIN_CLASSES = {"one": [5], "wrap": [15, 0], "perq": [3, 7, 11, 15]}
SWEEP_NF, SWEEP_BOX, SWEEP_CELL = 120, 32, 5
CORNERS = [(0, 0), (0, 15), (15, 0), (15, 15)]  # (row, column) of the patch
NF1 = 20  # features of a level-1 half
GROUPS = ["sat", "planted", "thin", "sweep", "edges", "all"]
LOW, HIGH = 55.0, 96.0
MAX_CANDIDATES = 1 << 16

# rows, cols, T; sx: the saturated region is x < sx (M: y < sy, the neighbour region below ny); ox: the texture starts at x = ox;
# sat / planted: boxes (w, h) in pixels; homes: coarse cells (cx, cy) where level-1 halves sit
WORLDS = {
    "M": dict(kind="maps", T=(4, 8), rows=256, cols=320, sx=136, sy=124, ny=128, ox=140, sat=(64, 56), planted=(100, 180),
              a_homes=[(2, 2), (2, 13), (0, 2), (2, 0)], p_home=(11, 2), sw_home=(17, 13), r_home=(17, 2), b_home=(11, 13)),
    "I48": dict(kind="image", T=(4, 8), rows=256, cols=320, sx=136, ox=140, sat=(64, 64), planted=(100, 180),
                p_home=(11, 2), sw_home=(17, 13), r_home=(17, 2), b_home=(11, 13)),
    "I88": dict(kind="image", T=(8, 8), rows=320, cols=512, sx=264, ox=268, sat=(128, 64), planted=(100, 120),
                p_home=(21, 3), sw_home=(29, 17), r_home=(29, 3), b_home=(21, 17)),
    "I17": dict(kind="image", T=(4, 8), rows=256, cols=272, sx=136, ox=140, sat=(64, 64), planted=(56, 180),
                p_home=(11, 2), sw_home=(14, 13), r_home=(14, 2), b_home=(11, 13)),
}

FORMS = {  # the process-wide knobs of each child (read once per process)
    "waves4": {"SBM_LOCAL_WAVES": "4"},
    "waves16": {"SBM_LOCAL_WAVES": "16"},
    "grid3": {"SBM_LOCAL_GRID": "3"},
    "strip_lm0": {"SBM_STRIP_LM": "0"},
    "full_lm1": {"SBM_FULL_LM": "1"},
    "lm_allty0": {"SBM_LM_ALLTY": "0"},
    "sparse_strips0": {"SBM_SPARSE_STRIPS": "0"},
    "local_bits0": {"SBM_LOCAL_BITS": "0"},
}
KNOBS = ("SBM_LOCAL_WAVES", "SBM_LOCAL_GRID", "SBM_LOCAL_ORDER", "SBM_STRIP_LM", "SBM_FULL_LM", "SBM_LM_ALLTY", "SBM_SPARSE_STRIPS",
         "SBM_SPARSE_GRADIENT", "SBM_LOCAL_BITS")
BITS_MODES = (None, True, False)  # set_refine_bits
CHILD_GROUPS = ("all",)  # what a child runs of every world: every template, at the group's thresholds (the groups matter to the coarse pass)


def offset_of(T):
    return T // 2 + (T % 2 - 1)


def refine_origin(cx, cy, width, height, rows, cols, T):
    """matchClass :1236-1245: (x, y) of the candidate at the finer level, clamped, lower bound first"""
    border = 8 * T
    x, y = 2 * cx + 1, 2 * cy + 1
    x, y = max(x, border), max(y, border)
    return min(x, cols - width - border), min(y, rows - height - border)


def window_of_home(home, width, height, rows, cols, T):
    """the window origin (gx, gy) in cells of the candidate that the coarse cell `home` sends to the finer level"""
    x, y = refine_origin(home[0] * T[1] + offset_of(T[1]), home[1] * T[1] + offset_of(T[1]), width, height, rows, cols, T[0])
    return x // T[0] - 8, y // T[0] - 8


# ---- the maps ------------------------------------------------------------------------------------------------------------

def block_field(rs, rows, cols):
    """one random label per 8 x 8 pixels, every pixel set: a 4 x 4 cell lies inside one block or straddles two to four"""
    lab = rs.randint(0, 8, ((rows + 7) // 8, (cols + 7) // 8))
    return (1 << np.kron(lab, np.ones((8, 8), np.int64))[:rows, :cols]).astype(np.uint8)


def ring0(q):
    q[0, :] = q[-1, :] = 0
    q[:, 0] = q[:, -1] = 0
    return q


def build_maps(p, rs):
    """world M: level 0 = saturated | neighbour | texture regions, level 1 = a sparse synth.onehot_map that carries the level-1
    halves: the same NF1 features at every a_home, NF1 random ones at each of the four other homes"""
    rows, cols = p["rows"], p["cols"]
    q0 = np.zeros((rows, cols), np.uint8)
    q0[:, p["ox"]:] = block_field(rs, rows, cols - p["ox"])
    q0[: p["sy"], : p["sx"]] = 1 << 2
    q0[p["ny"]:, : p["sx"]] = 1 << 3
    # two equal maxima: a block of the texture repeated six cells to the right, another six cells below
    T0, box = p["T"][0], 24
    for name, (dr, dc) in (("tie_row", (0, 6)), ("tie_col", (6, 0))):
        (gx, gy), (r, c) = window_of_home(p["p_home"], *p["planted"], rows, cols, p["T"]), TIE_CELL[name]
        y, x = (gy + r) * T0, (gx + c) * T0
        q0[y + dr * T0: y + dr * T0 + box, x + dc * T0: x + dc * T0 + box] = q0[y: y + box, x: x + box]
    q1 = synth.onehot_map(rs, rows // 2, cols // 2, 3)
    def distinct(n, side):  # n features on distinct pixels of [1, side) x [1, side)
        k = rs.choice((side - 1) ** 2, n, replace=False)
        return np.stack([1 + k % (side - 1), 1 + k // (side - 1), rs.randint(0, 8, n)], axis=1)

    half_a = distinct(NF1, 16)
    for hx, hy in p["a_homes"]:  # (boxes of two coarse cells: the clamped homes at cell 0 do not touch those at cell 2)
        q1[hy * 8: hy * 8 + 16, hx * 8: hx * 8 + 16] = 0
        q1[hy * 8 + half_a[:, 1], hx * 8 + half_a[:, 0]] = (1 << half_a[:, 2]).astype(np.uint8)
    for key in ("p_home", "sw_home", "r_home", "b_home"):
        hx, hy = p[key]
        f = distinct(NF1, 23)
        q1[hy * 8 + f[:, 1], hx * 8 + f[:, 0]] = (1 << f[:, 2]).astype(np.uint8)
    return [ring0(q0), ring0(q1)], half_a


TIE_CELL = {"tie_row": (2, 3), "tie_col": (3, 12)}  # (row, column) of the first of the two maxima; the second is six cells on
TIE_NF = 40


def build_image(p):
    """worlds I: a sawtooth ramp of slope RAMP_SLOPE along x left of the texture (its falling edges have the same orientation
    as the ramp), random shapes over random 12 x 12 tiles from x = ox - 2 on"""
    rows, cols = p["rows"], p["cols"]
    img = np.tile(((RAMP_SLOPE * np.arange(cols)) % 256).astype(np.uint8), (rows, 1))
    x0 = p["ox"] - 2
    rs = np.random.RandomState([SEED, rows, cols])
    tiles = np.kron(rs.randint(0, 128, ((rows + 11) // 12, (cols - x0 + 11) // 12)), np.ones((12, 12), np.int64))[:rows, : cols - x0]
    img[:, x0:] = synth.scene_gray(SEED + cols, rows, cols - x0, n_shapes=60) // 2 + tiles  # no box of 24 pixels without an edge
    return img


class Scene:
    """what the reference reads of one frame: both levels' orientation maps and response planes, from the oracle"""

    def __init__(self, O, T, maps=None, img=None):
        pyr = O.Pyramid.from_quantized(maps, list(T)) if maps is not None else O.Pyramid.build(img, list(T), WEAK_I)
        self.q = [pyr.quantized(l) for l in range(2)]
        self.lm = [pyr.lm(l) for l in range(2)]
        pyr.free()
        self.patches, self.refs = {}, {}  # what the reference computed so far (they travel with the pickled world)


def cut(rs, q, nf, x, y, w, h):
    """nf features out of the set pixels of q in the box (w, h) at (x, y), relative to it; with repeats where the box holds fewer"""
    ys, xs = np.nonzero(q[y: y + h, x: x + w])
    assert len(ys) > 0, (x, y, w, h)
    k = rs.choice(len(ys), nf, replace=len(ys) < nf)
    lab = np.log2(q[y + ys[k], x + xs[k]].astype(np.float64)).astype(np.int64)
    return np.stack([xs[k], ys[k], lab], axis=1)


class World:
    def __init__(self, name, O=None):
        O = O or oracle_module()
        p = self.p = WORLDS[name]
        self.name, self.T, self.rows, self.cols = name, p["T"], p["rows"], p["cols"]
        T0, T1 = self.T
        self.W, self.H = self.cols // T0, self.rows // T0
        self.W1, self.H1 = self.cols // 2 // T1, self.rows // 2 // T1
        rs = np.random.RandomState([SEED, self.cols, T0])
        if p["kind"] == "maps":
            self.maps, half_a = build_maps(p, rs)
            self.img = None
            self.scene = Scene(O, self.T, maps=self.maps)
            self.sat_label = 2
            a_box = (16, 16)
        else:
            self.img = build_image(p)
            self.scene = Scene(O, self.T, img=self.img)
            self.maps = self.scene.q
            q0s = self.maps[0][8:-8, 8: p["sx"] - 8]
            self.sat_label = int(np.log2(np.bincount(q0s.ravel(), minlength=256).argmax()))
            # the level-1 half of the saturated templates spans the ramp at level 1, so it fits in at a few coarse cells only
            a_box = (p["sx"] // 2 - 4, self.rows // 2 - 8)
            lab1 = int(np.log2(np.bincount(self.maps[1][8:-8, 8: p["sx"] // 2 - 8].ravel(), minlength=256).argmax()))
            half_a = np.stack([rs.randint(1, a_box[0], 2 * NF1), rs.randint(1, a_box[1], 2 * NF1), np.full(2 * NF1, lab1)], axis=1)
        q0, q1 = self.maps
        self.specs, pyramids = [], []

        def add(kind, f0, w0, h0, f1, w1, h1, **note):
            self.specs.append(dict(kind=kind, nf=len(f0), w=w0, h=h0, **note))
            pyramids.append([{"width": w0, "height": h0, "features": f0}, {"width": w1, "height": h1, "features": f1}])

        def half(home):
            return cut(rs, q1, NF1, home[0] * T1, home[1] * T1, 24, 24)

        def sat_feats(nf, classes=None):
            bw, bh = p["sat"]
            x = rs.randint(0, bw, nf) if classes is None else T0 * np.asarray(classes)[rs.randint(0, len(classes), nf)] + rs.randint(0, T0, nf)
            return np.stack([x, rs.randint(0, bh, nf), np.full(nf, self.sat_label)], axis=1)

        def planted(nf, home, cell, w, h, box=None, spoil=0):
            """cut where the window of `home` puts patch cell `cell` (row, column): the candidate's best cell"""
            gx, gy = window_of_home(home, w, h, self.rows, self.cols, self.T)
            bw, bh = box or (w, h)
            f = cut(rs, q0, nf, (gx + cell[1]) * T0, (gy + cell[0]) * T0, bw, bh)
            if spoil and nf >= 8:  # a share of the labels moved on by one (3 instead of 4) or by four (0): scores below 100
                k = rs.choice(nf, max(1, nf * spoil // 10), replace=False)
                f[k, 2] = (f[k, 2] + rs.choice([1, 4], len(k))) % 8
            return f

        pw, ph = p["planted"]
        for nf in COUNTS:
            add("sat", sat_feats(nf), *p["sat"], half_a, *a_box)
        for i, nf in enumerate(COUNTS):
            cell = ((5 * i + 1) % 16, (7 * i + 2) % 16)
            add("planted", planted(nf, p["p_home"], cell, pw, ph, spoil=i % 3), pw, ph, half(p["p_home"]), 24, 24, cell=cell, spoil=i % 3)
        for cname, classes in THIN_CLASSES.items():
            for nf in THIN_COUNTS:
                add("thin", sat_feats(nf, classes), *p["sat"], half_a, *a_box, classes=classes)
        # the sweep: the declared box clamps the candidate of sw_home to max_x = T0 (m0 + k) + k % T0, max_y likewise
        x_home, y_home = 2 * (p["sw_home"][0] * T1 + offset_of(T1)) + 1, 2 * (p["sw_home"][1] * T1 + offset_of(T1)) + 1
        m0 = min(x_home // T0, (self.cols - 8 * T0 - SWEEP_BOX) // T0) - 15
        n0 = min(y_home // T0, (self.rows - 8 * T0 - SWEEP_BOX) // T0) - 15
        assert m0 >= 8 and n0 >= 8
        sw_half = half(p["sw_home"])
        for k in range(16):
            w, h = self.cols - 8 * T0 - (T0 * (m0 + k) + k % T0), self.rows - 8 * T0 - (T0 * (n0 + k) + (3 * k) % T0)
            f = planted(SWEEP_NF, p["sw_home"], (SWEEP_CELL, SWEEP_CELL), w, h, box=(SWEEP_BOX, SWEEP_BOX), spoil=k % 2)  # (odd copies score below 100)
            add("sweep", f, w, h, sw_half, 24, 24, cell=(SWEEP_CELL, SWEEP_CELL), window=(m0 + k - 8, n0 + k - 8))
        p_half = half(p["p_home"])
        for cell in CORNERS:
            add("corner", planted(90, p["p_home"], cell, pw, ph, box=(48, 48)), pw, ph, p_half, 24, 24, cell=cell)
        if p["kind"] == "maps":
            for name in ("tie_row", "tie_col"):
                add(name, planted(TIE_NF, p["p_home"], TIE_CELL[name], pw, ph, box=(24, 24)), pw, ph, p_half, 24, 24, cell=TIE_CELL[name])
        f = planted(60, p["p_home"], (4, 9), pw, ph, box=(48, 48))
        out = np.array([[self.cols + 3, 5, 1], [self.cols + 40, 9, 2], [7, self.rows + 1, 3], [11, self.rows + 30, 4], [self.cols, self.rows, 5]])
        add("outside", np.concatenate([f[:20], out, f[20:]]), pw, ph, p_half, 24, 24, cell=(4, 9))
        add("clamp_right", planted(70, p["r_home"], (6, 3), pw, ph, box=(48, 48)), pw, ph, half(p["r_home"]), 24, 24, cell=(6, 3))
        add("clamp_bottom", planted(70, p["b_home"], (2, 11), pw, ph, box=(48, 48)), pw, ph, half(p["b_home"]), 24, 24, cell=(2, 11))
        self.ts = from_pyramids(pyramids, "refine")
        self.nf = np.array([s["nf"] for s in self.specs])
        n = len(self.specs)
        self.feats0 = [self._feats(t, 0) for t in range(n)]
        self.raw1 = self.coarse_raws(self.scene)
        kinds = [s["kind"] for s in self.specs]
        by = lambda *ks: [t for t in range(n) if kinds[t] in ks]  # noqa: E731
        self.groups = {"sat": by("sat"), "planted": by("planted"), "thin": by("thin"), "sweep": by("sweep"),
                       "edges": by("corner", "tie_row", "tie_col", "outside", "clamp_right", "clamp_bottom"), "all": list(range(n))}
        self.thresholds = {g: self._thresholds(g) for g in GROUPS}

    def _feats(self, t, l):
        f = self.ts.feats_of(t, l)
        return np.stack([f["x"], f["y"], f["label"]], axis=1).astype(np.int64)

    def coarse_raws(self, scene):
        T1 = self.T[1]
        return [raw_scores(scene.lm[1], T1, self.W1, self.H1, self.rows // 2, self.cols // 2, int(self.ts.levels[t, 1]["width"]),
                           int(self.ts.levels[t, 1]["height"]), self._feats(t, 1).tolist()) for t in range(len(self.specs))]

    def patch(self, t, gx, gy, scene=None):
        """local[16][16] of template t with the window origin at cell (gx, gy), int64 (similarityLocal :860-922, :986-1048)"""
        scene = scene or self.scene
        key = (t, gx, gy)
        if key not in scene.patches:
            T, W, H, lm = self.T[0], self.W, self.H, scene.lm[0]
            f = self.feats0[t]
            x, y = f[:, 0] + gx * T, f[:, 1] + gy * T
            ok = (x >= 0) & (y >= 0) & (x < self.cols) & (y < self.rows)
            x, y, lab = x[ok], y[ok], f[ok, 2]
            base = ((y % T) * T + x % T) * (W * H) + (y // T) * W + x // T
            out = np.zeros(256, np.int64)
            cell = (np.arange(16)[:, None] * W + np.arange(16)[None, :]).ravel()
            for i in range(0, len(base), 1024):
                idx = base[i: i + 1024, None] + cell[None, :]
                assert idx.max() < lm.shape[1]
                out += lm[lab[i: i + 1024, None], idx].sum(axis=0, dtype=np.int64)
            scene.patches[key] = out.reshape(16, 16)
        return scene.patches[key]

    def candidates(self, t, thr, scene=None, raw1=None):
        """[(x, y, gx, gy, patch, coarse score)] of template t's coarse candidates above thr, at the refinement level"""
        raw1 = self.raw1[t] if raw1 is None else raw1[t]
        T0, T1 = self.T
        lv = self.ts.levels[t]
        sc = score_of(raw1, int(lv[1]["n_features"]))
        out = []
        for j in np.nonzero(sc > np.float32(thr))[0]:
            x, y = refine_origin((j % self.W1) * T1 + offset_of(T1), (j // self.W1) * T1 + offset_of(T1), int(lv[0]["width"]), int(lv[0]["height"]),
                                 self.rows, self.cols, T0)
            gx, gy = x // T0 - 8, y // T0 - 8
            out.append((x, y, gx, gy, self.patch(t, gx, gy, scene), sc[j]))
        return out

    def reference(self, templates, thr, scene=None, raw1=None):
        """the match list of `templates` at thr as sorted int64 rows (as_rows)"""
        refs, key = (scene or self.scene).refs, (tuple(templates), float(thr))
        if key in refs:
            return refs[key]
        T0, off, thr32, rows = self.T[0], offset_of(self.T[0]), np.float32(thr), []
        for t in templates:
            nf = int(self.nf[t])
            for x, y, gx, gy, local, _ in self.candidates(t, thr, scene, raw1):
                best, br, bc = 0, -1, -1
                if local.max() > 0:  # the first maximum in row-major order (argmax returns the first)
                    k = int(local.argmax())
                    best, br, bc = int(local.flat[k]), k // 16, k % 16
                sc = score_of(best, nf)
                if sc < thr32:
                    continue
                rows.append(((gx + bc) * T0 + off, (gy + br) * T0 + off, int(np.asarray(sc, np.float32).view(np.uint32)), best,
                             int(self.ts.class_idx[t]), int(self.ts.template_id[t])))
        a = np.array(rows, np.int64).reshape(-1, 6)
        refs[key] = a[np.lexsort(a.T[::-1])] if len(a) else a
        return refs[key]

    def _thresholds(self, g):
        """[(threshold, name, template or None, raw or None)]: low, high and, for up to three refined candidates of the group
        that score below 100 (smallest, middle and largest feature count), the score itself and one float32 ulp either side"""
        out = [(LOW, "low", None, None), (HIGH, "high", None, None)]
        pick = {}
        for t in self.groups[g]:
            nf = int(self.nf[t])
            for c in self.candidates(t, LOW):
                raw = int(c[4].max())
                s = np.float32(score_of(raw, nf))
                # below 100, kept at LOW, and still a coarse candidate one ulp above its own score
                if 0 < raw < 4 * nf and s >= np.float32(LOW) and c[5] > np.nextafter(s, np.float32(200)) and raw > pick.get(t, 0):
                    pick[t] = raw
        ts = sorted(pick, key=lambda t: (self.nf[t], t))
        for t in dict.fromkeys([ts[0], ts[len(ts) // 2], ts[-1]] if ts else []):
            s = np.float32(score_of(pick[t], int(self.nf[t])))
            for name, v in (("eq", s), ("below", np.nextafter(s, np.float32(0))), ("above", np.nextafter(s, np.float32(200)))):
                out.append((float(v), "%s_of_%d" % (name, self.nf[t]), t, pick[t]))
        return out

    def cases(self):
        return [(g, thr, name) for g in GROUPS for thr, name, _, _ in self.thresholds[g]]


CACHE_ENV = "SBM_REFINE_CASES_CACHE"  # a directory: the parent test leaves its worlds there, references computed, for its children


def _cached(key, make):
    path = os.path.join(os.environ[CACHE_ENV], key + ".pickle") if os.environ.get(CACHE_ENV) else None
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            return pickle.load(f)
    return make()


def save_cache(directory):
    """every world and batched slice, with the patches their references took so far, for processes started with CACHE_ENV"""
    for name in WORLDS:
        with open(os.path.join(directory, "world_%s.pickle" % name), "wb") as f:
            pickle.dump(world(name), f, pickle.HIGHEST_PROTOCOL)
    for name in BATCH:
        with open(os.path.join(directory, "batch_%s.pickle" % name), "wb") as f:
            pickle.dump(batch_slice(name), f, pickle.HIGHEST_PROTOCOL)


@functools.lru_cache(maxsize=None)
def world(name):
    return _cached("world_" + name, lambda: World(name))


# ---- the host rule of enqueue_local, restated ----------------------------------------------------------------------------

def expected_form(name, entry, bits, frames=1, knobs=None, order="auto", depth=1):
    """(kind, LW, order, t8, sparse, slots) of level 0.  entry: "templates" (set_quantized, then match_templates) | "match" (a
    match entry point built the pyramid, frames of them); bits: set_refine_bits; order: set_refine_order; depth:
    set_pipeline_depth; knobs: the SBM_* settings of the process"""
    knobs = knobs or {}
    p = WORLDS[name]
    T, cols = p["T"], p["cols"]
    rows_ok = [T[l] in (4, 8) and ((cols >> l) // T[l]) % 4 == 0 and (cols >> l) % 16 == 0 for l in range(2)]
    full_lm, strip_lm = knobs.get("SBM_FULL_LM", "0") != "0", knobs.get("SBM_STRIP_LM", "1") != "0"
    mode = (1 if bits else 0) if bits is not None else int(knobs.get("SBM_LOCAL_BITS", "1"))
    W0 = cols // T[0]
    wanted = not full_lm and strip_lm and knobs.get("SBM_LM_ALLTY", "1") != "0" and mode != 0 and T[0] == 4 and W0 % 16 == 0
    sparse = 0
    if entry == "templates":  # response planes from set_quantized; ensure_local_forms adds whole bit strips where they are wanted
        kind = 4 if wanted and rows_ok[0] else 1
    elif not all(rows_ok):  # off the one-launch builder's grid: the generic builder's planes, or the any-stride batch builder's spread plane
        kind = 2 if frames > 1 and not full_lm else 1
    elif full_lm:
        kind = 1
    else:
        kind = 4 if wanted else (3 if strip_lm and W0 % 16 == 0 else 2)
        sparse = int(kind == 4 and knobs.get("SBM_SPARSE_STRIPS", "1") != "0")
    waves = int(knobs.get("SBM_LOCAL_WAVES", "0"))
    LW = 1 if kind == 4 else (4 if (waves == 4 if waves else frames >= 4) else 16)
    grid = int(knobs.get("SBM_LOCAL_GRID", "0"))
    slots = grid if grid else (128 if depth >= 2 else 512) * (4 if kind == 4 else 1)
    o = {"auto": int(knobs.get("SBM_LOCAL_ORDER", "0")) if knobs.get("SBM_LOCAL_ORDER") in ("0", "2") else 0, "slots": 0, "list": 2}[order]
    return (kind, LW, o, int(kind == 3 and T[0] == 8), sparse, slots)


# ---- the batched slice ---------------------------------------------------------------------------------------------------

BATCH = {"I48": 8, "I17": 4}  # frames: the world's image, its shifts by multiples of 16 pixels, and an all-zero frame (the last but one)


def batch_templates(w):
    """templates of a few hundred features at the most: eight frames' references stay quick"""
    return [t for t in w.groups["all"] if w.nf[t] <= 300 and w.specs[t]["kind"] in ("sat", "planted", "thin", "sweep", "corner")]


@functools.lru_cache(maxsize=None)
def batch_slice(name):
    return _cached("batch_" + name, lambda: _batch_slice(name))


def _batch_slice(name):
    """(frames [B][rows][cols], per frame (scene, coarse raws), thresholds)"""
    O = oracle_module()
    w = world(name)
    B = BATCH[name]
    frames = np.stack([np.roll(w.img, 16 * (3 * b % 5), axis=1) if b else w.img for b in range(B)])
    frames[B - 2] = 0
    per = []
    for f in frames:
        sc = Scene(O, w.T, img=f)
        per.append((sc, w.coarse_raws(sc)))
    eq = [t for t in w.thresholds["sweep"] if t[1].startswith("eq_")]
    return frames, per, [50.0] + [eq[0][0]] if eq else [50.0]


def run_batch_slice(name, ctx, bits, order, knobs, tag, fail):
    """every threshold of the slice on ctx (templates uploaded): each frame's list against numpy, the record; returns (cases, records, form)"""
    import torch

    w = world(name)
    frames, per, thrs = batch_slice(name)
    idx = batch_templates(w)
    dev = torch.device("cuda", 0)
    B, cap, rec = len(frames), 1 << 14, MATCH_DTYPE.itemsize
    d_img = torch.from_numpy(frames).to(dev)
    d_out = torch.zeros(B * cap * rec, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(B * 2, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    ctx.set_refine_bits(bits)
    ctx.set_refine_order(order)
    ctx.select_templates(idx)
    want_form = expected_form(name, "match", bits, B, knobs, order)
    n_cases = n_recs = 0
    for thr in thrs:
        torch.cuda.synchronize()
        ctx.match_batch_device(d_img.data_ptr(), frames[0].size, B, w.rows, w.cols, w.cols, 1, thr, d_out.data_ptr(), cap, d_cnt.data_ptr(),
                               stream=st.cuda_stream)
        st.synchronize()
        form = ctx.refine_form(0)
        if form != want_form:
            fail((tag, name, "batch", bits, order, thr, "refine_form", want_form, form))
        cnt = d_cnt.cpu().numpy().reshape(B, 2)
        if cnt[:, 1].any() or (cnt[:, 0] > cap).any():
            fail((tag, name, "batch", bits, order, thr, "overflow", 0, cnt.tolist()))
        out = d_out.cpu().numpy().view(MATCH_DTYPE).reshape(B, cap)
        for b in range(B):
            want, got = w.reference(idx, thr, per[b][0], per[b][1]), as_rows(out[b, : cnt[b, 0]])
            d = first_difference(want, got)
            if d:
                fail((tag, name, "batch frame %d" % b, bits, order, thr) + d)
            n_cases += 1
            n_recs += len(want)
    ctx.set_refine_order("auto")
    ctx.select_templates(list(range(w.ts.n_templates)))
    return n_cases, n_recs, want_form


# ---- single frames -------------------------------------------------------------------------------------------------------

def make_context(name):
    from shape_based_matching_amd import capi

    w = world(name)
    ctx = capi.Context(T=w.T, weak_threshold=WEAK_I if w.img is not None else 30.0, device_id=0, max_candidates=MAX_CANDIDATES)
    ctx.upload_templates(w.ts)
    return ctx


def run_world(name, ctx, bits, knobs, tag, fail, groups=GROUPS, depth=1):
    """every (group, threshold) of the world on ctx in one set_refine_bits mode: the list against numpy and the record against the
    host rule; returns (cases, records, form)"""
    w = world(name)
    entry = "templates" if w.img is None else "match"
    ctx.set_refine_bits(bits)
    if entry == "templates":
        for l in range(2):
            ctx.set_quantized(l, w.maps[l])
    want_form = expected_form(name, entry, bits, 1, knobs, depth=depth)
    n_cases = n_recs = 0
    for g in groups:
        ctx.select_templates(w.groups[g])
        for thr, tname, _, _ in w.thresholds[g]:
            got = as_rows(ctx.match_templates(thr) if entry == "templates" else ctx.match(w.img, thr))
            form = ctx.refine_form(0)
            if form != want_form:
                fail((tag, name, g, bits, tname, thr, "refine_form", want_form, form))
            d = first_difference(w.reference(w.groups[g], thr), got)
            if d:
                fail((tag, name, g, bits, tname, thr) + d)
            n_cases += 1
            n_recs += len(got)
    ctx.select_templates(list(range(w.ts.n_templates)))
    return n_cases, n_recs, want_form


# ---- a threshold exactly on the score of an INTERMEDIATE level: three levels, the oracle as the reference ------------------

THREE_T, THREE_NF, THREE_SPOILED = (4, 8, 8), (60, 40, 20), 4


@functools.lru_cache(maxsize=None)
def three_level_case():
    """(maps, templates, thr, want at thr, want one ulp above): synth.stage_b maps with template 0 planted at every level, and
    THREE_SPOILED of its level-1 labels turned by four (they score 0, or what a neighbour's spread gives), so that its candidate's weakest score is the level-1
    one.  thr is the largest float32 threshold at which the oracle still reports the planted record, found by bisection: the
    refined level-1 score itself, kept by >= there and dropped one ulp above while the final score is far higher."""
    O = oracle_module()
    maps, ts = synth.stage_b(31, 512, 512, THREE_T, 12, list(THREE_NF), templ_size=128, plant_every=12)
    o = int(ts.levels[0, 1]["feature_offset"])
    ts.features["label"][o: o + THREE_SPOILED] = (ts.features["label"][o: o + THREE_SPOILED] + 4) % 8
    pyr = O.Pyramid.from_quantized(maps, list(THREE_T))
    match = lambda thr: as_rows(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, float(thr), n_threads=4))  # noqa: E731
    home = match(50.0)
    home = home[(home[:, 5] == 0) & (home[:, 3] == home[home[:, 5] == 0][:, 3].max())][0]
    has = lambda thr: bool(((match(thr)[:, [0, 1, 3, 5]] == home[[0, 1, 3, 5]]).all(axis=1)).any())  # noqa: E731
    lo, hi = np.float32(50.0), np.float32(100.0)  # present at lo, absent at hi: bisect over the float32 bit patterns
    assert has(lo) and not has(hi)
    while int(hi.view(np.uint32)) - int(lo.view(np.uint32)) > 1:
        mid = np.uint32((int(lo.view(np.uint32)) + int(hi.view(np.uint32))) // 2).view(np.float32)
        lo, hi = (mid, hi) if has(mid) else (lo, mid)
    out = (maps, ts, float(lo), match(lo), match(hi), home)
    pyr.free()
    return out


# ---- the worker ----------------------------------------------------------------------------------------------------------

def run_form(form):
    """one knob set in this (fresh) process: CHILD_GROUPS of every world at every threshold in every set_refine_bits mode, then
    the batched slices; prints one JSON line of counts, or raises SystemExit with the first difference"""
    knobs = FORMS[form]
    for k in KNOBS:  # the knobs are read when the library first looks at them: set before it is loaded
        if k in knobs:
            os.environ[k] = knobs[k]
        else:
            os.environ.pop(k, None)
    t0 = time.time()

    def fail(what):
        print("DIFFERENCE " + json.dumps([str(v) for v in what]))
        raise SystemExit(3)

    counts = {"form": form, "cases": 0, "records": 0, "batch_cases": 0, "batch_records": 0, "forms": []}
    seen = set()
    for name in WORLDS:
        ctx = make_context(name)
        for bits in BITS_MODES:
            c, r, f = run_world(name, ctx, bits, knobs, form, fail, groups=CHILD_GROUPS)
            counts["cases"] += c
            counts["records"] += r
            seen.add((name, "single") + f)
        if name in BATCH:
            for bits in (True, False):
                for order in ("slots", "list"):
                    c, r, f = run_batch_slice(name, ctx, bits, order, knobs, form, fail)
                    counts["batch_cases"] += c
                    counts["batch_records"] += r
                    seen.add((name, "batch") + f)
        ctx.close()
    counts["forms"] = sorted(seen)
    counts["seconds"] = round(time.time() - t0, 2)
    print("COUNTS " + json.dumps(counts))


def expected_child_forms(form):
    """the records run_form proves under the knobs of `form`"""
    knobs, out = FORMS[form], set()
    for name, p in WORLDS.items():
        for bits in BITS_MODES:
            out.add((name, "single") + expected_form(name, "templates" if p["kind"] == "maps" else "match", bits, 1, knobs))
        if name in BATCH:
            for bits in (True, False):
                for order in ("slots", "list"):
                    out.add((name, "batch") + expected_form(name, "match", bits, BATCH[name], knobs, order))
    return sorted(out)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--run" or sys.argv[2] not in FORMS:
        raise SystemExit("usage: refine_form_cases.py --run {%s}" % "|".join(FORMS))
    import refine_form_cases  # the module under its own name: the parent's pickled worlds name their classes by it

    refine_form_cases.run_form(sys.argv[2])
