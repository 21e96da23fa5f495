"""Inputs shared by the tests that compare with the reference's own match half (test_reference_match_half.py on the CPU,
test_gpu_reference_match.py on the GPU): quantized maps with empty regions and templates that sit on the edges where
line2Dup.cpp's similarity code has corner cases."""
import numpy as np

from shape_based_matching_amd.templates import TemplateSet, from_pyramids

# feature counts: 1; similarity_64 and its boundary (< 64); the HIP counter widths (124 / 1020); the largest admitted
NFS = (1, 63, 64, 65, 124, 125, 1020, 1021, 8191)


def onehot_with_holes(rs, rows, cols, density=0.25, holes=3):
    """rows x cols one-hot orientation map (bit 0..7 where set) with `holes` empty rectangles, one of them on an edge"""
    q = np.where(rs.rand(rows, cols) < density, 1 << rs.randint(0, 8, (rows, cols)), 0).astype(np.uint8)
    for k in range(holes):
        h, w = rs.randint(rows // 8, rows // 3 + 1), rs.randint(cols // 8, cols // 3 + 1)
        y = 0 if k == 0 else rs.randint(0, rows - h + 1)
        x = cols - w if k == 0 else rs.randint(0, cols - w + 1)
        q[y : y + h, x : x + w] = 0
    return q


def _features(rs, nf, w, h, rows, cols, kind, negative):
    """nf features of a w x h template; the first ones sit on the corners that matter"""
    f = np.stack([rs.randint(0, w + 1, nf), rs.randint(0, h + 1, nf), rs.randint(0, 8, nf)], axis=1)
    pins = [(w, rs.randint(0, h + 1)), (rs.randint(0, w + 1), h), (w, h), (0, 0), (w, 0), (0, h)]
    if kind == "outside":
        pins += [(cols, 1), (1, rows), (cols + 5, rows + 5)]
        if negative:  # the reference skips them (its f.x >= 0 check is a CV_DbgAssert); the C ABI refuses them
            pins += [(-1, 3), (2, -1), (-(w + 1), h)]
    for i, (x, y) in enumerate(pins[:nf]):
        f[i, 0], f[i, 1] = x, y
    return f


def edge_specs(cols, rows, T):
    """(name, width, height, nf, kind) of one pyramid level of cols x rows with step T"""
    a = 8 * T  # a multiple of T: features at x == width start one linear-memory cell further than the span assumes
    specs = [(f"nf{nf}", a, a, nf, "inside") for nf in NFS]
    specs += [
        ("odd_size", a + T - 1, a + 1, 70, "inside"),
        ("outside_64", a, a, 40, "outside"),
        ("outside_16", a, a, 300, "outside"),
        ("as_wide", cols, 2 * T, 90, "inside"),
        ("as_high", 2 * T, rows, 30, "inside"),
        ("as_both", cols, rows, 200, "inside"),
        ("wider", cols + T, a, 50, "inside"),
        ("higher", a, rows + 1, 100, "inside"),
        ("one_short", cols - 1, rows - T, 80, "inside"),
    ]
    return specs


def edge_templates(shapes, Ts, seed, negative=True):
    """one pyramid per edge spec over levels of `shapes` [(rows, cols)] with steps `Ts`; each level follows the spec for
    its own size, so the coarse scan and the refinement both see the corner"""
    rs = np.random.RandomState(seed)
    per_level = [edge_specs(c, r, T) for (r, c), T in zip(shapes, Ts)]
    names = [s[0] for s in per_level[0]]
    pyramids = []
    for i in range(len(names)):
        tp = []
        for l, ((r, c), specs) in enumerate(zip(shapes, per_level)):
            _, w, h, nf, kind = specs[i]
            tp.append({"width": w, "height": h, "pyramid_level": l, "features": _features(rs, nf, w, h, r, c, kind, negative)})
        pyramids.append(tp)
    return from_pyramids(pyramids, "edge"), names


def with_classes(ts: TemplateSet, n_classes: int) -> TemplateSet:
    """the same pyramids dealt round-robin into n_classes classes; template_id counts within each class"""
    out = ts.subset(range(ts.n_templates))
    out.class_idx = (np.arange(ts.n_templates) % n_classes).astype(np.int32)
    out.template_id = (np.arange(ts.n_templates) // n_classes).astype(np.int32)
    out.class_ids = [f"class{c}" for c in range(n_classes)]
    return out


def zero_fill_similarity(lm, rows, cols, T, feats, width, height):
    """similarity() with every read past the end of a linear-memory row taken as 0: the model the reference does NOT
    follow (it reads on into the next row of the same continuous Mat).  lm: [8][>= T*T*W*H]."""
    W, H = cols // T, rows // T
    wf, hf = (width - 1) // T + 1, (height - 1) // T + 1
    npos = (H - hf) * W + (W - wf) + 1
    out = np.zeros(H * W, np.int64)
    if npos <= 0:
        return out.reshape(H, W)
    for x, y, lab in feats.tolist():
        if x < 0 or x >= cols or y < 0 or y >= rows:
            continue
        row = lm[lab][((y % T) * T + x % T) * W * H : ((y % T) * T + x % T + 1) * W * H]
        start = (y // T) * W + x // T
        seg = np.zeros(npos, np.int64)
        n = max(0, min(npos, W * H - start))
        seg[:n] = row[start : start + n]
        out[:npos] += seg
    return out.reshape(H, W)
