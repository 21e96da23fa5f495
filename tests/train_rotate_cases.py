"""Inputs shared by the rotation tests (test_rotate_math.py on the CPU, test_gpu_train_rotate.py on the GPU): trained
bases made by hand so that they sit on the edges of Detector::addTemplate_rotate's rule (line2Dup.cpp:1395-1451), the
angles and centres they are rotated with, and the oracle's add_template_rotate results, computed once per process and
handed out as copies.  A case is (name, base, centre, thetas); a base is (levels, feats) in the oracle's dtypes, as the
training calls write them: features relative to the level's tl, feature_offset packed."""
import numpy as np

ANGLES = [0.0, 1e-3, -1e-3, 360.0, -360.0, 720.5, -36000.0, 36000.0]
QUARTERS = [90.0, 180.0, 270.0]


def base_from_points(per_level):
    """per_level[l]: rows of (x, y, theta) in level l's own coordinates (x, y >= 0).  Cropped as cropTemplates crops."""
    from oracle.oracle import LEVEL_DTYPE, TRAIN_FEATURE_DTYPE

    pts = [np.asarray(p, np.float64).reshape(-1, 3) for p in per_level]
    xs = np.concatenate([p[:, 0].astype(np.int64) << l for l, p in enumerate(pts)])
    ys = np.concatenate([p[:, 1].astype(np.int64) << l for l, p in enumerate(pts)])
    min_x, min_y = int(xs.min()), int(ys.min())
    min_x -= min_x % 2
    min_y -= min_y % 2
    levels = np.zeros(len(pts), LEVEL_DTYPE)
    feats = np.zeros(sum(len(p) for p in pts), TRAIN_FEATURE_DTYPE)
    off = 0
    for l, p in enumerate(pts):
        n = len(p)
        levels[l] = ((int(xs.max()) - min_x) >> l, (int(ys.max()) - min_y) >> l, min_x >> l, min_y >> l, l, n, off)
        feats["x"][off: off + n] = p[:, 0].astype(np.int64) - (min_x >> l)
        feats["y"][off: off + n] = p[:, 1].astype(np.int64) - (min_y >> l)
        feats["theta"][off: off + n] = p[:, 2].astype(np.float32)
        feats["label"][off: off + n] = (np.floor(p[:, 2] * 16 / 360 + 0.5).astype(np.int64)) & 7
        off += n
    return levels, feats


def random_base(counts, seed, extent=400):
    """counts[l] features at level l, scattered over [0, extent >> l)^2, orientations over [0, 360)"""
    rs = np.random.RandomState(seed)
    per_level = []
    for l, n in enumerate(counts):
        e = max(extent >> l, 4)
        per_level.append(np.stack([rs.randint(0, e, n), rs.randint(0, e, n), rs.uniform(0, 360, n).astype(np.float32)], axis=1) if n else np.zeros((0, 3)))
    return base_from_points(per_level)


def _ulp_thetas():
    """every k * 22.5 and every label boundary (k + 0.5) * 22.5, each one float ulp below, exact, and one above"""
    out = []
    for k in range(0, 33):
        v = np.float32(k * 11.25)
        out += [np.nextafter(v, np.float32(-1e9)), v, np.nextafter(v, np.float32(1e9))]
    return [float(t) for t in out]


def negative_cases():
    """a half turn about a centre left of / above the features: x' = 2 cx - x.  Level-0 features at x in {2, 6}: cx = -1
    makes x' in {-4, -8}, which int(x' + 0.5f) truncates to {-3, -7}, an odd negative minimum; cx = 20 gives an even
    positive one; y likewise."""
    pts0 = [(2, 2, 10.0), (6, 6, 100.0), (2, 6, 200.0)]
    pts1 = [(1, 1, 300.0), (2, 2, 45.0)]
    base = base_from_points([pts0, pts1])
    return [("neg_x_only", base, (-1.0, 20.0), [180.0]), ("neg_y_only", base, (20.0, -1.0), [180.0]), ("neg_both", base, (-1.0, -1.0), [180.0, 135.0, 225.0])]


def tie_cases():
    """quarter turns about half-integer centres: a rotated coordinate lands on k + 0.5, on either side of zero"""
    pts0 = [(0, 0, 0.0), (3, 1, 90.0), (7, 12, 180.0), (20, 4, 270.0), (11, 8, 359.5)]
    pts1 = [(0, 0, 22.5), (5, 6, 337.5), (10, 2, 11.25)]
    base = base_from_points([pts0, pts1])
    return [(f"tie_{cx}_{cy}", base, (cx, cy), QUARTERS) for cx, cy in ((10.5, 7.0), (10.0, 7.5), (10.5, 7.5), (-3.5, 2.0), (0.5, -0.5), (21.0, 15.0))]


def theta_cases():
    """f.theta - theta exactly 0 and exactly 360, and as far out as the domain goes; the label at its boundaries"""
    pts = [(4, 4, 90.0), (6, 9, 360.0), (9, 6, 0.0), (12, 3, 720.0), (3, 12, -720.0), (8, 8, 450.0), (5, 7, -0.0)]
    edges = base_from_points([pts, [(2, 2, 720.0), (4, 3, -720.0)]])
    ulps = base_from_points([[(k % 17, k // 17, t) for k, t in enumerate(_ulp_thetas())], [(1, 1, 5.0)]])
    return [("theta_edges", edges, (8.0, 8.0), [90.0, 0.0, 360.0, -270.0, 450.0, -36000.0, 36000.0, 720.0, -720.0]),
            ("theta_ulps", ulps, (8.0, 3.0), [0.0, 22.5, -22.5, 360.0])]


def angle_cases():
    return [("angles", random_base((40, 17), 1), (200.0, 200.0), ANGLES)]


def level_cases():
    """one, two and three pyramid levels"""
    return [("levels_1", random_base((33,), 2), (100.25, 37.0), [17.0, 180.0]), ("levels_2", random_base((33, 9), 3), (100.25, 37.0), [17.0, 180.0]),
            ("levels_3", random_base((33, 9, 5), 4), (100.25, 37.0), [17.0, 180.0, -45.5])]


def cpu_cases():
    return negative_cases() + tie_cases() + theta_cases() + angle_cases() + level_cases()


# feature counts at wave and workgroup edges (level 0, with a short level 1), and an empty level beside a filled one
COUNT_EDGES = [(1, 1), (63, 2), (64, 0), (65, 3), (255, 64), (256, 65), (257, 1), (8191, 2047), (0, 5)]


def count_cases():
    return [(f"count_{a}_{b}", random_base((a, b), 100 + i, extent=2000), (1000.0 + i, 990.5), [33.0]) for i, (a, b) in enumerate(COUNT_EDGES)]


_WANT = {}


def want(oracle, base, theta, center):
    """oracle.add_template_rotate, cached by content"""
    levels, feats = base
    key = (levels.tobytes(), feats.tobytes(), float(np.float32(theta)), float(np.float32(center[0])), float(np.float32(center[1])))
    if key not in _WANT:
        _WANT[key] = oracle.add_template_rotate(levels, feats, float(theta), (float(center[0]), float(center[1])))
    res = _WANT[key]
    return res[0].copy(), res[1].copy()


def same_pair(got, want_):
    """level records and features equal, theta as bits"""
    (gl, gf), (wl, wf) = got, want_
    for k in ("width", "height", "tl_x", "tl_y", "pyramid_level", "n_features", "feature_offset"):
        if not np.array_equal(np.asarray(gl[k], np.int64), np.asarray(wl[k], np.int64)):
            return False
    if len(gf) != len(wf):
        return False
    return all(np.array_equal(gf[k], wf[k]) for k in ("x", "y", "label")) and np.array_equal(gf["theta"].view(np.uint32), wf["theta"].view(np.uint32))
