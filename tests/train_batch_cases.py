"""Inputs shared by the batched-training tests (test_train_select.py and test_reference_train_half.py on the CPU,
test_gpu_train_batch.py and test_gpu_facade_train_batch.py on the GPU): images, their masks, and the oracle's
add_template results (two levels unless asked otherwise), computed once per process and handed out as copies."""
import numpy as np

N_LEVELS = 2
WEAK = 30.0
STRONG = 60.0


def rectangle(rows, cols):
    """background 20, a rectangle of value 220 over the middle half in each direction"""
    img = np.full((rows, cols, 3), 20, np.uint8)
    img[rows // 4: rows // 4 + rows // 2, cols // 4: cols // 4 + cols // 2] = 220
    return img


def left_half(rows, cols):
    m = np.zeros((rows, cols), np.uint8)
    m[:, : cols // 2] = 255
    return m


def cut_edge(rows, cols):
    """everything but a band that cuts through the rectangle's top edge"""
    m = np.full((rows, cols), 255, np.uint8)
    m[rows // 4 - 3: rows // 4 + 4, cols // 2 - 9: cols // 2 + 10] = 0
    return m


def constant(rows, cols):
    return np.full((rows, cols, 3), 77, np.uint8)


def noise(rows, cols, seed):
    return np.random.RandomState(seed).randint(0, 256, (rows, cols, 3)).astype(np.uint8)


def checkerboard(rows, cols, block=8, lo=40, hi=200):
    """two values in blocks of block x block: every block corner and edge is a plateau, with ties along rows and columns"""
    r, c = np.arange(rows)[:, None] // block, np.arange(cols)[None, :] // block
    g = np.where((r + c) % 2 == 0, lo, hi).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def gray(img):
    """the green channel as a single-channel image"""
    return np.ascontiguousarray(img[:, :, 1])


# k_train_resolve gives each of its 64 lanes (cols + 63) / 64 columns: one at 64 columns, two from 65 (with lanes left
# without a column), two at 128, three from 129.  Per width, the seed of a 24-row noise image whose candidates at
# strong_threshold 10 reach the last three scanned columns (cols - 5 .. cols - 3), where the last lanes with work are.
SEGMENT_ROWS = 24
SEGMENT_SEEDS = {64: 4, 65: 2, 128: 2, 129: 3}


def candidates_in_last_columns(oracle, img, strong, n=3):
    """how many level-0 candidates the oracle finds in the last n scanned columns (with every candidate kept)"""
    levels, feats = oracle.add_template(img, None, 1, 100000, WEAK, strong)
    x = feats["x"][: int(levels[0]["n_features"])] + int(levels[0]["tl_x"])
    return int(np.count_nonzero(x >= img.shape[1] - 2 - n))


def nearest_mask(mask):
    """resize(mask, INTER_NEAREST) to half the size (line2Dup.cpp:439), restated"""
    r, c = mask.shape
    dr, dc = r // 2, c // 2
    sy = np.minimum(np.floor(np.arange(dr) * (r / dr)).astype(np.int64), r - 1)
    sx = np.minimum(np.floor(np.arange(dc) * (c / dc)).astype(np.int64), c - 1)
    return np.ascontiguousarray(mask[sy][:, sx])


def s_pairs(mag, strong=STRONG, mask=None):
    """pairs of pixels of S (above strong^2, no strictly larger 5x5 neighbour, inside [2, rows-2) x [2, cols-2), eroded mask)
    within Chebyshev distance 2 of each other"""
    rows, cols = mag.shape
    s = np.zeros((rows, cols), bool)
    core = mag[2:-2, 2:-2]
    ok = core > np.float32(strong) * np.float32(strong)
    for dr in range(-2, 3):
        for dc in range(-2, 3):
            ok &= ~(core < mag[2 + dr: rows - 2 + dr, 2 + dc: cols - 2 + dc])
    if mask is not None:
        p = np.pad(mask, 1, mode="edge")
        er = np.ones((rows, cols), bool)
        for dr in range(3):
            for dc in range(3):
                er &= p[dr: dr + rows, dc: dc + cols] != 0
        ok &= er[2:-2, 2:-2]
    s[2:-2, 2:-2] = ok
    pairs = 0
    for dr in range(0, 3):
        for dc in range(-2, 3):
            if dr == 0 and dc <= 0:
                continue
            a = s[: rows - dr, max(0, -dc): cols - max(0, dc)]
            b = s[dr:, max(0, dc): cols - max(0, -dc)]
            pairs += int(np.count_nonzero(a & b))
    return pairs


_WANT = {}


def want(oracle, img, mask, num_features, strong=STRONG, n_levels=N_LEVELS):
    """oracle.add_template(img, mask), cached by content"""
    key = (img.shape, img.tobytes(), None if mask is None else mask.tobytes(), num_features, float(strong), n_levels)
    if key not in _WANT:
        _WANT[key] = oracle.add_template(img, mask, n_levels, num_features, WEAK, strong)
    res = _WANT[key]
    return None if res is None else (res[0].copy(), res[1].copy())


def counts(want_):
    """features per level"""
    return tuple(int(v) for v in want_[0]["n_features"])


def fixture_roi(case1):
    """the test.cpp ROI, padded as the facade test pads it"""
    roi = case1["train"][110:380, 130:400]
    padded = np.zeros((470, 470, 3), np.uint8)
    padded[100:370, 100:370] = roi
    mask = np.zeros((470, 470), np.uint8)
    mask[100:370, 100:370] = 255
    return padded, mask


def same_template(got, want_):
    """levels and features equal, theta as bits; None where the oracle fails"""
    if want_ is None or got is None:
        return got is None and want_ is None
    (gl, gf), (wl, wf) = got, want_
    for k in ("width", "height", "tl_x", "tl_y", "pyramid_level", "n_features", "feature_offset"):
        if not np.array_equal(np.asarray(gl[k], np.int64), np.asarray(wl[k], np.int64)):
            return False
    if len(gf) != len(wf):
        return False
    return all(np.array_equal(gf[k], wf[k]) for k in ("x", "y", "label")) and np.array_equal(gf["theta"].view(np.uint32), wf["theta"].view(np.uint32))


# ---- tests/golden/ref_train_cases.npz: the reference training half's recorded output (tools/make_fixtures.py --ref-train)
RECORDED_LEVEL_FIELDS = ("width", "height", "tl_x", "tl_y", "pyramid_level", "n_features")


def recorded_cases():
    """name -> (img, mask): the 96 x 96 rectangle under its four masks, and a failing case; two levels, 63 features"""
    img = rectangle(96, 96)
    return {"none": (img, None), "all_set": (img, np.full((96, 96), 255, np.uint8)), "left_half": (img, left_half(96, 96)),
            "cut_edge": (img, cut_edge(96, 96)), "failing": (rectangle(64, 64), left_half(64, 64))}


def pack_recorded(name, result, RT):
    """a ref_train result as the fixture's arrays: levels [L][6] i32, feats [n][4] i32 (theta as bits), failed level or -1"""
    if isinstance(result, RT.Failed):
        return {name + "_failed": np.int32(result.level), name + "_levels": np.zeros((0, 6), np.int32), name + "_feats": np.zeros((0, 4), np.int32)}
    levels, feats = result
    lv = np.stack([levels[k].astype(np.int32) for k in RECORDED_LEVEL_FIELDS], axis=1)
    ft = np.stack([feats["x"], feats["y"], feats["label"], feats["theta"].view(np.int32)], axis=1).astype(np.int32)
    return {name + "_failed": np.int32(-1), name + "_levels": lv, name + "_feats": ft}
