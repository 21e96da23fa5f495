"""Inputs shared by the batched-training tests (test_train_select.py on the CPU, test_gpu_train_batch.py and
test_gpu_facade_train_batch.py on the GPU): BGR images for a two-level pyramid, their masks, and the oracle's
add_template results, computed once per process and handed out as copies."""
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


def want(oracle, img, mask, num_features, strong=STRONG):
    """oracle.add_template(img, mask), cached by content"""
    key = (img.shape, img.tobytes(), None if mask is None else mask.tobytes(), num_features, float(strong))
    if key not in _WANT:
        _WANT[key] = oracle.add_template(img, mask, N_LEVELS, num_features, WEAK, strong)
    res = _WANT[key]
    return None if res is None else (res[0].copy(), res[1].copy())


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
