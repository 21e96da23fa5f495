"""Shared inputs of the per-frame-mask tests (test_emu_quantize_stream_masks.py, test_gpu_frame_masks.py): frames with
oriented edges everywhere, the mask classes, and the oracle's maps, computed once per case and never modified.

The reference is always ``oracle.Pyramid.build(frame, T, weak, mask=masks[f])``, frame by frame: the mask belongs to one
match() call (line2Dup.cpp:1078), quantize() applies it at every level (:446-450) and pyrDown() resizes it with
nearest-neighbour sampling (:439)."""
import numpy as np

WEAK = 30.0


def textured_frames(seed, n, rows, cols, ch):
    """n frames of 4 x 4 blocks of random grey levels (edges of one orientation along every block side, so the 3x3 vote
    passes all over the frame) plus noise in [0, 2]"""
    rs = np.random.RandomState(seed)
    shape = (n, (rows + 3) // 4, (cols + 3) // 4) + ((3,) if ch == 3 else ())
    low = rs.randint(0, 254, shape)
    up = np.repeat(np.repeat(low, 4, axis=1), 4, axis=2)[:, :rows, :cols]
    return np.ascontiguousarray(up + rs.randint(0, 3, up.shape), np.uint8)


def noise_mask(rs, rows, cols):
    """arbitrary values; the rule is `!= 0` (1 and 128 keep a pixel as 255 does)"""
    vals = np.array([0, 0, 0, 1, 128, 255, 7, 64], np.uint8)
    m = vals[rs.randint(0, len(vals), (rows, cols))]
    m.flat[rs.randint(0, m.size, 8)] = 1
    m.flat[rs.randint(0, m.size, 8)] = 128
    return m


def rect_mask(rs, rows, cols, n_rects=3):
    m = np.zeros((rows, cols), np.uint8)
    for _ in range(n_rects):
        h, w = rs.randint(rows // 4 + 1, rows + 1), rs.randint(cols // 8 + 1, cols // 2 + 1)
        y, x = rs.randint(0, rows - h + 1), rs.randint(0, cols - w + 1)
        m[y:y + h, x:x + w] = rs.choice([255, 1, 128, 200])
    return m


def frame_masks(seed, n, rows, cols, full_at=2):
    """one mask per frame: noise (even frames) and rectangles (odd frames), frame 1 all zero and -- where the batch has
    more than three frames -- frame `full_at` all 255: inside the first group of a packed wave"""
    rs = np.random.RandomState(seed)
    masks = np.stack([noise_mask(rs, rows, cols) if f % 2 == 0 else rect_mask(rs, rows, cols) for f in range(n)])
    masks[1] = 0
    if n > 3:
        masks[full_at] = 255
    return masks


def strided(masks, seed=99):
    """the masks at a stride of two masks, garbage in between: (buffer, stride in bytes)"""
    n, rows, cols = masks.shape
    buf = np.random.RandomState(seed).randint(0, 256, (2 * n, rows, cols)).astype(np.uint8)
    buf[0::2] = masks
    return buf, 2 * rows * cols


def pyramid_T(rows, cols):
    """[4, 8] where the reference's preconditions hold at both levels (line2Dup.cpp:639, :751-752), else level 0 alone"""
    r1, c1 = rows // 2, cols // 2
    ok = rows % 4 == 0 and cols % 4 == 0 and r1 % 8 == 0 and c1 % 8 == 0 and (r1 * c1) % 16 == 0
    return [4, 8] if ok else [4]


def oracle_maps(oracle, frames, masks, T):
    """[frame][level] one-hot maps of Pyramid.build(frame, T, WEAK, mask); masks None = unmasked"""
    out = []
    for f in range(len(frames)):
        p = oracle.Pyramid.build(frames[f], T, WEAK, mask=None if masks is None else masks[f])
        out.append([p.quantized(l) for l in range(len(T))])
        p.free()
    return out


def assert_masks_matter(oracle, frames, masks, T):
    """On the oracle alone: the masked maps of at least two frames differ from their unmasked maps and are not empty (a
    test on masks that change nothing, or wipe everything, would show nothing).  Returns the masked maps."""
    want = oracle_maps(oracle, frames, masks, T)
    plain = oracle_maps(oracle, frames, None, T)
    telling = [f for f in range(len(frames)) if want[f][0].any() and not np.array_equal(want[f][0], plain[f][0])]
    assert len(telling) >= 2, telling
    for w in want:
        for q in w:
            q.setflags(write=False)
    return want
