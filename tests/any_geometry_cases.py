"""Shared inputs of the any-geometry batch tests (test_gpu_batch_any_geometry.py): pyramids and frame geometries that
the one-launch linear-memory builder does not take -- a stride other than 4 or 8, or a level whose width is no multiple of
16 -- with frames, templates cut from frame 0's own orientation maps, and the CPU oracle's answers, computed once per case
and kept read-only."""
import numpy as np

from shape_based_matching_amd import synth
from shape_based_matching_amd.templates import MATCH_DTYPE

WEAK = 30.0
THRS = (60.0, 85.0)
N_TEMPLATES = 8

# name -> (T, rows, cols, channels, nf per level, template box): why each is here
GEOS = {
    "bgr_4_8": ((4, 8), 208, 272, 3, [48, 24], 64),        # level 1 is 136 columns (136 % 16 == 8), W1 = 17 odd, W1 * H1 = 221
    "gray_4_8": ((4, 8), 208, 272, 1, [48, 24], 64),       # the same, gray: the per-frame masks' case
    "bgr_5_8": ((5, 8), 240, 320, 3, [48, 24], 64),        # a stride that is not 4 or 8 on a refinement level
    "gray_2_4": ((2, 4), 200, 264, 1, [48, 24], 64),       # small strides, W1 = 33, H1 = 25
    "bgr_4_8_8": ((4, 8, 8), 384, 416, 3, [80, 40, 20], 128),  # three levels, only the coarsest unaligned (104 columns)
    "bgr_4_4_8": ((4, 4, 8), 256, 288, 3, [60, 30, 16], 96),   # candidates pass through a middle level
    "gray_1": ((1,), 208, 211, 1, [40], 64),               # single level, odd width, map rows start on any byte
    "bgr_8_16": ((8, 16), 256, 288, 3, [48, 20], 96),      # the largest stride the batched builder takes
}


def multiset(recs):
    return sorted(np.ascontiguousarray(recs, MATCH_DTYPE).tolist())


def packed(lm):
    """[8][stride] response bytes -> [16][stride / 8] bit planes, little-endian bit order (as test_gpu_coarse_bits.py)"""
    return np.concatenate([np.packbits(lm > 0, axis=1, bitorder="little"), np.packbits(lm == 4, axis=1, bitorder="little")])


def make_frames(rows, cols, ch, n=5):
    """the scene, two rolled copies (so that lists differ between frames), an all-zero frame, a scene of another seed"""
    scene = synth.scene_bgr if ch == 3 else synth.scene_gray
    base = scene(7, rows, cols, n_shapes=36)
    frames = [base, np.roll(base, 12, axis=1), np.roll(np.roll(base, 8, axis=0), -20, axis=1), np.zeros_like(base), scene(19, rows, cols, n_shapes=30)]
    return np.ascontiguousarray(np.stack(frames[:n]))


class Case:
    """frames [5], templates, and per (frame, threshold) the oracle's list; maps and linear memories on request"""

    def __init__(self, oracle, name):
        self.oracle = oracle
        self.name = name
        self.T, self.rows, self.cols, self.ch, nf, box = GEOS[name]
        self.L = len(self.T)
        self.frames = make_frames(self.rows, self.cols, self.ch)
        self.frames.setflags(write=False)
        pyr0 = oracle.Pyramid.build(self.frames[0], list(self.T), WEAK)
        self.ts, got = synth.templates_from_maps([pyr0.quantized(l) for l in range(self.L)], nf, box, N_TEMPLATES, 11)
        assert min(got) >= 8, (name, got)
        pyr0.free()
        self._want = {}
        self._maps = {}

    def pyramid(self, f, mask=None):
        return self.oracle.Pyramid.build(self.frames[f], list(self.T), WEAK, mask)

    def want(self, f, thr):
        if (f, thr) not in self._want:
            pyr = self.pyramid(f)
            ts = self.ts
            for t in sorted(set(THRS) | {thr}):
                self._want[(f, t)] = multiset(pyr.match(ts.levels, ts.features, ts.class_idx, ts.template_id, t))
            self._maps[f] = [pyr.quantized(l) for l in range(self.L)]
            pyr.free()
        return self._want[(f, thr)]

    def maps(self, f):
        self.want(f, THRS[0])
        return self._maps[f]

    def check_not_empty(self, n, thr):
        assert sum(len(self.want(f, thr)) for f in range(n)) > 0, (self.name, thr)


_cases = {}


def case(oracle, name):
    if name not in _cases:
        _cases[name] = Case(oracle, name)
    return _cases[name]
