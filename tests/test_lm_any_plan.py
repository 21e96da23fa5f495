"""CPU (not gpu): the index arithmetic of the batched any-stride linear-memory builder
(shape_based_matching_amd/csrc/sbm_lm_any_plan.h, used by k_build_lm_any and its host side), the plan branch that takes it
(sbm_level_forms.h, PlanInputs::any_batch), and the sequence fuzzer's generator profiles.  The header is compiled here for
the CPU (tests/emu/lm_any_emu.cpp); the reference for orders and contents is the oracle's spread() and linearize()."""
import ctypes as C
import itertools
import json
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "lm_any_emu.cpp")

NONE, PLANES8, SPREAD = -1, 0, 1
B_PLANES8, B_SPREAD, B_STRIP, B_BIT_STRIPS, B_BIT_PLANES = 1, 2, 4, 8, 16
WIDTHS = (1, 3, 4, 17, 33, 64, 75, 153)
HEIGHTS = (1, 2, 9, 13, 25)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("lma_emu") / "liblma_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so, EMU_SRC])
    L = C.CDLL(so)
    L.sbm_emu_lma_shape.argtypes = [C.c_int, C.c_void_p]
    L.sbm_emu_lma_level_blocks.argtypes = [C.c_int] * 3
    L.sbm_emu_lma_block.argtypes = [C.c_int] * 4 + [C.c_void_p]
    L.sbm_emu_lma_find_level.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.sbm_emu_lma_dst.argtypes = [C.c_int] * 5
    L.sbm_emu_lma_dst.restype = C.c_int64
    L.sbm_emu_lma_build.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
    L.sbm_emu_lma_build.restype = C.c_int64
    L.sbm_emu_lma_plan.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]
    L.sbm_emu_lma_plan.restype = C.c_int64
    return L


def shape(emu, T):
    out = np.zeros(4, np.int32)
    emu.sbm_emu_lma_shape(T, out.ctypes.data)
    return [int(v) for v in out]  # cells, grows, LDS bytes, pitch


def test_lds_footprint_and_sizing_rule(emu):
    """every stride 1 .. 16: at most 64 KiB (what a kernel gets without asking), two workgroups in a CU's 160 KiB -- the rule
    keeps four --, cells a multiple of 8 (dword rows in LDS, dword-aligned first pixel column), the footprint restated"""
    for T in range(1, 17):
        cells, grows, lds, pitch = shape(emu, T)
        assert lds <= 64 * 1024 and 2 * lds <= 160 * 1024 and 4 * lds <= 160 * 1024, (T, lds)
        assert cells % 8 == 0 and cells in (64, 32, 16, 8) and grows in (1, 2, 4, 8), (T, cells, grows)
        assert pitch % 4 == 0 and pitch >= cells * T + T - 1
        assert lds == ((grows + 1) * T - 1) * pitch + grows * T * pitch + grows * T * T * cells
    assert shape(emu, 4)[:2] == [64, 8] and shape(emu, 8)[:2] == [64, 2] and shape(emu, 16)[:2] == [32, 1]


def test_blocks_tile_every_grid_exactly_once(emu):
    out = np.zeros(4, np.int32)
    for T in range(1, 17):
        cells, grows = shape(emu, T)[:2]
        for W, H in itertools.product(WIDTHS, HEIGHTS):
            n = emu.sbm_emu_lma_level_blocks(T, W, H)
            seen = np.zeros((H, W), np.int32)
            for blk in range(n):
                emu.sbm_emu_lma_block(T, W, H, blk, out.ctypes.data)
                gx0, nc, gy0, nr = (int(v) for v in out)
                assert 0 < nc <= cells and 0 < nr <= grows and gx0 % cells == 0 and gy0 % grows == 0, (T, W, H, blk)
                assert gx0 + nc <= W and gy0 + nr <= H, (T, W, H, blk)
                seen[gy0: gy0 + nr, gx0: gx0 + nc] += 1
            assert (seen == 1).all(), (T, W, H)


def test_block_ranges_name_their_level(emu):
    begin = np.array([0, 40, 47, 300], np.int32)  # coarsest level first, as the host orders them
    for blk, want in ((0, 0), (39, 0), (40, 1), (46, 1), (47, 2), (299, 2), (300, 3), (100000, 3)):
        assert emu.sbm_emu_lma_find_level(begin.ctypes.data, 4, blk) == want
    shuffled = np.array([47, 0, 300, 40], np.int32)
    for blk, want in ((0, 1), (45, 3), (47, 0), (301, 2)):
        assert emu.sbm_emu_lma_find_level(shuffled.ctypes.data, 4, blk) == want


def test_destinations_are_linearize_order(oracle, emu):
    """the offsets of all (sub-plane, cell) pairs are a permutation of 0 .. T*T*W*H - 1, and cell (gx, gy) of sub-plane
    (ty, tx) lands where oracle.linearize puts pixel (gy*T + ty, gx*T + tx)"""
    for T, W, H in ((1, 17, 3), (2, 33, 5), (3, 8, 16), (4, 17, 13), (5, 3, 16), (8, 75, 2), (16, 3, 1), (7, 16, 16)):
        rows, cols = H * T, W * T
        pix = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
        lin = sum(oracle.linearize(((pix >> (8 * k)) & 255).astype(np.uint8), T).astype(np.int64).reshape(-1)[: rows * cols] << (8 * k) for k in range(3))
        where = np.empty(rows * cols, np.int64)  # pixel index -> offset in the linear memory
        where[lin] = np.arange(rows * cols)
        got = np.array([[[emu.sbm_emu_lma_dst(sub, gy, gx, W, H) for gx in range(W)] for gy in range(H)] for sub in range(T * T)])
        assert sorted(got.reshape(-1).tolist()) == list(range(T * T * W * H)), (T, W, H)
        for sub in range(T * T):
            ty, tx = divmod(sub, T)
            assert np.array_equal(got[sub], where[pix[ty::T, tx::T]]), (T, W, H, sub)


def build_cases():
    rs = np.random.RandomState(5)
    for T in range(1, 17):
        for W, H in ((1, 16), (3, 16), (17, 13), (33, 5), (75, 2), (153, 1), (64, 9), (4, 4)):
            rows, cols = H * T, W * T
            if rows * cols % 16:  # the reference's third condition (computeResponseMaps)
                rows, cols, H = rows * 16, cols, H * 16
                if rows * cols > 600000:
                    continue
            q = (1 << rs.randint(0, 8, (rows, cols))).astype(np.uint8)
            q[rs.randint(0, 100, (rows, cols)) < 90] = 0
            q[-1, -1] = 0x80  # the clipped window's corner
            q[-1, 0] = 0x01
            yield T, rows, cols, q


def test_walk_of_a_level_stores_every_byte_once_and_nothing_else(oracle, emu):
    """the kernel's walk restated on the header (lm_any_emu.cpp): the spread bytes in linear-memory order equal
    linearize(spread(q)), every byte of T*T*W*H is stored exactly once, nothing lands in the zero tail, no LDS index
    leaves the footprint, every piece is an aligned dword"""
    n = 0
    for T, rows, cols, q in build_cases():
        size = rows * cols
        tail = 64
        out = np.full(size + tail, 0x5A, np.uint8)
        hits = np.zeros(size + tail, np.int32)
        bad = emu.sbm_emu_lma_build(q.ctypes.data, rows, cols, T, out.ctypes.data, hits.ctypes.data, size + tail)
        assert bad == 0, (T, rows, cols, bad)
        assert (hits[:size] == 1).all() and (hits[size:] == 0).all() and (out[size:] == 0x5A).all(), (T, rows, cols)
        want = oracle.linearize(oracle.spread(q, T), T).reshape(-1)[:size]
        assert np.array_equal(out[:size], want), (T, rows, cols, np.argwhere(out[:size] != want)[:5])
        n += 1
    assert n >= 100


def plan(emu, Ts, rows0, cols0, full_lm, fused, mode, thr_state, has_spread, any_batch, match, empty):
    L = len(Ts)
    geo = np.array([L, *Ts, *[rows0 >> l for l in range(L)], *[cols0 >> l for l in range(L)]], np.int32)
    knobs = np.array([full_lm, fused], np.int32)
    out = np.zeros(3 * L + 2, np.int32)
    sig = emu.sbm_emu_lma_plan(geo.ctypes.data, knobs.ctypes.data, mode, thr_state, has_spread, any_batch, match, empty, out.ctypes.data)
    return ([int(out[3 * l]) for l in range(L)], [int(out[3 * l + 1]) for l in range(L)], [int(out[3 * l + 2]) for l in range(L)],
            bool(out[3 * L]), bool(out[3 * L + 1]), sig)


def test_plan_of_a_batch_through_the_any_stride_builder(emu):
    """refinement levels as one plane of spread bytes, the coarsest level the same plus the pack launch where the coarse pass
    runs on bit planes, else -- and everywhere under SBM_FULL_LM -- the 8 response planes; never strips, bit strips, a sparse
    level 0 or fused bit planes; the record says what the launches left and its signature tells the outcomes apart; without
    the flag the plan is today's (8 planes everywhere)"""
    by_sig = {}
    n = 0
    for Ts, (rows0, cols0) in (((4, 8), (208, 272)), ((5, 8), (240, 320)), ((2, 4), (200, 264)), ((4, 8, 8), (384, 416)), ((1,), (208, 211)),
                               ((8, 16), (256, 288)), ((4, 8), (1024, 1024))):
        L, lc = len(Ts), len(Ts) - 1
        for full_lm, fused, mode, thr_state, has_spread, match, empty in itertools.product((0, 1), (1, 0), (0, 3, 4), (0, 1, 2), (1, 0), (1, 0), (0, 1)):
            if (match and thr_state == 0) or (not match and empty):
                continue
            form, bits, reads, pack, sparse_grad, sig = plan(emu, Ts, rows0, cols0, full_lm, fused, mode, thr_state, has_spread, 1, match, empty)
            case = (Ts, full_lm, fused, mode, thr_state, has_spread, match, empty)
            n += 1
            on_bits = mode in (0, 3) and thr_state == 2
            assert not sparse_grad and set(form) <= {PLANES8, SPREAD}, case
            for l in range(lc):
                assert form[l] == (SPREAD if has_spread and not full_lm else PLANES8), case
                assert reads[l] == form[l] and bits[l] == (B_SPREAD if form[l] == SPREAD else B_PLANES8), case
            want_pack = bool(match and on_bits and fused and has_spread and not full_lm)
            assert pack == want_pack and form[lc] == (SPREAD if want_pack else PLANES8), case
            want_bits = (B_SPREAD if want_pack else B_PLANES8) | (B_BIT_PLANES if want_pack or (match and on_bits and not empty) else 0)
            assert bits[lc] == want_bits, case
            if match and not empty:
                assert bits[lc] & (B_BIT_PLANES if on_bits else B_PLANES8), case  # the coarse pass's operand is current
            readers = (tuple(reads[:lc]), bits[lc])
            assert by_sig.setdefault((L, sig), readers) == readers, case
            # without the flag: today's plan for a pyramid off the one-launch builder's grid
            form0, bits0, _, pack0, _, _ = plan(emu, Ts, rows0, cols0, full_lm, fused, mode, thr_state, has_spread, 0, match, empty)
            assert form0 == [PLANES8] * L and not pack0 and all(b & ~B_BIT_PLANES == B_PLANES8 for b in bits0), case
    assert n > 500
    # the three outcomes at the coarsest level, and spread against planes at a refinement level, have different signatures
    sigs = {plan(emu, (4, 8), 208, 272, *k)[5] for k in ((0, 1, 0, 2, 1, 1, 1, 0), (0, 1, 0, 1, 1, 1, 1, 0), (1, 1, 0, 2, 1, 1, 1, 0), (1, 1, 0, 1, 1, 1, 1, 0))}
    assert len(sigs) == 4


# digests of generate(seed, index, steps, profile) taken on the commit before the "anygeo" profile was added
GENERATOR_DIGESTS = {("default", 1, 0, 25): 3602548322, ("default", 1, 5, 25): 3121649287, ("default", 7, 2, 40): 275590922,
                     ("default", 12345, 11, 12): 2429647069, ("sparse", 1, 0, 25): 2225508954, ("sparse", 1, 5, 25): 1603272282,
                     ("sparse", 7, 2, 40): 2900385535, ("sparse", 12345, 11, 12): 1790139860}


def test_generator_profiles():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_sequence as F

    def digest(T, ops):
        return zlib.crc32(json.dumps([list(T), ops], sort_keys=True).encode())

    for (profile, seed, index, steps), want in GENERATOR_DIGESTS.items():
        assert digest(*F.generate(seed, index, steps, profile)) == want, (profile, seed, index, steps)
    seen_T, seen_ops, seen_geo = set(), set(), set()
    for seed, index in itertools.product((1, 3), range(24)):
        T, ops = F.generate(seed, index, 30, "anygeo")
        assert (T, ops) == F.generate(seed, index, 30, "anygeo") and len(ops) == 30
        seen_T.add(tuple(T))
        for op in ops:
            seen_ops.add(op["op"])
            if "geo" in op:
                rows, cols, _ = F.ALL_GEOS[op["geo"]]
                seen_geo.add(op["geo"])
                assert op["geo"] in F.ANYGEO_GEOS[tuple(T)]
                for l, t in enumerate(T):  # the reference's three conditions hold at every level
                    r, c = rows >> l, cols >> l
                    assert r % t == 0 and c % t == 0 and r * c % 16 == 0, (T, op["geo"], l)
            assert op["op"] != "match_banded"
    assert seen_T == set(F.ANYGEO_PYRAMIDS) == {(4, 8), (2, 4), (5, 8), (4, 8, 8), (1,)}
    assert {"match_batch_device", "match_batch_host", "nms", "get_quantized_frame", "get_coarse_bitplanes", "match_templates"} <= seen_ops
    assert "O" in seen_geo and len(seen_geo) >= 8
