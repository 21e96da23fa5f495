"""CPU (not gpu): the inputs of tests/test_gpu_lm_forms.py (lm_form_cases.py) are what they claim to be, checked with the
oracle and the product's plain headers alone.

  decoders   invert the product's offset functions (csrc/sbm_lm_layout.h, compiled here through tests/emu/lm_layout_emu.cpp) on
             every cell of every world's geometry: random planes encoded by offset decode to themselves
  numpy      np_spread / linear / response, the base of the mutants, equal the oracle's spread, linearize and response maps
  mutants    in every world, at every level and in every frame that holds anything, each mutant that applies changes the
             planes; into the all-zero frame its neighbours leak; in the last frame "into the next frame" is the right answer
  edges      every world has the geometry facts it is listed for, activity in the last grid row and the last strip, frames
             that differ pairwise; every row's expected sbm_get_level_build record is the one plan_build and lm_work
             (csrc/sbm_level_forms.h) give for its geometry, knobs and entry point"""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import any_geometry_cases as AG
import lm_form_cases as LF

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "lm_layout_emu.cpp")
ALL_ROWS = LF.ROWS + [r for rows in LF.CHILD_ROWS.values() for r in rows]
WORLDS = sorted({r["world"] for r in ALL_ROWS})


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("lml_emu") / "liblml_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so, EMU_SRC])
    L = C.CDLL(so)
    L.sbm_emu_lml_strip_offsets.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.sbm_emu_lml_strip_offsets.restype = None
    L.sbm_emu_lml_bits_offsets.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.sbm_emu_lml_bits_offsets.restype = C.c_int64
    L.sbm_emu_lml_any_shape.argtypes = [C.c_int, C.c_void_p]
    L.sbm_emu_lml_any_shape.restype = None
    L.sbm_emu_lml_plan.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]
    L.sbm_emu_lml_plan.restype = None
    return L


def strip_geometries():
    """(T, W, H) of every level of every world that can be held in strips, and a few more heights"""
    out = set()
    for name in WORLDS:
        w = LF.world(name)
        for l in range(w.L):
            W, H = w.geometry(l)
            if W % 16 == 0:
                out.add((w.T[l], W, H))
    return sorted(out | {(4, 16, 1), (4, 32, 15), (8, 48, 31)})


def test_strip_decoder_inverts_the_offset_function(emu):
    rs = np.random.RandomState(3)
    for T, W, H in strip_geometries():
        off = np.zeros(T * T * H * W, np.int64)
        emu.sbm_emu_lml_strip_offsets(T * T, W, H, off.ctypes.data)
        assert sorted(off.tolist()) == list(range(T * T * W * H)), (T, W, H)  # a permutation of the plane: no cell lost, none twice
        data = rs.randint(0, 256, (T * T, H, W)).astype(np.uint8)
        flat = np.full(T * T * W * H + 77, 0xEE, np.uint8)
        flat[off] = data.reshape(-1)
        got, tail = LF.rows_from_strips(flat, T, W, H)
        assert np.array_equal(got, data), (T, W, H)
        assert len(tail) == 77 and (tail == 0xEE).all()
        lin, tail = LF.rows_from_linear(np.concatenate([data.reshape(-1), np.zeros(5, np.uint8)]), T, W, H)
        assert np.array_equal(lin, data) and len(tail) == 5


def test_bit_strip_decoder_inverts_the_offset_function(emu):
    rs = np.random.RandomState(4)
    for T, W, H in strip_geometries():
        if T != 4:
            continue
        S = W // 16
        off = np.zeros(128 * S * H, np.int64)
        n = emu.sbm_emu_lml_bits_offsets(128, W, H, off.ctypes.data)
        assert n == 128 * S * H and sorted(off.tolist()) == list(range(n)), (W, H)
        any_ = rs.randint(0, 2, (16, 8, H, W)).astype(bool)
        exact = rs.randint(0, 2, (16, 8, H, W)).astype(bool)
        # the dword of (plane, strip, gy): bit b = any of cell strip * 16 + b, bit 16 + b = exact
        cells = lambda x: x.reshape(128, H, S, 16).transpose(0, 2, 1, 3).astype(np.uint32)  # noqa: E731
        w16 = (1 << np.arange(16, dtype=np.uint32))
        dwords = (cells(any_) * w16).sum(axis=3, dtype=np.uint32) | ((cells(exact) * w16).sum(axis=3, dtype=np.uint32) << 16)
        flat = np.full(n + 9, 0xA5A5A5A5, np.uint32)
        flat[off] = dwords.reshape(-1)
        a, e, tail = LF.bits_from_strips(flat.view(np.uint8), W, H)
        assert np.array_equal(a, any_) and np.array_equal(e, exact), (W, H)
        assert len(tail) == 36 and (tail.view(np.uint32) == 0xA5A5A5A5).all()


def test_tile_decoder():
    flags = np.array([[1, 0, 1], [0, 0, 1]], np.uint8)
    assert np.array_equal(LF.tiles_from_flags(flags.reshape(-1), 80, 36), flags)
    m = LF.cells_of_tiles(flags, 80, 36)
    assert m.shape == (36, 80) and m[:32, :32].all() and not m[:32, 32:64].any() and m[:, 64:].all() and not m[32:, :64].any()


def test_any_builder_shape_restated(emu):
    out = np.zeros(2, np.int32)
    for T in range(1, 17):
        emu.sbm_emu_lml_any_shape(T, out.ctypes.data)
        assert LF.lma_shape(T) == (int(out[0]), int(out[1])), T


@pytest.mark.parametrize("name", WORLDS)
def test_world(oracle, name):
    """numpy base == oracle; edges; every applicable mutant is caught at every level in every frame"""
    w = LF.world(name)
    dims = [tuple(d) for d in w.dims]
    have = LF.facts(w.T, dims)
    for k, v in w.edges.items():
        assert have[k] == v, (name, k, have[k], v)
    if name in AG.GEOS:
        assert not LF.one_launch(w.T, dims), name  # what sends a batch to k_build_lm_any
    B = w.B
    for a, b in itertools.combinations(range(B), 2):
        for l in range(w.L):
            assert not np.array_equal(w.maps[a][l], w.maps[b][l]), (name, a, b, l)  # frames differ pairwise, at every level
    zero = [f for f in range(B) if not any(m.any() for m in w.maps[f])]
    if w.frames is not None:
        assert len(zero) == 1 and 0 < zero[0] < B - 1, (name, zero)  # one all-zero frame, with a neighbour on either side
    caught = set()
    for l in range(w.L):
        T = w.T[l]
        W, H = w.geometry(l)
        qs = [w.maps[f][l] for f in range(B)]
        labels = set()
        for f in range(B):
            e = w.expect(f, l)
            true = e.planes()
            mine = LF.planes_of(LF.linear(LF.np_spread(qs[f], T), T))
            assert not LF.planes_differ(true, mine), (name, l, f)
            if f in zero:
                for m in LF.ZERO_FRAME_MUTANTS:
                    applies, make = LF.MUTANTS[m]
                    if m == "e_into_next_frame" and not qs[f + 1][: T - 1].any():
                        continue  # (T = 2: the one row behind the frame is the next map's first, which the gradient stage leaves empty)
                    if applies(T, W, H, B, f):
                        assert LF.planes_differ(true, make(qs, f, T)), (name, l, f, m)
                continue
            labels |= set(np.unique(qs[f]).tolist())
            assert e.sp[:, :, W - min(W, 16):].any(), (name, l, f, "nothing in the last strip")
            if T > 1:  # (a stride of 1 has no windows: its grid is the map itself, whose border ring the gradient stage leaves empty)
                assert e.sp[:, H - 1, :].any(), (name, l, f, "nothing in the last grid row")
                assert e.sp[:, :, W - 1].any() and e.sp[:, 0, :].any() and e.sp[:, :, 0].any(), (name, l, f)
            for m, (applies, make) in LF.MUTANTS.items():
                if m == "i_no_last_grid_row" and T == 1:
                    continue
                if m == "e_into_next_frame" and f + 1 < B and not qs[f + 1][: T - 1].any():
                    continue  # (nothing in the rows that lie behind this frame: the all-zero frame follows)
                if applies(T, W, H, B, f):
                    assert LF.planes_differ(true, make(qs, f, T)), (name, l, f, m)
                    caught.add(m)
            if f == B - 1 and B > 1 and T > 1:  # nothing lies behind the last frame: the wrong answer is the right one
                assert not LF.planes_differ(true, LF.planes_of(LF.linear(LF.np_spread(qs[f], T, below=np.zeros_like(qs[f])), T))), (name, l)
        if w.frames is not None:
            assert labels >= {1 << o for o in range(8)}, (name, l, labels)  # all 8 orientations at every level
    assert {"a_window_narrow", "b_window_short", "g_any_of_two", "g_halves_swapped"} <= caught, (name, caught)
    assert "i_no_last_grid_row" in caught or max(w.T) == 1, (name, caught)
    if B > 1:
        assert "h_previous_frame" in caught and ("e_into_next_frame" in caught or max(w.T) == 1), (name, caught)


def test_every_mutant_applies_somewhere():
    """... and the strip and workgroup mutants in the worlds that are there for them"""
    seen = {}
    for name in WORLDS:
        w = LF.world(name)
        for l in range(w.L):
            W, H = w.geometry(l)
            for m, (applies, _) in LF.MUTANTS.items():
                if applies(w.T[l], W, H, w.B, 0):
                    seen.setdefault(m, set()).add((name, l))
    assert set(seen) == set(LF.MUTANTS)
    assert ("i48_144x320", 0) in seen["j_last_strip_left"] and ("i48_144x320", 0) in seen["d_no_halo_32_rows"]
    assert ("i48_272x448", 0) in seen["d_no_halo_32_rows"] and ("m42_132x128", 0) in seen["d_no_halo_32_rows"]
    assert any(n in AG.GEOS for n, _ in seen["c_no_halo_any_cells"]) and any(n in AG.GEOS for n, _ in seen["d_no_halo_any_rows"])


def plan_of(emu, w, r):
    dims = [tuple(d) for d in w.dims]
    geo = np.array([w.L, *w.T, *[d[0] for d in dims], *[d[1] for d in dims]], np.int32)
    kn = dict(LF.KNOB_DEFAULTS)
    kn.update({k: int(v) for k, v in r["knobs"].items()})
    knobs = np.array([kn["SBM_FULL_LM"], kn["SBM_STRIP_LM"], kn["SBM_LM_ALLTY"], kn["SBM_FUSED_BITS"], kn["SBM_LOCAL_BITS"], kn["SBM_SPARSE_STRIPS"]],
                     np.int32)
    one = LF.one_launch(w.T, dims)
    any_batch = not one and r["frames"] > 1 and max(w.T) <= 16
    mode = {"auto": 0, "block": 1}[r["coarse"]]
    refine = -1 if r["bits"] is None else int(r["bits"])
    out = np.zeros(3 * w.L + 1, np.int32)
    emu.sbm_emu_lml_plan(geo.ctypes.data, knobs.ctypes.data, mode, refine, int(one), int(any_batch), 1, r["frames"], out.ctypes.data)
    return one, any_batch, [tuple(int(v) for v in out[3 * l: 3 * l + 3]) for l in range(w.L)], bool(out[3 * w.L])


@pytest.mark.parametrize("rid", [r["id"] for r in ALL_ROWS])
def test_row_expects_what_the_plan_gives(emu, rid):
    """a match entry point's row: form, split and allty per level from plan_build and lm_work, the builder from the geometry, the
    pack from the plan (1) or from the coarse pass on bit planes over response planes (2), the current buffers from the form"""
    r = [x for x in ALL_ROWS if x["id"] == rid][0]
    w = LF.world(r["world"])
    assert len(r["want"]) == w.L and r["frames"] <= w.B and r["edge"]
    if r["entry"] in ("stage", "set"):
        # the stage path is not planned: set_quantized builds the 8 planes with whichever builder takes the level
        for l, want in enumerate(r["want"]):
            rows, cols = w.dims[l]
            T = w.T[l]
            builder = LF.B_ROWS if T in (4, 8) and cols % 16 == 0 and (cols // T) % 4 == 0 else (LF.B_GENERIC if T <= 8 else LF.B_UNFUSED)
            if want[1] == LF.F_PLANES8:
                assert want[2] == builder and want[0] & LF.C_PLANES8, (rid, l)
            else:  # whole strips from ensure_local_forms: a T = 4 level below the coarsest with whole strips of 16 cells
                assert want == LF.STAGE_BITS and T == 4 and l < w.L - 1 and (cols // T) % 16 == 0 and builder == LF.B_ROWS, (rid, l)
        return
    one, any_batch, plan, pack_spread = plan_of(emu, w, r)
    assert one or any_batch, rid
    for l, want in enumerate(r["want"]):
        form, split, allty = plan[l]
        lc = l == w.L - 1
        packed = 1 if lc and pack_spread else (2 if lc and form == LF.F_PLANES8 and r["coarse"] == "auto" else 0)
        cur = {LF.F_PLANES8: LF.C_PLANES8, LF.F_SPREAD: LF.C_SPREAD, LF.F_STRIP: LF.C_SPREAD | LF.C_STRIP, LF.F_BIT_PLANES: LF.C_BIT_PLANES,
               LF.F_BIT_STRIPS: LF.C_BIT_STRIPS, LF.F_SPARSE: 0}[form] | (LF.C_BIT_PLANES if packed else 0)
        assert tuple(want) == (cur, form, LF.B_ROWS if one else LF.B_ANY, split, allty, packed), (rid, l, want, plan[l], pack_spread)


def test_the_table_of_forms_is_covered():
    """every form x builder the issue lists has a row"""
    have = {(want[1], want[2], want[3], want[4], want[5]) for r in ALL_ROWS for want in r["want"]}
    for need in [(LF.F_SPARSE, 1, 1, 1, 0), (LF.F_BIT_STRIPS, 1, 1, 1, 0), (LF.F_STRIP, 1, 1, 1, 0), (LF.F_STRIP, 1, 1, 0, 0), (LF.F_SPREAD, 1, 1, 0, 0),
                 (LF.F_SPREAD, 1, 1, 0, 1), (LF.F_BIT_PLANES, 1, 1, 0, 0), (LF.F_PLANES8, 1, 1, 0, 0), (LF.F_PLANES8, 1, 4, 0, 0), (LF.F_PLANES8, 1, 1, 0, 2),
                 (LF.F_PLANES8, 1, 4, 0, 2), (LF.F_SPREAD, 2, 0, 0, 0), (LF.F_SPREAD, 2, 0, 0, 1), (LF.F_PLANES8, 2, 0, 0, 0), (LF.F_PLANES8, 2, 0, 0, 2),
                 (LF.F_PLANES8, 3, 0, 0, 0), (LF.F_PLANES8, 4, 0, 0, 0)]:
        assert need in have, need
    assert {r["world"] for r in LF.ROWS} >= set(AG.GEOS)
    assert any((c & 3) for n in AG.GEOS for c in [AG.GEOS[n][2]]) and any(not (AG.GEOS[n][2] & 3) for n in AG.GEOS)  # both source loops


@pytest.fixture(scope="module")
def tiles_emu(tmp_path_factory):
    """csrc/sbm_refine_tiles.h as tests/test_refine_tiles.py compiles it: where a candidate's refinement looks, which tiles it reads"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    so = str(tmp_path_factory.mktemp("lml_tiles") / "libtiles_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, os.path.join(ROOT, "tests", "emu", "refine_tiles_emu.cpp")])
    L = C.CDLL(so)
    L.sbm_emu_refine_tiles.argtypes = [C.c_int64, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
    return L


def predicted_flags(tiles_emu, oracle, w, f):
    """the tiles of level 0 that frame f's coarse candidates flag: the oracle's coarse scores above the rows' threshold (a
    candidate at cell (gx, gy) is Match (gx T + T / 2 - 1, gy T + T / 2 - 1) for even T), the product's tile rule"""
    lc, (rows, cols) = w.L - 1, w.dims[0]
    T1, (W, H) = w.T[lc], w.geometry(0)
    pyr = oracle.Pyramid.from_quantized(w.maps[f], list(w.T))
    marks, n_cand = 0, 0
    for t in range(w.ts.n_templates):
        lv = w.ts.levels[t, lc]
        sim = pyr.similarity(lv, w.ts.features, lc)
        ys, xs = np.nonzero(sim.astype(np.float32) * np.float32(100.0) / np.float32(4 * int(lv["n_features"])) > np.float32(LF.THR))
        if len(ys) == 0:
            continue
        off = T1 // 2 + (T1 % 2 - 1)
        box = [int(w.ts.levels[t, 0]["width"]), int(w.ts.levels[t, 0]["height"])]
        cand = np.ascontiguousarray(np.stack([xs * T1 + off, ys * T1 + off, np.full(len(xs), box[0]), np.full(len(xs), box[1])], axis=1), np.int32)
        origin, mask = np.zeros((len(xs), 4), np.int32), np.zeros(len(xs), np.uint64)
        # (cut_templates takes features up to x = width, y = height: one pixel past the declared box)
        assert tiles_emu.sbm_emu_refine_tiles(len(xs), cand.ctypes.data, rows, cols, w.T[0], W, H, 1, origin.ctypes.data, mask.ctypes.data) > 0
        for m in mask:
            marks |= int(m)
        n_cand += len(xs)
    pyr.free()
    shape = ((H + 31) // 32, (W + 31) // 32)
    return n_cand, np.array([(marks >> i) & 1 for i in range(shape[0] * shape[1])]).reshape(shape)


@pytest.mark.parametrize("rid", [r["id"] for r in ALL_ROWS if r["flags"]])
def test_flag_rows_flag_what_they_are_listed_for(tiles_emu, oracle, rid):
    """by the oracle's coarse scores and the product's tile rule (compiled for the CPU), the row's frames flag a tile in the last
    tile row and in the last tile column, and leave one unflagged beside flagged ones: the conditions the GPU test then checks
    on the flags it reads back"""
    r = [x for x in ALL_ROWS if x["id"] == rid][0]
    w = LF.world(r["world"])
    assert tuple(r["want"][0]) == LF.SPARSE and w.L == 2
    flags = []
    for f in r["pick"]:
        n, fl = predicted_flags(tiles_emu, oracle, w, f)
        print("%s frame %d: %d coarse candidates, flags %s" % (rid, f, n, fl.tolist()))
        flags.append(fl)
    LF.check_flags(r, np.stack(flags))
