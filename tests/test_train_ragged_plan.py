"""CPU (not gpu): the host rules of sbm_train_ragged_device (shape_based_matching_amd/csrc/sbm_train_plan.h), compiled here
for the CPU.  The host never reads an image, so the per-image level records, the scratch layout (a running sum over the images),
the grid sizes and the argument verdict follow from the call's integers alone."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "train_ragged_plan_emu.cpp")
OK, COUNT, CHANNELS, GEOMETRY, STRIDE, FEATURES, FEAT_CAP, OVERLAP, NULL_IMAGE = range(9)
REC = ("rows", "cols", "cand_cap", "nf", "pix_off", "cand_off", "sort_off", "img_off", "mask_off", "stride", "feat_first", "feat_cap")
SUMS = ("img_bytes", "pix_elems", "cand_elems", "sort_elems", "o_mag", "o_ori", "o_quant", "o_flags", "o_cand", "o_keys", "o_sel", "o_kept",
        "o_counts", "o_table", "total")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("train_ragged_plan_emu") / "libtrain_ragged_plan_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so, EMU_SRC])
    L = C.CDLL(so)
    L.sbm_emu_train_ragged_error.argtypes = [C.c_int]
    L.sbm_emu_train_ragged_error.restype = C.c_char_p
    L.sbm_emu_train_cand_bound.restype = C.c_int64
    return L


class Image(C.Structure):  # sbm_train_image, restated
    _fields_ = [("img", C.c_void_p), ("mask", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32), ("stride", C.c_int32),
                ("num_features", C.c_int32), ("feat_first", C.c_int64), ("feat_cap", C.c_int64)]


def image(rows, cols, nf=63, first=0, cap=0, ch=3, stride=None, img=0x1000, mask=None):
    return Image(img, mask, rows, cols, cols * ch if stride is None else stride, nf, first, cap)


def plan(emu, images, ch=3, L=2, n=None):
    n = len(images) if n is None else n
    arr = (Image * max(len(images), 1))(*images)
    rec = np.zeros((max(n, 1) * L, len(REC)), np.int64)
    sums = np.zeros(len(SUMS), np.int64)
    grids = np.zeros(9, np.int32)
    where = C.c_int32(-7)
    e = emu.sbm_emu_train_ragged_plan(arr, n, ch, L, rec.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p),
                                      grids.ctypes.data_as(C.c_void_p), C.byref(where))
    if e:
        return e, where.value
    recs = [[dict(zip(REC, (int(v) for v in rec[i * L + l]))) for l in range(L)] for i in range(n)]
    return recs, dict(zip(SUMS, (int(v) for v in sums))), [int(g) for g in grids]


MIXED = [(64, 48), (33, 57), (65, 129), (473, 600), (24, 200), (96, 96), (5, 5), (1, 7)]


def test_struct_sizes(emu):
    assert emu.sbm_emu_sizeof_train_image() == 48 == C.sizeof(Image)
    assert emu.sbm_emu_sizeof_train_scale() == 40
    from shape_based_matching_amd import capi

    assert C.sizeof(capi.SbmTrainImage) == 48 and C.sizeof(capi.SbmTrainScale) == 40
    assert emu.sbm_emu_sizeof_train_record() % 8 == 0  # a table of records keeps its 64-bit fields aligned


@pytest.mark.parametrize("L", [1, 2, 3])
def test_offsets_are_disjoint_and_aligned(emu, L):
    masks = [None, 0x2000, None, 0x2000, 0x2000, None, 0x2000, None]
    recs, sums, _ = plan(emu, [image(r, c, mask=m) for (r, c), m in zip(MIXED, masks)], L=L)
    cand_bytes = emu.sbm_emu_sizeof_train_cand()
    for space, size in (("pix_off", lambda v: v["rows"] * v["cols"]), ("cand_off", lambda v: v["cand_cap"]),
                        ("sort_off", lambda v: 1 << max(v["cand_cap"] - 1, 0).bit_length())):
        spans = sorted((v[space], v[space] + size(v)) for im in recs for v in im if v["rows"])
        assert all(a % 256 == 0 for a, _ in spans)
        assert all(spans[k][1] <= spans[k + 1][0] for k in range(len(spans) - 1)), space
        assert spans[-1][1] <= sums[{"pix_off": "pix_elems", "cand_off": "cand_elems", "sort_off": "sort_elems"}[space]]
    # the level images and masks the engine makes: bytes of the scratch's first section
    spans = []
    for im, m in zip(recs, masks):
        for l, v in enumerate(im):
            assert (v["img_off"] >= 0) == (l > 0 and v["rows"] > 0)
            assert (v["mask_off"] >= 0) == (l > 0 and v["rows"] > 0 and m is not None)
            if v["img_off"] >= 0:
                spans.append((v["img_off"], v["img_off"] + v["rows"] * v["cols"] * 3 + 64))  # the row reads of the gradient stage run on
            if v["mask_off"] >= 0:
                spans.append((v["mask_off"], v["mask_off"] + v["rows"] * v["cols"]))
            assert v["stride"] == (v["cols"] * 3 if l else MIXED[recs.index(im)][1] * 3)
    spans.sort()
    assert all(a % 256 == 0 for a, _ in spans)
    assert all(spans[k][1] <= spans[k + 1][0] for k in range(len(spans) - 1))
    assert not spans or spans[-1][1] <= sums["img_bytes"]
    # the sections behind each other, none overlapping, all aligned
    order = ("o_mag", "o_ori", "o_quant", "o_flags", "o_cand", "o_keys", "o_sel", "o_kept", "o_counts", "o_table", "total")
    need = (sums["pix_elems"] * 4, sums["pix_elems"] * 4, sums["pix_elems"], sums["pix_elems"], sums["cand_elems"] * cand_bytes,
            sums["sort_elems"] * 8, sums["cand_elems"] * 4, sums["cand_elems"] * 4, len(MIXED) * L * 8,
            len(MIXED) * L * emu.sbm_emu_sizeof_train_record())
    assert sums["o_mag"] == sums["img_bytes"]
    for k, nbytes in enumerate(need):
        assert sums[order[k]] % 256 == 0
        assert sums[order[k]] + nbytes <= sums[order[k + 1]], order[k]


@pytest.mark.parametrize("L", [2, 3])
def test_total_is_the_sum_of_the_single_image_plans(emu, L):
    masks = [0x2000, None, None, 0x2000, None, 0x2000, None, 0x2000]
    images = [image(r, c, mask=m) for (r, c), m in zip(MIXED, masks)]
    recs, sums, _ = plan(emu, images, L=L)
    parts = ("img_bytes", "pix_elems", "cand_elems", "sort_elems")
    single = [plan(emu, [im], L=L) for im in images]
    for k in parts:
        assert sums[k] == sum(s[1][k] for s in single), k
    # and every image's records are its single plan's, moved by what lies before it
    before = dict.fromkeys(parts, 0)
    for im, (srecs, ssums, _) in zip(recs, single):
        for v, w in zip(im, srecs[0]):
            for k in ("rows", "cols", "cand_cap", "nf", "stride"):
                assert v[k] == w[k]
            assert v["pix_off"] == w["pix_off"] + before["pix_elems"]
            assert v["cand_off"] == w["cand_off"] + before["cand_elems"]
            assert v["sort_off"] == w["sort_off"] + before["sort_elems"]
            for k in ("img_off", "mask_off"):
                assert v[k] == (w[k] + before["img_bytes"] if w[k] >= 0 else -1)
        for k in parts:
            before[k] += ssums[k]


def test_grids_come_from_the_largest_image(emu):
    small, large = (33, 57), (473, 600)
    want0 = (473 * 600 + 255) // 256
    want1 = (236 * 300 + 255) // 256
    for pos in range(4):
        sizes = [small] * 4
        sizes[pos] = large
        _, _, grids = plan(emu, [image(r, c) for r, c in sizes], L=2)
        assert grids[0] == want0 and grids[1] == 0 and grids[2] == want1, pos
    _, _, grids = plan(emu, [image(3000, 3000), image(40, 40)], L=2)
    assert grids[0] == 4096 and grids[2] == 4096  # the kernels stride over what a grid of 4096 leaves
    _, _, grids = plan(emu, [image(1, 7), image(4, 40)], L=2)
    assert grids[0] == 1 and grids[2] == 0  # nothing built: a grid of one block that finds no pixel, no level step
    _, _, grids = plan(emu, [image(5, 5), image(9, 9)], L=2)
    assert grids[0] == 1 and grids[2] == 0  # 9 x 9 halves to 4 x 4


@pytest.mark.parametrize("L", [2, 3])
def test_too_small_is_not_an_error(emu, L):
    """levels are built while both sides are >= 5; the first smaller level and all after it have rows = 0"""
    built = {(10, 10): 2, (11, 23): 2, (5, 5): 1, (4, 40): 0, (1, 7): 0, (9, 9): 1, (3, 3): 0, (20, 40): 3, (40, 19): 2}
    sizes = list(built)
    recs, sums, _ = plan(emu, [image(r, c, nf=8) for r, c in sizes], L=L)
    for (r, c), im in zip(sizes, recs):
        for l, v in enumerate(im):
            if l < min(built[(r, c)], L):
                assert (v["rows"], v["cols"]) == (r >> l, c >> l)
                assert v["cand_cap"] == emu.sbm_emu_train_cand_bound(r >> l, c >> l) > 0
            else:
                assert (v["rows"], v["cols"], v["cand_cap"]) == (0, 0, 0) and v["img_off"] == -1
            assert v["nf"] == 8 >> l  # a level that is not built still asks for features: no candidate fails it


def test_argument_errors_in_order(emu):
    good = image(64, 48)

    def err(images, **kw):
        r = plan(emu, images, **kw)
        assert isinstance(r[0], int), "no error"
        return r

    assert err([good], n=0) == (COUNT, -1)
    assert err([good], n=-3) == (COUNT, -1)
    assert err([good] * 2, n=65536) == (COUNT, -1)
    assert err([good], ch=2) == (CHANNELS, -1)
    assert err([good], ch=4) == (CHANNELS, -1)
    for r, c in ((0, 48), (64, 0), (-1, 48), (32768, 48), (64, 32768)):
        assert err([good, image(r, c)]) == (GEOMETRY, 1)
    assert err([good, good, image(64, 48, stride=143)]) == (STRIDE, 2)
    assert err([image(64, 48, stride=47, ch=1)], ch=1) == (STRIDE, 0)
    assert err([image(64, 48, nf=0), good]) == (FEATURES, 0)
    assert err([good, image(64, 48, nf=-5)]) == (FEATURES, 1)
    assert err([good, image(64, 48, nf=1)], L=2) == (FEATURES, 1)  # halved to 0 at level 1
    # ... or to ONE: selectScatteredFeatures never returns for one feature (its first candidate is always enough), so a
    # level is asked for two at least
    for L, refused, taken in ((1, 1, 2), (2, 3, 4), (3, 7, 8)):
        assert err([good, image(64, 48, nf=refused)], L=L) == (FEATURES, 1), L
        assert err([good, image(64, 48, nf=refused - 1)], L=L) == (FEATURES, 1), L
        assert isinstance(plan(emu, [good, image(64, 48, nf=taken)], L=L)[0], list), L
    assert err([good, image(64, 48, cap=-1)]) == (FEAT_CAP, 1)
    assert err([good, image(64, 48, first=-1, cap=4)]) == (FEAT_CAP, 1)
    assert err([image(64, 48, first=0, cap=10), image(33, 57, first=9, cap=10)]) == (OVERLAP, 1)
    assert err([image(64, 48, first=20, cap=10), image(33, 57, first=0, cap=5), image(40, 40, first=4, cap=3)]) == (OVERLAP, 2)
    assert err([image(64, 48, first=5, cap=10), image(33, 57, first=5, cap=1)]) == (OVERLAP, 1)
    # blocks that touch, and blocks of no record anywhere, do not overlap
    assert isinstance(plan(emu, [image(64, 48, first=10, cap=10), image(33, 57, first=0, cap=10), image(40, 40, first=15, cap=0)])[0], list)
    assert err([good, image(64, 48, img=None)]) == (NULL_IMAGE, 1)
    # the first failing rule is the one reported, whatever image it fails on
    worst = image(0, 48, nf=0, cap=-1, stride=1, img=None)
    assert err([worst], n=0, ch=2)[0] == COUNT
    assert err([worst], ch=2)[0] == CHANNELS
    assert err([good, worst]) == (GEOMETRY, 1)
    assert err([image(64, 48, nf=0, cap=-1, img=None), image(64, 48, stride=1)]) == (STRIDE, 1)
    assert err([image(64, 48, cap=-1, img=None), image(64, 48, nf=0)]) == (FEATURES, 1)
    assert err([image(64, 48, img=None), image(64, 48, cap=-1)]) == (FEAT_CAP, 1)
    assert err([image(64, 48, img=None, first=0, cap=4), image(64, 48, first=3, cap=4)]) == (OVERLAP, 1)
    # every code has a message of its own
    assert emu.sbm_emu_train_ragged_errors() == 9
    msgs = [emu.sbm_emu_train_ragged_error(e) for e in range(1, 9)]
    assert all(msgs) and len(set(msgs)) == 8
    assert emu.sbm_emu_train_ragged_error(OK) == b""
