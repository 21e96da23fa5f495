"""CPU (not gpu): the host rules of sbm_upload_templates_device (shape_based_matching_amd/csrc/sbm_install_plan.h and the
numbering of sbm_install_math.h), compiled here for the CPU.  The host never reads a level record or a feature, so the argument
verdict, the flat order of the pyramids, the scratch layout, the sizes of the ten tables, the decoding of the kernels' verdict
words and the numbering of the kept pyramids follow from the call's integers alone."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "install_plan_emu.cpp")
OK, COUNT, NEGATIVE, NULL, SPAN, PYRAMIDS = range(6)
FIELDS = ("n_pyramids", "o_header", "o_table", "o_src_kept", "o_index", "o_items", "o_src_t0", "o_src_base", "total")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("install_plan_emu") / "libinstall_plan_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so, EMU_SRC])
    L = C.CDLL(so)
    L.sbm_emu_install_error.argtypes = [C.c_int]
    L.sbm_emu_install_error.restype = C.c_char_p
    L.sbm_emu_install_table_bytes.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int64]
    L.sbm_emu_install_table_bytes.restype = C.c_int64
    L.sbm_emu_install_level_verdict.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int]
    L.sbm_emu_install_level_verdict.restype = C.c_uint64
    L.sbm_emu_install_where_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p]
    L.sbm_emu_install_where_feature.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_uint32, C.c_void_p]
    L.sbm_emu_install_where_feature.restype = C.c_int64
    L.sbm_emu_install_level_fault.argtypes = [C.c_int32, C.c_int64, C.c_int64]
    L.sbm_emu_install_number.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


class Source(C.Structure):  # sbm_template_source, restated
    _fields_ = [("d_levels", C.c_void_p), ("d_feats", C.c_void_p), ("d_status", C.c_void_p), ("n_pyramids", C.c_int32), ("class_idx", C.c_int32),
                ("feat_first", C.c_int64), ("feat_pitch", C.c_int64), ("feat_cap", C.c_int64)]


def source(n=3, cls=0, first=0, pitch=100, cap=100, levels=0x1000, feats=0x2000, status=None):
    return Source(levels, feats, status, n, cls, first, pitch, cap)


def plan(emu, sources, L=2, n=None):
    n = len(sources) if n is None else n
    arr = (Source * max(len(sources), 1))(*sources)
    fields = np.zeros(len(FIELDS), np.int64)
    firsts = np.zeros(max(n, 1), np.int32)
    where = C.c_int32(-7)
    e = emu.sbm_emu_install_plan(arr, n, L, fields.ctypes.data_as(C.c_void_p), firsts.ctypes.data_as(C.c_void_p), C.byref(where))
    if e:
        return e, where.value
    return dict(zip(FIELDS, (int(v) for v in fields))), [int(v) for v in firsts[:n]]


def test_struct_sizes(emu):
    from shape_based_matching_amd import capi

    assert emu.sbm_emu_sizeof_template_source() == 56 == C.sizeof(Source) == C.sizeof(capi.SbmTemplateSource)
    assert [f[0] for f in capi.SbmTemplateSource._fields_] == [f[0] for f in Source._fields_]
    assert emu.sbm_emu_sizeof_install_source() == 64 and emu.sbm_emu_sizeof_install_item() == 24 and emu.sbm_emu_sizeof_install_header() == 32


def test_flat_order_and_layout(emu):
    """the pyramids of all sources in one flat list, sources without pyramids among them; the sections of the scratch behind each
    other, aligned, each with room for what it holds"""
    counts = [3, 0, 1, 0, 0, 700, 2, 0]
    sums, firsts = plan(emu, [source(n=c, cls=k) for k, c in enumerate(counts)], L=3)
    assert firsts == [int(v) for v in np.cumsum([0] + counts)[:-1]]
    S, P = len(counts), sum(counts)
    assert sums["n_pyramids"] == P
    order = ("o_header", "o_table", "o_src_kept", "o_index", "o_items", "o_src_t0", "o_src_base", "total")
    need = (32, S * 64, S * 4, P * 4, P * 24, S * 4, S * 4)
    assert sums["o_header"] == 0
    for k, nbytes in enumerate(need):
        assert sums[order[k]] % 256 == 0
        assert sums[order[k]] + nbytes <= sums[order[k + 1]], order[k]
    # a call without a pyramid is a plan too
    sums, firsts = plan(emu, [source(n=0), source(n=0)])
    assert sums["n_pyramids"] == 0 and firsts == [0, 0] and sums["total"] > 0


def test_argument_errors_and_where_they_are_reported(emu):
    good = source()

    def err(sources, **kw):
        r = plan(emu, sources, **kw)
        assert isinstance(r[0], int), "no error"
        return r

    assert err([good], n=0) == (COUNT, -1)
    assert err([good], n=-2) == (COUNT, -1)
    assert err([good, source(n=-1)]) == (NEGATIVE, 1)
    assert err([source(first=-1), good]) == (NEGATIVE, 0)
    assert err([good, good, source(pitch=-1)]) == (NEGATIVE, 2)
    assert err([good, source(cap=-1)]) == (NEGATIVE, 1)
    assert err([good, source(levels=None)]) == (NULL, 1)
    assert err([source(feats=None), good]) == (NULL, 0)
    big = (1 << 63) // 16
    assert err([good, source(cap=big)]) == (SPAN, 1)
    assert err([good, source(first=big - 50, cap=100)]) == (SPAN, 1)
    assert err([good, source(n=3, pitch=big // 2, cap=10)]) == (SPAN, 1)
    assert isinstance(plan(emu, [source(n=1, pitch=big * 2, cap=10)])[0], dict)  # one pyramid: the pitch is not used
    assert isinstance(plan(emu, [source(n=2, first=big - 300, pitch=100, cap=100)])[0], dict)
    # more than 2^31 / n_levels pyramids
    most = ((1 << 31) - 1) // 3
    assert isinstance(plan(emu, [source(n=most - 5), source(n=5)], L=3)[0], dict)
    assert err([source(n=most - 5), source(n=5), source(n=0), source(n=1)], L=3) == (PYRAMIDS, 3)
    # what is no error: a source without pyramids needs no addresses, a block without records no feature array; status may be null
    assert isinstance(plan(emu, [source(n=0, levels=None, feats=None), source(cap=0, feats=None), source(status=0x3000)])[0], dict)
    # the first failing rule is the one reported, whatever source it fails on
    worst = source(n=-1, levels=None, feats=None, cap=big)
    assert err([worst], n=0)[0] == COUNT
    assert err([source(levels=None), worst]) == (NEGATIVE, 1)
    assert err([source(cap=big), source(levels=None)]) == (NULL, 1)
    assert err([source(cap=big), source(n=most), source(n=most)], L=3) == (SPAN, 0)
    # every code has a message of its own
    assert emu.sbm_emu_install_errors() == 6
    msgs = [emu.sbm_emu_install_error(e) for e in range(1, 6)]
    assert all(msgs) and len(set(msgs)) == 5
    assert emu.sbm_emu_install_error(OK) == b""


def test_level_record_rule(emu):
    """n_features in 0 .. 8191 first, then [feature_offset, + n_features) inside [0, feat_cap)"""
    f = emu.sbm_emu_install_level_fault
    assert [f(0, 0, 0), f(8191, 0, 8191), f(5, 95, 100), f(0, 100, 100)] == [0, 0, 0, 0]
    assert [f(-1, 0, 100), f(8192, 0, 1 << 40), f(-1, -1, 0)] == [1, 1, 1]
    assert [f(5, -1, 100), f(5, 96, 100), f(1, 0, 0), f(0, 101, 100), f(3, (1 << 62), 100)] == [2, 2, 2, 2, 2]


def test_verdict_words_name_source_pyramid_and_level(emu):
    counts = [3, 0, 1, 0, 700, 2]
    arr = (Source * len(counts))(*[source(n=c) for c in counts])
    firsts = np.cumsum([0] + counts)
    out = np.zeros(4, np.int32)
    for L in (1, 2, 3):
        words = []
        for s, c in enumerate(counts):
            for i in sorted({0, c // 2, c - 1} & set(range(c))):
                for l in range(L):
                    for fault in (1, 2):
                        w = emu.sbm_emu_install_level_verdict(int(firsts[s]) + i, L, l, fault)
                        assert emu.sbm_emu_install_where_level(arr, len(counts), L, w, out.ctypes.data_as(C.c_void_p)) == 0
                        assert out.tolist() == [s, i, l, fault]
                        words.append(w)
        assert words == sorted(words) and len(set(words)) == len(words)  # source order is the order of the words: a minimum finds the first
        assert max(words) < (1 << 64) - 1


def test_feature_verdict_finds_its_level(emu):
    """the installed index of a feature against the running feature offsets, levels without features among them"""
    nfs = [0, 5, 0, 0, 1, 8191, 0, 3, 0]
    offs = np.cumsum([0] + nfs)[:-1].astype(np.int32)
    recs = np.zeros((len(nfs), 4), np.int32)
    recs[:, 2], recs[:, 3] = nfs, offs
    feature = C.c_int32(-1)
    for r, nf in enumerate(nfs):
        for i in sorted({0, nf // 2, nf - 1} & set(range(nf))):
            got = emu.sbm_emu_install_where_feature(recs[:, 3:].ctypes.data_as(C.c_void_p), 4, len(nfs), int(offs[r]) + i, C.byref(feature))
            assert (got, feature.value) == (r, i)


def numbering(kept, cls):
    """the rule restated: kept pyramids are templates 0, 1, ... in order; the id counts the kept pyramids of the class so far"""
    index, classes, ids, seen = [], [], [], {}
    for k, c in zip(kept, cls):
        if not k:
            index.append(-1)
            continue
        index.append(len(classes))
        classes.append(c)
        ids.append(seen.get(c, 0))
        seen[c] = seen.get(c, 0) + 1
    return index, classes, ids


@pytest.mark.parametrize("skip", ["none", "first", "middle", "last", "all"])
def test_numbering_over_two_interleaved_classes(emu, skip):
    """five sources of classes 4, 9, 4, 9, 4 with 3, 2, 4, 1, 3 pyramids: the ids of a class run on across the sources between"""
    counts, classes = [3, 2, 4, 1, 3], [4, 9, 4, 9, 4]
    cls = np.array([c for n, c in zip(counts, classes) for _ in range(n)], np.int32)
    kept = np.ones(len(cls), np.uint8)
    if skip != "none":
        kept[{"first": [0], "middle": [6], "last": [len(cls) - 1], "all": list(range(len(cls)))}[skip]] = 0
    index, c_out, i_out = np.full(len(cls), -7, np.int32), np.full(len(cls), -7, np.int32), np.full(len(cls), -7, np.int32)
    n = emu.sbm_emu_install_number(kept.ctypes.data_as(C.c_void_p), cls.ctypes.data_as(C.c_void_p), len(cls), index.ctypes.data_as(C.c_void_p),
                                   c_out.ctypes.data_as(C.c_void_p), i_out.ctypes.data_as(C.c_void_p))
    want = numbering(kept.tolist(), cls.tolist())
    assert n == len(want[1])
    assert (index.tolist(), c_out[:n].tolist(), i_out[:n].tolist()) == want
    if skip == "none":
        assert i_out[:n].tolist() == [0, 1, 2, 0, 1, 3, 4, 5, 6, 2, 7, 8, 9]


def test_table_sizes(emu):
    f = emu.sbm_emu_install_table_bytes
    assert [f(w, 7, 3, 1000) for w in range(10)] == [7 * 3 * 16, 4000, 1000, 1000, 4000, 1000, 7 * 3 * 17 * 2, 7 * 3 * 4, 28, 28]
    assert [f(w, 0, 2, 0) for w in range(10)] == [0] * 10
    assert f(10, 1, 1, 1) == -1 and f(-1, 1, 1, 1) == -1
