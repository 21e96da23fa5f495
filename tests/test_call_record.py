"""CPU (not gpu): what the replay of a captured graph restores of the context's call record
(shape_based_matching_amd/csrc/sbm_call_record.h, CallRecord::replayed), compiled here for the CPU.  A match call's graph
(kind >= 0) leaves the record its capture left, whatever the context held; the template loop's (kind < 0) takes from the
capture only what the loop's own launches note -- the coarse form, the refinement forms, level 0's build where the loop built
it sparsely -- and keeps everything else as the context has it."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "call_record_emu.cpp")

LEVELS, LEVEL_WORDS = 8, 12
BIT_STRIPS, BIT_STRIPS_SPARSE = 4, 5
# the words of a record (tests/emu/call_record_emu.cpp): per level, then the tail
PER_LEVEL = {"forms": slice(0, 1), "level_build": slice(1, 6), "refine_form": slice(6, 12)}
TAIL = {"levels_valid": slice(0, 1), "map0_whole": slice(1, 2), "src0_ch": slice(2, 3), "last_frames": slice(3, 4), "coarse_form": slice(4, 8),
        "source_form": slice(8, 9), "sparse_items": slice(9, 12), "sparse_items_pending": slice(12, 13), "sparse_list": slice(13, 15)}
FIELDS = {(name, l): slice(l * LEVEL_WORDS + s.start, l * LEVEL_WORDS + s.stop) for l in range(LEVELS) for name, s in PER_LEVEL.items()}
FIELDS.update({(name, None): slice(LEVELS * LEVEL_WORDS + s.start, LEVELS * LEVEL_WORDS + s.stop) for name, s in TAIL.items()})
WORDS = LEVELS * LEVEL_WORDS + 15


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("record_emu") / "librecord_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so, EMU_SRC])
    L = C.CDLL(so)
    L.sbm_emu_record_replayed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.sbm_emu_record_replayed.restype = None
    L.sbm_emu_record_begin.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.sbm_emu_record_begin.restype = None
    assert L.sbm_emu_record_words() == WORDS and sorted(i for s in FIELDS.values() for i in range(s.start, s.stop)) == list(range(WORDS))
    return L


def record(base, forms, flag, level0_form=None):
    """a record whose every word is its own value (base + index), the flag sets and booleans as given"""
    r = np.arange(base, base + WORDS, dtype=np.int32)
    for l in range(LEVELS):
        r[FIELDS["forms", l]] = forms
    r[FIELDS["map0_whole", None]] = flag
    r[FIELDS["sparse_items_pending", None]] = flag
    if level0_form is not None:
        r[FIELDS["level_build", 0].start] = level0_form
    return r


def replayed(emu, context, captured, kind):
    out = np.full(WORDS, -7, np.int32)
    emu.sbm_emu_record_replayed(context.ctypes.data, captured.ctypes.data, kind, out.ctypes.data)
    return out


@pytest.mark.parametrize("kind", [0, 2, 3, 16])
def test_a_match_graph_leaves_the_captured_record(emu, kind):
    """kind >= 0 (a single frame, a batch): every field is the captured one, whatever the context held before"""
    captured = record(1000, 0b10101, 0)  # (a captured record never has a count pending: no call is captured while profiling)
    contexts = [record(5000, 0b01010, 1), record(1000, 0b10101, 0), np.zeros(WORDS, np.int32),
                np.random.RandomState(7).randint(-3, 40, WORDS).astype(np.int32)]
    for context in contexts:
        got = replayed(emu, context, captured, kind)
        for (name, l), s in FIELDS.items():
            assert np.array_equal(got[s], captured[s]), (kind, name, l)


@pytest.mark.parametrize("level0_form", [BIT_STRIPS_SPARSE, BIT_STRIPS, 0, -1])
def test_a_template_loop_graph_takes_only_what_the_loop_notes(emu, level0_form):
    """kind < 0, from a context record and a captured record that differ in every field: coarse_form, every level's refine_form
    and -- only where the captured loop built level 0 as sparse bit strips -- level 0's level_build come from the capture;
    every other field, residency and source_form among them, stays the context's"""
    context = record(5000, 0b01010, 1, level0_form=1)
    captured = record(1000, 0b10101, 0, level0_form=level0_form)
    assert (context != captured).all()
    got = replayed(emu, context, captured, -1)
    taken = {("coarse_form", None)} | {("refine_form", l) for l in range(LEVELS)}
    if level0_form == BIT_STRIPS_SPARSE:
        taken.add(("level_build", 0))
    for (name, l), s in FIELDS.items():
        want = captured if (name, l) in taken else context
        assert np.array_equal(got[s], want[s]), (name, l, level0_form)


def test_a_build_begins_with_no_source_pass_and_no_sparse_launch(emu):
    """begin_build, which every pyramid build starts with (the forked single-frame graph's too): the call's frames, no source
    pass, no sparse launch, nothing pending -- and nothing else touched; a fresh record holds nothing"""
    context = record(5000, 0b01010, 1)
    fresh, got = np.full(WORDS, -7, np.int32), np.full(WORDS, -7, np.int32)
    emu.sbm_emu_record_begin(context.ctypes.data, 6, fresh.ctypes.data, got.ctypes.data)
    want = {"last_frames": [6], "source_form": [0], "sparse_items": [0, -1, 0], "sparse_items_pending": [0], "sparse_list": [0, 0]}
    for (name, l), s in FIELDS.items():
        assert got[s].tolist() == (want[name] if name in want else context[s].tolist()), (name, l)
    for (name, l), s in FIELDS.items():
        nothing = {"map0_whole": [1], "last_frames": [1], "level_build": [-1, 0, 0, 0, 0]}.get(name, [0] * (s.stop - s.start))
        assert fresh[s].tolist() == nothing, (name, l)
