"""CPU (not gpu): the per-level record of current linear-memory forms, the build plan and the reader choice of the host side
(shape_based_matching_amd/csrc/sbm_level_forms.h), compiled here for the CPU.  Every combination of pyramid depth, T per
level, grid shapes, coarse mode, refinement form, threshold, caller and selection is built, and what the record then says
is checked against the rules restated below: something is current at every level, a reader is only ever handed a current
buffer, bit planes are current only where a launch made them, and the signature tells apart whatever the readers do."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "level_forms_emu.cpp")

NONE, PLANES8, SPREAD, SPREAD_STRIP, BIT_PLANES, BIT_STRIPS = -1, 0, 1, 2, 3, 4
B_PLANES8, B_SPREAD, B_STRIP, B_BIT_STRIPS, B_BIT_PLANES = 1, 2, 4, 8, 16
# the record's bit a form needs to be current for a reader of that form
NEEDS = {PLANES8: B_PLANES8, SPREAD: B_SPREAD, SPREAD_STRIP: B_SPREAD | B_STRIP, BIT_STRIPS: B_BIT_STRIPS, BIT_PLANES: B_BIT_PLANES}


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("forms_emu") / "libforms_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so, EMU_SRC])
    L = C.CDLL(so)
    L.sbm_emu_forms_record.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.sbm_emu_forms_record.restype = C.c_int64
    L.sbm_emu_forms_build.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p]
    L.sbm_emu_forms_build.restype = C.c_int64
    return L


def test_record_reader_names_a_current_buffer_and_signature_is_injective(emu):
    """all 32 states of one level: the reader choice is a buffer the record calls current (or none when no byte or strip
    form is), the precedence is bit strips > spread plane unless the 8 planes are current > 8 planes, set() leaves exactly
    the built form, and two states with different readers never share a signature"""
    out = np.zeros(3, np.int32)
    by_sig = {}
    for bits in range(32):
        sig = emu.sbm_emu_forms_record(bits, PLANES8, out.ctypes.data)
        reads, source = int(out[0]), int(out[1])
        if bits & B_BIT_STRIPS:
            want = BIT_STRIPS
        elif bits & B_SPREAD and not bits & B_PLANES8:
            want = SPREAD_STRIP if bits & B_STRIP else SPREAD
        else:
            want = PLANES8 if bits & B_PLANES8 else NONE
        assert reads == want, bits
        if reads != NONE:
            assert bits & NEEDS[reads] == NEEDS[reads], bits
        if source != NONE:
            assert bits & NEEDS[source] == NEEDS[source], bits
        assert (source == NONE) == (bits & (B_PLANES8 | B_SPREAD | B_BIT_STRIPS | B_BIT_PLANES) == 0), bits
        assert by_sig.setdefault(sig, (reads, source, bool(bits & B_BIT_PLANES))) == (reads, source, bool(bits & B_BIT_PLANES)), bits
        for form in (PLANES8, SPREAD, SPREAD_STRIP, BIT_PLANES, BIT_STRIPS):
            emu.sbm_emu_forms_record(bits, form, out.ctypes.data)
            assert int(out[2]) == NEEDS[form], (bits, form)


# level-0 frames (rows, cols): grid widths that are and are not multiples of 16, coarsest grids that do and do not
# have W * H % 256 == 0 (asserted below, so that the enumeration cannot lose a case unnoticed)
FRAMES = [(1024, 1024), (768, 1088), (480, 672), (96, 160)]
KNOBS = [(0, 1, 1, 1, -1), (1, 1, 1, 1, -1), (0, 0, 1, 1, -1), (0, 1, 0, 1, -1), (0, 1, 1, 0, -1), (0, 1, 1, 1, 0)]


def test_every_build_leaves_readable_levels(emu):
    seen = {"w16": set(), "wh256": set(), "forms": set(), "bit_planes": set()}
    by_sig = {}
    n = 0
    for L in (1, 2, 3):
        for Ts in itertools.product((4, 8), repeat=L):
            for rows0, cols0 in FRAMES:
                rows = [rows0 >> l for l in range(L)]
                cols = [cols0 >> l for l in range(L)]
                W = [cols[l] // Ts[l] for l in range(L)]
                H = [rows[l] // Ts[l] for l in range(L)]
                geo = np.array([L, *Ts, *rows, *cols], np.int32)
                seen["w16"].update(w % 16 == 0 for w in W[:-1])
                seen["wh256"].add(W[-1] * H[-1] % 256 == 0)
                for knobs, mode, refine, thr_state, has_spread, one_launch, match, empty in itertools.product(
                        KNOBS, (0, 3, 4), (-1, 0, 1), (0, 1, 2), (1, 0), (1, 0), (1, 0), (0, 1)):
                    if match and thr_state == 0:
                        continue  # a match entry point has set its threshold
                    if not match and empty:
                        continue  # a stage entry point runs no template loop
                    k = np.array(knobs, np.int32)
                    out = np.zeros(3 * L + 2, np.int32)
                    sig = emu.sbm_emu_forms_build(geo.ctypes.data, k.ctypes.data, mode, refine, thr_state, has_spread, one_launch, match, empty,
                                                  out.ctypes.data)
                    n += 1
                    case = (Ts, rows0, cols0, knobs, mode, refine, thr_state, has_spread, one_launch, match, empty)
                    form = [int(out[3 * l]) for l in range(L)]
                    bits = [int(out[3 * l + 1]) for l in range(L)]
                    reads = [int(out[3 * l + 2]) for l in range(L)]
                    pack_spread, on_bits = bool(out[3 * L]), bool(out[3 * L + 1])
                    # the rules of the host side, restated: bit planes for thresholds >= 0 in the modes auto and bits
                    assert on_bits == (mode in (0, 3) and thr_state == 2), case
                    for l in range(L):
                        # 1. something is current, and nothing that this build did not make (but the coarsest level's bit planes)
                        assert bits[l] & (B_PLANES8 | B_SPREAD | B_BIT_STRIPS | B_BIT_PLANES), case
                        assert bits[l] & ~B_BIT_PLANES == NEEDS[form[l]] & ~B_BIT_PLANES, case
                        if l < L - 1:
                            assert not bits[l] & B_BIT_PLANES, case
                            # 2. the refinement pass is handed a current buffer of that very layout
                            assert reads[l] == form[l] and reads[l] in (PLANES8, SPREAD, SPREAD_STRIP, BIT_STRIPS), case
                            assert bits[l] & NEEDS[reads[l]] == NEEDS[reads[l]], case
                            if form[l] == BIT_STRIPS:
                                assert match and one_launch and Ts[l] == 4 and W[l] % 16 == 0 and refine != 0, case
                            if form[l] == SPREAD_STRIP:
                                assert W[l] % 16 == 0, case
                            if not one_launch:
                                assert form[l] == PLANES8, case
                    lc = L - 1
                    # 2. (coarsest level) after a match call with templates selected, the coarse pass's operand is current
                    if match and not empty:
                        assert bits[lc] & (B_BIT_PLANES if on_bits else B_PLANES8), case
                    if not match:
                        assert form[lc] == PLANES8 and not bits[lc] & B_BIT_PLANES, case
                    # 3. bit planes are current only where a launch made them: the linear-memory launch, the pack from the
                    # spread plane, or the coarse pass's own pack from the 8 planes, which an empty selection skips
                    built = form[lc] == BIT_PLANES or pack_spread
                    assert bool(bits[lc] & B_BIT_PLANES) == (built or (match and on_bits and not empty)), case
                    if built:
                        assert match and one_launch and on_bits and knobs[3], case
                        assert (form[lc] == BIT_PLANES) == (W[lc] * H[lc] % 256 == 0), case
                    if pack_spread:
                        assert form[lc] == SPREAD and has_spread, case
                    # 4. the signature determines what every reader takes
                    key = (L, sig)
                    readers = (tuple(reads[:lc]), bool(bits[lc] & B_BIT_PLANES), bool(bits[lc] & B_PLANES8), bool(bits[lc] & B_SPREAD))
                    assert by_sig.setdefault(key, readers) == readers, case
                    seen["forms"].update(form)
                    seen["bit_planes"].add((bool(bits[lc] & B_BIT_PLANES), bool(empty)))
    assert seen["w16"] == {True, False} and seen["wh256"] == {True, False}
    assert seen["forms"] == {PLANES8, SPREAD, SPREAD_STRIP, BIT_PLANES, BIT_STRIPS}
    assert seen["bit_planes"] == {(True, False), (False, False), (True, True), (False, True)}
    assert n > 10000
