"""CPU (not gpu): the host rules of sbm_match_batch_device_ptrs (shape_based_matching_amd/csrc/sbm_frame_ptrs_plan.h), compiled
here for the CPU.  The host never reads the table of frame pointers, so it decides from the call's integers alone: the argument
check, and which form of the sparse path's source pass the call takes -- whole lines (k_source_lines) iff the caller promises
4-byte aligned frame pointers (SBM_PTRS_ALIGNED4), stride % 4 == 0, cols % 64 == 0, a frame that fits the 32-bit lane offsets
and SBM_SOURCE_LINES is not 0; the strided form otherwise."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "frame_ptrs_plan_emu.cpp")
ALIGNED4 = 1
OK, NULL_TABLE, NO_FRAMES, UNKNOWN_FLAGS, SHORT_STRIDE = range(5)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("frame_ptrs_plan_emu") / "libframe_ptrs_plan_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so, EMU_SRC])
    L = C.CDLL(so)
    i, i64 = C.c_int, C.c_int64
    L.sbm_emu_frame_ptrs_check.argtypes = [i, i, i, i, i, i]
    L.sbm_emu_frame_ptrs_error.argtypes = [i]
    L.sbm_emu_frame_ptrs_error.restype = C.c_char_p
    L.sbm_emu_frame_ptrs_lines.argtypes = [i, i64, i, i, i, i]
    L.sbm_emu_source_lines_ok.argtypes = [C.c_uint64, i64, i64, i, i, i, i]
    return L


def test_argument_check(emu):
    chk = emu.sbm_emu_frame_ptrs_check
    assert chk(1, 3, 576, 576 * 3, 3, 0) == OK
    assert chk(1, 1, 576, 576 * 3 + 13, 3, ALIGNED4) == OK
    assert chk(1, 65535, 64, 64, 1, ALIGNED4) == OK
    assert chk(0, 3, 576, 576 * 3, 3, 0) == NULL_TABLE
    assert chk(1, 0, 576, 576 * 3, 3, 0) == NO_FRAMES
    assert chk(1, -4, 576, 576 * 3, 3, 0) == NO_FRAMES
    for flags in (2, 3, 4, 0x100, -1, 1 << 30):
        assert chk(1, 3, 576, 576 * 3, 3, flags) == UNKNOWN_FLAGS, flags
    assert chk(1, 3, 576, 576 * 3 - 1, 3, 0) == SHORT_STRIDE
    assert chk(1, 3, 576, 576, 3, ALIGNED4) == SHORT_STRIDE  # a gray stride for BGR frames
    assert chk(1, 3, 576, 0, 1, 0) == SHORT_STRIDE
    assert chk(1, 3, 576, -1728, 3, 0) == SHORT_STRIDE
    # the first failing rule is the one reported, and every code has a message
    assert chk(0, 0, 576, 0, 3, 8) == NULL_TABLE
    assert chk(1, 0, 576, 0, 3, 8) == NO_FRAMES
    assert chk(1, 1, 576, 0, 3, 8) == UNKNOWN_FLAGS
    msgs = [emu.sbm_emu_frame_ptrs_error(e) for e in (NULL_TABLE, NO_FRAMES, UNKNOWN_FLAGS, SHORT_STRIDE)]
    assert all(m for m in msgs) and len(set(msgs)) == 4
    assert emu.sbm_emu_frame_ptrs_error(OK) == b""


def test_form_rule_table(emu):
    lines = emu.sbm_emu_frame_ptrs_lines
    # flags, stride, rows, cols, ch -> the line form?
    assert lines(ALIGNED4, 576 * 3, 448, 576, 3, 1) == 1          # flag set, stride % 4 == 0, cols % 64 == 0
    assert lines(0, 576 * 3, 448, 576, 3, 1) == 0                 # flag cleared
    assert lines(ALIGNED4, 576 * 3 + 13, 448, 576, 3, 1) == 0     # a row pad of 13 bytes
    assert lines(ALIGNED4, 576 * 3 + 12, 448, 576, 3, 1) == 1     # ... of 12 (a window's canvas row)
    assert lines(ALIGNED4, 576, 448, 576, 1, 1) == 1              # cols = 576
    assert lines(ALIGNED4, 560, 448, 560, 1, 1) == 0              # cols = 560
    assert lines(ALIGNED4, 560 * 3, 448, 560, 3, 1) == 0
    assert lines(ALIGNED4, 576 * 3, 448, 576, 3, 0) == 0          # SBM_SOURCE_LINES=0
    # a frame of exactly 0x7ff00000 bytes: (rows - 1) * stride + cols * ch with stride 64, gray, 64 columns
    rows = (0x7FF00000 - 64) // 64 + 1
    assert rows % 2 == 0 and (rows - 1) * 64 + 64 == 0x7FF00000
    assert lines(ALIGNED4, 64, rows, 64, 1, 1) == 0
    assert lines(ALIGNED4, 64, rows - 2, 64, 1, 1) == 1           # one pair of rows less fits
    # what the kernel cannot take at all stays strided whatever the flag says
    assert lines(ALIGNED4, 64 * 3, 447, 64, 3, 1) == 0            # odd rows
    assert lines(ALIGNED4, 64 * 2, 448, 64, 2, 1) == 0            # two channels


def test_rule_agrees_with_the_contiguous_rule(emu):
    """where both apply -- one block whose base and frame stride are multiples of 4 -- the table rule with the flag set is
    source_lines_ok of that block"""
    n = 0
    for rows, cols, ch, pad, frames in itertools.product((2, 16, 447, 448), (60, 64, 128, 560, 576), (1, 3), (0, 1, 4, 12, 13), (1, 3)):
        stride = cols * ch + pad
        for base, gap in ((0x1000, 0), (0x7F00_0000_0004, 8)):
            fs = rows * stride + gap
            if fs % 4:
                continue
            want = emu.sbm_emu_source_lines_ok(base, stride, fs, frames, rows, cols, ch)
            assert emu.sbm_emu_frame_ptrs_lines(ALIGNED4, stride, rows, cols, ch, 1) == want, (rows, cols, ch, pad, frames, base)
            n += want
    assert n > 20  # the grid holds layouts of both kinds
