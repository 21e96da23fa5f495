"""CPU (not gpu): the host rules of sbm_match_batch_device_planes (shape_based_matching_amd/csrc/sbm_frame_planes_plan.h), compiled
here for the CPU.  The host never reads the table of plane pointers, so it decides from the call's integers alone: the argument
check (in reporting order, a message per code) and the form of the source pass (always the strided one: whole lines of interleaved
pixels are not what planes hold).  How the call travels, and that its graph is none of a table of frame pointers:
tests/test_frame_source.py."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "frame_planes_plan_emu.cpp")
OK, NULL_TABLE, NO_FRAMES, UNKNOWN_FLAGS, SHORT_STRIDE = range(5)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("frame_planes_plan_emu") / "libframe_planes_plan_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so, EMU_SRC])
    L = C.CDLL(so)
    i, i64 = C.c_int, C.c_int64
    L.sbm_emu_frame_planes_check.argtypes = [i, i, i, i, i]
    L.sbm_emu_frame_planes_error.argtypes = [i]
    L.sbm_emu_frame_planes_error.restype = C.c_char_p
    L.sbm_emu_frame_planes_lines.argtypes = [i, i64, i, i, i]
    return L


def test_argument_check(emu):
    chk = emu.sbm_emu_frame_planes_check
    # have_table, n_frames, cols, stride (bytes per row of a PLANE), flags
    assert chk(1, 3, 576, 576, 0) == OK
    assert chk(1, 1, 576, 576 + 13, 0) == OK
    assert chk(1, 65535, 64, 672, 0) == OK  # a window of a wider canvas
    assert chk(0, 3, 576, 576, 0) == NULL_TABLE
    assert chk(1, 0, 576, 576, 0) == NO_FRAMES
    assert chk(1, -4, 576, 576, 0) == NO_FRAMES
    for flags in (1, 2, 3, 4, 0x100, -1, 1 << 30):  # reserved: every bit is unknown, SBM_PTRS_ALIGNED4 included
        assert chk(1, 3, 576, 576, flags) == UNKNOWN_FLAGS, flags
    assert chk(1, 3, 576, 575, 0) == SHORT_STRIDE
    assert chk(1, 3, 576, 0, 0) == SHORT_STRIDE
    assert chk(1, 3, 576, -576, 0) == SHORT_STRIDE
    # the first failing rule is the one reported, and every code has a message
    assert chk(0, 0, 576, 0, 8) == NULL_TABLE
    assert chk(1, 0, 576, 0, 8) == NO_FRAMES
    assert chk(1, 1, 576, 0, 8) == UNKNOWN_FLAGS
    assert chk(1, 1, 576, 0, 0) == SHORT_STRIDE
    msgs = [emu.sbm_emu_frame_planes_error(e) for e in (NULL_TABLE, NO_FRAMES, UNKNOWN_FLAGS, SHORT_STRIDE)]
    assert all(m for m in msgs) and len(set(msgs)) == 4
    assert emu.sbm_emu_frame_planes_error(OK) == b""
    assert emu.sbm_emu_frame_planes_channels() == 3


def test_source_pass_is_always_strided(emu):
    """layouts the line form of the interleaved table takes (stride % 4 == 0, cols % 64 == 0) and ones it refuses, knob on and off"""
    for stride_pad, rows, cols, knob, flags in itertools.product((0, 4, 12, 13, 64), (2, 16, 448), (64, 128, 560, 576), (0, 1), (0, 1)):
        assert emu.sbm_emu_frame_planes_lines(flags, cols + stride_pad, rows, cols, knob) == 0, (stride_pad, rows, cols, knob, flags)
