"""CPU (not gpu): the host rules of sbm_match_batch_device_planes (shape_based_matching_amd/csrc/sbm_frame_planes_plan.h), compiled
here for the CPU.  The host never reads the table of plane pointers, so it decides from the call's integers alone: the argument
check (in reporting order, a message per code), the form of the source pass (always the strided one: whole lines of interleaved
pixels are not what planes hold) and the mark by which the call travels in the place of a frame stride -- no stride a layout can
have, not the mark of a table of frame pointers, and a round trip of the (reserved) flags."""
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
ALIGNED4 = 1  # the one flag of sbm_match_batch_device_ptrs


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
    L.sbm_emu_frame_planes_fs.argtypes = [i]
    L.sbm_emu_frame_planes_fs.restype = i64
    L.sbm_emu_frame_ptrs_fs.argtypes = [i]
    L.sbm_emu_frame_ptrs_fs.restype = i64
    for f in (L.sbm_emu_fs_is_planes, L.sbm_emu_fs_planes_flags, L.sbm_emu_fs_names_table, L.sbm_emu_fs_is_table):
        f.argtypes = [i64]
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


def test_mark_is_no_frame_stride_and_no_ptrs_mark(emu):
    fs = emu.sbm_emu_frame_planes_fs(0)
    assert emu.sbm_emu_fs_is_planes(fs) == 1 and emu.sbm_emu_fs_planes_flags(fs) == 0 and emu.sbm_emu_fs_names_table(fs) == 1
    # unknown flag bits never enter the mark
    assert emu.sbm_emu_frame_planes_fs(0x7FFFFFFF) == fs and emu.sbm_emu_frame_planes_fs(-1) == fs
    # no _ptrs mark, whatever that call's flags: the two kinds of graph key differ in this field
    assert emu.sbm_emu_fs_is_table(fs) == 0
    for flags in (0, ALIGNED4):
        pfs = emu.sbm_emu_frame_ptrs_fs(flags)
        assert pfs != fs and emu.sbm_emu_fs_is_planes(pfs) == 0 and emu.sbm_emu_fs_names_table(pfs) == 1
    # no stride a layout can have: far below every frame stride a caller can mean, negative ones included
    assert fs < -(2 ** 62)
    for v in (0, 1, -1, 4096, -4096, 2 ** 62, -(2 ** 62), 2 ** 63 - 1, -(2 ** 63) + 2, fs - 1, fs + 1):
        assert emu.sbm_emu_fs_is_planes(v) == 0, v
        assert emu.sbm_emu_fs_planes_flags(v) == 0, v
    for v in (0, 1, -1, 4096, -4096, 2 ** 62, -(2 ** 62), 2 ** 63 - 1, -(2 ** 63) + 2, fs - 1, fs + 1):
        assert emu.sbm_emu_fs_names_table(v) == 0, v
