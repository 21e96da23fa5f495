"""CPU (not gpu): the typed record of where a call's frames and masks lie (shape_based_matching_amd/csrc/sbm_frame_source.h),
compiled here for the CPU.  A call's frames are strided, named by a device table of frame pointers or by one of plane pointers; the
record says which in words, and the key of a captured graph (GraphKey) compares it field by field.  What is checked: keys of the
three kinds never compare equal, whatever frame stride the strided one holds; every field of the key counts; the strides a kernel
gets (a table form's are 0); the one source-pass form function against the three rules it switches between; no packed last strip
behind a table."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "frame_source_emu.cpp")
STRIDED, TABLE, PLANES = range(3)
MASK_NONE, MASK_SHARED, MASK_STRIDED, MASK_TABLE = range(4)
ALIGNED4 = 1  # SBM_PTRS_ALIGNED4
INT64_MIN = -(2 ** 63)
# frame strides a caller can mean, and the values the two in-band marks of the table forms used to occupy
STRIDES = (0, 1, -1, 4096, -4096, 2 ** 62, -(2 ** 62), 2 ** 63 - 1, -(2 ** 63) + 2)
OLD_MARKS = (INT64_MIN, INT64_MIN + 1, INT64_MIN + 16, INT64_MIN + 17)


class Key(C.Structure):
    _fields_ = [("src_kind", C.c_int32), ("src_stride", C.c_int32), ("src_ch", C.c_int32), ("src_frames", C.c_int32), ("src_flags", C.c_int32),
                ("src_base", C.c_int64), ("src_frame_stride", C.c_int64),
                ("mask_kind", C.c_int32), ("mask_base", C.c_int64), ("mask_stride", C.c_int64),
                ("rows", C.c_int32), ("cols", C.c_int32), ("thr_bits", C.c_uint32),
                ("out", C.c_int64), ("cap", C.c_int64), ("count", C.c_int64), ("mirror_out", C.c_int64), ("mirror_count", C.c_int64),
                ("kind", C.c_int32), ("forms_signature", C.c_int64), ("sparse_grad", C.c_int32), ("sparse_rects", C.c_int32)]

    def copy(self, **changes):
        k = Key.from_buffer_copy(self)
        for name, value in changes.items():
            setattr(k, name, value)
        return k


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("frame_source_emu") / "libframe_source_emu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so, EMU_SRC])
    L = C.CDLL(so)
    i, i64, kp = C.c_int, C.c_int64, C.POINTER(Key)
    L.sbm_emu_graph_key_equal.argtypes = [kp, kp]
    L.sbm_emu_strided_frames.argtypes = [kp, i64, i, i, i, i64]
    L.sbm_emu_table_frames.argtypes = [kp, i, i64, i, i, i, i]
    L.sbm_emu_strided_masks.argtypes = [kp, i64, i64]
    L.sbm_emu_table_masks.argtypes = [kp, i64]
    for f in (L.sbm_emu_strided_frames, L.sbm_emu_table_frames, L.sbm_emu_strided_masks, L.sbm_emu_table_masks):
        f.restype = None
    for f in (L.sbm_emu_frames_in_table, L.sbm_emu_kernel_frame_stride, L.sbm_emu_source_may_pack):
        f.argtypes = [i, i64, i]
    L.sbm_emu_kernel_frame_stride.restype = i64
    L.sbm_emu_kernel_mask_stride.argtypes = [i, i64]
    L.sbm_emu_kernel_mask_stride.restype = i64
    L.sbm_emu_masks_per_frame.argtypes = [i]
    L.sbm_emu_source_takes_lines.argtypes = [i, i64, i, i, i, i64, i, i, i, i]
    L.sbm_emu_source_lines_ok.argtypes = [C.c_uint64, i64, i64, i, i, i, i]
    L.sbm_emu_frame_ptrs_lines.argtypes = [i, i64, i, i, i, i]
    L.sbm_emu_frame_planes_lines.argtypes = [i, i64, i, i, i]
    return L


def batch_key(emu, kind, frame_stride=0, flags=0):
    """a batch call's key: 4 frames of 448 x 576 x 3 at address 0x7f0000001000 (of the frames, or of the table that names them)"""
    k = Key(rows=448, cols=576, thr_bits=0x42B40000, out=0x7F0100000000, cap=4096, count=0x7F0200000000, kind=4)
    if kind == STRIDED:
        emu.sbm_emu_strided_frames(k, 0x7F0000001000, 1728, 3, 4, frame_stride)
    else:
        emu.sbm_emu_table_frames(k, int(kind == PLANES), 0x7F0000001000, 1728, 3, 4, flags)
    return k


def equal(emu, a, b):
    ab, ba = emu.sbm_emu_graph_key_equal(a, b), emu.sbm_emu_graph_key_equal(b, a)
    assert ab == ba
    return ab == 1


def test_the_three_kinds_of_source_are_three_graphs(emu):
    table, planes = batch_key(emu, TABLE), batch_key(emu, PLANES)
    assert not equal(emu, table, planes)  # a _ptrs and a _planes call at the same table address
    for fs in STRIDES + OLD_MARKS + (448 * 1728,):
        strided = batch_key(emu, STRIDED, fs)
        assert strided.src_frame_stride == fs
        assert not equal(emu, strided, table), fs
        assert not equal(emu, strided, planes), fs
        for flags in (0, ALIGNED4):
            assert not equal(emu, strided, batch_key(emu, TABLE, flags=flags)), (fs, flags)
        assert equal(emu, strided, strided.copy())
    # strided keys differ in their stride alone, also between the old marks
    for a, b in itertools.combinations(STRIDES + OLD_MARKS, 2):
        assert not equal(emu, batch_key(emu, STRIDED, a), batch_key(emu, STRIDED, b)), (a, b)
    assert equal(emu, table, table.copy()) and equal(emu, planes, planes.copy())


def test_a_table_calls_flags_are_part_of_the_key(emu):
    a, b = batch_key(emu, TABLE, flags=0), batch_key(emu, TABLE, flags=ALIGNED4)
    assert (a.src_flags, b.src_flags) == (0, ALIGNED4)
    assert not equal(emu, a, b)
    assert equal(emu, b, batch_key(emu, TABLE, flags=ALIGNED4))


def test_every_field_of_the_key_counts(emu):
    for base in (batch_key(emu, STRIDED, 448 * 1728), batch_key(emu, TABLE, flags=ALIGNED4), batch_key(emu, PLANES)):
        emu.sbm_emu_strided_masks(base, 0x7F0300000000, 448 * 576)
        assert equal(emu, base, base.copy())
        for name, _ in Key._fields_:
            if name == "forms_signature":
                continue  # (its own test below)
            changed = base.copy(**{name: getattr(base, name) + 1})
            assert not equal(emu, base, changed), name


def test_masks(emu):
    def with_mask(make, *args):
        k = batch_key(emu, STRIDED, 448 * 1728)
        make(k, *args)
        return k

    m = 0x7F0300000000
    none = with_mask(emu.sbm_emu_strided_masks, 0, 0)
    shared = with_mask(emu.sbm_emu_strided_masks, m, 0)
    strided = with_mask(emu.sbm_emu_strided_masks, m, 448 * 576)
    table = with_mask(emu.sbm_emu_table_masks, m)
    assert [k.mask_kind for k in (none, shared, strided, table)] == [MASK_NONE, MASK_SHARED, MASK_STRIDED, MASK_TABLE]
    for a, b in itertools.combinations((none, shared, strided, table), 2):
        assert not equal(emu, a, b), (a.mask_kind, b.mask_kind)
    # the mask stride counts only when there is a mask: without one the record holds neither address nor stride
    assert equal(emu, none, with_mask(emu.sbm_emu_strided_masks, 0, 448 * 576))
    assert equal(emu, none, with_mask(emu.sbm_emu_table_masks, 0))
    assert not equal(emu, strided, with_mask(emu.sbm_emu_strided_masks, m, 448 * 576 + 64))
    assert not equal(emu, shared, with_mask(emu.sbm_emu_strided_masks, m + 64, 0))
    # what the kernels get, and whether levels >= 1 hold a mask per frame
    for kind, want in ((MASK_NONE, 0), (MASK_SHARED, 0), (MASK_STRIDED, 448 * 576), (MASK_TABLE, 0)):
        assert emu.sbm_emu_kernel_mask_stride(kind, 448 * 576) == want
        assert emu.sbm_emu_masks_per_frame(kind) == int(kind in (MASK_STRIDED, MASK_TABLE))


def test_forms_signature_is_the_template_loops(emu):
    loop = Key(rows=448, cols=576, thr_bits=0x42B40000, out=0x7F0100000000, cap=4096, count=0x7F0200000000, kind=-1, src_frames=1,
               forms_signature=0x21)
    assert equal(emu, loop, loop.copy())
    assert not equal(emu, loop, loop.copy(forms_signature=0x28))
    # batch keys hold 0 there: two of them never differ by it
    a, b = batch_key(emu, STRIDED, 448 * 1728), batch_key(emu, STRIDED, 448 * 1728)
    assert a.forms_signature == 0 and b.forms_signature == 0 and equal(emu, a, b)


def test_kernel_side_strides(emu):
    for fs in STRIDES:
        assert emu.sbm_emu_kernel_frame_stride(STRIDED, fs, 0) == fs
        assert emu.sbm_emu_frames_in_table(STRIDED, fs, 0) == 0, fs
    for fs in OLD_MARKS:  # values like any other now
        assert emu.sbm_emu_kernel_frame_stride(STRIDED, fs, 0) == fs
        assert emu.sbm_emu_frames_in_table(STRIDED, fs, 0) == 0, fs
    for kind, flags in ((TABLE, 0), (TABLE, ALIGNED4), (PLANES, 0), (PLANES, ALIGNED4)):
        assert emu.sbm_emu_frames_in_table(kind, 0, flags) == 1
        for fs in (0,) + STRIDES:
            assert emu.sbm_emu_kernel_frame_stride(kind, fs, flags) == 0, (kind, flags, fs)


def test_no_packing_behind_a_table(emu):
    for fs in STRIDES + OLD_MARKS:
        assert emu.sbm_emu_source_may_pack(STRIDED, fs, 0) == 1, fs
    for kind, flags in itertools.product((TABLE, PLANES), (0, ALIGNED4)):
        assert emu.sbm_emu_source_may_pack(kind, 0, flags) == 0, (kind, flags)


def test_one_form_function_is_the_three_rules(emu):
    """the grid of test_frame_ptrs_plan.py::test_rule_agrees_with_the_contiguous_rule, knob on and off"""
    n = [0, 0]
    for rows, cols, ch, pad, frames, knob in itertools.product((2, 16, 447, 448), (60, 64, 128, 560, 576), (1, 3), (0, 1, 4, 12, 13), (1, 3), (0, 1)):
        stride = cols * ch + pad
        for base, gap in ((0x1000, 0), (0x7F00_0000_0004, 8)):
            fs = rows * stride + gap
            where = (rows, cols, ch, pad, frames, knob, base)
            want = emu.sbm_emu_source_lines_ok(base, stride, fs, frames, rows, cols, ch) if knob else 0
            assert emu.sbm_emu_source_takes_lines(STRIDED, base, stride, ch, frames, fs, 0, rows, cols, knob) == want, where
            n[0] += want
            for flags in (0, ALIGNED4):
                want = emu.sbm_emu_frame_ptrs_lines(flags, stride, rows, cols, ch, knob)
                assert emu.sbm_emu_source_takes_lines(TABLE, base, stride, ch, frames, 0, flags, rows, cols, knob) == want, where
                n[1] += want
                want = emu.sbm_emu_frame_planes_lines(flags, stride, rows, cols, knob)
                assert want == 0 and emu.sbm_emu_source_takes_lines(PLANES, base, stride, 3, frames, 0, flags, rows, cols, knob) == 0, where
    assert n[0] > 20 and n[1] > 20  # the grid holds layouts of both forms
