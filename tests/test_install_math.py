"""CPU (not gpu): the dataflow of the kernels of sbm_upload_templates_device (shape_based_matching_amd/csrc/sbm_install_kernels.h)
walked on the CPU in chunks of 256 (tests/emu/install_math_emu.cpp, with the scalar rules of sbm_install_math.h) against a numpy
restatement of the host loop of sbm_upload_templates (sbm_capi_match.inc): the packed tables, the level's extent, the 17 class
offsets and the class-sorted copies, which must be the host's stable counting sort exactly; the scan's template indices, feature
offsets and ids against the numbering rule; and the same sources as a stand-alone program under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shape_based_matching_amd", "csrc")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "install_math_emu.cpp")
TRAIN_FEATURE = np.dtype([("x", "<i4"), ("y", "<i4"), ("label", "<i4"), ("theta", "<f4")])
LEVEL = np.dtype([("width", "<i4"), ("height", "<i4"), ("tl_x", "<i4"), ("tl_y", "<i4"), ("pyramid_level", "<i4"), ("n_features", "<i4"),
                  ("feature_offset", "<i8")])
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 8191)
NO_FAULT = 0xFFFFFFFF


def cxx():
    c = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if c is None:
        pytest.fail("no host C++ compiler")
    return c


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("install_math_emu") / "libinstall_math_emu.so")
    subprocess.check_call([cxx(), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so, EMU_SRC])
    L = C.CDLL(so)
    L.sbm_emu_install_features.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_int32] + [C.c_void_p] * 8
    L.sbm_emu_install_features.restype = None
    L.sbm_emu_install_scan.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
    L.sbm_emu_install_ext_merge.argtypes = [C.c_uint32, C.c_uint32]
    L.sbm_emu_install_ext_merge.restype = C.c_uint32
    L.sbm_emu_install_class.argtypes = [C.c_uint32, C.c_int]
    return L


def host_level(x, y, label, T):
    """sbm_upload_templates' loop for one (template, level), restated: fxy, flabel, fext, the 17 offsets, the sorted copies"""
    fxy = x.astype(np.uint32) | (y.astype(np.uint32) << np.uint32(16))
    flabel = label.astype(np.uint8)
    fext = (int(x.max()) if len(x) else 0) | ((int(y.max()) if len(y) else 0) << 16)
    log2t = {4: 2, 8: 3}.get(T, -1)
    if log2t < 0:  # never read sorted: offsets {0, nf x 16}, the copies unsorted
        return fxy, flabel, fext, np.array([0] + [len(x)] * 16, np.uint16), fxy.copy(), flabel.copy()
    k = ((fxy & 0xFFFF) >> log2t) & 15
    cnt = np.zeros(17, np.int64)
    for c in k:
        cnt[c + 1] += 1
    cnt = np.cumsum(cnt)
    pos = cnt[:16].copy()
    fxy_s, flabel_s = fxy.copy(), flabel.copy()
    for i in range(len(fxy)):
        fxy_s[pos[k[i]]] = fxy[i]
        flabel_s[pos[k[i]]] = flabel[i]
        pos[k[i]] += 1
    return fxy, flabel, fext, cnt.astype(np.uint16), fxy_s, flabel_s


def features(pattern, nf, T, seed=0):
    rng = np.random.default_rng(seed * 100003 + nf * 17 + T)
    y = rng.integers(0, 65536, nf)
    label = rng.integers(0, 8, nf)
    if pattern == "one class":  # every x in strip column 5, whatever is left of it varies
        x = (5 * T + rng.integers(0, T, nf)) + 16 * T * rng.integers(0, 8, nf)
    elif pattern == "round robin":
        x = (np.arange(nf) % 16) * T + rng.integers(0, T, nf)
    elif pattern == "random":
        x = rng.integers(0, 65536, nf)
    elif pattern == "x edges":
        x = np.where(np.arange(nf) % 2 == 0, 0, 65535)
        y = np.where(np.arange(nf) % 3 == 0, 65535, y)
    else:
        raise ValueError(pattern)
    f = np.zeros(nf, TRAIN_FEATURE)
    f["x"], f["y"], f["label"] = x, y, label
    f["theta"] = rng.random(nf).astype(np.float32) * 360
    return f


def run_level(emu, feats, nf_record, T, level, feat_off, total):
    """the emulated k_install_features workgroup of one level, into tables pre-filled with 0x5A that hold `total` features"""
    fxy, fxy_s = np.full(total, 0x5A5A5A5A, np.uint32), np.full(total, 0x5A5A5A5A, np.uint32)
    flabel, flevel, flabel_s = (np.full(total, 0x5A, np.uint8) for _ in range(3))
    fcls, fext, verdict = np.full(17, 0x5A5A, np.uint16), np.full(1, 0x5A5A5A5A, np.uint32), np.full(1, NO_FAULT, np.uint32)
    src = np.ascontiguousarray(feats)
    keep = src.copy()
    emu.sbm_emu_install_features(src.ctypes.data_as(C.c_void_p), nf_record, T, level, feat_off,
                                 *[a.ctypes.data_as(C.c_void_p) for a in (fxy, flabel, flevel, fxy_s, flabel_s, fcls, fext, verdict)])
    assert src.tobytes() == keep.tobytes()
    return fxy, flabel, flevel, fxy_s, flabel_s, fcls, int(fext[0]), int(verdict[0])


@pytest.mark.parametrize("T", [4, 8, 16])
@pytest.mark.parametrize("pattern", ["one class", "round robin", "random", "x edges"])
def test_level_tables_equal_the_host_loop(emu, T, pattern):
    for nf in COUNTS:
        f = features(pattern, nf, T)
        off, total = 11, nf + 30  # the level lies inside larger tables: nothing outside [off, off + nf) may change
        fxy, flabel, flevel, fxy_s, flabel_s, fcls, fext, verdict = run_level(emu, f, nf, T, 1, off, total)
        w_fxy, w_flabel, w_fext, w_fcls, w_fxy_s, w_flabel_s = host_level(f["x"], f["y"], f["label"], T)
        inside = slice(off, off + nf)
        assert verdict == NO_FAULT and fext == w_fext, (nf, pattern)
        assert np.array_equal(fxy[inside], w_fxy) and np.array_equal(flabel[inside], w_flabel) and (flevel[inside] == 1).all(), (nf, pattern)
        assert np.array_equal(fcls, w_fcls), (nf, pattern)
        assert np.array_equal(fxy_s[inside], w_fxy_s) and np.array_equal(flabel_s[inside], w_flabel_s), (nf, pattern)  # the stable order, not a permutation of it
        for a in (fxy, fxy_s):
            assert (np.delete(a, np.arange(off, off + nf)) == 0x5A5A5A5A).all()
        for a in (flabel, flevel, flabel_s):
            assert (np.delete(a, np.arange(off, off + nf)) == 0x5A).all()


def test_a_count_beyond_the_bound_is_clamped(emu):
    """the loops end on the record's count clamped to 0 .. 8191, whatever the record says (the scan refuses such a record before)"""
    f = features("random", 8191, 4)
    for bad in (8192, 1 << 30, -1, -(1 << 31)):
        fxy, *_rest, fcls, _fext, _verdict = run_level(emu, f, bad, 4, 0, 0, 8191)
        assert int(fcls[16]) == (8191 if bad > 0 else 0)


@pytest.mark.parametrize("T", [4, 16])
def test_first_feature_out_of_bounds_is_the_verdict(emu, T):
    base = features("random", 300, T)
    cases = {"x negative": ("x", -1), "x beyond": ("x", 65536), "y negative": ("y", -5), "y beyond": ("y", 1 << 20), "label negative": ("label", -1),
             "label 8": ("label", 8)}
    for name, (field, value) in cases.items():
        for where in ([0], [299], [17, 256, 299], [255, 64]):
            f = base.copy()
            f[field][where] = value
            *_tables, verdict = run_level(emu, f, 300, T, 0, 1000, 1300)
            assert verdict == 1000 + min(where), (name, where)
    # the edge values themselves are inside
    f = base.copy()
    f["x"][0], f["y"][1], f["label"][2], f["x"][3], f["y"][4], f["label"][5] = 0, 0, 0, 65535, 65535, 7
    assert run_level(emu, f, 300, T, 0, 0, 300)[-1] == NO_FAULT


def test_scalar_rules(emu):
    merge = emu.sbm_emu_install_ext_merge
    assert merge(0, 0) == 0 and merge(0x00050009, 0x00090005) == 0x00090009 and merge(0xFFFF0000, 0x0000FFFF) == 0xFFFFFFFF
    for T, log2t in ((4, 2), (8, 3)):
        for x in (0, T - 1, T, 15 * T, 16 * T - 1, 16 * T, 65535):
            assert emu.sbm_emu_install_class(x | (0xABCD << 16), T) == (x >> log2t) & 15


class Source(C.Structure):  # sbm_template_source, restated
    _fields_ = [("d_levels", C.c_void_p), ("d_feats", C.c_void_p), ("d_status", C.c_void_p), ("n_pyramids", C.c_int32), ("class_idx", C.c_int32),
                ("feat_first", C.c_int64), ("feat_pitch", C.c_int64), ("feat_cap", C.c_int64)]


def make_sources(counts, classes, L, statuses, rng, cap=40):
    keep, srcs, flat = [], [], []
    for n, cls, st in zip(counts, classes, statuses):
        lv = np.zeros((n, L), LEVEL)
        for i in range(n):
            off = 0
            for l in range(L):
                nf = int(rng.integers(0, cap // L + 1))
                lv[i, l] = (int(rng.integers(1, 500)), int(rng.integers(1, 500)), 3, 4, l, nf, off)
                off += nf
        stat = None if st is None else np.ascontiguousarray(st, np.int32).reshape(n, 2)
        keep.append((lv, stat))
        srcs.append(Source(lv.ctypes.data, 0x1000, None if stat is None else stat.ctypes.data, n, cls, 5, cap + 3, cap))
        for i in range(n):
            flat.append((lv[i], cls, True if stat is None else stat[i, 0] == 0))
    return keep, srcs, flat


def run_scan(emu, srcs, L, P):
    arr = (Source * len(srcs))(*srcs)
    header = np.zeros(3, np.int64)
    index, ip, isrc, cls, tid = (np.full(max(P, 1), -7, np.int32) for _ in range(5))
    tls = np.full((max(P, 1) * L, 4), -7, np.int32)
    assert emu.sbm_emu_install_scan(arr, len(srcs), L, *[a.ctypes.data_as(C.c_void_p) for a in (header, index, ip, isrc, tls, cls, tid)]) == 0
    return header, index[:P], ip, isrc, tls, cls, tid


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("skip", ["none", "first", "middle", "last", "all"])
def test_scan_numbers_the_kept_pyramids(emu, L, skip):
    """two classes that interleave across five sources, one of them without status pairs, one without pyramids, more pyramids than
    one chunk of 256: template indices, feature offsets as the running sum, class and id against the rule restated here"""
    rng = np.random.default_rng(7 + L)
    counts, classes = [3, 300, 0, 2, 260], [4, 9, 4, 9, 4]
    P = sum(counts)
    codes = np.zeros(P, np.int32)
    if skip != "none":
        where = {"first": [0], "middle": [3 + 255, 3 + 256, 400], "last": [P - 1], "all": list(range(P))}[skip]
        codes[where] = [1 + k % 3 for k in range(len(where))]  # status 1, 2 and 3 all skip
    statuses, at = [], 0
    for n in counts:
        statuses.append(np.stack([codes[at: at + n], np.full(n, 77, np.int32)], axis=1))
        at += n
    if skip in ("none", "last"):
        statuses[0] = None  # NULL d_status: every pyramid of the source is ok
    keep, srcs, flat = make_sources(counts, classes, L, statuses, rng)
    header, index, ip, isrc, tls, cls, tid = run_scan(emu, srcs, L, P)
    t, off, seen = 0, 0, {}
    for j, (lv, c, kept) in enumerate(flat):
        if not kept:
            assert index[j] == -1
            continue
        assert index[j] == t and ip[t] == j and cls[t] == c and tid[t] == seen.get(c, 0), j
        seen[c] = seen.get(c, 0) + 1
        for l in range(L):
            assert tls[t * L + l].tolist() == [int(lv[l]["width"]), int(lv[l]["height"]), int(lv[l]["n_features"]), off], (j, l)
            off += int(lv[l]["n_features"])
        t += 1
    assert header.tolist() == [-1, off, t]
    assert (tls[t * L:] == -7).all() and (cls[t:] == -7).all() and (tid[t:] == -7).all()


def test_scan_reports_the_first_faulty_level(emu):
    """a kept pyramid's n_features outside 0 .. 8191 or a range that leaves its block: the first such level in source order is the
    verdict, a skipped pyramid's records are never judged, and a faulty pyramid is not kept"""
    L = 2
    rng = np.random.default_rng(3)
    counts = [2, 300, 4]
    statuses = [np.zeros((n, 2), np.int32) for n in counts]
    statuses[1][10, 0] = 1
    keep, srcs, flat = make_sources(counts, [0, 1, 0], L, statuses, rng)
    keep[1][0]["n_features"][10, 1] = 9000  # skipped: not judged
    assert run_scan(emu, srcs, L, sum(counts))[0][0] == -1
    keep[2][0]["n_features"][3, 0] = -1
    keep[1][0]["feature_offset"][299, 1] = 39  # + its count leaves [0, 40) unless the count is below 2
    keep[1][0]["n_features"][299, 1] = 2
    header, index, *_ = run_scan(emu, srcs, L, sum(counts))
    assert header[0] == ((2 + 299) * L + 1) * 4 + 2 and index[2 + 299] == -1 and index[2 + 300 + 3] == -1
    keep[1][0]["n_features"][256, 0] = 8192
    assert run_scan(emu, srcs, L, sum(counts))[0][0] == ((2 + 256) * L + 0) * 4 + 1
    keep[0][0]["feature_offset"][0, 1] = -1
    assert run_scan(emu, srcs, L, sum(counts))[0][0] == (0 * L + 1) * 4 + 2


def test_emulation_runs_clean_under_the_sanitizers(tmp_path):
    """the same sources with their small main as a stand-alone program, tables exactly as large as the plan says"""
    exe = str(tmp_path / "install_math_emu_asan")
    subprocess.check_call([cxx(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DINSTALL_EMU_MAIN", "-Wall",
                           "-Wextra", "-Werror", "-I", CSRC, "-o", exe, EMU_SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "install emulation ok: 3 templates" in out.stdout
