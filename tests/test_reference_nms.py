"""The NMS stage's restatements against the reference's own nms.hpp.

oracle/_ref/ref_nms is oracle/ref_nms_driver.cpp compiled against the reference's nms.hpp on stand-in headers (build() makes
it by oracle/ref_nms.mk where the reference tree exists): cv_dnn::NMSBoxes with GetMaxScoreIndex's std::stable_sort, NMSFast_'s
walk under the adaptive threshold and jaccardDistance__'s arithmetic.  Everything else here that claims to be that function must
agree with it: test_nms.py::py_nms (the expectation of every device test), include/nms.hpp (sbm_nms_boxes of the facade
library), and the chunked walk of csrc/sbm_nms_math.h (tests/emu/nms_math_emu.cpp) -- on every case of tests/nms_form_cases.py,
on lists with heavy score ties, and, for the overlap arithmetic, bit for bit through keep / drop decisions.  The one piece the
binary cannot pin is cv::Rect_::operator& of the stand-in (oracle/ref_cv), our restatement of OpenCV's documented behaviour.
tests/golden/ref_nms_cases.npz, recorded from the binary, stands in for it where neither the tree nor the binary exists."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import nms_form_cases as NC
from conftest import GOLDEN, ROOT
from oracle import ref_nms as RN
from test_nms import py_nms
from test_nms_math import emu  # noqa: F401  (the fixture: the host pass of sbm_nms_math.h, compiled into a temporary directory)

LIB = os.path.join(ROOT, "shape_based_matching_amd", "libsbm_facade.so")
FIXTURE = os.path.join(GOLDEN, "ref_nms_cases.npz")
TREE = RN.reference_tree_present()


def test_the_binary_this_host_runs():
    """where the reference tree is present build() must have made the binary; elsewhere the binary built earlier or, without
    one, the recorded fixture stands in"""
    if TREE:
        assert not RN.missing_binaries(), "run __graft_entry__.build(): the reference tree is present"
    else:
        assert not RN.missing_binaries() or os.path.exists(FIXTURE)


def reference(problems):
    """{key: kept indices} by the binary, or, where neither it nor the reference tree exists, by the recorded fixture"""
    if not RN.missing_binaries():
        return dict(zip(problems, RN.run_many(list(problems.values()))))
    assert not TREE, f"{RN.missing_binaries()} missing: run __graft_entry__.build() where the reference tree is present"
    z = NC.load_recorded(FIXTURE)
    return {k: z[k] for k in problems}


def facade(problem):
    boxes, scores, score_thr, nms_thr, eta, top_k = problem
    L = C.CDLL(LIB)
    b = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
    s = np.ascontiguousarray(scores, np.float32)
    out = np.zeros(len(s) + 1, np.int32)
    n_out = C.c_int(0)
    rc = L.sbm_nms_boxes(b.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), len(s), C.c_float(score_thr), C.c_float(nms_thr),
                         C.c_float(eta), top_k, out.ctypes.data_as(C.c_void_p), C.byref(n_out))
    assert rc == 0
    return out[: n_out.value].tolist()


def emu_walk(lib, problem):
    """the chunked walk from the candidate list on: the kept candidates as indices of the problem's list"""
    boxes, scores, score_thr, nms_thr, eta, top_k = problem
    cand = [i for i in range(len(scores)) if scores[i] > score_thr]
    assert all(scores[a] >= scores[b] for a, b in zip(cand, cand[1:])), "the epilogue list is sorted: the stable sort leaves it alone"
    if 0 < top_k < len(cand):
        cand = cand[:top_k]
    b = np.ascontiguousarray([boxes[i] for i in cand], np.int32).reshape(-1, 4)
    keep = np.zeros(len(cand) + 1, np.int32)
    k = lib.sbm_emu_nms_walk(b.ctypes.data, len(cand), C.c_float(nms_thr), C.c_float(eta), keep.ctypes.data)
    return [cand[j] for j in keep[:k].tolist()]


def py_kept(case):
    """py_nms's kept indices into the epilogue list, from the shared expectation (raw is the gathered position: unique)"""
    pos = {int(m["raw"]): k for k, m in enumerate(NC.epi(case))}
    assert len(pos) == len(NC.epi(case))
    return [pos[int(m["raw"])] for m in NC.want(case)]


def test_label_table(case1):
    assert NC.sizes_of(NC.label_table(case1["templates"])) == NC.SIZES
    assert {(40, 40), (80, 40), (33, 57), (1, 1), (0, 0), (0, 7)} <= set(NC.SIZES.values()) and NC.UNKNOWN not in NC.SIZES


def test_all_disjoint_lists_are_kept_whole():
    """the all-disjoint cases take the epilogue list as their expectation; py_nms itself says so on the smallest"""
    c = NC.smallest_disjoint_case()
    assert c.check(c) and len(NC.epi(c)) == 130
    assert py_nms(*NC.problem(c)) == list(range(130))
    assert NC.rows_of(NC.expected(c.used(), NC.SIZES, *c.params)) == NC.rows_of(NC.want(c))


@pytest.mark.parametrize("group", list(NC.GROUPS))
def test_case_predicates(group):
    """every case reaches the edge it exists for, and states the flags word the expectation side derives"""
    for launch in NC.launches(group):
        buf, hdr, stride = launch.buffer()
        assert len(buf) == launch.n_parts * stride and stride % 8 == 0 and stride % 16 != 0
        for c in launch.cases:
            assert c.check(c), (c.name, c.edge)
            assert NC.flags_of(c) == c.flags, c.name


@pytest.mark.parametrize("group", list(NC.GROUPS))
def test_four_way_agreement(emu, group):  # noqa: F811
    """the reference binary, py_nms, include/nms.hpp and the chunked walk keep the same boxes of every case"""
    cases = [c for l in NC.launches(group) for c in l.cases]
    problems = {NC.recorded_key(c): NC.problem(c) for c in cases}
    ref = reference(problems)
    for c in cases:
        prob = problems[NC.recorded_key(c)]
        want = py_kept(c)
        assert ref[NC.recorded_key(c)] == want, c.name
        assert facade(prob) == want, c.name
        assert emu_walk(emu, prob) == want, c.name


def _pairs():
    small = list(itertools.product(range(3), range(3), range(4), range(4)))
    pairs = [(a, b) for a in small for b in small]
    rs = np.random.RandomState(11)  # test_nms_math.py::test_overlap_random_boxes_and_py_nms_decision's pairs, the first 2000
    for _ in range(2000):
        a = [int(rs.randint(-50, 400)), int(rs.randint(-50, 400)), int(rs.randint(0, 300)), int(rs.randint(0, 300))]
        if rs.rand() < 0.3:
            b = [a[0] + int(rs.randint(-3, 4)), a[1] + int(rs.randint(-3, 4)), a[2] + int(rs.randint(-2, 3)), a[3] + int(rs.randint(-2, 3))]
            b[2], b[3] = max(b[2], 0), max(b[3], 0)
        else:
            b = [int(rs.randint(-50, 400)), int(rs.randint(-50, 400)), int(rs.randint(0, 300)), int(rs.randint(0, 300))]
        pairs.append((tuple(a), tuple(b)))
    return pairs


def test_overlap_bits_decide_as_the_reference(emu):  # noqa: F811
    """nms_rect_overlap's bit pattern o is the reference's: at threshold o the reference keeps the second box of the pair, at
    the next float below it drops it.  Two problems per pair, all of them in one start of the binary."""
    pairs = _pairs()
    A = np.array([p[0] for p in pairs], np.int32)
    B = np.array([p[1] for p in pairs], np.int32)
    o = np.array([emu.sbm_emu_nms_overlap(A[k].ctypes.data, B[k].ctypes.data) for k in range(len(pairs))], np.float32)
    assert ((o >= 0) & (o <= 1)).all() and (o == 0).any() and (o == 1).any() and ((o > 0) & (o < 1)).sum() > 1000
    below = np.nextafter(o, np.float32(-1))
    assert (below < o).all()
    if RN.missing_binaries():
        assert not TREE, "run __graft_entry__.build() where the reference tree is present"
        for k in range(0, len(pairs), 7):  # no binary on this host: py_nms decides, as in test_nms_math.py
            a, b = list(pairs[k][0]), list(pairs[k][1])
            assert py_nms([a, b], [2.0, 1.0], 0.0, float(o[k])) == [0, 1] and py_nms([a, b], [2.0, 1.0], 0.0, float(below[k])) == [0], pairs[k]
        return
    # the driver's input, laid out at once: per problem {2, score 0, thr, eta 1, top_k 0} and two boxes scored 2 and 1
    dt = np.dtype([("n", "<i4"), ("score", "<f4"), ("thr", "<f4"), ("eta", "<f4"), ("top_k", "<i4"),
                   ("a", "<i4", 4), ("sa", "<f4"), ("b", "<i4", 4), ("sb", "<f4")])
    prob = np.zeros((len(pairs), 2), dt)
    prob["n"], prob["eta"], prob["sa"], prob["sb"] = 2, 1.0, 2.0, 1.0
    prob["a"], prob["b"] = A[:, None, :], B[:, None, :]
    prob["thr"][:, 0], prob["thr"][:, 1] = o, below
    assert prob[:3].tobytes() == RN.encode([([list(A[k]), list(B[k])], [2.0, 1.0], 0.0, t, 1.0, 0) for k in range(3)
                                            for t in (o[k], below[k])])[8:]
    import struct
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<2i", RN.MAGIC, prob.size) + prob.tobytes())
        p = subprocess.run([RN.binary(), src, dst], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr
        with open(dst, "rb") as f:
            got = RN.decode(f.read(), prob.size)
    for k in range(len(pairs)):
        assert got[2 * k] == [0, 1] and got[2 * k + 1] == [0], (pairs[k], o[k], got[2 * k], got[2 * k + 1])


def test_ties_and_parameters():
    """heavy score ties under top_k and eta: GetMaxScoreIndex's stable sort and cut against py_nms's"""
    problems = NC.tie_problems()
    ref = reference(problems)
    sizes = set()
    for k, prob in problems.items():
        want = py_nms(*prob)
        assert ref[k] == want, k
        sizes.add(len(prob[1]))
        if len(prob[1]) == 300:
            assert 1 < len(want) < 300 and len(set(prob[1])) <= 40
    assert sizes == {0, 1, 300}


def test_recorded_reference_output():
    """tests/golden/ref_nms_cases.npz (tools/make_fixtures.py --ref-nms): py_nms keeps what the binary kept when it was recorded,
    and the binary, where this host has it, still does"""
    z = NC.load_recorded(FIXTURE)
    cases = {NC.recorded_key(c): c for _, _, c in NC.all_cases()}
    ties = NC.tie_problems()
    assert sorted(z) == sorted(list(cases) + list(ties))
    fresh = {}
    if not RN.missing_binaries():
        problems = {k: NC.problem(c) for k, c in cases.items()}
        problems.update(ties)
        fresh = dict(zip(problems, RN.run_many(list(problems.values()))))
    for k, rec in z.items():
        assert rec == (py_kept(cases[k]) if k in cases else py_nms(*ties[k])), k
        if fresh:
            assert fresh[k] == rec, k
