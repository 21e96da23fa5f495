"""-m gpu: every stored form of the linear memories read back as it lies in device memory, for every frame of the batch and
every level, and compared bit for bit with the oracle's spread -> response maps -> linearize of that frame's orientation map
(inputs, layout decoders and the shared check: lm_form_cases.py; tests/test_lm_form_cases.py proves them without a GPU).

The bytes come from sbm_get_level_stored, which copies and nothing else; which form and builder made them is read from
sbm_get_level_build and compared with what the row names -- forcing a knob proves nothing if the plan decides otherwise.  Behind
the extent of every layout the frame's share of the buffer is zero.  Level 0 of a sparse call holds the expectation in the
flagged tiles and, on a fresh context, nothing elsewhere.  Afterwards the orientation maps of every frame equal the oracle's and
sbm_get_linear_memories (k_expand_lm, or the rebuild from the map) hands out the oracle's planes of frame 0.

  in process   LF.ROWS: sparse and whole bit strips, the strip plane by all-ty and per-ty threads, the spread plane row-major, the
               fused bit planes, spread + pack, the 8 planes with split 4 and 1, k_build_lm_any on every geometry of
               any_geometry_cases in both forms, the generic builder and the unfused path
  children     one fresh process per knob set (read once per process), one after another: LF.CHILD_ROWS

A child that ends by a signal or at its timeout stops the remaining children: nothing more is started on a GPU behind a fault
or a hang."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import lm_form_cases as LF
from shape_based_matching_amd import capi

pytestmark = pytest.mark.gpu

# measured on an MI355X (profiles/lm_forms_tests.txt): a child takes a few seconds, start of the interpreter included
CHILD_TIMEOUT = 120
SBM_ERR_INVALID, SBM_ERR_STATE = -1, -4  # include/sbm.h
_stopped = []  # the form whose child ended by a signal or at its timeout: no further child is started


def fail(what):
    pytest.fail(repr(what))


@pytest.mark.parametrize("rid", [r["id"] for r in LF.ROWS])
def test_stored_form_in_process(rid):
    r = [x for x in LF.ROWS if x["id"] == rid][0]
    done = LF.run_row(r, fail)
    w = LF.world(r["world"])
    assert done["levels"] == w.L and done["frames"] == w.L * r["frames"]
    if r["want"][0] == LF.SPARSE:
        assert done["flags"] is not None
        print("FLAGS", rid, json.dumps(done["flags"]))
    if r["flags"]:
        LF.check_flags(r, done["flags"])


def test_accessors_on_a_fresh_context_and_their_errors():
    """nothing built: no form, no builder; a buffer that is not allocated is a state error, a frame outside the batch an invalid one"""
    c = capi.Context(T=(4, 8), weak_threshold=LF.WEAK, device_id=0)
    try:
        for l in range(2):
            assert c.level_build(l) == (0, -1, 0, 0, 0, 0)
        with pytest.raises(capi.SbmError) as e:
            c.level_stored(0, 0, 0)
        assert e.value.code == SBM_ERR_STATE
        with pytest.raises(capi.SbmError) as e:
            c.level_build(2)
        assert e.value.code == SBM_ERR_INVALID
        w = LF.world("m48_144x320")
        for l in range(2):
            c.set_quantized(l, w.maps[0][l])
        assert c.level_build(0) == LF.w8(4) and c.level_build(1) == LF.w8(4)
        assert c.level_stored(0, 0, 0).size == 8 * c.get_linear_memories(0).shape[1]
        for args in ((0, 1, 0), (0, -1, 0), (0, 0, 4), (1, 0, 3), (2, 0, 0)):
            with pytest.raises(capi.SbmError) as e:
                c.level_stored(*args)
            assert e.value.code == SBM_ERR_INVALID, args
        with pytest.raises(capi.SbmError) as e:
            c.level_stored(0, 0, 2)  # set_quantized holds no bit strips
        assert e.value.code == SBM_ERR_STATE
    finally:
        c.close()


def test_a_replayed_graph_reports_the_build_it_was_captured_with():
    """the same batch three times with graph replay on: the record and the stored planes after the capture and after the replays"""
    import torch

    r = [x for x in LF.ROWS if x["id"] == "whole5_448"][0]
    w = LF.world(r["world"])
    c = capi.Context(T=w.T, weak_threshold=LF.WEAK, device_id=0)
    try:
        c.upload_templates(w.ts)
        c.set_graph_mode(True)
        B = r["frames"]
        fr = np.array(w.frames[:B])
        rows, cols, ch = fr.shape[1], fr.shape[2], fr.shape[3]
        dev = torch.device("cuda", 0)
        d_img = torch.from_numpy(np.ascontiguousarray(fr)).to(dev)
        d_out = torch.zeros(B * LF.CAP * LF.MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_cnt = torch.zeros(B * 2, dtype=torch.int32, device=dev)
        st = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        for call in range(3):
            c.match_batch_device(d_img.data_ptr(), rows * cols * ch, B, rows, cols, cols * ch, ch, LF.THR, d_out.data_ptr(), LF.CAP, d_cnt.data_ptr(),
                                 stream=st.cuda_stream)
            st.synchronize()
            assert c.graph_count() == 1
            for l in range(w.L):
                build = c.level_build(l)
                assert build == tuple(r["want"][l]), (call, l, build)
                for f in range(B):
                    LF.check_level(c, w, l, f, f, build, fail, "replay %d" % call)
    finally:
        c.close()


@pytest.mark.parametrize("form", list(LF.FORMS))
def test_forced_knobs_in_a_child(form):
    if _stopped:
        pytest.fail("the child of form %s ended by a signal or at its timeout: no further child is started" % _stopped[0])
    env = {k: v for k, v in os.environ.items() if k not in LF.KNOBS}
    env.update(LF.FORMS[form], PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lm_form_cases.py"), "--run", form], env=env, cwd=ROOT,
                             capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _stopped.append(form)
        pytest.fail("the child of form %s did not end within %d s" % (form, CHILD_TIMEOUT))
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139):
        _stopped.append(form)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    verdict = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("VERDICT ")][-1][8:])
    print("VERDICT", json.dumps(verdict))
    rows = LF.CHILD_ROWS[form]
    assert verdict["form"] == form and verdict["ok"] is True and verdict["rows"] == [r["id"] for r in rows]
    assert verdict["levels"] == sum(LF.world(r["world"]).L for r in rows)
    assert verdict["frames"] == sum(LF.world(r["world"]).L * r["frames"] for r in rows)
