"""-m gpu: every form of the coarse pass at its feature-count and position-count edges (inputs and the numpy reference:
coarse_form_cases.py; tests/test_coarse_form_cases.py proves them without a GPU).

On a one-level pyramid the coarse pass emits the match list itself, so the list is the whole score map above the threshold:
a raw score off by one, a position lost at a work-item boundary or a record kept at score == threshold shows as a differing
record.  Which kernel ran is read from sbm_get_coarse_form and compared with the host rule restated in
coarse_form_cases.expected_form -- forcing a knob proves nothing if the heuristics win anyway.

  in process   modes auto | block | wave | bits on both geometries, every group and threshold; the batched slice in auto
  children     one fresh process per forced form (the SBM_BITS_* knobs are read once per process), one after another:
               the eight-wave form, and the one-wave form with 1 | 2 dwords per lane x the wide | narrow schedule --
               <13, true, 2> and the narrow schedule at 64 features or more are reached only this way

A child that ends by a signal or at its timeout stops the remaining children: nothing more is started on a GPU behind a
fault or a hang."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import coarse_form_cases as CF
from shape_based_matching_amd import capi

pytestmark = pytest.mark.gpu

# measured on an MI355X (profiles/coarse_forms.txt): a child takes 2.6 - 3.6 s, start of the interpreter included
CHILD_TIMEOUT = 60
_stopped = []  # the form whose child ended by a signal or at its timeout: no further child is started


def n_simd():
    import torch

    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def contexts():
    """one context per geometry, the map installed once"""
    made = {}
    for geo in CF.GEOS:
        w = CF.world(geo)
        c = capi.Context(T=(w.T,), weak_threshold=30.0, device_id=0, max_candidates=CF.MAX_CANDIDATES)
        c.upload_templates(w.ts)
        c.set_quantized(0, w.q)
        made[geo] = c
    yield made
    for c in made.values():
        c.close()


@pytest.mark.parametrize("mode", ["auto", "block", "wave", "bits"])
@pytest.mark.parametrize("geo", list(CF.GEOS))
def test_every_group_and_threshold_in_process(contexts, geo, mode):
    w, c = CF.world(geo), contexts[geo]
    c.set_coarse_mode(mode)
    simd = n_simd()
    n = 0
    for g in CF.GROUPS:
        c.select_templates(w.groups[g])
        for thr, name, _, _ in w.thresholds[g]:
            got = CF.as_rows(c.match_templates(thr))  # (a candidate or output overflow is an error of the call)
            form = c.coarse_form()
            want = w.reference(w.groups[g], thr)
            assert CF.first_difference(want, got) is None, (mode, geo, g, name, thr, CF.first_difference(want, got))
            if mode in ("auto", "bits"):
                # the host rule: P by the group's largest count, wide iff that count >= 64, P = 13 always with one dword
                assert form == CF.group_form(w, g, 1, simd, {}), (mode, geo, g, name)
                P = 7 if w.nf[w.groups[g]].max() < 128 else (10 if w.nf[w.groups[g]].max() < 1024 else 13)
                assert form[1] == P and (form[0] == 4 or (form[2] == int(w.nf[w.groups[g]].max() >= 64) and (P < 13 or form[3] == 1)))
            else:
                assert form == ({"block": 1, "wave": 2}[mode], 0, 0, 0), (mode, geo, g, name)
            n += 1
    assert n == len(w.cases())
    c.set_coarse_mode("auto")
    c.select_templates(list(range(w.ts.n_templates)))


def test_coarse_form_accessor_changes_nothing(contexts):
    """read before, between and after two identical calls: the same lists, the same record"""
    w, c = CF.world("T4"), contexts["T4"]
    c.set_coarse_mode("auto")
    c.select_templates(w.groups["mid"])
    thr = w.thresholds["mid"][3][0]
    a = CF.as_rows(c.match_templates(thr))
    f1 = c.coarse_form()
    f2 = c.coarse_form()
    b = CF.as_rows(c.match_templates(thr))
    assert f1 == f2 == c.coarse_form() and f1[0] in (3, 4)
    assert np.array_equal(a, b) and CF.first_difference(w.reference(w.groups["mid"], thr), b) is None
    fresh = capi.Context(T=(4,), weak_threshold=30.0, device_id=0)
    assert fresh.coarse_form() == (0, 0, 0, 0)  # nothing launched yet
    fresh.close()
    c.select_templates(list(range(w.ts.n_templates)))


def test_batched_slice_in_process():
    """three frames (noise, scene, all zero) through sbm_match_batch_device: the frame index and the planes' frame stride"""
    w = CF.world("T4")
    c = capi.Context(T=(4,), weak_threshold=30.0, device_id=0, max_candidates=CF.MAX_CANDIDATES)
    c.upload_templates(w.ts)

    def fail(what):
        pytest.fail(repr(what))

    try:
        cases, records = CF.run_batch_slice(c, {}, n_simd(), "auto", fail)
    finally:
        c.close()
    assert cases == CF.batch_case_count() and records > 0


@pytest.mark.parametrize("form", list(CF.FORMS))
def test_forced_form_in_a_child(form):
    if _stopped:
        pytest.fail("the child of form %s ended by a signal or at its timeout: no further child is started" % _stopped[0])
    env = {k: v for k, v in os.environ.items() if k not in CF.KNOBS}
    env.update(CF.FORMS[form], PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "coarse_form_cases.py"), "--run", form], env=env, cwd=ROOT,
                             capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _stopped.append(form)
        pytest.fail("the child of form %s did not end within %d s" % (form, CHILD_TIMEOUT))
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139):
        _stopped.append(form)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    counts = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("COUNTS ")][-1][7:])
    print("COUNTS", json.dumps(counts))
    n_cases = sum(len(CF.world(geo).cases()) for geo in CF.GEOS)
    assert counts["form"] == form and counts["cases"] == n_cases == 90 and counts["records"] > 0
    assert counts["batch_cases"] == (CF.batch_case_count() if form in CF.BATCH_FORMS else 0)
    assert counts["two_level"] == len(CF.TWO_LEVEL)
    # the forms the child proved by sbm_get_coarse_form: every counter width, under the forced schedule
    ran = {tuple(f) for f in counts["forms"]}
    if form == "block":
        assert ran == {(4, 7, 0, 0), (4, 10, 0, 0), (4, 13, 0, 0)}
    else:
        dw, wide = int(CF.FORMS[form]["SBM_BITS_DW"]), int(CF.FORMS[form]["SBM_BITS_WIDE"])
        assert ran == {(3, 7, wide, dw), (3, 10, wide, dw), (3, 13, 1, dw)}
