"""-m gpu: every form of the refinement pass at its counter, accumulator, class-run and patch edges (inputs and the numpy
reference: refine_form_cases.py; tests/test_refine_form_cases.py proves them without a GPU).

Two-level pyramids whose candidates refine over saturated regions (every feature scores 4 at every patch cell: slot counters
and byte accumulators run full, the whole patch ties), at all 16 window columns and rows, with the best cell in every patch
corner, at thresholds exactly on a refined score and one ulp either side.  Which kernel ran is read from sbm_get_refine_form
and compared with the host rule restated in refine_form_cases.expected_form.

  in process   world M through set_quantized + match_templates (8 response planes | whole bit strips), worlds I48 / I88 / I17
               through match (spread strips at T = 4 and T = 8 | sparse bit strips | response planes), every group and threshold
               in every set_refine_bits mode; the batched slices through match_batch_device in both refinement orders
  children     one fresh process per knob set (the SBM_* knobs are read once per process), one after another; each runs
               every template of every world at every threshold of the group "all" in every set_refine_bits mode and the
               batched slices, and reports the set of records it saw

A child that ends by a signal or at its timeout stops the remaining children: nothing more is started on a GPU behind a
fault or a hang."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import refine_form_cases as RF
from coarse_form_cases import as_rows, first_difference
from shape_based_matching_amd.templates import MATCH_DTYPE

pytestmark = pytest.mark.gpu

# measured on an MI355X (profiles/refine_forms.txt): a child takes 5.1 - 6.6 s, start of the interpreter included
CHILD_TIMEOUT = 120
_stopped = []  # the form whose child ended by a signal or at its timeout: no further child is started


ENV_KNOBS = {k: os.environ[k] for k in RF.KNOBS if os.environ.get(k)}  # what this process itself runs under: none, normally


def fail(what):
    pytest.fail(repr(what))


@pytest.fixture(scope="module")
def contexts():
    """one context per world"""
    made = {name: RF.make_context(name) for name in RF.WORLDS}
    yield made
    for c in made.values():
        c.close()


@pytest.mark.parametrize("bits", RF.BITS_MODES, ids=["default", "bits", "bytes"])
@pytest.mark.parametrize("name", list(RF.WORLDS))
def test_every_group_and_threshold_in_process(contexts, name, bits):
    w = RF.world(name)
    cases, records, form = RF.run_world(name, contexts[name], bits, ENV_KNOBS, "in process", fail)
    assert cases == len(w.cases()) and records > 0
    want = {"M": {True: (4, 1, 0, 0, 0, 2048), False: (1, 16, 0, 0, 0, 512)}, "I48": {True: (4, 1, 0, 0, 1, 2048), False: (3, 16, 0, 0, 0, 512)},
            "I88": {True: (3, 16, 0, 1, 0, 512), False: (3, 16, 0, 1, 0, 512)}, "I17": {True: (1, 16, 0, 0, 0, 512), False: (1, 16, 0, 0, 0, 512)}}
    if bits is not None or not bool(ENV_KNOBS):
        assert form == want[name][bits is not False]


def test_slots_follow_the_pipeline_depth(contexts):
    """several batches in flight: 128 slots per frame (512 for the bit form) instead of 512 (2048)"""
    c = contexts["M"]
    c.set_pipeline_depth(2)
    try:
        for bits, slots in ((True, 512), (False, 128)):
            _, _, form = RF.run_world("M", c, bits, ENV_KNOBS, "depth 2", fail, groups=["thin"], depth=2)
            assert form[5] == slots or bool(ENV_KNOBS)
    finally:
        c.set_pipeline_depth(1)


def test_refine_form_accessor_changes_nothing(contexts):
    """read before, between and after two identical calls: the same lists, the same record; a fresh context reports kind 0"""
    w, c = RF.world("M"), contexts["M"]
    c.set_refine_bits(True)
    c.select_templates(w.groups["thin"])
    thr = w.thresholds["thin"][2][0]
    f0 = c.refine_form(0)
    a = as_rows(c.match_templates(thr))
    f1 = c.refine_form(0)
    f2 = c.refine_form(0)
    b = as_rows(c.match_templates(thr))
    assert f1 == f2 == c.refine_form(0) and f1[0] in (1, 4) and f0[0] in (0, 1, 4)
    assert np.array_equal(a, b) and first_difference(w.reference(w.groups["thin"], thr), b) is None
    from shape_based_matching_amd import capi

    fresh = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0)
    assert fresh.refine_form(0) == (0, 0, 0, 0, 0, 0)  # nothing launched yet
    with pytest.raises(capi.SbmError):
        fresh.refine_form(1)  # the coarsest level has no refinement pass
    fresh.close()
    c.select_templates(list(range(w.ts.n_templates)))


def test_a_replayed_graph_reports_the_form_it_was_captured_with():
    """the template loop captured on whole bit strips, then replayed on the same maps installed again: the same list and the same
    record.  (Every call that changes the form -- sbm_set_refine_bits, sbm_set_refine_order, another entry point -- drops the
    captured graphs, so a replay never meets a record other than its own.)"""
    import torch

    dev = torch.device("cuda", 0)
    w = RF.world("M")
    c = RF.make_context("M")
    try:
        c.set_refine_bits(True)
        c.set_pipeline_depth(2)
        c.set_graph_mode(True)
        c.select_templates(w.groups["thin"])
        thr = w.thresholds["thin"][2][0]
        want = w.reference(w.groups["thin"], thr)
        cap = 4096
        d_out = torch.zeros(cap * MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
        st = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()

        def loop():
            for l in range(2):
                c.set_quantized(l, w.maps[l])
            c.match_templates_device(thr, d_out.data_ptr(), cap, d_cnt.data_ptr(), stream=st.cuda_stream)
            st.synchronize()
            rows = as_rows(d_out.cpu().numpy().view(MATCH_DTYPE)[: int(d_cnt.cpu().numpy()[0])])
            assert first_difference(want, rows) is None
            return c.refine_form(0)

        captured = loop()
        n_graphs = c.graph_count()
        assert captured == RF.expected_form("M", "templates", True, depth=2) or bool(ENV_KNOBS)
        assert loop() == captured and c.graph_count() == n_graphs >= 1  # a replay
        assert loop() == captured and c.graph_count() == n_graphs
    finally:
        c.close()


@pytest.mark.parametrize("order", ["slots", "list"])
@pytest.mark.parametrize("bits", [True, False], ids=["bits", "bytes"])
@pytest.mark.parametrize("name", list(RF.BATCH))
def test_batched_slice_in_process(contexts, name, bits, order):
    """eight (four) frames -- the world's image, its shifts, an all-zero frame -- through sbm_match_batch_device"""
    cases, records, form = RF.run_batch_slice(name, contexts[name], bits, order, ENV_KNOBS, "in process", fail)
    assert cases == RF.BATCH[name] * len(RF.batch_slice(name)[2]) and records > 0
    if not bool(ENV_KNOBS):
        kind = {"I48": 4 if bits else 3, "I17": 2}[name]
        assert form == (kind, 1 if kind == 4 else 4, 2 if order == "list" else 0, 0, int(kind == 4), 2048 if kind == 4 else 512)


@pytest.mark.parametrize("bits", [True, False], ids=["bits", "bytes"])
def test_threshold_on_an_intermediate_level_score(bits):
    """three levels: the planted candidate's level-1 score equals the threshold (kept: raw == next_keep where the record goes on
    to level 0), and is one ulp below it (dropped, though its level-0 score is far higher); the oracle is the reference"""
    from shape_based_matching_amd import capi

    maps, ts, thr, at, above, home = RF.three_level_case()
    c = capi.Context(T=RF.THREE_T, weak_threshold=30.0, device_id=0, max_candidates=1 << 16)
    try:
        c.upload_templates(ts)
        c.set_refine_bits(bits)
        for l in range(3):
            c.set_quantized(l, maps[l])
        assert first_difference(at, as_rows(c.match_templates(thr))) is None
        assert first_difference(above, as_rows(c.match_templates(float(np.nextafter(np.float32(thr), np.float32(200)))))) is None
        if not bool(ENV_KNOBS):
            assert c.refine_form(0)[0] == (4 if bits else 1) and c.refine_form(1)[0] == 1  # level 1 (T = 8) on the response planes
    finally:
        c.close()


@pytest.fixture(scope="module")
def cache_dir(tmp_path_factory):
    """the worlds with every reference computed, for the children to load instead of building them again"""
    d = tmp_path_factory.mktemp("refine_form_cases")
    for name in RF.WORLDS:
        w = RF.world(name)
        for g, thr, _ in w.cases():
            w.reference(w.groups[g], thr)
    for name in RF.BATCH:
        w = RF.world(name)
        _, per, thrs = RF.batch_slice(name)
        for sc, raw1 in per:
            for thr in thrs:
                w.reference(RF.batch_templates(w), thr, sc, raw1)
    RF.save_cache(str(d))
    return str(d)


@pytest.mark.parametrize("form", list(RF.FORMS))
def test_forced_knobs_in_a_child(form, cache_dir):
    if _stopped:
        pytest.fail("the child of form %s ended by a signal or at its timeout: no further child is started" % _stopped[0])
    env = {k: v for k, v in os.environ.items() if k not in RF.KNOBS}
    env.update(RF.FORMS[form], PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    env[RF.CACHE_ENV] = cache_dir
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "refine_form_cases.py"), "--run", form], env=env, cwd=ROOT,
                             capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _stopped.append(form)
        pytest.fail("the child of form %s did not end within %d s" % (form, CHILD_TIMEOUT))
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139):
        _stopped.append(form)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    counts = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("COUNTS ")][-1][7:])
    print("COUNTS", json.dumps(counts))
    n_cases = sum(len(RF.world(name).thresholds[g]) for name in RF.WORLDS for g in RF.CHILD_GROUPS) * len(RF.BITS_MODES)
    n_batch = sum(B * len(RF.batch_slice(name)[2]) for name, B in RF.BATCH.items()) * 4
    assert counts["form"] == form and counts["cases"] == n_cases and counts["records"] > 0
    assert counts["batch_cases"] == n_batch and counts["batch_records"] > 0
    # the records the child proved by sbm_get_refine_form, under its knobs
    ran = sorted(tuple(f) for f in counts["forms"])
    assert ran == RF.expected_child_forms(form)
    rec = {f[2:] for f in ran}
    if form == "waves4":
        assert (3, 4, 0, 0, 0, 512) in rec and not any(f[1] == 16 for f in rec)  # LW 4 meets a single frame
    elif form == "waves16":
        assert (3, 16, 2, 0, 0, 512) in rec and not any(f[1] == 4 for f in rec)  # LW 16 meets a batch, in both orders
    elif form == "grid3":
        assert {f[5] for f in rec} == {3}
    elif form == "strip_lm0":
        assert {f[0] for f in rec} == {1, 2}  # no strips of either kind
    elif form == "full_lm1":
        assert {f[0] for f in rec} == {1}
    elif form == "lm_allty0":
        assert {f[0] for f in rec} == {1, 2, 3}  # strips built by the per-row threads, never bit strips
    elif form == "sparse_strips0":
        assert 4 in {f[0] for f in rec} and {f[4] for f in rec} == {0}
    elif form == "local_bits0":
        assert ("I48", "single", 4, 1, 0, 0, 1, 2048) in ran and ("I48", "single", 3, 16, 0, 0, 0, 512) in ran
