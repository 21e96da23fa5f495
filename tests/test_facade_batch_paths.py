"""CPU (not gpu): the batch entry points of line2Dup::Detector (shape_based_matching_amd/facade/line2Dup_amd.cpp) pinned to
the engine calls they make, on a stand-in for the engine.

tests/emu/facade_driver.cpp (public include/line2Dup.h API only) is compiled here with the host compiler together with the
facade sources and tests/emu/fake_engine.cpp, which stands in for the C ABI functions the facade links: no GPU, no HIP, made-up
but deterministic records, a log of every call, failures and oversized lists where the driver scripts them.  The driver runs
matchBatch, matchAsync + wait and matchBatchNMS -- shared mask, a mask per frame (with an empty entry and a view that is not
continuous), no mask -- over 1, 2, 3 and 5 frames of 16 x 16 and 32 x 32, gray and BGR, on 1, 2 and 3 contexts, compares every
list with a loop of match() and prints the engine log.

tests/golden/facade_engine_trace.txt is that output recorded from the facade of the commit BEFORE the batch flow was written
once (three copies of it then), never from the tree under test: from the repository root, with PARENT that commit,

    d=$(mktemp -d); f=shape_based_matching_amd/facade
    mkdir -p $d/include $d/$f $d/tests/emu $d/shape_based_matching_amd/csrc
    cp include/*.h include/*.hpp $d/include/; git show PARENT:include/line2Dup.h > $d/include/line2Dup.h
    git show PARENT:$f/line2Dup_amd.cpp > $d/$f/line2Dup_amd.cpp; cp $f/cvlite.cpp $f/nms_c.cpp $d/$f/
    cp shape_based_matching_amd/csrc/sbm_resize_table.h $d/shape_based_matching_amd/csrc/
    cp tests/emu/facade_driver.cpp tests/emu/fake_engine.cpp tests/emu/fake_engine.h $d/tests/emu/
    src="tests/emu/facade_driver.cpp tests/emu/fake_engine.cpp $f/line2Dup_amd.cpp $f/cvlite.cpp $f/nms_c.cpp"
    (cd $d && g++ -std=c++14 -O1 -o driver $src -lz -lpthread)
    $d/driver 'tests/golden/case0_%s_templ.yaml.gz' circle all > tests/golden/facade_engine_trace.txt

The `threads` scenario (8 threads x 200 calls on one detector, every fifth a matchBatch of 3) is a stand-alone program built
with -fsanitize=thread: the lane pool's vector grows under the pool's mutex while other callers run, and a caller that indexed
it unlocked (that commit did) is a reported race."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

FACADE = os.path.join(ROOT, "shape_based_matching_amd", "facade")
SOURCES = [os.path.join(ROOT, "tests", "emu", n) for n in ("facade_driver.cpp", "fake_engine.cpp")] + [
    os.path.join(FACADE, n) for n in ("line2Dup_amd.cpp", "cvlite.cpp", "nms_c.cpp")]
TEMPLATES = [os.path.join(ROOT, "tests", "golden", "case0_%s_templ.yaml.gz"), "circle"]  # 89 templates
GOLDEN = os.path.join(ROOT, "tests", "golden", "facade_engine_trace.txt")
BEGIN, END = "sbm_match_batch_host_begin", "sbm_match_batch_host_end"


def cxx():
    found = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if found is None:
        pytest.fail("no host C++ compiler")
    return found


def build(out, *flags):
    subprocess.check_call([cxx(), "-std=c++14", "-Wall", "-Wextra", "-Wno-unused-parameter", *flags, "-o", out, *SOURCES, "-lz", "-lpthread"])
    return out


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    """the driver's output for every single-threaded scenario; the time limit turns a lane that was never given back (the
    scenarios after a failure run with one lane) into a failure instead of a hang"""
    exe = build(str(tmp_path_factory.mktemp("facade_driver") / "facade_driver"), "-O1")
    r = subprocess.run([exe, *TEMPLATES, "all"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.fixture(scope="module")
def scenarios(output):
    out = {}
    for block in output.split("== ")[1:]:
        title, _, body = block.partition("\n")
        assert title not in out
        out[title] = body.splitlines()
    return out


def calls(lines, name, ctx=None):
    """the logged calls of one engine function (exact name), optionally on one context"""
    return [l for l in lines if l.split(" ")[0] == name and (ctx is None or " ctx=%d " % ctx in l)]


def batch_calls(lines, ctx):
    return ([l for l in lines if l.startswith(BEGIN) and " ctx=%d " % ctx in l], [l for l in lines if l.startswith(END) and " ctx=%d " % ctx in l])


def test_every_batch_entry_point_returns_the_lists_of_match(scenarios):
    equal = {t: b for t, b in scenarios.items() if t.startswith("equal ")}
    seen = set()
    for title, body in equal.items():
        assert body[0] == "same=1 nonempty=1", title
        _, entry, masks, frames, shape, contexts = title.split(" ")
        n, d = int(frames.split("=")[1]), int(contexts.split("=")[1])
        seen.add((entry, masks))
        seen.add(("frames", n))
        seen.add(("contexts", d))
        seen.add(shape)
        # frames dealt in contiguous groups: every context with frames begins once and ends once, the others see neither
        for c in range(d):
            share = n * (c + 1) // d - n * c // d
            begins, ends = batch_calls(body, c)
            assert (len(begins), len(ends)) == ((1, 1) if share else (0, 0)), (title, c)
            if share:
                assert " n_frames=%d " % share in begins[0] and begins[0].endswith("-> 0")
        assert all(l.endswith("pending=0") for l in calls(body, "sbm_destroy")) and len(calls(body, "sbm_destroy")) == d
    for entry in ("matchBatch", "matchAsync+wait", "matchBatchNMS"):
        assert (entry, "no_mask") in seen and (entry, "mask_vector") in seen and (entry, "empty_mask_vector") in seen
        assert (entry, "shared_mask") in seen or (entry, "shared_mask_view") in seen
    assert {("frames", n) for n in (1, 2, 3, 5)} <= seen and {("contexts", d) for d in (1, 2, 3)} <= seen
    assert {"16x16x1", "16x16x3", "32x32x1", "32x32x3"} <= seen
    assert "equal matchBatch empty_mask_vector frames=2 32x32x1 contexts=3" in equal  # a context without frames
    # a mask per frame: the empty entry travels as NULL, the view as a continuous copy; no masks at all: the plain begin
    body = equal["equal matchBatch mask_vector frames=5 16x16x3 contexts=3"]
    assert re.search(r" masks=-,copy:[0-9a-f]{8} ", calls(body, BEGIN + "_masked", 1)[0])
    assert all(" mask=- " in l for l in calls(equal["equal matchBatch empty_mask_vector frames=2 32x32x1 contexts=3"], BEGIN))
    assert re.search(r" mask=copy:[0-9a-f]{8} ", calls(equal["equal matchAsync+wait shared_mask_view frames=5 32x32x1 contexts=2"], BEGIN, 0)[0])
    # NMS that drops boxes, against match() + NMSBoxes on the host
    assert equal["equal matchBatchNMS mask_vector frames=3 32x32x3 contexts=2"][0] == "same=1 nonempty=1"
    assert len(calls(equal["equal matchBatchNMS mask_vector frames=3 32x32x3 contexts=2"], END + "_nms")) == 2


def test_an_unknown_class_gives_empty_lists_and_no_batch(scenarios):
    body = scenarios["unknown_class"]
    assert body[:3] == ["matchBatch all_empty=1", "matchAsync+wait all_empty=1", "matchBatchNMS all_empty=1"]
    assert not [l for l in body if l.startswith(BEGIN) or l.startswith(END) or l.startswith("sbm_match ")]


@pytest.mark.parametrize("entry", ["matchBatch", "matchAsync+wait", "matchBatchNMS"])
def test_frames_over_the_batch_capacity_are_matched_again_alone(scenarios, entry):
    """frame 1 reports 1500 records (capacity 1024), frame 2 a negative count, frame 3 its overflow word, frame 5 5000 records
    (more than the 4096 the single-frame call starts with): each is matched again on context 0 under ITS mask (none, a copied
    view, M3, a copied view), frames 0 and 4 come from the batch; for NMS the host NMSBoxes finishes the redo"""
    body = scenarios["capacity %s mask_vector frames=6 16x16x3 contexts=2" % entry]
    assert body[0] == "same=1"
    redo = calls(body, "sbm_match")
    assert all(" ctx=0 " in l for l in redo)
    got = [(re.search(r"frame=(\S+)", l).group(1), re.search(r"mask=(\S+)", l).group(1).split(":")[0], re.search(r"cap=(\d+) -> (-?\d+)", l).groups())
           for l in redo]
    assert got == [("F1", "-", ("4096", "0")), ("F2", "copy", ("4096", "0")), ("F3", "M3", ("4096", "0")), ("F5", "copy", ("4096", "-3")),
                   ("F5", "copy", ("5000", "0"))]
    for c in (0, 1):
        begins, ends = batch_calls(body, c)
        assert len(begins) == 1 and len(ends) == 1 and ends[0].startswith(END + ("_nms " if entry == "matchBatchNMS" else " "))


@pytest.mark.parametrize("entry,where,code", [("matchBatch", "begin", "StsBadArg"), ("matchAsync+wait", "begin", "StsError"),
                                              ("matchBatchNMS", "begin", "StsError"), ("matchBatch", "end", "StsError"),
                                              ("matchAsync+wait", "end", "StsBadArg"), ("matchBatchNMS", "end", "StsBadArg")])
def test_a_failing_context_leaves_every_context_ended_and_the_lane_free(scenarios, entry, where, code):
    """SBM_ERR_INVALID becomes StsBadArg, every other code StsError (the scripted codes are -1, -2, -4 / -2, -1, -1); the text
    names the call that failed.  Afterwards, with ONE lane, a batch and an async batch go through"""
    title = ("begin_fails %s mask_vector frames=5 16x16x1 contexts=3" if where == "begin" else "end_fails %s mask_vector frames=3 16x16x1 contexts=2") % entry
    body = scenarios[title]
    failed = END + "_nms" if (entry, where) == ("matchBatchNMS", "end") else BEGIN if where == "begin" else END
    assert body[0] == "%s throws %s text=[%s: scripted: %s refused]" % (entry, code, failed, where)
    cut = body.index("-- afterwards, on the one lane")
    before, after = body[:cut], body[cut + 1:]
    if where == "begin":  # on context 1 of 3: context 0 is ended exactly once, context 2 sees nothing
        assert [len(x) for x in batch_calls(before, 0)] == [1, 1] and batch_calls(before, 0)[1][0].startswith(END + " ")
        assert [len(x) for x in batch_calls(before, 1)] == [1, 0] and not batch_calls(before, 1)[0][0].endswith("-> 0")
        assert [len(x) for x in batch_calls(before, 2)] == [0, 0]
    else:  # on context 0 of 2: context 1 is still ended
        for c in (0, 1):
            assert [len(x) for x in batch_calls(before, c)] == [1, 1]
        assert not batch_calls(before, 0)[1][0].split(" counts")[0].endswith("-> 0")
    assert all(" pending=1 " in l for l in before if l.startswith(END))  # nothing was ended twice
    assert after[:2] == ["recovered_batch=1", "recovered_async=1"]
    assert all(l.endswith("pending=0") for l in calls(after, "sbm_destroy"))


def test_one_batch_in_flight_and_a_match_in_between(scenarios):
    body = scenarios["async_rules"]
    assert body[:9] == ["wait with nothing in flight throws StsAssert", "match between matchAsync and wait, one lane: same=1",
                        "second matchAsync throws StsAssert", "wait same=1", "matchAsync without frames throws StsAssert",
                        "matchBatch without frames: lists=0", "matchBatchNMS without frames: lists=0", "recovered_batch=1", "recovered_async=1"]
    # the batch in flight keeps its lane (context 0), the match in between gets a second one although one is the limit
    assert len(calls(body, "sbm_create")) == 2 and " ctx=1 " in calls(body, "sbm_match")[0]


def test_pinned_buffers_and_a_list_longer_than_the_first_buffer(scenarios):
    body = scenarios["pins_and_growth"]
    assert body[0] == "same=1"
    assert [l.split(" buffer=")[1].split(" ")[0] for l in body if "pin_host_buffer" in l] == ["F0", "F0"]
    assert [re.search(r"cap=(\d+) -> (-?\d+)", l).groups() for l in calls(body, "sbm_match") if "frame=F1" in l] == [("4096", "-3"), ("5000", "0")]


def test_the_engine_calls_are_those_of_the_three_copies(output):
    """every single-threaded scenario: results, exception texts and the engine log, line for line what the facade made when
    each entry point carried its own copy of the batch flow (recorded from that commit, see the module docstring)"""
    with open(GOLDEN) as f:
        golden = f.read()
    assert 100 < golden.count("\n") < 600
    assert output.splitlines() == golden.splitlines()


def tsan_works(tmp):
    src, exe = os.path.join(tmp, "hello.cpp"), os.path.join(tmp, "hello")
    with open(src, "w") as f:
        f.write("#include <thread>\nint main() { int x = 0; std::thread t([&] { x = 1; }); t.join(); return x - 1; }\n")
    try:
        subprocess.check_call([cxx(), "-fsanitize=thread", "-static-libtsan", "-O1", "-g", "-o", exe, src, "-lpthread"], stderr=subprocess.DEVNULL)
        return subprocess.run([exe], timeout=60, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    except (subprocess.CalledProcessError, OSError, subprocess.TimeoutExpired):
        return False


def test_concurrent_callers_under_thread_sanitizer(tmp_path):
    """8 threads x 200 calls, every fifth a matchBatch of 3, on one detector with 8 lanes and with 2: no report, exit 0, every
    list equal to the single caller's.  A host program on the fake engine, run on its own (nothing is preloaded)"""
    if not tsan_works(str(tmp_path)):
        pytest.skip("the host compiler cannot build and run a ThreadSanitizer program")
    exe = build(str(tmp_path / "facade_driver_tsan"), "-fsanitize=thread", "-static-libtsan", "-O1", "-g")
    for lanes in (8, 2):
        r = subprocess.run([exe, *TEMPLATES, "threads", str(lanes)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert "ThreadSanitizer" not in r.stdout, r.stdout[:4000]
        assert r.returncode == 0, r.stdout[-2000:]
        assert re.search(r"^threads 8 calls 200 lanes %d matches \d+ \d+ different 0$" % lanes, r.stdout, re.M), r.stdout[-2000:]
