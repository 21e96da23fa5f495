"""tools/fuzz_sequence.py's generator on the CPU (no torch.cuda, no GPU): deterministic operation lists, coverage of every
operation kind, pyramid and graph mode over the GPU slice's seeds, the stream rule, and replayable prefixes; the "sparse"
profile's slice counted against the conditions it exists for (sparse-eligible calls per entry point, readers behind them)."""
import os
import shlex
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_sequence as F  # noqa: E402

SLICE = (5, 12, 25)  # seed, sequences, steps of tests/test_gpu_sequences.py::test_sequence_fuzz_slice


def test_same_seed_same_operations():
    seed, n, steps = SLICE
    for i in range(n):
        assert F.generate(seed, i, steps) == F.generate(seed, i, steps)
    assert F.generate(seed, 0, steps) != F.generate(seed + 1, 0, steps)


def test_slice_covers_every_operation_pyramid_and_graph_mode():
    seed, n, steps = SLICE
    kinds, pyramids, graph = set(), set(), set()
    for i in range(n):
        T, ops = F.generate(seed, i, steps)
        assert len(ops) == steps
        pyramids.add(T)
        kinds.update(o["op"] for o in ops)
        graph.update(o["mode"] for o in ops if o["op"] == "set_graph_mode")
        # an asynchronous stretch in every sequence: two device calls with no checkpoint between them
        run, best = 0, 0
        for o in ops:
            run = 0 if o["op"] in ("checkpoint", "switch_stream") else run + (o["op"] in ("match_device", "match_batch_device",
                                                                                            "match_banded", "match_templates_device"))
            best = max(best, run)
        assert best >= 2, i
    assert kinds == set(F.ALL_OPS), set(F.ALL_OPS) - kinds
    assert pyramids == set(F.PYRAMIDS)
    assert graph == set(F.GRAPH_MODES)


def test_stream_switch_only_after_synchronisation():
    for seed in (1, 5, 7, 123):
        for i in range(40):
            _, ops = F.generate(seed, i, 60)
            for k, o in enumerate(ops):
                if o["op"] == "switch_stream":
                    assert k > 0 and ops[k - 1]["op"] == "checkpoint", (seed, i, k)
                if o["op"] == "nms":  # the previous batch call ran on the same stream, under the same template upload
                    prev = [p["op"] for p in ops[:k]]
                    last_switch = max([j for j, p in enumerate(prev) if p in ("switch_stream", "upload_templates")], default=-1)
                    assert any(p in ("match_batch_device", "match_banded") for p in prev[last_switch + 1:]), (seed, i, k)


def test_thresholds_at_or_below_zero_only_with_one_template_or_none():
    for seed in (1, 5):
        for i in range(30):
            _, ops = F.generate(seed, i, 60)
            n_set = n_active = F.SET_SIZES[0]
            for o in ops:
                if o["op"] == "upload_templates":
                    n_set = n_active = F.SET_SIZES[o["set"]]
                elif o["op"] == "select_all":
                    n_active = n_set
                elif o["op"] == "select_empty":
                    n_active = 0
                elif o["op"] in ("select_range", "select_templates"):
                    n_active = o.get("count", len(o.get("idx", [])))
                elif o["op"] == "select_classes":
                    n_active = sum((n_set + 1 - c) // 2 for c in o["classes"])
                if "thr" in o and o["thr"] <= 0:
                    assert n_active <= 1, (seed, i, o)


def test_replayed_prefix_equals_original_prefix():
    seed, n, steps = SLICE
    for i in range(n):
        _, ops = F.generate(seed, i, steps)
        for stop in (0, 7, steps - 1):
            # the replay line of a failure: --only i --steps steps --stop stop
            T, again = F.generate(seed, i, steps)
            assert again[: stop + 1] == ops[: stop + 1]
        # a longer run of the same sequence starts with the same operations
        assert F.generate(seed, i, steps + 10)[1][:steps] == ops


def test_printed_replay_line_parses_back_to_the_same_prefix():
    """the replay line a failure prints, parsed by the tool's own argument parser, names the same sequence and prefix"""
    seed, n, steps = SLICE
    for i, stop in ((0, 0), (3, 11), (n - 1, steps - 1)):
        argv = shlex.split(F.replay_command(seed, i, steps, stop))
        assert argv[:2] == ["python", "tools/fuzz_sequence.py"]
        a = F.parse_args(argv[2:])
        assert (a.n, a.seed, a.only, a.steps, a.stop) == (1, seed, i, steps, stop)
        # Runner.run(seed, only, steps, stop) applies generate(seed, only, steps)[1][: stop + 1]
        assert F.generate(a.seed, a.only, a.steps)[1][: a.stop + 1] == F.generate(seed, i, steps)[1][: stop + 1]


# ---- the sparse profile -------------------------------------------------------------------------------------------------

SPARSE_SLICE = (3, 8, 30)  # seed, sequences, steps of tests/test_gpu_sequences.py::test_sparse_sequence_fuzz_slice
NEW_GEOS = {"P": (448, 576, 3), "Q": (512, 704, 1)}


def eligible(T, qmode, op):
    """the issue's predicate, restated: T = (4, 8), stream mode, a 16-cell-aligned geometry, no mask, not banded"""
    return (T == (4, 8) and qmode == "stream" and op["op"] in ("match", "match_device", "match_batch_device", "match_batch_host")
            and (F.ALL_GEOS[op["geo"]][1] // 4) % 16 == 0 and not op["mask"])


def sparse_counts(seed, n, steps):
    """what the sparse slice contains, from the operation lists alone"""
    FRAME_TAKING = ("match", "match_device", "match_batch_device", "match_batch_host", "match_banded", "build_pyramid")
    READERS = ("get_quantized", "get_quantized_frame", "match_templates", "match_templates_device", "set_quantized")
    c = {"eligible": 0, "by": {}, "readers": 0, "clobbered_readers": 0, "grow": 0, "shrink": 0, "channel_switch_readers": 0,
         "geos": set(), "row_pads": set(), "frame_pads": set(), "left_and_back": 0, "frame_reads_past_0": 0, "profiled": {}}
    for i in range(n):
        T, ops = F.generate(seed, i, steps, "sparse")
        assert T == (4, 8) and len(ops) == steps
        assert ops[0]["op"] == "set_quantize_mode" and ops[0]["mode"] == "stream" and ops[0]["hs"] in (8, 18, 32)
        qmode = "auto"
        behind_sparse_batch = clobbered = False  # no frame-taking call since a sparse-eligible device batch / a clobber since it
        last_eligible_B = None                   # frames of the last eligible device batch of this sequence
        last_ch = None                           # channels of the last frame-taking call
        switched = False                         # ... which differed from those of the one before; no frame-taking call since
        last_B = 0
        for k, o in enumerate(ops):
            name = o["op"]
            if name == "set_quantize_mode":
                c["left_and_back"] += qmode != "stream" and o["mode"] == "stream" and k > 0
                qmode = o["mode"]
            is_reader = name in READERS or (name in ("get_linear_memories", "similarity_local") and o["level"] == 0)
            if name in ("get_quantized", "get_quantized_frame") and o["level"] != 0:
                is_reader = False
            if is_reader:
                c["readers"] += behind_sparse_batch
                c["clobbered_readers"] += behind_sparse_batch and clobbered
                c["channel_switch_readers"] += switched
                switched = False
            if name == "get_quantized_frame":
                assert 0 <= o["frame"] < max(last_B, 1), (i, k)
                c["frame_reads_past_0"] += o["frame"] > 0
            if name == "clobber_inputs":
                assert ops[k - 1]["op"] == "checkpoint", (i, k)
                clobbered = True
            if name in FRAME_TAKING or name == "set_quantized":
                ch = F.ALL_GEOS[o["geo"]][2]
                if name != "set_quantized":
                    switched = last_ch is not None and ch != last_ch
                    last_ch = ch
                behind_sparse_batch = clobbered = False
                last_B = len(o["vars"]) if name == "match_batch_device" else 1
                c["geos"].add(o["geo"])
                if "row_pad" in o:
                    c["row_pads"].add(o["row_pad"])
                if "frame_pad" in o:
                    c["frame_pads"].add(o["frame_pad"])
                assert ("row_pad" in o) == (name in ("match_device", "match_batch_device", "match_banded")), (i, k)
                assert ("frame_pad" in o) == (name in ("match_batch_device", "match_banded")), (i, k)
            if name in FRAME_TAKING and eligible(T, qmode, o):
                c["eligible"] += 1
                c["by"][name] = c["by"].get(name, 0) + 1
                if o["profiled"]:  # the Runner counts the gradient launches of these
                    c["profiled"][name] = c["profiled"].get(name, 0) + 1
                if name == "match_batch_device":
                    B = len(o["vars"])
                    if last_eligible_B is not None:
                        c["grow"] += B > last_eligible_B
                        c["shrink"] += B < last_eligible_B
                    last_eligible_B = B
                    behind_sparse_batch = True
    return c


def test_sparse_profile_is_deterministic_and_leaves_the_default_profile_alone():
    seed, n, steps = SPARSE_SLICE
    for i in range(n):
        assert F.generate(seed, i, steps, "sparse") == F.generate(seed, i, steps, "sparse")
        assert F.generate(seed, i, steps + 7, "sparse")[1][:steps] == F.generate(seed, i, steps, "sparse")[1]
        assert F.generate(seed, i, steps, "default") == F.generate(seed, i, steps)
        assert F.generate(seed, i, steps, "sparse") != F.generate(seed, i, steps)
    for name, g in NEW_GEOS.items():
        assert F.SPARSE_GEOS[name] == g and name not in F.GEOS  # the default profile draws from GEOS: it must not grow
        assert (g[1] // 4) % 32 == 16                            # a cut last tile column
    assert set(F.SPARSE_GEOS) == {"A", "B", "G", "P", "Q"}
    a = F.parse_args(shlex.split(F.replay_command(seed, 3, steps, 11, "sparse"))[2:])
    assert (a.n, a.seed, a.only, a.steps, a.stop, a.profile) == (1, seed, 3, steps, 11, "sparse")
    assert F.parse_args(shlex.split(F.replay_command(seed, 3, steps, 11))[2:]).profile == "default"


def test_default_slice_has_no_sparse_eligible_call():
    """why the second profile exists: the default slice never takes the sparse level-0 path"""
    seed, n, steps = SLICE
    total = 0
    for i in range(n):
        T, ops = F.generate(seed, i, steps)
        qmode = "auto"
        for o in ops:
            if o["op"] == "set_quantize_mode":
                qmode = o["mode"]
            total += eligible(T, qmode, o)
            assert eligible(T, qmode, o) == F.sparse_eligible(T, qmode, o) if "geo" in o and "mask" in o else True
    assert total == 0


def test_sparse_slice_meets_its_conditions():
    """conditions on the generator (not measurements), for the pinned seed of the GPU slice"""
    seed, n, steps = SPARSE_SLICE
    assert n <= 8 and steps <= 30
    c = sparse_counts(seed, n, steps)
    assert c["eligible"] >= 40, c
    for entry in ("match_batch_device", "match_device", "match", "match_batch_host"):
        assert c["by"].get(entry, 0) >= 4, c
    assert c["readers"] >= 10, c
    assert c["clobbered_readers"] >= 3, c
    assert c["grow"] >= 3 and c["shrink"] >= 3, c
    assert c["channel_switch_readers"] >= 2, c
    assert c["geos"] >= set(NEW_GEOS), c
    assert c["row_pads"] == {0, 13, 64} and c["frame_pads"] == {0, 1000, -1}, c
    assert c["left_and_back"] >= 1 and c["frame_reads_past_0"] >= 1, c
    for entry in ("match_batch_device", "match_device", "match", "match_batch_host"):
        assert c["profiled"].get(entry, 0) >= 2, c  # ... each proven sparse on the GPU by its launch count
