"""tools/fuzz_sequence.py's generator on the CPU (no torch.cuda, no GPU): deterministic operation lists, coverage of every
operation kind, pyramid and graph mode over the GPU slice's seeds, the stream rule, and replayable prefixes."""
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
