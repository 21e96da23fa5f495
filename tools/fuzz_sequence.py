#!/usr/bin/env python3
"""Randomised call sequences on ONE engine context against the CPU oracle (GPU box; test infrastructure).

tools/fuzz_match.py makes a fresh context per case, so it never reaches a state transition of an ``sbm_ctx``: the per-level
record of current forms (``LevelForms``, sbm_level_forms.h), the forms rebuilt lazily by the stage and template-loop
entry points, the graph cache, cached thresholds and feature offsets, and the caller's stream next to the context's own.
Here every sequence creates one context with a drawn pyramid, draws ``steps`` operations (match entry points, pyramid
state, stage reads, template uploads and selections, mode switches, thresholds) and applies them to it.  Device entry
points are enqueued on a caller-owned non-blocking torch stream and are NOT synchronised one by one: each writes its own
output buffers, and the results are synchronised and compared with the oracle at drawn checkpoints and at the end.

The generator obeys the caller's side of the contract (include/sbm.h):
  * a sequence switches to a second caller stream only right after a host synchronisation (a checkpoint);
  * host-memory entry points (match, match_batch_host, build_pyramid, set_quantized, match_templates) and stage reads
    (get_*, similarity*) may synchronise inside the library, and are ordered after everything enqueued before them;
  * a device buffer handed to a call is not reused before the call's results were synchronised.
Under these rules any wrong list, map or refusal is a library bug.

No oracle work stands between two library calls: the oracle pyramids of every frame a sequence uses are built before its
first call, and expected lists are evaluated only at checkpoints, after the host synchronisation.  After a host or banded
batch the resident frame is not named by the ABI; results that depend on it are counted as unchecked and reported.

Expected values: match lists as multisets against oracle.Pyramid.match (active template subset, the context's T, the
threshold and the mask); stage reads byte for byte against the oracle's maps, linear memories, packed bit planes and
similarity maps; device NMS against tests/test_gpu_nms_device.expected.  Where the library legitimately refuses
(SBM_ERR_STATE: a template loop or stage read before any pyramid, coarse bit planes the last call did not build) the model
predicts the refusal; an unexpected success or failure is a finding.

The operation list of a sequence is a pure function of (seed, sequence index, steps): generate() needs neither torch nor
a GPU.  On the first failure run() raises with the seed, the step, the operation log up to it and a command line that
replays exactly that prefix; nothing is retried.

A second generator profile, "sparse" (_generate_sparse), stays on the (4, 8) pyramid with the streaming gradient kernel forced,
where a frame-taking match call makes level 0 only where its coarse candidates read it: padded and interleaved caller layouts,
two geometries with a cut tile column, batches that grow and shrink, readers of level 0 behind such a call -- also after
clobber_inputs overwrote the caller's device buffers -- and get_quantized_frame of every frame of the last device batch.

A third profile, "anygeo" (_generate_anygeo), draws the pyramids and frame geometries that the one-launch linear-memory builder
does not take -- strides 1, 2, 5 beside 4 and 8, level widths that are no multiple of 16, an odd width -- where a batch of
frames goes through the batched any-stride builder (csrc/sbm_lm_any.h): device and host batches and device NMS at every one
of them, geometry changes to and from an aligned frame, and the maps and coarse bit planes of any frame of the last device
batch.  Its templates are cut from the orientation maps of one of its own scene frames (the case1 templates are larger than
most of its frames).

usage: python tools/fuzz_sequence.py [n_sequences] [seed] [--steps S] [--only I] [--stop K] [--profile default|sparse|anygeo]
       (--only I: sequence I alone; --stop K: its first K + 1 steps)"""
import argparse
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PYRAMIDS = [(4, 8), (4,), (8, 8), (4, 8, 8)]
# name -> (rows, cols, channels).  "O": (cols / 4) & 15 != 0 and level 1 not 16-cell aligned, so the register-only
# linear-memory builder, the strip and bit-strip forms give way to the byte fall-backs (single-frame entry points only)
GEOS = {"A": (512, 768, 3), "B": (448, 640, 3), "G": (512, 768, 1), "O": (480, 608, 3)}
BATCH_GEOS = ("A", "B", "G")
# The sparse profile's geometries: A, B, G and two whose last refinement tile column is cut to 16 cells ((cols / 4) % 32 == 16).
# "P": 3.5 x 4.5 tiles, a 96-column last strip packed two frames per wave; "Q": gray, 4 x 5.5 tiles.  Kept apart from GEOS: the
# default profile draws from tuple(GEOS), and its output must not change.
SPARSE_GEOS = {"A": GEOS["A"], "B": GEOS["B"], "G": GEOS["G"], "P": (448, 576, 3), "Q": (512, 704, 1)}
# The anygeo profile's pyramids and geometries: per pyramid the frames that meet the reference's three conditions at every
# level (rows % T == 0, cols % T == 0, rows * cols % 16 == 0).  All but "c" under (4, 8) and (2, 4) have a level off the
# one-launch builder's grid; "c" is there for the change to an aligned geometry and back.  The first geometry of a pyramid
# is the one its templates are cut from.
ANYGEO_ONLY_GEOS = {"a": (208, 272, 3), "b": (208, 272, 1), "c": (240, 320, 3), "d": (200, 264, 1), "e": (384, 416, 3), "f": (256, 288, 3),
                    "g": (208, 211, 1)}
ANYGEO_PYRAMIDS = [(4, 8), (2, 4), (5, 8), (4, 8, 8), (1,)]
ANYGEO_GEOS = {(4, 8): ("a", "b", "c", "e", "f", "O"), (2, 4): ("d", "a", "b", "c", "f", "O"), (5, 8): ("c",), (4, 8, 8): ("e", "f", "O"),
               (1,): ("g", "a", "b", "d")}
ALL_GEOS = {**GEOS, **SPARSE_GEOS, **ANYGEO_ONLY_GEOS}
PROFILES = ("default", "sparse", "anygeo")
ROW_PADS = (0, 13, 64)        # bytes behind every row of a device frame
FRAME_PADS = (0, 1000, -1)    # bytes behind every frame of a device batch; -1: one whole frame (the inverted frame lies there)
SPARSE_HS = (8, 18, 32)
N_VARIANTS = 4
THRESHOLDS = (98.0, 90.0, 80.0, 60.0, 0.0, -5.0)
GRAPH_MODES = (-1, 0, 1)
COARSE_MODES = ("auto", "block", "wave", "bits", "bytes")
SET_SIZES = (41, 40)  # template sets 0 and 1 (tools: template_set)
CAP = 1 << 15         # records per frame slot
MATCH_OPS = ("match", "match_device", "match_batch_device", "match_batch_host", "match_banded", "match_templates",
             "match_templates_device", "nms")
STATE_OPS = ("build_pyramid", "set_quantized")
READ_OPS = ("get_quantized", "get_linear_memories", "get_coarse_bitplanes", "similarity", "similarity_local")
# the sparse profile's own operations: a frame of the last device batch read back, and the caller's device buffers of every
# synchronised call overwritten (legal for a caller: the library keeps what it needs)
SPARSE_ONLY_OPS = ("get_quantized_frame", "clobber_inputs")
FRAME_MATCH_OPS = ("match", "match_device", "match_batch_device", "match_batch_host")  # entry points that can take the sparse path
LEVEL0_READERS = ("get_quantized", "get_quantized_frame", "get_linear_memories", "match_templates", "match_templates_device",
                  "similarity_local", "set_quantized")
_SPARSE_WEIGHTS = {"match_batch_device": 10, "match_device": 5, "match": 4, "match_batch_host": 4, "match_banded": 1, "nms": 2,
                   "match_templates": 2, "match_templates_device": 2, "get_quantized": 2, "get_quantized_frame": 4,
                   "get_linear_memories": 2, "similarity_local": 2, "set_quantized": 2, "build_pyramid": 1, "set_graph_mode": 2,
                   "set_pipeline_depth": 1, "set_quantize_mode": 1, "checkpoint": 2, "clobber_inputs": 2, "stall": 1}
_SPARSE_FOLLOWERS = ("get_quantized", "get_quantized_frame", "get_quantized_frame", "get_linear_memories", "match_templates",
                     "match_templates_device", "similarity_local", "set_quantized")
_ANYGEO_WEIGHTS = {"match": 2, "match_device": 4, "match_batch_device": 10, "match_batch_host": 5, "match_templates": 2,
                   "match_templates_device": 3, "nms": 3, "build_pyramid": 1, "set_quantized": 1, "get_quantized": 1, "get_quantized_frame": 4,
                   "get_linear_memories": 3, "get_coarse_bitplanes": 4, "similarity": 1, "similarity_local": 2, "upload_templates": 1,
                   "select_range": 1, "select_classes": 1, "select_all": 1, "set_coarse_mode": 2, "set_quantize_mode": 1,
                   "set_pipeline_depth": 1, "set_graph_mode": 3, "checkpoint": 2, "stall": 1}
TEMPLATE_OPS = ("upload_templates", "select_range", "select_classes", "select_templates", "select_empty", "select_all")
MODE_OPS = ("set_coarse_mode", "set_refine_bits", "set_refine_order", "set_quantize_mode", "set_pipeline_depth", "set_graph_mode")
SYNC_OPS = ("checkpoint", "switch_stream")
STALL_OPS = ("stall",)  # a spin kernel on the caller's stream: the launches behind it are still queued when the host returns
ALL_OPS = MATCH_OPS + STATE_OPS + READ_OPS + TEMPLATE_OPS + MODE_OPS + SYNC_OPS + STALL_OPS
_WEIGHTS = {"match": 3, "match_device": 8, "match_batch_device": 7, "match_batch_host": 2, "match_banded": 2, "match_templates": 3,
            "match_templates_device": 8, "nms": 2, "build_pyramid": 3, "set_quantized": 3, "get_quantized": 1, "get_linear_memories": 2,
            "get_coarse_bitplanes": 2, "similarity": 1, "similarity_local": 2, "upload_templates": 1, "select_range": 1,
            "select_classes": 1, "select_templates": 1, "select_empty": 1, "select_all": 1, "set_coarse_mode": 3,
            "set_refine_bits": 2, "set_refine_order": 1, "set_quantize_mode": 1, "set_pipeline_depth": 2, "set_graph_mode": 3,
            "checkpoint": 2, "switch_stream": 1, "stall": 4}


def sequence_seed(seed, index):
    return (int(seed) * 1000003 + int(index) * 7919 + 17) % (1 << 31)


def sparse_eligible(T, qmode, op):
    """the call can take the sparse level-0 path: a frame-taking match entry point on the (4, 8) pyramid, the streaming kernel
    forced, level 0 a grid of whole 16-cell strips, no mask (a banded call is another operation)"""
    return (tuple(T) == (4, 8) and qmode == "stream" and op["op"] in FRAME_MATCH_OPS and not op["mask"]
            and (ALL_GEOS[op["geo"]][1] // 4) % 16 == 0)


def generate(seed, index, steps, profile="default"):
    """(pyramid, [op dict]) of sequence `index` of `seed`: deterministic, no torch, no GPU"""
    if profile == "sparse":
        return _generate_sparse(seed, index, steps)
    if profile == "anygeo":
        return _generate_anygeo(seed, index, steps)
    if profile != "default":
        raise ValueError(f"profile {profile!r}: one of {PROFILES}")
    rs = np.random.RandomState(sequence_seed(seed, index))
    T = PYRAMIDS[index % len(PYRAMIDS)] if index < len(PYRAMIDS) else PYRAMIDS[int(rs.randint(len(PYRAMIDS)))]
    names = list(ALL_OPS)
    p = np.array([_WEIGHTS[n] for n in names], np.float64)
    p /= p.sum()
    n_set = SET_SIZES[0]
    n_active = n_set
    qmode = "auto"
    batch_since_switch = False
    ops = [{"op": "set_graph_mode", "mode": int(GRAPH_MODES[int(rs.randint(3))])}]
    if int(rs.randint(2)):
        ops.append({"op": "set_pipeline_depth", "depth": int(rs.choice([2, 4]))})

    def thr():
        # thresholds <= 0 make every position a candidate (below 0: the byte kernels): only with one template or none
        t = float(THRESHOLDS[int(rs.randint(len(THRESHOLDS)))])
        return t if t > 0 or n_active <= 1 else float(THRESHOLDS[int(rs.randint(4))])

    def frame(batch=False):
        g = str(rs.choice(BATCH_GEOS if batch else tuple(GEOS)))
        return g, int(rs.randint(N_VARIANTS)), bool(rs.randint(4) == 0)

    since_sync = 0
    while len(ops) < steps:
        name = names[int(rs.choice(len(names), p=p))]
        if since_sync >= 6 and name not in SYNC_OPS and rs.randint(3) == 0:
            name = "checkpoint"  # asynchronous stretches of a few calls, then a look at their results
        op = {"op": name}
        if name in ("match", "match_device", "build_pyramid", "set_quantized"):
            op["geo"], op["var"], op["mask"] = frame()
            if name in ("match", "match_device"):
                op["thr"] = thr()
        elif name in ("match_batch_device", "match_batch_host", "match_banded"):
            op["geo"], _, op["mask"] = frame(True)
            if name == "match_banded":
                if T != (4, 8) or qmode == "tile":
                    op["op"] = name = "match_batch_device"
                else:
                    op["geo"] = str(rs.choice(["A", "G"]))
                    op["n_bands"] = int(rs.choice([2, 4, 8]))
            B = int(rs.randint(1, 10 if name != "match_batch_host" else 6))
            op["vars"] = [int(rs.randint(N_VARIANTS)) for _ in range(B)]
            op["thr"] = thr()
            if name == "match_batch_host":
                op["sub_batch"] = int(rs.randint(1, 5))
                op["split"] = bool(rs.randint(2))
                op["pinned"] = bool(rs.randint(2))
            if name != "match_batch_host":
                batch_since_switch = True
        elif name in ("match_templates", "match_templates_device"):
            op["thr"] = thr()
        elif name == "nms":
            if not batch_since_switch:
                continue
            op["score"] = float(rs.choice([0.0, 85.0, 95.0]))
            op["nms"] = float(rs.choice([0.3, 0.5, 1.0]))
        elif name in ("get_quantized", "get_linear_memories"):
            op["level"] = int(rs.randint(len(T)))
        elif name == "similarity":
            op["t"] = int(rs.randint(n_set))
        elif name == "similarity_local":
            op["level"] = int(rs.randint(len(T)))
            op["t"] = int(rs.randint(n_set))
            op["fx"], op["fy"] = float(rs.uniform(0.05, 0.95)), float(rs.uniform(0.05, 0.95))
        elif name == "upload_templates":
            op["set"] = int(rs.randint(2))
            n_set = n_active = SET_SIZES[op["set"]]
            batch_since_switch = False  # device NMS sizes boxes by the templates uploaded now: only lists of this upload
        elif name == "select_range":
            op["count"] = int(rs.choice([1, 2, 3, 9, 20]))
            op["first"] = int(rs.randint(0, n_set - op["count"] + 1))
            n_active = op["count"]
        elif name == "select_classes":
            op["classes"] = [[0], [1], [0, 1]][int(rs.randint(3))]
            n_active = sum((n_set + 1 - c) // 2 for c in op["classes"])
        elif name == "select_templates":
            k = int(rs.choice([1, 2, 5, 17]))
            op["idx"] = sorted(int(i) for i in rs.choice(n_set, k, replace=False))
            if rs.randint(2):
                op["idx"] = op["idx"][::-1]
            n_active = k
        elif name == "select_empty":
            n_active = 0
        elif name == "select_all":
            n_active = n_set
        elif name == "set_coarse_mode":
            op["mode"] = str(rs.choice(COARSE_MODES))
        elif name == "set_refine_bits":
            op["mode"] = int(rs.choice([-1, 0, 1]))
        elif name == "set_refine_order":
            op["order"] = str(rs.choice(["auto", "slots", "list"]))
        elif name == "set_quantize_mode":
            qmode = op["mode"] = str(rs.choice(["auto", "tile", "stream"]))
            op["hs"] = int(rs.choice([0, 8, 16]))
        elif name == "set_pipeline_depth":
            op["depth"] = int(rs.choice([1, 2, 4]))
        elif name == "set_graph_mode":
            op["mode"] = int(GRAPH_MODES[int(rs.randint(3))])
        elif name == "stall":
            op["cycles"] = int(rs.choice([1_000_000, 10_000_000]))
        elif name == "switch_stream":
            # a second caller stream only after a host synchronisation
            ops.append({"op": "checkpoint"})
            since_sync = 0
            batch_since_switch = False
            if len(ops) >= steps:
                break
        if name == "checkpoint":
            since_sync = 0
        elif name != "switch_stream":
            since_sync += 1
        ops.append(op)
    return T, ops[:steps]


def _generate_sparse(seed, index, steps):
    """The sparse profile: the (4, 8) pyramid with the streaming kernel forced, so that most frame-taking calls take the sparse
    level-0 path (source pass, mark tiles, flagged gradient, flagged strips) and the operations between them read, replace or
    outlive what such a call leaves: padded and interleaved caller layouts, batches that grow and shrink, 1- and 3-channel
    geometries in turn, readers right behind a sparse batch -- also after the caller's buffers were overwritten.  A call drawn
    as "profiled" runs under sbm_set_profiling, and the Runner counts its gradient launches: three where it is sparse-eligible."""
    rs = np.random.RandomState((sequence_seed(seed, index) ^ 0x5a17e5) % (1 << 31))
    T = PYRAMIDS[0]
    names = list(_SPARSE_WEIGHTS)
    p = np.array([_SPARSE_WEIGHTS[n] for n in names], np.float64)
    p /= p.sum()
    geos = tuple(SPARSE_GEOS)
    n_set = SET_SIZES[0]
    qmode = "stream"
    have_batch = False   # a device batch ran since the start: device NMS has lists to work on
    last_B = 1           # frames of the last device batch still resident (1 after a single-frame call or a state call)
    forced = []          # operations that follow the last one at once
    since_sync = 0
    ops = [{"op": "set_quantize_mode", "mode": "stream", "hs": int(rs.choice(SPARSE_HS))}]
    if int(rs.randint(2)):
        ops.append({"op": "set_graph_mode", "mode": int(GRAPH_MODES[int(rs.randint(3))])})
    if int(rs.randint(2)):
        ops.append({"op": "set_pipeline_depth", "depth": int(rs.choice([2, 4]))})

    def thr():
        return float(THRESHOLDS[int(rs.randint(4))])  # every template stays selected: thresholds above 0 only

    while len(ops) < steps:
        if forced:
            name = forced.pop(0)
        elif qmode != "stream" and rs.randint(3) == 0:
            name = "set_quantize_mode"  # ... and back into stream mode
        else:
            name = names[int(rs.choice(len(names), p=p))]
            if since_sync >= 6 and name not in ("checkpoint", "clobber_inputs") and rs.randint(3) == 0:
                name = "checkpoint"
        op = {"op": name}
        if name in ("match", "match_device", "build_pyramid", "set_quantized"):
            op["geo"], op["var"], op["mask"] = str(rs.choice(geos)), int(rs.randint(N_VARIANTS)), bool(rs.randint(8) == 0)
            if name in ("match", "match_device"):
                op["thr"] = thr()
            if name == "match_device":
                op["row_pad"] = int(rs.choice(ROW_PADS))
            if name in ("match", "match_device"):
                op["profiled"] = bool(rs.randint(3) == 0)
            last_B = 1
        elif name in ("match_batch_device", "match_batch_host", "match_banded"):
            op["geo"] = str(rs.choice(geos))
            op["mask"] = bool(rs.randint(5 if name == "match_batch_device" else 8) == 0)
            if name == "match_banded":
                if qmode == "tile":
                    op["op"] = name = "match_batch_device"
                else:
                    op["geo"] = str(rs.choice(["A", "G"]))
                    op["n_bands"] = int(rs.choice([2, 4, 8]))
            B = int(rs.randint(1, 10 if name != "match_batch_host" else 6))
            op["vars"] = [int(rs.randint(N_VARIANTS)) for _ in range(B)]
            op["thr"] = thr()
            if name == "match_batch_host":
                op["sub_batch"] = int(rs.randint(1, 5))
                op["split"] = bool(rs.randint(2))
                op["pinned"] = bool(rs.randint(2))
                last_B = 1  # (which sub-batch stays resident is not part of the ABI: frame 0 only, unchecked)
            else:
                op["row_pad"] = int(rs.choice(ROW_PADS))
                op["frame_pad"] = int(rs.choice(FRAME_PADS))
                have_batch = True
                last_B = B if name == "match_batch_device" else 1
            if name != "match_banded":
                op["profiled"] = bool(rs.randint(3) == 0)
            if name == "match_batch_device" and rs.randint(5) < 3:
                # a reader right behind the batch, sometimes with the caller's buffers overwritten first
                if rs.randint(5) < 2:
                    forced += ["checkpoint", "clobber_inputs"]
                forced.append(_SPARSE_FOLLOWERS[int(rs.randint(len(_SPARSE_FOLLOWERS)))])
        elif name in ("match_templates", "match_templates_device"):
            op["thr"] = thr()
        elif name == "nms":
            if not have_batch:
                continue
            op["score"] = float(rs.choice([0.0, 85.0, 95.0]))
            op["nms"] = float(rs.choice([0.3, 0.5, 1.0]))
        elif name in ("get_quantized", "get_linear_memories"):
            op["level"] = int(rs.randint(4) == 0)  # level 0 three times in four
        elif name == "get_quantized_frame":
            op["level"] = int(rs.randint(4) == 0)
            op["frame"] = int(rs.randint(last_B))
        elif name == "similarity_local":
            op["level"] = 0
            op["t"] = int(rs.randint(n_set))
            op["fx"], op["fy"] = float(rs.uniform(0.05, 0.95)), float(rs.uniform(0.05, 0.95))
        elif name == "set_quantize_mode":
            qmode = op["mode"] = "stream" if qmode != "stream" else str(rs.choice(["stream", "tile", "auto"]))
            op["hs"] = int(rs.choice(SPARSE_HS))
        elif name == "set_pipeline_depth":
            op["depth"] = int(rs.choice([1, 2, 4]))
        elif name == "set_graph_mode":
            op["mode"] = int(GRAPH_MODES[int(rs.randint(3))])
        elif name == "stall":
            op["cycles"] = int(rs.choice([1_000_000, 10_000_000]))
        elif name == "clobber_inputs":
            # only buffers of synchronised calls: a checkpoint stands right in front
            if ops[-1]["op"] != "checkpoint":
                ops.append({"op": "checkpoint"})
                if len(ops) >= steps:
                    break
            since_sync = 0
        if name == "checkpoint":
            since_sync = 0
        elif name != "clobber_inputs":
            since_sync += 1
        ops.append(op)
    return T, ops[:steps]


def _generate_anygeo(seed, index, steps):
    """The anygeo profile: one of ANYGEO_PYRAMIDS, frames of ANYGEO_GEOS for it.  Device batches (padded caller layouts too),
    host batches and device NMS at every geometry, no banded call (it refuses these geometries); behind a device batch often a
    reader of what it left: the map or the coarse bit planes of any of its frames, linear memories, the template loop."""
    rs = np.random.RandomState((sequence_seed(seed, index) ^ 0x0a9e0) % (1 << 31))
    T = ANYGEO_PYRAMIDS[index % len(ANYGEO_PYRAMIDS)] if index < len(ANYGEO_PYRAMIDS) else ANYGEO_PYRAMIDS[int(rs.randint(len(ANYGEO_PYRAMIDS)))]
    geos = ANYGEO_GEOS[T]
    names = list(_ANYGEO_WEIGHTS)
    p = np.array([_ANYGEO_WEIGHTS[n] for n in names], np.float64)
    p /= p.sum()
    n_set = SET_SIZES[0]
    n_active = n_set
    have_batch = False
    last_B = 1
    forced = []
    since_sync = 0
    followers = ("get_quantized_frame", "get_coarse_bitplanes", "get_coarse_bitplanes", "get_linear_memories", "match_templates",
                 "match_templates_device", "similarity_local")
    ops = [{"op": "set_graph_mode", "mode": int(GRAPH_MODES[int(rs.randint(3))])}]
    if int(rs.randint(2)):
        ops.append({"op": "set_pipeline_depth", "depth": int(rs.choice([2, 4]))})

    def thr():
        t = float(THRESHOLDS[int(rs.randint(len(THRESHOLDS)))])
        return t if t > 0 or n_active <= 1 else float(THRESHOLDS[int(rs.randint(4))])

    while len(ops) < steps:
        if forced:
            name = forced.pop(0)
        else:
            name = names[int(rs.choice(len(names), p=p))]
            if since_sync >= 6 and name != "checkpoint" and rs.randint(3) == 0:
                name = "checkpoint"
        op = {"op": name}
        if name in ("match", "match_device", "build_pyramid", "set_quantized"):
            op["geo"], op["var"], op["mask"] = str(rs.choice(geos)), int(rs.randint(N_VARIANTS)), bool(rs.randint(5) == 0)
            if name in ("match", "match_device"):
                op["thr"] = thr()
            if name == "match_device":
                op["row_pad"] = int(rs.choice(ROW_PADS))
            last_B = 1
        elif name in ("match_batch_device", "match_batch_host"):
            op["geo"], op["mask"] = str(rs.choice(geos)), bool(rs.randint(5) == 0)
            B = int(rs.randint(1, 8 if name == "match_batch_device" else 6))
            op["vars"] = [int(rs.randint(N_VARIANTS)) for _ in range(B)]
            op["thr"] = thr()
            if name == "match_batch_host":
                op["sub_batch"] = int(rs.randint(1, 5))
                op["split"] = bool(rs.randint(2))
                op["pinned"] = bool(rs.randint(2))
                last_B = 1
            else:
                op["row_pad"] = int(rs.choice(ROW_PADS))
                op["frame_pad"] = int(rs.choice(FRAME_PADS))
                have_batch = True
                last_B = B
                if rs.randint(5) < 3:
                    forced.append(followers[int(rs.randint(len(followers)))])
        elif name in ("match_templates", "match_templates_device"):
            op["thr"] = thr()
        elif name == "nms":
            if not have_batch:
                continue
            op["score"] = float(rs.choice([0.0, 85.0, 95.0]))
            op["nms"] = float(rs.choice([0.3, 0.5, 1.0]))
        elif name in ("get_quantized", "get_linear_memories"):
            op["level"] = int(rs.randint(len(T)))
        elif name == "get_quantized_frame":
            op["level"] = int(rs.randint(len(T)))
            op["frame"] = int(rs.randint(last_B))
        elif name == "get_coarse_bitplanes":
            op["frame"] = int(rs.randint(last_B))
        elif name == "similarity":
            op["t"] = int(rs.randint(n_set))
        elif name == "similarity_local":
            op["level"] = int(rs.randint(len(T)))
            op["t"] = int(rs.randint(n_set))
            op["fx"], op["fy"] = float(rs.uniform(0.05, 0.95)), float(rs.uniform(0.05, 0.95))
        elif name == "upload_templates":
            op["set"] = int(rs.randint(2))
            n_set = n_active = SET_SIZES[op["set"]]
            have_batch = False  # device NMS sizes boxes by the templates uploaded now: only lists of this upload
        elif name == "select_range":
            op["count"] = int(rs.choice([1, 2, 3, 9, 20]))
            op["first"] = int(rs.randint(0, n_set - op["count"] + 1))
            n_active = op["count"]
        elif name == "select_classes":
            op["classes"] = [[0], [1], [0, 1]][int(rs.randint(3))]
            n_active = sum((n_set + 1 - c) // 2 for c in op["classes"])
        elif name == "select_all":
            n_active = n_set
        elif name == "set_coarse_mode":
            op["mode"] = str(rs.choice(COARSE_MODES))
        elif name == "set_quantize_mode":
            op["mode"] = str(rs.choice(["auto", "tile", "stream"]))
            op["hs"] = int(rs.choice([0, 8, 16]))
        elif name == "set_pipeline_depth":
            op["depth"] = int(rs.choice([1, 2, 4]))
        elif name == "set_graph_mode":
            op["mode"] = int(GRAPH_MODES[int(rs.randint(3))])
        elif name == "stall":
            op["cycles"] = int(rs.choice([1_000_000, 10_000_000]))
        since_sync = 0 if name == "checkpoint" else since_sync + 1
        ops.append(op)
    return T, ops[:steps]


def padded_layout(frames, row_pad, frame_pad):
    """the frames (equal shapes, uint8) in one host buffer of a caller's layout: `row_pad` bytes behind every row, `frame_pad`
    bytes behind every frame (-1: a whole frame, which holds the inverted frame); all padding is 0xA5.
    -> (buffer, row stride, frame stride)"""
    rows, line = frames[0].shape[0], frames[0].size // frames[0].shape[0]
    stride = line + row_pad
    fb = rows * stride
    fs = 2 * fb if frame_pad < 0 else fb + frame_pad
    buf = np.full(len(frames) * fs, 0xA5, np.uint8)
    for f, fr in enumerate(frames):
        buf[f * fs: f * fs + fb].reshape(rows, stride)[:, :line] = fr.reshape(rows, line)
        if frame_pad < 0:
            buf[f * fs + fb: f * fs + 2 * fb].reshape(rows, stride)[:, :line] = 255 - fr.reshape(rows, line)
    return buf, stride, fs


def fmt(op):
    return op["op"] + "(" + ", ".join(f"{k}={v}" for k, v in op.items() if k != "op") + ")"


class Finding(AssertionError):
    pass


def template_set(all_ts, which, T):
    """set 0 / set 1 of the case1 fixture, re-cut to the pyramid as tools/fuzz_match.py does; classes alternate 0, 1"""
    from shape_based_matching_amd.templates import TemplateSet, from_pyramids

    idx = list(range(280, 361, 2)) if which == 0 else list(range(1, 361, 9))
    assert len(idx) == SET_SIZES[which]
    ts = all_ts.subset(idx)
    if tuple(T) != (4, 8):
        pyrs = []
        for t in idx:
            lv = []
            for l in range(len(T)):
                src = all_ts.levels[t, min(l, 1)]
                f = all_ts.features[src["feature_offset"]: src["feature_offset"] + src["n_features"]]
                scale = 1 if l < 2 else 2
                feats = np.stack([f["x"] // scale, f["y"] // scale, f["label"]], axis=1)
                lv.append({"width": int(src["width"]) // scale, "height": int(src["height"]) // scale, "tl_x": 0, "tl_y": 0,
                           "pyramid_level": l, "features": feats})
            pyrs.append(lv)
        ts = from_pyramids(pyrs, "t")
    n = ts.n_templates
    return TemplateSet(ts.n_levels, ts.levels, ts.features, (np.arange(n) % 2).astype(np.int32), ts.template_id, ["a", "b"])


def anygeo_template_set(O, frames, which, T):
    """set 0 / set 1 of the anygeo profile: SET_SIZES templates cut from the orientation maps of the scene frame (variant 3) of
    the pyramid's first geometry, so that they score 100 there and something between on every other frame; classes alternate"""
    from shape_based_matching_amd import synth
    from shape_based_matching_amd.templates import TemplateSet

    L = len(T)
    pyr = O.Pyramid.build(frames[ANYGEO_GEOS[tuple(T)][0], 3], list(T), 30.0)
    qs = [pyr.quantized(l) for l in range(L)]
    pyr.free()
    ts, _ = synth.templates_from_maps(qs, [48, 24, 12][:L], 64 if L < 3 else 128, SET_SIZES[which], 11 + which)
    n = ts.n_templates
    return TemplateSet(ts.n_levels, ts.levels, ts.features, (np.arange(n) % 2).astype(np.int32), ts.template_id, ["a", "b"])


class Runner:
    """applies one sequence to one context and checks it against the oracle"""

    def __init__(self, O, capi, torch, frames, masks, all_ts, pyr_cache):
        self.O, self.capi, self.torch = O, capi, torch
        self.frames, self.masks, self.all_ts, self.pyr_cache = frames, masks, all_ts, pyr_cache
        self.dev = torch.device("cuda", 0)
        self.d_frames = {k: torch.from_numpy(v).to(self.dev) for k, v in frames.items()}
        self.d_masks = {k: torch.from_numpy(v).to(self.dev) for k, v in masks.items()}
        self.want_cache = {}
        self.n_unchecked = 0  # results not compared: the resident frame is not known after a host or banded batch
        self.n_sparse_proven = 0  # profiled sparse-eligible calls that made the sparse path's three gradient launches
        self.sparse_on = os.environ.get("SBM_SPARSE_GRADIENT", "1") != "0" and os.environ.get("SBM_SPARSE_STRIPS", "1") != "0"
        torch.cuda.synchronize()

    # -- oracle -----------------------------------------------------------------------------------------------------
    def pyr(self, T, geo, var, mask):
        img = self.frames[(geo, var)]
        k = (zlib.crc32(img.tobytes()), tuple(T), mask)
        if k not in self.pyr_cache:
            if len(self.pyr_cache) >= 40:
                old = next(iter(self.pyr_cache))
                self.pyr_cache.pop(old).free()
            self.pyr_cache[k] = self.O.Pyramid.build(img, list(T), 30.0, mask=self.masks[geo] if mask else None)
        return self.pyr_cache[k]

    def want(self, fk, thr):
        """the oracle list of frame fk under the current templates and selection, as a key: it is evaluated (want_of) only
        when the results are checked, after a host synchronisation, so that no oracle work stands between two library calls"""
        return (fk, self.set_id, tuple(self.active), thr)

    def want_of(self, k):
        if k not in self.want_cache:
            fk, set_id, active, thr = k
            if not active:
                from shape_based_matching_amd.templates import MATCH_DTYPE

                self.want_cache[k] = np.zeros(0, MATCH_DTYPE)
            else:
                sub = self.sets[set_id].subset(list(active))
                p = self.pyr(self.T, *fk)
                self.want_cache[k] = p.match(sub.levels, sub.features, sub.class_idx, sub.template_id, thr,
                                             n_threads=min(16, os.cpu_count() or 1))
        return self.want_cache[k]

    # -- one sequence ------------------------------------------------------------------------------------------------
    def run(self, seed, index, steps, stop=None, profile="default"):
        from shape_based_matching_amd.templates import MATCH_DTYPE

        torch, capi = self.torch, self.capi
        T, ops = generate(seed, index, steps, profile)
        if stop is not None:
            ops = ops[: stop + 1]
        self.T, self.L = T, len(T)
        self.rec = MATCH_DTYPE.itemsize
        if profile == "anygeo":
            self.sets = [anygeo_template_set(self.O, self.frames, 0, T), anygeo_template_set(self.O, self.frames, 1, T)]
        else:
            self.sets = [template_set(self.all_ts, 0, T), template_set(self.all_ts, 1, T)]
        self.set_id, self.ts = 0, self.sets[0]
        self.active = list(range(self.ts.n_templates))
        self.want_cache = {}
        # every oracle pyramid the sequence can read (set_quantized, stage reads) is built before the first call
        for p in self.pyr_cache.values():
            p.free()
        self.pyr_cache.clear()
        for op in ops:
            if "geo" in op:
                for v in op.get("vars", [op.get("var")]):
                    self.pyr(T, op["geo"], v, op["mask"])
        ctx = capi.Context(T=T, weak_threshold=30.0, device_id=0)
        streams = [torch.cuda.Stream(device=self.dev), torch.cuda.Stream(device=self.dev)]
        si = 0
        resident = None       # (geo, var, mask) of frame 0 of the resident pyramid, "unknown", or None (nothing built)
        blm = False           # the coarsest level's bit planes of `resident` are there (True), not (False), unknown (None)
        blm_all = False       # ... and those of every frame of batch_res: the last pyramid was a device batch that made them
        coarse = "auto"
        last_batch = None     # pending record of the last batch call on the current stream
        qmode = "auto"        # the gradient kernel asked for (set_quantize_mode)
        batch_res = []        # (geo, var, mask) of every frame of the resident pyramid; None: unknown; []: nothing built
        handed = []           # device buffers of frames handed to device entry points (the sparse profile's clobber_inputs)
        pending = []          # enqueued device calls whose results are not checked yet
        log = []
        n_cmp = 0

        def fail(step, msg):
            # the replay runs up to the step at which the failure was SEEN: a deferred check fails at a checkpoint, and the
            # calls between the enqueue and it may be the cause
            seen = len(log) - 1
            where = f"step {step}" if step == seen else f"step {step} (seen at step {seen})"
            raise Finding(f"sequence fuzzer: seed {seed}, sequence {index} (pyramid {T}), {where}: {msg}\n"
                          + "\n".join(f"  {i:3d} {l}" for i, l in enumerate(log))
                          + "\nreplay: " + replay_command(seed, index, steps, seen, profile))

        def cmp(step, what, got, want):
            nonlocal n_cmp
            g = sorted(np.ascontiguousarray(got, MATCH_DTYPE).tolist())
            w = sorted(np.ascontiguousarray(want, MATCH_DTYPE).tolist())
            if g != w:
                fail(step, f"{what}: {len(g)} records, oracle {len(w)}; first difference "
                           f"{next((a, b) for a, b in zip(g + [None] * len(w), w + [None] * len(g)) if a != b)}")
            n_cmp += len(w)

        def check_pending():
            streams[si].synchronize()
            torch.cuda.synchronize()
            for p in pending:
                wants = [None if k is None else (k() if callable(k) else self.want_of(k)) for k in p["want"]]
                if "lists" in p:  # a host entry point: its lists, compared here to keep oracle work out of the stretch
                    for f, w in enumerate(wants):
                        cmp(p["step"], f"{p['what']} frame {f}", p["lists"][f], w)
                    continue
                cnt = p["cnt"].cpu().numpy().reshape(-1, 2)
                out = p["out"].cpu().numpy().reshape(len(cnt), -1)
                for f, w in enumerate(wants):
                    if w is None:
                        self.n_unchecked += 1
                        continue
                    if cnt[f, 1] != 0 or cnt[f, 0] != len(w):
                        fail(p["step"], f"{p['what']} frame {f}: count {cnt[f].tolist()}, oracle {len(w)}")
                    cmp(p["step"], f"{p['what']} frame {f}", out[f].view(MATCH_DTYPE)[: cnt[f, 0]], w)
            pending.clear()

        def expect_refusal(step, what, fn, code):
            try:
                fn()
            except capi.SbmError as e:
                if e.code != code:
                    fail(step, f"{what}: error {e.code}, expected {code}: {e}")
                return
            fail(step, f"{what}: succeeded where the library must refuse with {code}")

        def profiled(step, op, n_calls, wait=None):
            """behind a call that ran under set_profiling: a sparse-eligible call made the sparse path's three gradient launches
            (source pass, level 1, the flagged items), n_calls times for the sub-batches of a host batch"""
            if wait is not None:
                wait.synchronize()
            n_q = sum(1 for n, _ in ctx.timings() if n == "k_quantize")
            ctx.set_profiling(False)
            if self.sparse_on and sparse_eligible(T, qmode, op):
                if n_q != 3 * n_calls:
                    fail(step, f"{op['op']}: {n_q} gradient launches, the sparse path makes {3 * n_calls}")
                self.n_sparse_proven += 1

        def laid_out(geo, variants, row_pad, frame_pad):
            """the frames in a fresh device buffer of the caller's layout: `row_pad` bytes behind every row, `frame_pad` bytes
            behind every frame (-1: a whole frame, which holds the inverted frame); all padding is 0xA5.  -> buffer, row
            stride, frame stride"""
            rows, cols, ch = ALL_GEOS[geo]
            line = cols * ch
            stride = line + row_pad
            fb = rows * stride
            fs = 2 * fb if frame_pad < 0 else fb + frame_pad
            with torch.cuda.stream(streams[si]):
                buf = torch.full((len(variants) * fs,), 0xA5, dtype=torch.uint8, device=self.dev)
                for f, v in enumerate(variants):
                    src = self.d_frames[geo, v].view(rows, line)
                    buf[f * fs: f * fs + fb].view(rows, stride)[:, :line].copy_(src)
                    if frame_pad < 0:
                        buf[f * fs + fb: f * fs + 2 * fb].view(rows, stride)[:, :line].copy_(torch.bitwise_not(src))
            handed.append(buf)
            return buf, stride, fs

        def slot(n_frames):
            with torch.cuda.stream(streams[si]):
                out = torch.empty(n_frames * CAP * self.rec, dtype=torch.uint8, device=self.dev)
                cnt = torch.full((2 * n_frames,), -1, dtype=torch.int32, device=self.dev)
            return out, cnt

        try:
            ctx.upload_templates(self.ts)
            for step, op in enumerate(ops):
                log.append(fmt(op))
                name = op["op"]
                s = streams[si]
                sp = s.cuda_stream
                if name == "checkpoint":
                    check_pending()
                elif name == "stall":
                    with torch.cuda.stream(s):
                        torch.cuda._sleep(op["cycles"])
                elif name == "switch_stream":
                    si ^= 1
                    last_batch = None
                elif name == "clobber_inputs":
                    # every call that read these buffers was synchronised by the checkpoint in front
                    assert not pending
                    with torch.cuda.stream(s):
                        for t in handed:
                            t.fill_(0xFF)
                    handed.clear()
                elif name == "set_graph_mode":
                    ctx.set_graph_mode({-1: None, 0: False, 1: True}[op["mode"]])
                elif name == "set_pipeline_depth":
                    ctx.set_pipeline_depth(op["depth"])
                elif name == "set_coarse_mode":
                    ctx.set_coarse_mode(op["mode"])
                    coarse = op["mode"]
                elif name == "set_refine_bits":
                    ctx.set_refine_bits({-1: None, 0: False, 1: True}[op["mode"]])
                elif name == "set_refine_order":
                    ctx.set_refine_order(op["order"])
                elif name == "set_quantize_mode":
                    ctx.set_quantize_mode(op["mode"], op["hs"])
                    qmode = op["mode"]
                elif name == "upload_templates":
                    self.set_id, self.ts = op["set"], self.sets[op["set"]]
                    ctx.upload_templates(self.ts)
                    self.active = list(range(self.ts.n_templates))
                    last_batch = None
                elif name == "select_range":
                    ctx.select_range(op["first"], op["count"])
                    self.active = list(range(op["first"], op["first"] + op["count"]))
                elif name == "select_classes":
                    ctx.select_classes(op["classes"])
                    self.active = [t for t in range(self.ts.n_templates) if int(self.ts.class_idx[t]) in op["classes"]]
                elif name == "select_templates":
                    ctx.select_templates(op["idx"])
                    self.active = list(op["idx"])
                elif name == "select_empty":
                    ctx.select_templates([])
                    self.active = []
                elif name == "select_all":
                    ctx.select_range(0, self.ts.n_templates)
                    self.active = list(range(self.ts.n_templates))
                elif name in ("match", "match_device"):
                    fk = (op["geo"], op["var"], op["mask"])
                    rows, cols, ch = ALL_GEOS[op["geo"]]
                    if op.get("profiled"):
                        ctx.set_profiling(True)
                    if name == "match":
                        got = ctx.match(self.frames[op["geo"], op["var"]], op["thr"], mask=self.masks[op["geo"]] if op["mask"] else None)
                        pending.append({"step": step, "what": name, "lists": [got], "want": [self.want(fk, op["thr"])]})
                    else:
                        out, cnt = slot(1)
                        d_img, stride = self.d_frames[op["geo"], op["var"]], cols * ch
                        if "row_pad" in op:
                            d_img, stride, _ = laid_out(op["geo"], [op["var"]], op["row_pad"], 0)
                        ctx.match_device(d_img.data_ptr(), rows, cols, stride, ch, op["thr"], out.data_ptr(),
                                         CAP, cnt.data_ptr(), stream=sp,
                                         d_mask=self.d_masks[op["geo"]].data_ptr() if op["mask"] else 0)
                        pending.append({"step": step, "what": name, "out": out, "cnt": cnt, "want": [self.want(fk, op["thr"])], "keep": d_img})
                    if op.get("profiled"):
                        profiled(step, op, 1, None if name == "match" else s)
                    resident = fk
                    batch_res = [fk]
                    blm = (op["thr"] >= 0 and coarse in ("auto", "bits")) if self.active else None
                    blm_all = False
                elif name in ("match_batch_device", "match_banded", "match_batch_host"):
                    rows, cols, ch = ALL_GEOS[op["geo"]]
                    B = len(op["vars"])
                    wants = [self.want((op["geo"], v, op["mask"]), op["thr"]) for v in op["vars"]]
                    if op.get("profiled"):
                        ctx.set_profiling(True)
                    if name == "match_batch_host":
                        stack = np.stack([self.frames[op["geo"], v] for v in op["vars"]])
                        if op["pinned"]:
                            pin = torch.from_numpy(stack).pin_memory()
                            stack = pin.numpy()
                        lists = ctx.match_batch_host(list(stack), op["thr"], cap=CAP, sub_batch=op["sub_batch"],
                                                     mask=self.masks[op["geo"]] if op["mask"] else None, split=op["split"])
                        pending.append({"step": step, "what": name, "lists": lists, "want": wants})
                        if op.get("profiled"):
                            sub = max(1, min(op["sub_batch"], B))
                            profiled(step, op, -(-B // sub))
                        resident, blm, batch_res = "unknown", None, None  # (which sub-batch's frame stays resident is not part of the ABI)
                        blm_all = False
                    else:
                        if "row_pad" in op:
                            d_imgs, stride, fs = laid_out(op["geo"], op["vars"], op["row_pad"], op["frame_pad"])
                        else:
                            with torch.cuda.stream(s):
                                d_imgs = torch.stack([self.d_frames[op["geo"], v] for v in op["vars"]])
                            stride, fs = cols * ch, rows * cols * ch
                        dm = self.d_masks[op["geo"]].data_ptr() if op["mask"] else 0
                        if name == "match_batch_device":
                            out, cnt = slot(B)
                            ctx.match_batch_device(d_imgs.data_ptr(), fs, B, rows, cols, stride, ch, op["thr"], out.data_ptr(),
                                                   CAP, cnt.data_ptr(), stream=sp, d_mask=dm)
                            p = {"step": step, "what": name, "out": out, "cnt": cnt, "want": wants, "keep": d_imgs}
                            resident = (op["geo"], op["vars"][0], op["mask"])
                            batch_res = [(op["geo"], v, op["mask"]) for v in op["vars"]]
                            if op.get("profiled"):
                                profiled(step, op, 1, s)
                            blm = (op["thr"] >= 0 and coarse in ("auto", "bits")) if self.active else None
                            blm_all = blm is True
                        else:
                            hdr = (8 * B + 15) // 16 * 16
                            with torch.cuda.stream(s):
                                buf = torch.full((hdr + B * CAP * self.rec,), 0xff, dtype=torch.uint8, device=self.dev)
                            ctx.match_batch_device_banded(d_imgs.data_ptr(), fs, B, rows, cols, stride, ch, op["thr"],
                                                          buf.data_ptr(), CAP, n_bands=op["n_bands"], stream=sp, d_mask=dm)
                            p = {"step": step, "what": name, "out": buf[hdr:], "cnt": buf[: 8 * B].view(torch.int32), "want": wants,
                                 "keep": d_imgs}
                            resident, blm, batch_res = "unknown", None, None  # (the banded build's resident frame is not part of the ABI either)
                            blm_all = False
                        pending.append(p)
                        last_batch = {"p": p, "B": B, "ts": self.ts}
                elif name in ("match_templates", "match_templates_device"):
                    if resident is None:
                        if name == "match_templates":
                            expect_refusal(step, name, lambda: ctx.match_templates(op["thr"]), -4)
                        else:
                            out, cnt = slot(1)
                            expect_refusal(step, name, lambda: ctx.match_templates_device(op["thr"], out.data_ptr(), CAP, cnt.data_ptr(), stream=sp), -4)
                        continue
                    w = self.want(resident, op["thr"]) if resident != "unknown" else None
                    if name == "match_templates":
                        got = ctx.match_templates(op["thr"])
                        if w is not None:
                            pending.append({"step": step, "what": name, "lists": [got], "want": [w]})
                        else:
                            self.n_unchecked += 1
                    else:
                        out, cnt = slot(1)
                        ctx.match_templates_device(op["thr"], out.data_ptr(), CAP, cnt.data_ptr(), stream=sp)
                        pending.append({"step": step, "what": name, "out": out, "cnt": cnt, "want": [w]})
                    if not self.active:
                        blm = None  # (the non-graph coarse pass packs the planes only for a non-empty selection)
                    elif op["thr"] >= 0 and coarse in ("auto", "bits"):
                        blm = True if resident != "unknown" else None
                elif name == "nms":
                    from test_gpu_nms_device import expected, sizes_of

                    lb = last_batch["p"]
                    B = last_batch["B"]
                    out, cnt = slot(B)
                    ctx.nms_batch_device(lb["out"].data_ptr(), lb["cnt"].data_ptr(), CAP, B, out.data_ptr(), CAP, cnt.data_ptr(),
                                         op["score"], op["nms"], stream=sp)
                    sizes = sizes_of(last_batch["ts"])
                    pending.append({"step": step, "what": name, "out": out, "cnt": cnt, "keep": lb,
                                    "want": [(lambda k=k, sc=op["score"], th=op["nms"]: expected(self.want_of(k), sizes, sc, th))
                                             if k is not None else None for k in lb["want"]]})
                elif name in ("build_pyramid", "set_quantized"):
                    fk = (op["geo"], op["var"], op["mask"])
                    if name == "build_pyramid":
                        ctx.build_pyramid(self.frames[op["geo"], op["var"]], mask=self.masks[op["geo"]] if op["mask"] else None)
                    else:
                        p = self.pyr(T, *fk)
                        for l in range(self.L):
                            ctx.set_quantized(l, p.quantized(l))
                    resident, blm, batch_res = fk, False, [fk]
                    blm_all = False
                elif name == "get_quantized_frame":
                    if batch_res == []:
                        expect_refusal(step, name, lambda: ctx.get_quantized_frame(op["level"], op["frame"]), -4)
                        continue
                    got = ctx.get_quantized_frame(op["level"], op["frame"])
                    if batch_res is None:
                        self.n_unchecked += 1
                        continue
                    want = self.pyr(T, *batch_res[op["frame"]]).quantized(op["level"])
                    if got.shape != want.shape or not np.array_equal(got, want):
                        bad = int(np.count_nonzero(got != want)) if got.shape == want.shape else -1
                        fail(step, f"{name}: differs from the oracle in {bad} elements (shape {got.shape} vs {want.shape})")
                    n_cmp += 1
                elif name in READ_OPS:
                    if resident is None:
                        fn = {"get_quantized": lambda: ctx.get_quantized(op["level"]),
                              "get_linear_memories": lambda: ctx.get_linear_memories(op["level"]),
                              "get_coarse_bitplanes": lambda: ctx.get_coarse_bitplanes(),
                              "similarity": lambda: ctx.similarity(op["t"]),
                              "similarity_local": lambda: ctx.similarity_local(op["level"], op["t"], 8, 8)}[name]
                        expect_refusal(step, name, fn, -4)
                        continue
                    p = self.pyr(T, *resident) if resident != "unknown" else None
                    lc = self.L - 1
                    if name == "get_quantized":
                        got, want = ctx.get_quantized(op["level"]), p and p.quantized(op["level"])
                    elif name == "get_linear_memories":
                        got, want = ctx.get_linear_memories(op["level"]), p and p.lm(op["level"])
                    elif name == "get_coarse_bitplanes":
                        if blm is False:
                            expect_refusal(step, name, lambda: ctx.get_coarse_bitplanes(), -4)
                            continue
                        # a frame behind the first only where the last pyramid was a device batch that made every frame's planes
                        fr = op.get("frame", 0) if blm_all and batch_res and op.get("frame", 0) < len(batch_res) else 0
                        try:
                            got = ctx.get_coarse_bitplanes(fr)
                        except capi.SbmError as e:
                            if blm is None and e.code == -4:
                                continue
                            raise
                        from test_gpu_coarse_bits import packed

                        want = p and packed((self.pyr(T, *batch_res[fr]) if fr else p).lm(lc))
                    elif name == "similarity":
                        got = ctx.similarity(op["t"])
                        want = p and p.similarity(self.ts.levels[op["t"], lc], self.ts.features, lc)
                    else:
                        l = op["level"]
                        r, c = ctx.level_dims(l)
                        cx, cy = int(op["fx"] * c), int(op["fy"] * r)
                        got = ctx.similarity_local(l, op["t"], cx, cy)
                        want = p and p.similarity_local(self.ts.levels[op["t"], l], self.ts.features, l, cx, cy)
                    if p is None:
                        self.n_unchecked += 1
                    else:
                        if got.shape != want.shape or not np.array_equal(got, want):
                            bad = int(np.count_nonzero(got != want)) if got.shape == want.shape else -1
                            fail(step, f"{name}: differs from the oracle in {bad} elements (shape {got.shape} vs {want.shape})")
                        n_cmp += 1
                else:
                    raise ValueError(name)
            log.append("end")
            check_pending()
        except Finding:
            raise
        except Exception as e:  # an unexpected refusal or error of the library is a finding too
            fail(len(log) - 1, f"{type(e).__name__}: {e}")
        finally:
            try:
                torch.cuda.synchronize()
            finally:
                pending.clear()
                ctx.close()
        return n_cmp


def setup():
    import torch

    from oracle import oracle as O
    from shape_based_matching_amd import capi, synth
    from shape_based_matching_amd.templates import TemplateSet

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    O.build()
    O.lib()
    torch.cuda.init()
    all_ts = TemplateSet.load_npz(os.path.join(ROOT, "tests", "golden", "case1_templates.npz"))
    img = np.load(os.path.join(ROOT, "tests", "golden", "case1_test_bgr.npz"))["bgr"]
    frames, masks = {}, {}
    offs = [(40, 60), (100, 180), (0, 0)]
    for g, (rows, cols, ch) in ALL_GEOS.items():
        h, w = min(rows, img.shape[0]), min(cols, img.shape[1])
        for v in range(N_VARIANTS):
            if g in ANYGEO_ONLY_GEOS and v in (0, 1):
                # the scene (variant 3, which the profile's templates are cut from) rolled: lists that differ from frame to frame
                sc = synth.scene_bgr(1000 + rows + cols, rows, cols)
                fr = np.roll(sc, 12, axis=1) if v == 0 else np.roll(np.roll(sc, 8, axis=0), -20, axis=1)
            elif v < 3:
                r0, c0 = min(offs[v][0], rows - h), min(offs[v][1], cols - w)
                fr = synth.embed(img[:h, :w], rows, cols, r0, c0)
            else:
                fr = synth.scene_bgr(1000 + rows + cols, rows, cols)
            frames[g, v] = np.ascontiguousarray(fr if ch == 3 else fr[:, :, 1])
        m = np.zeros((rows, cols), np.uint8)
        m[rows // 8: rows - rows // 6, cols // 7: cols - cols // 9] = 255
        masks[g] = m
    return Runner(O, capi, torch, frames, masks, all_ts, {})


LAST_RUN = {}  # what the last run() counted, beside the matches it returns


def run(n_sequences, seed, steps=25, verbose=True, only=None, stop=None, profile="default"):
    """n_sequences sequences of `steps` operations of the profile, one context each; returns the number of matches compared"""
    runner = setup()
    t0 = time.time()
    n = 0
    runner.n_unchecked = runner.n_sparse_proven = 0
    idx = [only] if only is not None else range(n_sequences)
    try:
        for i in idx:
            c = runner.run(seed, i, steps, stop, profile)
            n += c
            if verbose:
                print(f"ok sequence {i} pyramid {generate(seed, i, steps, profile)[0]}: {c} compared ({time.time() - t0:.0f} s)", flush=True)
    finally:
        for p in runner.pyr_cache.values():
            p.free()
        runner.pyr_cache.clear()
    LAST_RUN.update(compared=n, unchecked=runner.n_unchecked, sparse_proven=runner.n_sparse_proven, sparse_on=runner.sparse_on)
    if verbose:
        print(f"{len(idx)} sequences x {steps} steps, seed {seed}, profile {profile}: {n} matches compared, {runner.n_unchecked} results unchecked "
              f"(resident frame unknown after a host or banded batch), {runner.n_sparse_proven} profiled calls on the sparse path, "
              f"{time.time() - t0:.0f} s", flush=True)
    return n


def replay_command(seed, index, steps, stop, profile="default"):
    """the command line that replays sequence `index` of `seed` (of the profile) up to and including step `stop`"""
    return (f"python tools/fuzz_sequence.py 1 {seed} --only {index} --steps {steps} --stop {stop}"
            + (f" --profile {profile}" if profile != "default" else ""))


def parse_args(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=20)
    ap.add_argument("seed", type=int, nargs="?", default=1)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--stop", type=int, default=None)
    ap.add_argument("--profile", choices=PROFILES, default="default")  # default | sparse | anygeo
    return ap.parse_args(argv)


if __name__ == "__main__":
    a = parse_args(sys.argv[1:])
    run(a.n, a.seed, a.steps, only=a.only, stop=a.stop, profile=a.profile)
