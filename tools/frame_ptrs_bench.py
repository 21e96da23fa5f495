"""The price of the frame-pointer table: sbm_match_batch_device against sbm_match_batch_device_ptrs on the same frames.

One process, the headline workload of bench.py (16 x 1024 x 1024 x 3 frames of the scene, 360 templates, pyramid {4, 8}, threshold
90), the frames packed in a ring of 8 device blocks.  Three variants, alternating round by round:
  contiguous     sbm_match_batch_device(block, frame_stride)
  ptrs_aligned4  sbm_match_batch_device_ptrs with the identity table of the same block and SBM_PTRS_ALIGNED4 (the line-shaped source pass)
  ptrs           the same table with flags = 0 (the strided source pass)
each one batch at a time on one context (sbm_set_pipeline_depth(1)) and with four batches in flight on four contexts and streams
(depth 4: the library replays captured graphs there, as in bench.py).  Time is device-event time per step after a warm-up.
The table form launches the last strip unpacked; run once more with SBM_QS_PACK=0 in the environment to see the contiguous call
unpacked too, which tells the price of the table from the price of the packing.

    python tools/frame_ptrs_bench.py [--rounds 5] [--steps 300]           prints one JSON line
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the headline workload's frames and templates)
from shape_based_matching_amd import capi  # noqa: E402
from shape_based_matching_amd.templates import MATCH_DTYPE  # noqa: E402

ROWS = COLS = 1024
CH, B, CAP, RING = 3, 16, 256, 8
FRAME_BYTES = ROWS * COLS * CH
VARIANTS = ("contiguous", "ptrs_aligned4", "ptrs")


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=40)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ts = bench.case1_templates(360)
    frame = bench.case1_frame("scene", ROWS, COLS)
    frames = np.stack([np.roll(frame, 8 * b, axis=1) for b in range(B)])
    ring = [torch.from_numpy(frames).to(dev) for _ in range(RING)]

    class Slot:
        def __init__(self):
            self.ctx = capi.Context(T=bench.T_LEVELS, weak_threshold=30.0, device_id=0)
            self.ctx.upload_templates(ts)
            self.stream = torch.cuda.Stream(device=dev)
            self.d_out = torch.zeros(B * CAP * MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            self.d_cnt = torch.zeros(B * 2, dtype=torch.int32, device=dev)
            # one identity table per block of the ring
            self.tabs = [torch.tensor([blk.data_ptr() + f * FRAME_BYTES for f in range(B)], dtype=torch.int64, device=dev) for blk in ring]
            self.calls = 0

        def run(self, variant):
            k = self.calls % RING
            self.calls += 1
            s = self.stream.cuda_stream
            if variant == "contiguous":
                self.ctx.match_batch_device(ring[k].data_ptr(), FRAME_BYTES, B, ROWS, COLS, COLS * CH, CH, bench.THRESHOLD, self.d_out.data_ptr(), CAP,
                                            self.d_cnt.data_ptr(), stream=s)
            else:
                self.ctx.match_batch_device_ptrs(self.tabs[k].data_ptr(), B, ROWS, COLS, COLS * CH, CH, bench.THRESHOLD, self.d_out.data_ptr(), CAP,
                                                 self.d_cnt.data_ptr(), flags=capi.SBM_PTRS_ALIGNED4 if variant == "ptrs_aligned4" else 0, stream=s)

    slots = [Slot() for _ in range(4)]
    torch.cuda.synchronize()

    def counts(sl):
        return sl.d_cnt.cpu().numpy().reshape(B, 2).tolist()

    def timed(variant, active):
        for sl in active:
            sl.ctx.set_pipeline_depth(len(active))
        for i in range(args.warmup):
            active[i % len(active)].run(variant)
        torch.cuda.synchronize()
        start = torch.cuda.Event(enable_timing=True)
        ends = [torch.cuda.Event(enable_timing=True) for _ in active]
        start.record(active[0].stream)
        for i in range(args.steps):
            active[i % len(active)].run(variant)
        for sl, e in zip(active, ends):
            e.record(sl.stream)
        torch.cuda.synchronize()
        return max(start.elapsed_time(e) for e in ends) * 1e3 / args.steps  # us per step

    # the three variants give the same lists
    ref = None
    for v in VARIANTS:
        slots[0].run(v)
        torch.cuda.synchronize()
        got = counts(slots[0])
        assert all(c[1] == 0 for c in got) and sum(c[0] for c in got) > 0, got
        assert ref is None or got == ref, (v, got, ref)
        ref = got
    forms = {}
    out = {"workload": f"{B} x {ROWS} x {COLS} x {CH} scene frames, 360 templates, ring of {RING} blocks", "steps": args.steps, "rounds": args.rounds,
           "SBM_QS_PACK": os.environ.get("SBM_QS_PACK", "(unset: 1)"), "us_per_step": {}}
    for label, active in (("one_at_a_time", slots[:1]), ("four_in_flight", slots)):
        samples = {v: [] for v in VARIANTS}
        for _ in range(args.rounds):
            for v in VARIANTS:
                samples[v].append(timed(v, active))
                forms[v] = active[0].ctx.source_form()
        out["us_per_step"][label] = {v: {"median": round(statistics.median(x), 2), "min": round(min(x), 2), "max": round(max(x), 2),
                                         "all": [round(t, 2) for t in x]} for v, x in samples.items()}
    out["source_form"] = forms
    for sl in slots:
        sl.ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
