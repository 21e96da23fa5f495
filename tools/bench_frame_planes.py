"""The price and the gain of planar frames: sbm_match_batch_device_planes against the interleaved table call, and against what a
holder of a [B, 3, H, W] tensor does without it.

One process, the headline workload of bench.py (16 x 1024 x 1024 x 3 frames of the scene, 360 templates, pyramid {4, 8}, threshold
90), the frames in a ring of 8 device batches, interleaved [B, H, W, 3] and planar [B, 3, H, W].  Three variants, alternating round
by round:
  A ptrs            sbm_match_batch_device_ptrs, flags 0, on the interleaved frames (the strided source pass: the same bytes loaded)
  B planes          sbm_match_batch_device_planes on the same pixels as planes
  C permute_ptrs    permute(0, 2, 3, 1) of the planar batch copied into a resident interleaved buffer on the stream (the kernel of
                    .contiguous(), without the allocator), then sbm_match_batch_device_ptrs with SBM_PTRS_ALIGNED4 on that buffer
each one batch at a time on one context (sbm_set_pipeline_depth(1)) and with four batches in flight on four contexts and streams
(depth 4: the library replays captured graphs there, as in bench.py).  Time is device-event time per step after a warm-up; the
median of the rounds is reported with their minimum, maximum and every sample.

    python tools/bench_frame_planes.py [--rounds 5] [--steps 300]          prints one JSON line
    python tools/bench_frame_planes.py --only planes --steps 20            one variant, one batch at a time (for a kernel trace)
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
from shape_based_matching_amd import capi, torch_frames  # noqa: E402
from shape_based_matching_amd.templates import MATCH_DTYPE  # noqa: E402

ROWS = COLS = 1024
CH, B, CAP, RING = 3, 16, 256, 8
FRAME_BYTES = ROWS * COLS * CH
VARIANTS = ("ptrs", "planes", "permute_ptrs")


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--only", choices=VARIANTS, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ts = bench.case1_templates(360)
    frame = bench.case1_frame("scene", ROWS, COLS)
    frames = np.stack([np.roll(frame, 8 * b, axis=1) for b in range(B)])
    ring = [torch.from_numpy(frames).to(dev) for _ in range(RING)]                                          # [B, H, W, 3]
    ring_planar = [torch.from_numpy(np.ascontiguousarray(np.moveaxis(frames, -1, 1))).to(dev) for _ in range(RING)]  # [B, 3, H, W]

    class Slot:
        def __init__(self):
            self.ctx = capi.Context(T=bench.T_LEVELS, weak_threshold=30.0, device_id=0)
            self.ctx.upload_templates(ts)
            self.stream = torch.cuda.Stream(device=dev)
            self.d_out = torch.zeros(B * CAP * MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            self.d_cnt = torch.zeros(B * 2, dtype=torch.int32, device=dev)
            # one table per batch of the ring, of either kind; the interleaved copy of variant C and its table
            self.tabs = [torch.tensor([blk.data_ptr() + f * FRAME_BYTES for f in range(B)], dtype=torch.int64, device=dev) for blk in ring]
            self.ptabs = [torch_frames.plane_table(blk, stream=self.stream)[0] for blk in ring_planar]
            self.copy = torch.empty((B, ROWS, COLS, CH), dtype=torch.uint8, device=dev)
            self.ctab = torch.tensor([self.copy.data_ptr() + f * FRAME_BYTES for f in range(B)], dtype=torch.int64, device=dev)
            self.calls = 0

        def run(self, variant):
            k = self.calls % RING
            self.calls += 1
            s = self.stream.cuda_stream
            out, cnt = self.d_out.data_ptr(), self.d_cnt.data_ptr()
            if variant == "ptrs":
                self.ctx.match_batch_device_ptrs(self.tabs[k].data_ptr(), B, ROWS, COLS, COLS * CH, CH, bench.THRESHOLD, out, CAP, cnt, flags=0, stream=s)
            elif variant == "planes":
                self.ctx.match_batch_device_planes(self.ptabs[k].data_ptr(), B, ROWS, COLS, COLS, bench.THRESHOLD, out, CAP, cnt, stream=s)
            else:
                with torch.cuda.stream(self.stream):
                    self.copy.copy_(ring_planar[k].permute(0, 2, 3, 1))
                self.ctx.match_batch_device_ptrs(self.ctab.data_ptr(), B, ROWS, COLS, COLS * CH, CH, bench.THRESHOLD, out, CAP, cnt,
                                                 flags=capi.SBM_PTRS_ALIGNED4, stream=s)

    slots = [Slot() for _ in range(1 if args.only else 4)]
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

    if args.only:
        us = timed(args.only, slots)
        print(json.dumps({"only": args.only, "steps": args.steps, "us_per_step": round(us, 2), "source_form": slots[0].ctx.source_form()}))
        slots[0].ctx.close()
        return
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
    out = {"workload": f"{B} x {ROWS} x {COLS} x {CH} scene frames, 360 templates, ring of {RING} batches", "steps": args.steps, "rounds": args.rounds,
           "us_per_step": {}}
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
