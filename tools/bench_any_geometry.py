#!/usr/bin/env python3
"""Batched match on frame geometries off the one-launch linear-memory builder's grid (GPU box; measurement tool).

Per geometry: 16 frames in HBM, 90 case1 templates, pyramid {4, 8}, one call in flight.  Timed alternately, in rounds:
  batch   one sbm_match_batch_device call per step (every level of every frame through k_build_lm_any)
  loop    16 sbm_match_device calls on one stream per step: the only way to serve these geometries before the batched
          any-stride builder (every level as 8 response planes through k_build_lm)
Each step ends in a stream synchronisation; the figure is host time over steps x 16 frames.  The lists of both are
compared first (as multisets, frame by frame).  Bytes written by the linear-memory stage come from the shapes.

usage: python tools/bench_any_geometry.py [--geo sensor|gray|both] [--steps 200] [--rounds 10] [--batch-only]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEOS = {"sensor": (2048, 2448, 3), "gray": (1600, 1200, 1)}  # rows, cols, channels: level 1 is 1224 / 600 columns wide
B, CAP, THR = 16, 4096, 90.0


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--geo", choices=("sensor", "gray", "both"), default="both")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--batch-only", action="store_true", help="the batched call alone (a profiler run)")
    a = ap.parse_args(argv)
    import torch

    from shape_based_matching_amd import capi, synth
    from shape_based_matching_amd.templates import MATCH_DTYPE, TemplateSet

    dev = torch.device("cuda", 0)
    rec = MATCH_DTYPE.itemsize
    ts = TemplateSet.load_npz(os.path.join(ROOT, "tests", "golden", "case1_templates.npz")).subset(range(0, 360, 4))
    img = np.load(os.path.join(ROOT, "tests", "golden", "case1_test_bgr.npz"))["bgr"]
    for name in (("sensor", "gray") if a.geo == "both" else (a.geo,)):
        rows, cols, ch = GEOS[name]
        base = synth.embed(img if ch == 3 else np.ascontiguousarray(img[:, :, 1]), rows, cols, 300, 200)
        frames = np.stack([np.roll(base, 40 * b, axis=1) for b in range(B)])
        fs, stride = rows * cols * ch, cols * ch
        d_imgs = torch.from_numpy(frames).to(dev)
        d_out = torch.zeros(B * CAP * rec, dtype=torch.uint8, device=dev)
        d_cnt = torch.zeros(B * 2, dtype=torch.int32, device=dev)
        stream = torch.cuda.Stream(device=dev)
        ctx_b = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0)
        ctx_l = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0)
        for c in (ctx_b, ctx_l):
            c.upload_templates(ts)
        torch.cuda.synchronize()

        def batch():
            ctx_b.match_batch_device(d_imgs.data_ptr(), fs, B, rows, cols, stride, ch, THR, d_out.data_ptr(), CAP, d_cnt.data_ptr(),
                                     stream=stream.cuda_stream)
            stream.synchronize()

        def loop():
            for f in range(B):
                ctx_l.match_device(d_imgs.data_ptr() + f * fs, rows, cols, stride, ch, THR, d_out.data_ptr() + f * CAP * rec, CAP,
                                   d_cnt.data_ptr() + 8 * f, stream=stream.cuda_stream)
            stream.synchronize()

        def lists():
            cnt = d_cnt.cpu().numpy().reshape(B, 2)
            out = d_out.cpu().numpy().reshape(B, CAP * rec)
            assert (cnt[:, 1] == 0).all() and (cnt[:, 0] <= CAP).all(), cnt
            return [sorted(out[f].view(MATCH_DTYPE)[: cnt[f, 0]].tolist()) for f in range(B)]

        batch()
        got_b = lists()
        if not a.batch_only:
            d_cnt.fill_(-1)
            torch.cuda.synchronize()
            loop()
            got_l = lists()
            assert got_b == got_l, "the batched call and the per-frame loop differ"
        n_matches = sum(len(g) for g in got_b)
        per_round = max(1, a.steps // a.rounds)
        for fn in ((batch,) if a.batch_only else (batch, loop)):  # warm-up of both
            for _ in range(10):
                fn()
        t_b = t_l = 0.0
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            for _ in range(per_round):
                batch()
            t_b += time.perf_counter() - t0
            if a.batch_only:
                continue
            t0 = time.perf_counter()
            for _ in range(per_round):
                loop()
            t_l += time.perf_counter() - t0
        n = a.rounds * per_round * B
        # bytes the linear-memory stage writes per frame: one spread byte per pixel of both levels + the coarsest level's 16 bit
        # planes (2 bits per pixel and orientation pair = 2 bytes per pixel) against 8 response bytes per pixel of both levels
        px0, px1 = rows * cols, (rows // 2) * (cols // 2)
        wr_new, wr_old = px0 + px1 + 2 * px1, 8 * (px0 + px1)
        line = (f"{name} {cols}x{rows}x{ch} T=(4,8) templates={ts.n_templates} frames/call={B} matches/call={n_matches} steps={a.rounds * per_round}: "
                f"batch {1e6 * t_b / n:.2f} us/frame")
        if not a.batch_only:
            line += f", loop of {B} sbm_match_device {1e6 * t_l / n:.2f} us/frame, loop/batch = {t_l / t_b:.2f}"
        line += f"; linear-memory bytes written per frame: {wr_new} (spread planes + packed bit planes) vs {wr_old} as LM_PLANES8 = {wr_new / wr_old:.3f}"
        print(line, flush=True)
        ctx_b.close()
        ctx_l.close()
        del d_imgs, d_out, d_cnt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main(sys.argv[1:])
