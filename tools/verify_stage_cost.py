"""Device time of the verify stage (sbm_verify_batch_device: k_verify_rois, k_verify_compact) next to the two stages it
follows, and what a caller pays without it: the frames over the link.

Workload: 16 frames of 1024 x 1024 x 3 (bench.py's scene, shifted 8 columns apart), the case1 family of 360 templates,
threshold 90; sbm_match_batch_device -> sbm_nms_batch_device(0, 0.5) -> sbm_verify_batch_device(0.8) on one stream.  A
template that matches on frame 0 gets the gray of frame 0 at its top match there as its patch, any other a constant one.

Kernel times: sbm_get_timings (the dispatch packets' own begin / end stamps), summed per kernel name and call, median of
--reps.  Stage times: HIP events around each call with profiling off.  The link: one hipMemcpy of the 16 frames from and
to pinned host memory, events around it.  Prints one JSON line and, with --out, a text file.

    python tools/verify_stage_cost.py [--reps 20] [--out profiles/verify_stage.txt]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from shape_based_matching_amd import capi  # noqa: E402
from shape_based_matching_amd.templates import MATCH_DTYPE  # noqa: E402

B = 16
REC = MATCH_DTYPE.itemsize


def gray_of(bgr):
    v = bgr.astype(np.int64)
    return ((v[..., 0] * 1868 + v[..., 1] * 9617 + v[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def main():
    import torch

    import bench

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = cols = 1024
    cap, ncap, out_cap = 1024, 256, 256
    ts = bench.case1_templates(360)
    frame = bench.case1_frame("scene", rows, cols)
    frames = np.stack([np.roll(frame, 8 * b, axis=1) for b in range(B)])
    ctx = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0)
    ctx.upload_templates(ts)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    d_imgs = torch.from_numpy(frames).to("cuda:0")
    d_raw = torch.zeros(B * cap * REC, dtype=torch.uint8, device="cuda:0")
    d_rawc = torch.zeros(B * 2, dtype=torch.int32, device="cuda:0")
    d_nms = torch.zeros(B * ncap * REC, dtype=torch.uint8, device="cuda:0")
    d_nmsc = torch.zeros(B * 2, dtype=torch.int32, device="cuda:0")
    d_out = torch.zeros(B * out_cap * REC, dtype=torch.uint8, device="cuda:0")
    d_sc = torch.zeros(B * out_cap, dtype=torch.float32, device="cuda:0")
    d_oc = torch.zeros(B * 2, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    fs = rows * cols * 3

    def match():
        ctx.match_batch_device(d_imgs.data_ptr(), fs, B, rows, cols, cols * 3, 3, 90.0, d_raw.data_ptr(), cap, d_rawc.data_ptr(), stream=s)

    def nms():
        ctx.nms_batch_device(d_raw.data_ptr(), d_rawc.data_ptr(), cap, B, d_nms.data_ptr(), ncap, d_nmsc.data_ptr(), 0.0, 0.5, stream=s)

    def verify():
        ctx.verify_batch_device(d_imgs.data_ptr(), fs, B, rows, cols, cols * 3, 3, d_nms.data_ptr(), d_nmsc.data_ptr(), ncap, 0.8, d_out.data_ptr(),
                                d_sc.data_ptr(), out_cap, d_oc.data_ptr(), stream=s)

    # the patch set, from frame 0's own raw list
    match()
    match()
    stream.synchronize()
    n0 = min(int(d_rawc.cpu().numpy()[0]), cap)
    top = capi.canonicalize(d_raw.cpu().numpy()[: n0 * REC].view(MATCH_DTYPE))
    g0 = gray_of(frames[0])
    patches, cut, sizes = [], 0, {}
    for t in range(ts.n_templates):
        w, h = int(ts.levels[t, 0]["width"]), int(ts.levels[t, 0]["height"])
        lab = (int(ts.class_idx[t]), int(ts.template_id[t]))
        sizes[lab] = (w, h)
        m = top[(top["class_idx"] == lab[0]) & (top["template_id"] == lab[1])]
        p = np.full((h, w), 128, np.uint8)
        if len(m) and int(m[0]["x"]) + w <= cols and int(m[0]["y"]) + h <= rows:
            p = g0[int(m[0]["y"]): int(m[0]["y"]) + h, int(m[0]["x"]): int(m[0]["x"]) + w].copy()
            cut += 1
        patches.append((lab[0], lab[1], p))
    ctx.upload_verify_patches(patches)
    for _ in range(2):
        match(), nms(), verify()
    stream.synchronize()
    raw_n = d_rawc.cpu().numpy().reshape(-1, 2)[:, 0].tolist()
    nms_pairs = d_nmsc.cpu().numpy().reshape(-1, 2)
    kept_pairs = d_oc.cpu().numpy().reshape(-1, 2)
    nms_recs = d_nms.cpu().numpy().reshape(B, ncap * REC)
    roi = [[sizes[(int(m["class_idx"]), int(m["template_id"]))] for m in nms_recs[f].view(MATCH_DTYPE)[: nms_pairs[f, 0]]] for f in range(B)]

    # stage times, profiling off: events around each call
    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            fn()
            b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    stage = {"match": [], "nms": [], "verify": []}
    for _ in range(args.reps):
        stage["match"].append(timed(match))
        stage["nms"].append(timed(nms))
        stage["verify"].append(timed(verify))
    # kernel times: the dispatch packets' stamps
    ctx.set_profiling(True, accumulate=True)
    per = {}
    for _ in range(args.reps):
        match(), nms(), verify()
        stream.synchronize()
        tot = {}
        for name, ms in ctx.timings():
            tot[name] = tot.get(name, 0.0) + ms * 1e3
        for k, v in tot.items():
            per.setdefault(k, []).append(v)
    ctx.set_profiling(False)
    kern = {k: statistics.median(v) for k, v in per.items()}
    match_kernels = sum(v for k, v in kern.items() if k not in ("k_nms_frames", "k_verify_rois", "k_verify_compact"))
    # the link: the 16 frames to the host and back, pinned memory
    h = torch.empty(frames.shape, dtype=torch.uint8).pin_memory()
    link = {"d2h": [], "h2d": []}
    for _ in range(max(5, args.reps // 2)):
        link["d2h"].append(timed(lambda: h.copy_(d_imgs, non_blocking=True)))
        link["h2d"].append(timed(lambda: d_imgs.copy_(h, non_blocking=True)))
    ctx.close()
    res = {
        "frames": B, "rows": rows, "cols": cols, "channels": 3, "templates": ts.n_templates, "templates_with_cut_patch": cut, "reps": args.reps,
        "raw_records_per_frame": raw_n, "nms_kept_per_frame": nms_pairs[:, 0].tolist(), "verify_kept_per_frame": kept_pairs[:, 0].tolist(),
        "verify_flags_per_frame": kept_pairs[:, 1].tolist(), "roi_sizes_frame0": roi[0],
        "roi_pixels_per_call": int(sum(w * h for r in roi for (w, h) in r)),
        "kernel_us": {k: round(v, 2) for k, v in sorted(kern.items())},
        "match_call_kernels_us": round(match_kernels, 2), "k_nms_frames_us": round(kern.get("k_nms_frames", 0.0), 2),
        "k_verify_rois_us": round(kern.get("k_verify_rois", 0.0), 2), "k_verify_compact_us": round(kern.get("k_verify_compact", 0.0), 2),
        "stage_event_us": {k: round(statistics.median(v), 2) for k, v in stage.items()},
        "frames_bytes": int(frames.nbytes), "link_d2h_us": round(statistics.median(link["d2h"]), 1), "link_h2d_us": round(statistics.median(link["h2d"]), 1),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        v = res
        with open(args.out, "w") as f:
            f.write("verify stage: device time per 16-frame call (tools/verify_stage_cost.py, MI355X, median of %d calls)\n" % args.reps)
            f.write("workload: 16 frames 1024 x 1024 x 3 (bench.py scene, 8 columns apart), case1 family of %d templates, threshold 90,\n" % ts.n_templates)
            f.write("          NMSBoxes(0, 0.5), min_corr 0.8; %d templates have a patch cut from frame 0, the others a constant one\n\n" % cut)
            f.write("kernel time (dispatch stamps, sbm_get_timings), microseconds per call:\n")
            f.write("  match call, all kernels   %10.2f\n" % v["match_call_kernels_us"])
            f.write("  k_nms_frames              %10.2f\n" % v["k_nms_frames_us"])
            f.write("  k_verify_rois             %10.2f\n" % v["k_verify_rois_us"])
            f.write("  k_verify_compact          %10.2f\n" % v["k_verify_compact_us"])
            f.write("  every kernel: %s\n\n" % json.dumps(v["kernel_us"]))
            f.write("stage time (events around the call, profiling off), microseconds: %s\n\n" % json.dumps(v["stage_event_us"]))
            f.write("records per frame: raw %s\n                   after NMS %s\n                   after verify %s (flags %s)\n" %
                    (v["raw_records_per_frame"], v["nms_kept_per_frame"], v["verify_kept_per_frame"], v["verify_flags_per_frame"]))
            f.write("ROI sizes (w, h) of frame 0's records: %s; ROI pixels read per call: %d\n\n" % (v["roi_sizes_frame0"], v["roi_pixels_per_call"]))
            f.write("without the stage the caller brings the frames to the host: %d bytes, one copy to pinned memory, events around it:\n" % v["frames_bytes"])
            f.write("  device to host %10.1f us      host to device %10.1f us\n\n" % (v["link_d2h_us"], v["link_h2d_us"]))
            f.write(line + "\n")


if __name__ == "__main__":
    main()
