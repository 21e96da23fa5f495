"""Cost of the match epilogue + NMS stage (sbm_nms_batch_device) against the host alternative, on 16-frame calls.

Device: HIP events around one sbm_nms_batch_device call on the lists already in HBM (median of --reps).
Host alternative (what a caller of sbm_match_batch_device does without the stage): copy the raw lists and counts to the
host, then per frame sbm_canonicalize + the reference's adjacent unique + sbm_nms_boxes (include/nms.hpp) -- wall
time of the whole sequence (median of --reps).

Workloads: bench.py's headline (case1, 1024x1024x3 scene frames shifted 8 columns apart, 360 templates, threshold 90;
its raw lists come from sbm_match_batch_device) and synthetic lists of 256, 4096 and 65536 records per frame (clustered
positions, 40 similarity levels, labels of the uploaded templates).  Prints one JSON line per workload and, with --out,
writes them there too.

    python tools/nms_stage_cost.py [--reps 20] [--out profiles/nms_stage_cost.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from shape_based_matching_amd import capi  # noqa: E402
from shape_based_matching_amd.templates import MATCH_DTYPE  # noqa: E402

B = 16
REC = MATCH_DTYPE.itemsize


def host_alternative(facade, d_out, d_cnt, cap, sizes):
    """D2H of the raw lists, then per frame canonicalize, adjacent unique, NMSBoxes(0, 0.5); returns (seconds, kept)"""
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cnt = d_cnt.cpu().numpy().reshape(-1, 2)
    out = d_out.cpu().numpy().reshape(B, cap * REC)
    kept = []
    for f in range(B):
        r = capi.canonicalize(out[f].view(MATCH_DTYPE)[: min(int(cnt[f, 0]), cap)])
        if len(r):
            key = np.stack([r["x"], r["y"], r["similarity"].view(np.int32), r["class_idx"]], axis=1)
            first = np.ones(len(r), bool)
            first[1:] = np.any(key[1:] != key[:-1], axis=1)
            r = r[first]
        n = len(r)
        boxes = np.zeros((n, 4), np.int32)
        boxes[:, 0], boxes[:, 1] = r["x"], r["y"]
        boxes[:, 2:] = sizes[r["template_id"]]
        scores = np.ascontiguousarray(r["similarity"], np.float32)
        idx = np.zeros(max(n, 1), np.int32)
        n_out = C.c_int(0)
        facade.sbm_nms_boxes(boxes.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p), n, C.c_float(0.0), C.c_float(0.5),
                             C.c_float(1.0), 0, idx.ctypes.data_as(C.c_void_p), C.byref(n_out))
        kept.append(r[idx[: n_out.value]])
    return time.perf_counter() - t0, kept


def device_stage(ctx, d_out, d_cnt, cap, d_kept, d_kc, out_cap, stream):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record(stream)
        ctx.nms_batch_device(d_out.data_ptr(), d_cnt.data_ptr(), cap, B, d_kept.data_ptr(), out_cap, d_kc.data_ptr(), 0.0, 0.5,
                             stream=stream.cuda_stream)
        b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / 1e3


def measure(name, ctx, facade, d_out, d_cnt, cap, sizes, reps, stream):
    import torch

    out_cap = cap
    d_kept = torch.zeros(B * out_cap * REC, dtype=torch.uint8, device="cuda:0")
    d_kc = torch.zeros(B * 2, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    device_stage(ctx, d_out, d_cnt, cap, d_kept, d_kc, out_cap, stream)  # first call: label table, scratch
    dev = [device_stage(ctx, d_out, d_cnt, cap, d_kept, d_kc, out_cap, stream) for _ in range(reps)]
    host_alternative(facade, d_out, d_cnt, cap, sizes)
    host, kept = [], None
    for _ in range(reps):
        t, kept = host_alternative(facade, d_out, d_cnt, cap, sizes)
        host.append(t)
    kc = d_kc.cpu().numpy().reshape(-1, 2)
    ko = d_kept.cpu().numpy().reshape(B, out_cap * REC)
    same = all(ko[f].view(MATCH_DTYPE)[: kc[f, 0]].tolist() == kept[f].tolist() for f in range(B))
    raw = d_cnt.cpu().numpy().reshape(-1, 2)[:, 0]
    res = {"workload": name, "frames": B, "cap": cap, "raw_records_per_frame": float(np.mean(np.minimum(raw, cap))),
           "kept_per_frame": float(np.mean(kc[:, 0])), "device_stage_ms": statistics.median(dev) * 1e3,
           "host_alternative_ms": statistics.median(host) * 1e3, "same_kept_lists": bool(same), "reps": reps}
    res["speedup"] = res["host_alternative_ms"] / res["device_stage_ms"]
    return res


def main():
    import torch

    import bench

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    facade = C.CDLL(os.path.join(ROOT, "shape_based_matching_amd", "libsbm_facade.so"))
    facade.sbm_nms_boxes.restype = C.c_int
    ts = bench.case1_templates(360)
    sizes = np.zeros((ts.n_templates, 2), np.int32)
    sizes[ts.template_id, 0] = ts.levels[:, 0]["width"]
    sizes[ts.template_id, 1] = ts.levels[:, 0]["height"]
    ctx = capi.Context(T=(4, 8), weak_threshold=30.0, device_id=0)
    ctx.upload_templates(ts)
    stream = torch.cuda.Stream()
    rows = cols = 1024
    results = []
    # the headline workload's own lists
    frame = bench.case1_frame("scene", rows, cols)
    frames = np.stack([np.roll(frame, 8 * b, axis=1) for b in range(B)])
    cap = 1024
    d_imgs = torch.from_numpy(frames).to("cuda:0")
    d_out = torch.zeros(B * cap * REC, dtype=torch.uint8, device="cuda:0")
    d_cnt = torch.zeros(B * 2, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(2):
        ctx.match_batch_device(d_imgs.data_ptr(), rows * cols * 3, B, rows, cols, cols * 3, 3, 90.0, d_out.data_ptr(), cap, d_cnt.data_ptr(),
                               stream=stream.cuda_stream)
    stream.synchronize()
    results.append(measure("headline case1 (bench.py)", ctx, facade, d_out, d_cnt, cap, sizes, args.reps, stream))
    # synthetic lists
    rs = np.random.RandomState(1234)
    sims = np.linspace(99, 80, 40).astype(np.float32)
    for n in (256, 4096, 65536):
        recs = np.zeros((B, n), MATCH_DTYPE)
        for f in range(B):
            centres = rs.randint(0, 900, (max(n // 64, 4), 2))
            c = centres[rs.randint(0, len(centres), n)]
            recs[f]["x"] = c[:, 0] + rs.randint(-12, 13, n)
            recs[f]["y"] = c[:, 1] + rs.randint(-12, 13, n)
            recs[f]["similarity"] = rs.choice(sims, n)
            recs[f]["template_id"] = rs.randint(0, ts.n_templates, n)
        d_out = torch.from_numpy(recs.view(np.uint8).reshape(-1)).to("cuda:0")
        d_cnt = torch.from_numpy(np.tile(np.array([n, 0], np.int32), B)).to("cuda:0")
        results.append(measure(f"synthetic {n} records per frame", ctx, facade, d_out, d_cnt, n, sizes,
                               args.reps if n < 65536 else max(3, args.reps // 4), stream))
    ctx.close()
    lines = [json.dumps(r) for r in results]
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
