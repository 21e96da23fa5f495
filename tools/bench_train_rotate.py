#!/usr/bin/env python3
"""What a rotated template family costs: the facade demo's `train` mode (one addTemplate, then the reference's loop of
addTemplate_rotate on the host, test.cpp:303-313) against `train_rot` (the same addTemplate, then one
Detector::addTemplates_rotate call: upload, one kernel launch, download).  Both modes report the two parts of their
training section on stderr when SBM_DEMO_TIMING is set; the rotations are the part compared.  Two workloads from
tests/golden: the case1 ROI x 360 angles at 128 features (the reference's demo), and the same ROI asked for 8191 features
-- the selection keeps every candidate it has -- x 3 600 angles.  Medians of 5 alternating rounds with min - max.

    python tools/bench_train_rotate.py > profiles/train_rotate.txt
"""
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "shape_based_matching_amd", "sbm_facade_demo")
ROUNDS = 5


def write_pnm(path, magic, a):
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n255\n" % (magic, a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a).tobytes())


def run(mode, tmp, num_features, n_rot, step):
    env = dict(os.environ, SBM_DEMO_TIMING="1")
    r = subprocess.run([DEMO, mode, os.path.join(tmp, "src.ppm"), os.path.join(tmp, "mask.pgm"), str(num_features), str(n_rot), str(step), "/dev/null", "shape"],
                       capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.exit(f"{mode} failed: {r.stdout[-500:]}{r.stderr[-500:]}")
    m = re.search(r"add_template_ms ([0-9.]+) rotate_ms ([0-9.]+)", r.stderr)
    return float(m.group(1)), float(m.group(2)), r.stdout.strip().splitlines()[-1]


def features_of(tmp, num_features):
    """features per level of the trained base, from the class file of a family of one"""
    fmt = os.path.join(tmp, "%s_base.yaml")
    subprocess.run([DEMO, "train", os.path.join(tmp, "src.ppm"), os.path.join(tmp, "mask.pgm"), str(num_features), "0", "1", fmt, "shape"], check=True,
                   capture_output=True)
    sys.path.insert(0, ROOT)
    from shape_based_matching_amd.templates import read_class_yaml

    ts = read_class_yaml(fmt % "shape")
    return [int(v) for v in ts.levels[0]["n_features"]]


def main():
    train = np.load(os.path.join(ROOT, "tests", "golden", "case1_train_bgr.npz"))["bgr"]
    padded = np.zeros((470, 470, 3), np.uint8)
    padded[100:370, 100:370] = train[110:380, 130:400]
    mask = np.zeros((470, 470), np.uint8)
    mask[100:370, 100:370] = 255
    with tempfile.TemporaryDirectory() as tmp:
        write_pnm(os.path.join(tmp, "src.ppm"), b"P6", padded[:, :, ::-1])
        write_pnm(os.path.join(tmp, "mask.pgm"), b"P5", mask)
        print("rotated template families: the host loop of addTemplate_rotate (`train`) against one addTemplates_rotate call (`train_rot`)")
        print(f"facade demo, case1 ROI padded to 470 x 470, rotation part of the training section, ms; median of {ROUNDS} alternating rounds (min - max)")
        for name, nf, n_rot, step in (("case1 x 360 angles", 128, 360, 1), ("case1 at 8191 features asked x 3600 angles", 8191, 3600, 0.1)):
            counts = features_of(tmp, nf)
            times = {"train": [], "train_rot": []}
            base = []
            for _ in range(ROUNDS):
                for mode in ("train", "train_rot"):
                    add_ms, rot_ms, line = run(mode, tmp, nf, n_rot, step)
                    times[mode].append(rot_ms)
                    base.append(add_ms)
            print(f"\n{name}: base of {counts} features per level, {line}")
            print(f"  addTemplate of the base (both modes)       {statistics.median(base):10.2f}  ({min(base):.2f} - {max(base):.2f})")
            for mode, what in (("train", "host loop, addTemplate_rotate per angle "), ("train_rot", "one addTemplates_rotate call          ")):
                t = times[mode]
                print(f"  {what}    {statistics.median(t):10.2f}  ({min(t):.2f} - {max(t):.2f})")
            print(f"  ratio of the medians, loop / call          {statistics.median(times['train']) / statistics.median(times['train_rot']):10.2f}")


if __name__ == "__main__":
    main()
