#!/usr/bin/env python3
"""Generate tests/golden/* from the reference's own test data (run in the
authoring container only; /root/reference does not exist on the GPU box).

Every output is DATA held by the reference's tests, re-encoded compactly:
  case{0,1,2}_templates.npz  <- test/case*/{circle,test}_templ.yaml  (template fixtures)
  case1_train_bgr.npz        <- test/case1/train.png  (BGR pixels as cv::imread would return)
  case1_test_bgr.npz         <- test/case1/test.png
  case2_train_bgr.npz, case2_test_bgr.npz
  case0_circle_bgr.npz       <- test/case0/templ/circle.png (the training image of test.cpp:scale_test)
  case0_info_scales.npy      <- the `scale:` values of test/case0/circle_info.yaml (float32)
  similarity_lut.sha256      <- digest of the 256 SIMILARITY_LUT entries (line2Dup.cpp:635)
  similarity_lut.npy         <- the 256 SIMILARITY_LUT entries themselves (uint8)
  case0_circle_templ.yaml.gz, case1_test_templ.yaml.gz, case2_test_templ.yaml.gz
                             <- test/case*/{circle,test}_templ.yaml byte for byte, gzipped (the OpenCV-written
                                files the YAML readers are checked against)
With --ref, only:
  ref_match_case1.npz        <- what the reference's own match half (oracle/_ref/ref_match_avx2, built by
                                oracle/ref_match.mk) computes on the case1 test frame's quantized maps: matchClass's raw
                                list and match()'s epilogue list at three thresholds, and the SHA-256 of one level's
                                linear memories.  The maps (from the oracle's gradient stage) and the template subset
                                are stored with it, so the GPU suite can hold the HIP kernels to it without the binary.
With --ref-train, only:
  ref_train_cases.npz        <- what the reference's own training half (oracle/_ref/ref_train, built by
                                oracle/ref_train.mk) makes of the 96 x 96 rectangle of tests/train_batch_cases.py under its
                                four masks and of the 64 x 64 rectangle under its left half (which fails), two levels, 63
                                features: per case the level records, the features (theta as bits) and the failing level.
With --ref-nms, only:
  ref_nms_cases.npz          <- what the reference's own cv_dnn::NMSBoxes (oracle/_ref/ref_nms, built by oracle/ref_nms.mk)
                                keeps of every case of tests/nms_form_cases.py and of its lists with score ties: the kept
                                indices alone (one uint16 array, the keys -- case name and parameters -- and the offsets).
No reference source text is copied.
"""
import gzip
import hashlib
import os
import re
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from shape_based_matching_amd.templates import read_class_yaml  # noqa: E402

REF = os.environ.get("SBM_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")


def imread_bgr(path):
    """cv::imread(path) default flags: 8-bit, 3-channel BGR, alpha dropped."""
    return np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1].copy()


def parse_similarity_lut(src_path):
    txt = open(src_path).read()
    m = re.search(r"SIMILARITY_LUT\[256\]\s*=\s*\{([^}]*)\}", txt)
    lut3 = int(re.search(r"LUT3\s*=\s*(\d+)\s*;", txt).group(1))
    vals = [lut3 if t.strip() == "LUT3" else int(t) for t in m.group(1).split(",")]
    assert len(vals) == 256
    return np.asarray(vals, np.uint8)


def main():
    os.makedirs(OUT, exist_ok=True)
    for case, name in ((0, "circle"), (1, "test"), (2, "test")):
        ts = read_class_yaml(f"{REF}/test/case{case}/{name}_templ.yaml")
        ts.save_npz(f"{OUT}/case{case}_templates.npz")
        print(f"case{case}: {ts.n_templates} templates, {len(ts.features)} features")
    for case, which in ((1, "train"), (1, "test"), (2, "train"), (2, "test")):
        a = imread_bgr(f"{REF}/test/case{case}/{which}.png")
        np.savez_compressed(f"{OUT}/case{case}_{which}_bgr.npz", bgr=a)
        print(f"case{case}_{which}: {a.shape}")
    a = imread_bgr(f"{REF}/test/case0/templ/circle.png")
    np.savez_compressed(f"{OUT}/case0_circle_bgr.npz", bgr=a)
    scales = [float(x) for x in re.findall(r"scale: ([0-9.e+-]+)", open(f"{REF}/test/case0/circle_info.yaml").read())]
    np.save(f"{OUT}/case0_info_scales.npy", np.asarray(scales, np.float32))
    print(f"case0 circle: {a.shape}, {len(scales)} infos")
    lut = parse_similarity_lut(f"{REF}/line2Dup.cpp")
    with open(f"{OUT}/similarity_lut.sha256", "w") as fh:
        fh.write(hashlib.sha256(lut.tobytes()).hexdigest() + "\n")
    reference_data_fixtures()


def reference_data_fixtures():
    """the reference's template YAML files and its similarity table, kept as they are (gzip without name or time stamp,
    so that re-running this leaves the files unchanged)"""
    for case, name in ((0, "circle"), (1, "test"), (2, "test")):
        raw = open(f"{REF}/test/case{case}/{name}_templ.yaml", "rb").read()
        with open(f"{OUT}/case{case}_{name}_templ.yaml.gz", "wb") as fh, gzip.GzipFile("", "wb", 9, fh, mtime=0) as gz:
            gz.write(raw)
    np.save(f"{OUT}/similarity_lut.npy", parse_similarity_lut(f"{REF}/line2Dup.cpp"))


def ref_match_fixture():
    import hashlib

    from oracle import oracle as O
    from oracle import ref_match as R
    from shape_based_matching_amd import synth
    from shape_based_matching_amd.templates import TemplateSet

    img = np.load(f"{OUT}/case1_test_bgr.npz")["bgr"]
    pyr = O.Pyramid.build(synth.embed(img, 640, 768, 40, 60), [4, 8], 30.0)
    qs = [pyr.quantized(0), pyr.quantized(1)]
    idx = np.arange(0, 361, 3, dtype=np.int32)
    ts = R.dense_ids(TemplateSet.load_npz(f"{OUT}/case1_templates.npz").subset(idx))
    thresholds = [60.0, 75.0, 90.0]
    out = {"q0": qs[0], "q1": qs[1], "template_index": idx, "thresholds": np.asarray(thresholds, np.float32)}
    with R.Reference(qs, [4, 8], ts, "avx2") as ref:
        out["lm_level"] = np.int32(1)
        out["lm_sha256"] = np.array(hashlib.sha256(ref.lm()[1].tobytes()).hexdigest())
        for k, thr in enumerate(thresholds):
            out[f"raw{k}"], out[f"epi{k}"] = ref.match(thr)
            print(f"ref_match_case1: threshold {thr}: {len(out[f'raw{k}'])} raw, {len(out[f'epi{k}'])} after the epilogue")
    np.savez_compressed(f"{OUT}/ref_match_case1.npz", **out)


def ref_train_fixture():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import train_batch_cases as TC
    from oracle import oracle as O
    from oracle import ref_train as RT

    out = {}
    for name, (img, mask) in TC.recorded_cases().items():
        got = RT.run(RT.planes_of(O, img, mask, TC.N_LEVELS, TC.WEAK, TC.nearest_mask), 63, TC.STRONG)
        out.update(TC.pack_recorded(name, got, RT))
        print(f"ref_train_cases: {name}: {got if isinstance(got, RT.Failed) else TC.counts(got)}")
    np.savez_compressed(f"{OUT}/ref_train_cases.npz", **out)


def ref_nms_fixture():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nms_form_cases as NC
    from oracle import ref_nms as RN

    problems = {NC.recorded_key(c): NC.problem(c) for _, _, c in NC.all_cases()}
    problems.update(NC.tie_problems())
    kept = RN.run_many(list(problems.values()))
    assert all(len(p[1]) < 65536 for p in problems.values())
    np.savez_compressed(f"{OUT}/ref_nms_cases.npz", **NC.pack_recorded(dict(zip(problems, kept))))
    print(f"ref_nms_cases: {len(problems)} problems, {sum(len(v) for v in kept)} kept indices")


if __name__ == "__main__":
    if sys.argv[1:] == ["--ref-nms"]:
        ref_nms_fixture()
    elif sys.argv[1:] == ["--ref"]:
        ref_match_fixture()
    elif sys.argv[1:] == ["--ref-train"]:
        ref_train_fixture()
    else:
        main()
