"""Times of the detection mAP / AR (spacap3d_amd/detection_ap.py, csrc/detection_ap.hip), one JSON line each:

* device time of the ground-truth matching launch per batch (``DetectionAP.step``: both IoU thresholds in one launch) at
  the cfg2 (8 scenes, 256 proposals) and cfg5 (512 proposals) shapes with 128 label slots and 18 classes, HIP events
  around graph replays; also the median eager call (the wrapper's host work and dtype glue included);
* ``compute_metrics()`` (sort, curve launch, one device-to-host copy) after a validation-set-sized run of synthetic scenes,
  wall time with a device synchronisation on both sides;
* with ``--reference DIR`` (no GPU needed): the reference's ``APCalculator.compute_metrics`` for the same two thresholds
  on the SAME synthetic records, on this host's CPU -- the baseline.  DIR is a checkout of the reference.

Run:  timeout -k 10 300 python tools/bench_detection_ap.py [--iters 200] [--scenes 312]
      python tools/bench_detection_ap.py --reference DIR [--scenes 312]"""
import argparse
import json
import os
import sys
import time

import numpy as np

from _eval_bench import ROOT, eager_us, enter_reference, replay_us

sys.path.insert(0, ROOT)
NC, M, THRESHOLDS = 18, 128, (0.25, 0.5)


def scenes(B, K, seed):
    """About 14 live ground-truth boxes per scene, proposals jittered around them, ~80 % valid."""
    rng = np.random.default_rng(seed)
    signs = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    gc, gs = rng.uniform(-3, 3, (B, M, 3)), rng.uniform(0.3, 1.0, (B, M, 3))
    mask = (np.arange(M)[None] < rng.integers(8, 21, (B, 1))).astype(np.float32)
    gt_cls = rng.integers(0, NC, (B, M))
    pick = rng.integers(0, 20, (B, K))
    bi = np.arange(B)[:, None]
    jit = rng.uniform(0.0, 0.4, (B, K, 1))
    pc = gc[bi, pick] + rng.uniform(-1, 1, (B, K, 3)) * jit * gs[bi, pick]
    ps = gs[bi, pick] * (1 + rng.uniform(-1, 1, (B, K, 3)) * jit)
    logits = rng.normal(0, 1.5, (B, K, NC))
    logits[bi, np.arange(K)[None], gt_cls[bi, pick]] += 3.0
    e = np.exp(logits - logits.max(-1, keepdims=True))
    conf = (e / e.sum(-1, keepdims=True) * rng.uniform(0.05, 1, (B, K, 1))).astype(np.float32)
    return {"bbox_corner": pc[:, :, None] + signs * ps[:, :, None] / 2, "valid": rng.random((B, K)) < 0.8, "conf": conf,
            "gt_box_corner_label": (gc[:, :, None] + signs * gs[:, :, None] / 2).astype(np.float32),
            "sem_cls_label": gt_cls, "box_label_mask": mask}


def reference_baseline(ref_dir, n_scenes, K):
    enter_reference(ref_dir)
    import torch
    from lib.ap_helper import APCalculator, parse_groundtruths
    calcs = [APCalculator(t, None) for t in THRESHOLDS]
    records = 0
    for i in range(n_scenes // 8):
        d = scenes(8, K, seed=i)
        gts = parse_groundtruths({k: torch.from_numpy(d[k]) for k in ("gt_box_corner_label", "sem_cls_label",
                                                                       "box_label_mask")}, {})
        pred = []
        for b in range(8):    # lib/ap_helper.py:150-154 (per_class_proposal)
            keep = np.nonzero(d["valid"][b])[0]
            pred.append([(c, d["bbox_corner"][b, j], d["conf"][b, j, c]) for c in range(NC) for j in keep])
            records += len(pred[-1])
        for calc in calcs:
            calc.step(pred, gts)
    out = {"what": "reference APCalculator.compute_metrics on the host", "scenes": n_scenes // 8 * 8, "K": K,
           "records": records, "cpus": os.cpu_count()}
    devnull = open(os.devnull, "w")
    for t, calc in zip(THRESHOLDS, calcs):
        t0 = time.perf_counter()
        stdout, sys.stdout = sys.stdout, devnull
        try:
            ret = calc.compute_metrics()
        finally:
            sys.stdout = stdout
        out[f"seconds@{t}"] = round(time.perf_counter() - t0, 2)
        out[f"mAP@{t}"] = float(ret["mAP"])
    out["seconds_total"] = round(sum(out[f"seconds@{t}"] for t in THRESHOLDS), 2)
    print(json.dumps(out), flush=True)


def device_times(iters, n_scenes):
    import torch
    from spacap3d_amd.detection_ap import DetectionAP
    dev = "cuda:0"
    to = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}
    for name, K in (("cfg2", 256), ("cfg5", 512)):
        d = to(scenes(8, K, seed=0))
        ap = DetectionAP(NC, THRESHOLDS)
        step = lambda: ap.step(d, d)
        dev_us, _ = replay_us(step, iters)
        call_us = eager_us(step, iters, before=ap.reset)
        print(json.dumps({"shape": name, "B": 8, "K": K, "M": M, "NC": NC, "thresholds": len(THRESHOLDS),
                          "device_us_per_batch": round(dev_us, 1), "eager_call_us": round(call_us, 1), "iters": iters}),
              flush=True)
    ap = DetectionAP(NC, THRESHOLDS)
    records = 0
    for i in range(n_scenes // 8):
        h = scenes(8, 256, seed=i)
        records += int(h["valid"].sum()) * NC
        d = to(h)
        ap.step(d, d)
    torch.cuda.synchronize()
    ms = []
    for _ in range(7):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        m = ap.compute_metrics()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - w0) * 1e3)
    print(json.dumps({"what": "DetectionAP.compute_metrics", "scenes": n_scenes // 8 * 8, "K": 256, "records": records,
                      "ms_first": round(ms[0], 2), "ms_median_of_rest": round(float(np.median(ms[1:])), 2),
                      **{f"mAP@{t}": m[i]["mAP"] for i, t in enumerate(THRESHOLDS)}}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--scenes", type=int, default=312)
    p.add_argument("--reference", default=None, help="a checkout of the reference: time its APCalculator on the host instead")
    a = p.parse_args()
    if a.reference:
        reference_baseline(os.path.abspath(a.reference), a.scenes, 256)
    else:
        device_times(a.iters, a.scenes)


if __name__ == "__main__":
    main()
