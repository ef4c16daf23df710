"""Times of the dense-caption predictions (spacap3d_amd/predictions.py, csrc/predictions.hip), one JSON line each, on synthetic
batches of cfg2 (8 scenes x 256 proposals, L = 31) and cfg5 (8 scenes x 512 proposals, L = 31), about a third of the proposals
kept:

* device time of ``dense_caption_predictions`` (one launch) per batch, HIP events around graph replays after a warm-up, median
  of 5 groups; ``to_records`` (one device-to-host copy and the list building) as wall time between device synchronisations;
* with ``--reference DIR`` (no GPU needed): the host path it replaces, on this host's CPU -- the reference's
  ``parse_predictions`` with ``per_class_proposal=False`` (which also repeats the empty-box test and the NMS on the host) and a
  ``decode_caption`` loop over the kept boxes, timed separately.  The tokens are CPU tensors here: the reference reads each
  one from the device with ``.item()``, which costs more.  DIR is a checkout of the reference.

Run:  timeout -k 10 300 python tools/bench_predictions.py [--iters 200]
      python tools/bench_predictions.py --reference DIR"""
import argparse
import json
import os
import sys
import time

import numpy as np

from _eval_bench import ROOT, enter_reference, replay_us

sys.path.insert(0, ROOT)
SOS, EOS, V, NC, L = 2, 3, 3000, 18, 31
CONFIGS = {"cfg2": (8, 256, 40000), "cfg5": (8, 512, 80000)}


def word(i):
    return {2: "sos", 3: "eos"}.get(int(i), "w%d" % int(i))


def batch(B, K, seed=0):
    """The kernel's inputs: a third of the proposals valid, one eos somewhere in most captions."""
    rng = np.random.default_rng(seed)
    tokens = rng.integers(4, V, (B, K, L))
    tokens[np.arange(B)[:, None], np.arange(K)[None], rng.integers(2, L, (B, K))] = EOS
    return {"valid": rng.random((B, K)) < 0.33, "obj_prob": rng.uniform(0.05, 1.0, (B, K)).astype(np.float32),
            "sem_cls": rng.integers(0, NC, (B, K)), "bbox_corner": rng.normal(0, 2, (B, K, 8, 3)), "lang_cap": tokens}


def reference_baseline(ref_dir):
    corners_of = enter_reference(ref_dir).corners_of
    import types
    import torch
    import data.scannet.model_util_scannet as mus
    mus.ScannetDatasetConfig = lambda: types.SimpleNamespace(num_class=NC)   # its constructor reads a ScanNet label file
    from lib.ap_helper import parse_predictions, softmax
    from lib.eval_helper import decode_caption
    idx2word = {str(i): word(i) for i in range(V)}
    cfg = {"remove_empty_box": True, "use_3d_nms": True, "nms_iou": 0.25, "use_old_type_nms": False, "cls_nms": True,
           "per_class_proposal": False, "conf_thresh": 0.05, "dataset_config": types.SimpleNamespace(num_class=NC)}
    for name, (B, K, N) in CONFIGS.items():
        rng = np.random.default_rng(1)
        lo, hi = np.array([-3.5, -2.2, 0.0]), np.array([3.5, 2.2, 2.5])
        pc = rng.uniform(lo, hi, (B, N, 3)).astype(np.float32)
        corners = np.stack([corners_of(rng.uniform(lo + 0.5, hi - 0.5, (K, 3)), rng.uniform(0.3, 1.0, (K, 3))) for _ in range(B)])
        d = batch(B, K)
        prob = d["obj_prob"].astype(np.float64).clip(1e-3, 1 - 1e-3)
        obj = np.stack([np.zeros_like(prob), np.log(prob / (1 - prob))], -1).astype(np.float32)
        ep = {"center": torch.zeros(B, K, 3), "bbox_corner": torch.from_numpy(corners), "sem_cls": torch.from_numpy(d["sem_cls"]),
              "sem_cls_scores": torch.zeros(B, K, NC), "point_clouds": torch.from_numpy(pc),
              "objectness_scores": torch.from_numpy(obj)}
        tokens = torch.from_numpy(d["lang_cap"])
        t0 = time.perf_counter()
        lists = parse_predictions(ep, cfg)
        t1 = time.perf_counter()
        n = 0
        for b in range(B):
            for j in np.nonzero((ep["pred_mask"][b] == 1) & (softmax(obj[b])[:, 1] > 0.05))[0]:
                decode_caption(tokens[b, j], idx2word)
                n += 1
        t2 = time.perf_counter()
        assert n == sum(len(x) for x in lists)
        print(json.dumps({"what": "reference parse_predictions(per_class_proposal=False) + decode_caption loop on the host",
                          "config": name, "B": B, "K": K, "N": N, "L": L, "kept": n, "seconds_parse_predictions": round(t1 - t0, 3),
                          "seconds_decode_loop": round(t2 - t1, 4), "cpus": os.cpu_count()}), flush=True)


def device_times(iters):
    import torch
    from spacap3d_amd.predictions import dense_caption_predictions, to_records
    dev = "cuda:0"
    idx2word = {str(i): word(i) for i in range(V)}
    for name, (B, K, _) in CONFIGS.items():
        d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in batch(B, K).items()}
        us, pred = replay_us(lambda: dense_caption_predictions(d, d, SOS, EOS), iters, settle=20)
        kept = int(pred["count"].sum())
        print(json.dumps({"what": "dense_caption_predictions", "config": name, "B": B, "K": K, "L": L, "kept": kept,
                          "device_us_per_batch": round(us, 2), "iters": iters}), flush=True)
        ms = []
        for _ in range(7):
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            recs = to_records(pred, idx2word=idx2word)
            ms.append((time.perf_counter() - w0) * 1e3)
        assert sum(len(x) for x in recs) == kept
        print(json.dumps({"what": "to_records (copy + lists + strings)", "config": name, "kept": kept, "ms_first": round(ms[0], 3),
                          "ms_median_of_rest": round(float(np.median(ms[1:])), 3)}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--reference", default=None, help="a checkout of the reference: time the host path on this CPU instead")
    a = p.parse_args()
    if a.reference:
        reference_baseline(os.path.abspath(a.reference))
    else:
        device_times(a.iters)


if __name__ == "__main__":
    main()
