"""Device time of the evaluation post-processing (spacap3d_amd/postprocess.py: points-in-box counts + NMS / masks, two
launches) per batch, taken with HIP events around graph replays of one call, at the cfg2 (8 scenes x 40 000 points, 256 proposals) and cfg5 (512 proposals,
80 000 points) shapes; also the median time of one eager call (the Python wrapper's host work included).
Prints one JSON line per shape.

Run:  timeout -k 10 300 python tools/bench_postprocess.py [--iters 200]"""
import argparse
import json
import sys

import torch

from _eval_bench import ROOT, eager_us, replay_us

sys.path.insert(0, ROOT)
from spacap3d_amd.postprocess import detection_postprocess  # noqa: E402


def scenes(B, N, K, NC=18, seed=0):
    g = torch.Generator().manual_seed(seed)
    pc = torch.cat([torch.rand(B, N, 3, generator=g) * torch.tensor([8.0, 8.0, 3.0]) - torch.tensor([4.0, 4.0, 0.0]),
                    torch.rand(B, N, 1, generator=g)], 2)
    ctr = pc[:, torch.randint(0, N, (K,), generator=g), :3].double() + 0.05 * torch.randn(B, K, 3, generator=g).double()
    size = 0.2 + torch.rand(B, K, 3, generator=g).double()
    signs = torch.tensor([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=torch.float64)
    corners = ctr[:, :, None] + signs * (size[:, :, None] / 2)
    scores = torch.randn(B, K, NC, generator=g)
    dev = "cuda:0"
    return (pc.to(dev), corners.to(dev), torch.randn(B, K, 2, generator=g).to(dev), scores.argmax(-1).to(dev), scores.to(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    for name, (B, N, K) in (("cfg2", (8, 40000, 256)), ("cfg5", (8, 80000, 512))):
        inp = scenes(B, N, K)
        fn = lambda: detection_postprocess(*inp)
        dev_us, _ = replay_us(fn, args.iters)   # the two launches replayed back to back
        call_us = eager_us(fn, args.iters)
        print(json.dumps({"shape": name, "B": B, "N": N, "K": K, "device_us_per_batch": round(dev_us, 1),
                          "eager_call_us": round(call_us, 1), "iters": args.iters}), flush=True)


if __name__ == "__main__":
    main()
