"""Device time of the ENet image encoder (csrc/enet.hip) on the reference's own workload -- B = 256 frames
of 328 x 256 (scripts/compute_multiview_features.py), seeded random weights --, one JSON line each, in ONE run so that the
numbers share a device state:

* ``ENetEncoder.__call__`` from channels-last f32 input (spacap_enet_encode_f32) and ``from_uint8`` (spacap_enet_encode_u8);
* the initial block and every bottleneck kind at every stage alone (its two launches together);
* ``--torch``: the same network written with plain torch.nn.functional ops (conv2d / batch_norm / prelu / max_pool2d) on the
  same device from the same table -- what a user has without this module.  The reference's own module cannot run beside it
  (its file is not part of this repository), and its layers are these calls.

Also printed: the multiply-accumulates of the network counted from the table, and the bytes the launches move (every
activation tensor written once and read once per launch that reads it), with the time both would take at the chip's peaks.

Run:  timeout -k 10 600 python tools/bench_enet.py [--batch 256] [--iters 5] [--torch]"""
import argparse
import json
import os
import sys

import numpy as np

from _eval_bench import ROOT, eager_us

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MFMA_F32_TFLOPS = 155.0     # measured fp32-MFMA peak of one MI355X
HBM_TBPS = 8.0


def count(H, W, layers):
    """(MACs, bytes moved) per image, per launch group: [(name, macs, bytes)]"""
    h, w = H // 2, W // 2
    rows = [("initial", h * w * 27 * 13, 4 * (H * W * 3 + h * w * 16))]
    for i, (kind, cin, cout, dil, _) in enumerate(layers):
        m = cout // 4
        hi, wi = h, w
        if kind == "down":
            h, w = h // 2, w // 2
        taps1, taps2 = (4 if kind == "down" else 1), (25 if kind == "asym" else 9)
        macs = h * w * (taps1 * cin * m + taps2 * m * m + m * cout)
        # reduce: input read, inner map written; main: inner map read, input read again (skip), output written
        moved = 4 * (2 * hi * wi * cin + 2 * h * w * m + h * w * cout)
        rows.append((f"{i}:{kind}{cout}d{dil}", macs, moved))
    return rows


def torch_net(sd, x, layers):
    import torch.nn.functional as F
    bn = lambda p, t: F.batch_norm(t, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False,
                                   0.1, 1e-3)
    x = torch_cat([F.conv2d(x, sd["0.0.weight"], sd["0.0.bias"], 2, 1), F.max_pool2d(x, 2)])
    x = F.prelu(bn("2", x), sd["3.weight"])
    for i, (kind, cin, cout, dil, p) in enumerate(layers):
        g = lambda k, n="weight": sd[f"{4 + i}.0.0.{k}.{n}"]
        y = F.prelu(bn(f"{4 + i}.0.0.1", F.conv2d(x, g(0), None, 2 if kind == "down" else 1)), g(2))
        if kind == "asym":
            y = F.conv2d(F.conv2d(y, g(3), None, 1, (0, 2)), g(4), g(4, "bias"), 1, (2, 0))
            k = 5
        else:
            y = F.conv2d(y, g(3), g(3, "bias"), 1, dil, dil)
            k = 4
        y = F.prelu(bn(f"{4 + i}.0.0.{k}", y), g(k + 1))
        y = bn(f"{4 + i}.0.0.{k + 3}", F.conv2d(y, g(k + 2))) * (1 - p)
        if kind == "down":
            y = y + F.pad(F.max_pool2d(x, 2), (0, 0, 0, 0, 0, cout - cin))
        else:
            y = y + x
        x = F.prelu(y, sd[f"{4 + i}.2.weight"])
    return x


def torch_cat(ts):
    import torch
    return torch.cat(ts, 1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--height", type=int, default=256)
    p.add_argument("--width", type=int, default=328)
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--torch", action="store_true", help="also time the torch.nn.functional network")
    a = p.parse_args()
    import torch
    import enet_restated as R
    from spacap3d_amd.enet import ENetEncoder
    dev = "cuda:0"
    B, H, W = a.batch, a.height, a.width
    sd = R.random_state_dict(R.WEIGHT_SEED)
    enc = ENetEncoder.from_state_dict(sd, dev)
    shape = {"B": B, "H": H, "W": W, "iters": a.iters}
    rows = count(H, W, R.LAYERS)
    macs, moved = sum(r[1] for r in rows), sum(r[2] for r in rows)
    print(json.dumps(dict(shape, what="work", macs_per_frame=macs, gflop_per_frame=round(2 * macs / 1e9, 4),
                          bytes_per_frame=moved, ms_at_mfma_peak=round(2 * macs * B / MFMA_F32_TFLOPS / 1e9, 3),
                          ms_at_hbm_peak=round(moved * B / HBM_TBPS / 1e9, 3))), flush=True)

    torch.manual_seed(0)
    u8 = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev)
    mean, std = (torch.tensor(v, device=dev) for v in (enc.SCANNET_MEAN, enc.SCANNET_STD))
    x_nhwc = (u8.float() / torch.full((1,), 255.0, device=dev) - mean) / std
    images = x_nhwc.permute(0, 3, 1, 2)          # (B, 3, H, W), channels-last in memory: read as it is
    for _ in range(2):
        out = enc(images)
    us = eager_us(lambda: enc(images), a.iters)
    print(json.dumps(dict(shape, what="encode_f32", device_ms=round(us / 1e3, 3), tflops=round(2 * macs * B / us / 1e6, 2),
                          share_of_mfma_peak=round(2 * macs * B / us / 1e6 / MFMA_F32_TFLOPS, 3),
                          moved_TBps=round(moved * B / us / 1e6, 2))), flush=True)
    enc.from_uint8(u8)
    us8 = eager_us(lambda: enc.from_uint8(u8), a.iters)
    print(json.dumps(dict(shape, what="encode_u8", device_ms=round(us8 / 1e3, 3))), flush=True)
    planar = images.contiguous()
    usp = eager_us(lambda: enc(planar), a.iters)
    print(json.dumps(dict(shape, what="encode_f32 from planar (B, 3, H, W), transposing copy included",
                          device_ms=round(usp / 1e3, 3))), flush=True)

    # one layer at a time: the initial block, then every distinct (kind, width, dilation)
    t = eager_us(lambda: enc.initial(images), a.iters)
    print(json.dumps(dict(what="layer", name="initial", count=1, device_ms=round(t / 1e3, 3),
                          tflops=round(2 * rows[0][1] * B / t / 1e6, 2), moved_TBps=round(rows[0][2] * B / t / 1e6, 2))), flush=True)
    x = enc.initial(images)
    h, w = H // 2, W // 2
    seen, total = {}, t
    for i, (kind, cin, cout, dil, _) in enumerate(R.LAYERS):
        key = (kind, cout, dil)
        if key not in seen:
            enc.bottleneck(i, x, h, w)
            seen[key] = [eager_us(lambda: enc.bottleneck(i, x, h, w), a.iters), 0, rows[i + 1], (h, w)]
        seen[key][1] += 1
        x = enc.bottleneck(i, x, h, w)
        if kind == "down":
            h, w = h // 2, w // 2
    for (kind, cout, dil), (t, n, r, (hh, ww)) in seen.items():
        total += t * n
        print(json.dumps(dict(what="layer", name=f"{kind} -> {cout}, dilation {dil}", input_map=[hh, ww], count=n,
                              device_ms=round(t / 1e3, 3), tflops=round(2 * r[1] * B / t / 1e6, 2),
                              moved_TBps=round(r[2] * B / t / 1e6, 2))), flush=True)
    print(json.dumps(dict(what="layers summed", device_ms=round(total / 1e3, 3))), flush=True)
    assert torch.equal(x, out)

    if a.torch:
        tsd = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in sd.items()}
        with torch.no_grad():
            want = torch_net(tsd, planar, R.LAYERS)
            torch.cuda.synchronize()
            ust = eager_us(lambda: torch_net(tsd, planar, R.LAYERS), max(1, a.iters // 2))
        hh, ww = H // 8, W // 8
        diff = float((out.view(B, hh, ww, 128).permute(0, 3, 1, 2) - want).abs().max())
        print(json.dumps(dict(shape, what="torch.nn.functional network", device_ms=round(ust / 1e3, 3),
                              times_kernel=round(ust / us, 2), max_abs_difference=diff)), flush=True)


if __name__ == "__main__":
    main()
