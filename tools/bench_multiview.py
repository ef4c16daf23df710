"""Device time of the multiview feature projection at a ScanNet-like shape (N = 150 000 points, F = 300 frames of 41 x 32,
C = 128; the synthetic room of tests/multiview_restated.py scaled up), one JSON line each, in ONE run so that the numbers
share a device state:

* ``MultiviewProjector.project_features`` (csrc/multiview.hip), mode "max", all frames in one call,
  pixel-major input -- and once more from the reference's channel-major (F, C, H, W) layout, transposing copy included;
* ``MultiviewProjector.projection_map`` alone;
* for scale, a plain torch-op loop over the frames on the same device, written from the same rules (no host reads).

Also printed: the hits, and the bytes the launch has to move -- points and depth maps once, one C-float row per hit
(``gathered``; at most every row of the input once from HBM: ``feature_rows_unique``), the (N, C) result once.

Run:  timeout -k 10 600 python tools/bench_multiview.py [--iters 5] [--points 150000] [--frames 300] [--no-loop]"""
import argparse
import json
import os
import sys

import numpy as np

from _eval_bench import ROOT, eager_us

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_loop(points, depths, poses, feats_pm, cam, corners):
    """the five rules and the "max" aggregation as torch ops, one frame after the other; f32; feats_pm (F, H*W, C)"""
    import torch
    W, H = cam["image_dims"]
    fx, fy, cx, cy = (cam["intrinsic"][0][0], cam["intrinsic"][1][1], cam["intrinsic"][0][2], cam["intrinsic"][1][2])
    N, C = points.shape[0], feats_pm.shape[2]
    acc = torch.zeros(N, C, device=points.device)
    inv = torch.linalg.inv(poses.double()).float()
    hom = torch.cat([points, torch.ones(N, 1, device=points.device)], 1)
    cw = torch.cat([corners, torch.ones(8, 1, device=points.device)], 1)
    planes = ((0, 3, 0, 1), (1, 2, 1, 5), (2, 3, 2, 6), (3, 0, 3, 7), (0, 1, 0, 4), (5, 6, 5, 4))
    for f in range(depths.shape[0]):
        w = (cw @ poses[f].t())[:, :3]
        inside = torch.ones(N, dtype=torch.bool, device=points.device)
        for k, (a, b, c, d) in enumerate(planes):
            n = torch.linalg.cross(w[b] - w[a], w[d] - w[c])
            inside &= torch.round(((points - w[2 if k < 3 else 4]) @ n) * 100) / 100 < 0
        cam_p = hom @ inv[f].t()
        z = cam_p[:, 2]
        u, v = torch.round(cam_p[:, 0] * fx / z + cx), torch.round(cam_p[:, 1] * fy / z + cy)
        ok = inside & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        pix = torch.where(ok, v * W + u, torch.zeros_like(u)).long()
        d = depths[f].reshape(-1)[pix]
        ok &= (d >= cam["depth_min"]) & (d <= cam["depth_max"]) & ((d - z).abs() <= cam["accuracy"])
        vec = feats_pm[f][pix]
        covers = ok & (vec != 0).any(1)
        empty = (acc == 0).all(1)
        acc = torch.where((covers & empty)[:, None], vec, torch.where((covers & ~empty)[:, None], torch.maximum(acc, vec), acc))
    return acc


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--points", type=int, default=150000)
    p.add_argument("--frames", type=int, default=300)
    p.add_argument("--channels", type=int, default=128)
    p.add_argument("--no-loop", action="store_true", help="skip the torch-op loop")
    a = p.parse_args()
    import torch
    import multiview_restated as R
    from spacap3d_amd.multiview import MultiviewProjector
    dev = "cuda:0"
    N, F, C = a.points, a.frames, a.channels
    W, H = R.CAM["image_dims"]
    rng = np.random.default_rng(0)
    points = R.room_points(rng, N)
    poses = R.room_poses(rng, F)
    depths = R.zbuffer(points, poses, R.CAM["intrinsic"], R.CAM["image_dims"])
    proj = MultiviewProjector(**R.CAM)
    pts, dep, pos = (torch.as_tensor(x).to(dev) for x in (points, depths, poses))
    torch.manual_seed(0)
    feats_pm = torch.randn(F, H, W, C, device=dev)                       # pixel-major
    shape = {"N": N, "F": F, "C": C, "H": H, "W": W, "iters": a.iters}

    pmap = proj.projection_map(pts, dep, pos)
    hits = int((pmap >= 0).sum())
    del pmap
    moved = {"points": 12 * N, "depth": 4 * F * H * W, "gathered": 4 * C * hits, "feature_rows_unique": 4 * C * min(hits, F * H * W),
             "result": 4 * N * C}
    print(json.dumps(dict(shape, what="bytes", hits=hits, hit_share=round(hits / (N * F), 4), **moved)), flush=True)

    us_map = eager_us(lambda: proj.projection_map(pts, dep, pos), a.iters)
    print(json.dumps(dict(shape, what="projection_map", device_ms=round(us_map / 1e3, 3))), flush=True)
    us = eager_us(lambda: proj.project_features(pts, dep, pos, feats_pm, channels_last=True), a.iters)
    gbs = (moved["points"] + moved["depth"] + moved["gathered"] + moved["result"]) / us / 1e3
    print(json.dumps(dict(shape, what="project_features", layout="pixel-major", device_ms=round(us / 1e3, 3),
                          gathered_GBps=round(gbs, 1))), flush=True)
    got = proj.project_features(pts, dep, pos, feats_pm, channels_last=True)
    feats_cm = feats_pm.permute(0, 3, 1, 2).contiguous()                 # the reference's layout
    us_cm = eager_us(lambda: proj.project_features(pts, dep, pos, feats_cm), a.iters)
    print(json.dumps(dict(shape, what="project_features", layout="channel-major, transposing copy included",
                          device_ms=round(us_cm / 1e3, 3))), flush=True)
    del feats_cm
    if a.no_loop:
        return
    corners = torch.as_tensor(R.camera_corners(**{k: R.CAM[k] for k in ("intrinsic", "depth_min", "depth_max", "image_dims")})).to(dev)
    want = torch_loop(pts, dep, pos, feats_pm.view(F, H * W, C), R.CAM, corners)      # warm-up
    us_loop = eager_us(lambda: torch_loop(pts, dep, pos, feats_pm.view(F, H * W, C), R.CAM, corners), max(1, a.iters // 3))
    same = float((got == want).all(1).float().mean())
    print(json.dumps(dict(shape, what="torch_loop", device_ms=round(us_loop / 1e3, 3), times_kernel=round(us_loop / us, 1),
                          rows_equal_to_kernel=round(same, 5))), flush=True)


if __name__ == "__main__":
    main()
