"""Generates tests/golden/postprocess_ref.npz by RUNNING THE REFERENCE'S OWN post-processing in this container:
``parse_predictions`` (lib/ap_helper.py:45-160: scipy Delaunay hull per box, utils/nms.py class-aware 3D NMS),
``extract_pc_in_box3d`` (data/scannet/model_util_scannet.py:18-21) for the per-box point counts and
``box3d_iou_batch_tensor`` (utils/box_util.py:183-209) for the IoU against the assigned ground-truth box.

Nothing of the reference is copied.  Shims: the easydict stand-in of make_fixtures_pipeline.py and empty ``plyfile`` /
``trimesh`` / ``matplotlib`` modules (imported at module level by utils/pc_utils.py, unused here; ``pyplot.cm.jet`` is a
default argument value there, so the stand-in carries it).  ``box3d_iou_batch_tensor`` moves a zero tensor to the GPU
(``.cuda()``): on this CPU-only run that call is the identity.

Cases (each with its inputs and the reference's outputs, keys prefixed ``<case>/``):
  main    B=3, N=3000, K=256: clusters of jittered near-duplicate boxes of one class and of mixed classes (NMS really
          suppresses), boxes outside the cloud, boxes holding exactly 4 and exactly 5 points, boxes with flipped
          (negative-size) corners, ground-truth corners (f32, as the reference's dataset stores them) and assignments with
          IoUs on both sides of 0.5;
  k512    B=2, N=4000, K=512;
  nocls / oldtype / oldnocls: the main inputs under cls_nms=False, use_old_type_nms=True, and both.
The generator asserts that no point lies within 1e-5 of a box face (Delaunay's tolerance band), that the sorted obj_prob
values of a scene are more than 1e-6 apart (relative) and that no obj_prob lies within 1e-6 of conf_thresh.

Run:  python tests/golden/make_fixtures_postprocess.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
NC = 18
SIGNS = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64)


def corners_of(center, size):
    """(K,3), (K,3) -> (K,8,3) f64; a negative size component flips the corner order along that axis."""
    return center[:, None, :] + SIGNS[None] * (size[:, None, :] / 2)


def make_scene(rng, N, K, M=16):
    lo_room, hi_room = np.array([-3.0, -3.0, 0.0]), np.array([3.0, 3.0, 2.5])
    base_c = rng.uniform(lo_room + 0.6, hi_room - 0.6, (M, 3))
    base_s = rng.uniform(0.4, 1.0, (M, 3))
    n_obj = N // 3 // M
    pts = [rng.uniform(lo_room, hi_room, (N - n_obj * M, 3))]
    for m in range(M):
        pts.append(base_c[m] + rng.uniform(-0.5, 0.5, (n_obj, 3)) * base_s[m])
    pts = np.concatenate(pts)
    centers, sizes, cls, assign = [], [], [], []
    base_cls = rng.integers(0, NC, M)
    k = 0
    m = 0
    while k < K - 40:        # clusters: 3..8 near-duplicates around a ground-truth box
        n = int(rng.integers(3, 9))
        mixed = rng.random() < 0.35
        for _ in range(n):
            jit = rng.uniform(0.02, 0.25)
            centers.append(base_c[m % M] + rng.normal(0, 1, 3) * jit * base_s[m % M] * 0.3)
            sizes.append(base_s[m % M] * rng.uniform(1 - jit, 1 + jit, 3))
            cls.append(int(rng.integers(0, NC)) if mixed else int(base_cls[m % M]))
            assign.append(m % M)
        k += n
        m += 1
    while k < K - 12:        # lone random boxes
        centers.append(rng.uniform(lo_room, hi_room))
        sizes.append(rng.uniform(0.1, 0.8, 3))
        cls.append(int(rng.integers(0, NC)))
        assign.append(int(rng.integers(0, M)))
        k += 1
    special = []
    for kind in ("out", "out", "out", "four", "four", "four", "five", "five", "five", "flip", "flip", "flip"):
        if kind == "out":     # entirely outside the cloud
            c = rng.uniform(lo_room, hi_room) + np.array([0, 0, 5.0])
            s = rng.uniform(0.2, 0.6, 3)
        elif kind == "flip":  # negative sizes: the corner order is reversed along those axes
            c = base_c[int(rng.integers(0, M))] + rng.normal(0, 0.02, 3)
            s = -rng.uniform(0.3, 0.9, 3) * np.array([1, -1 if rng.random() < 0.5 else 1, 1])
        else:                 # a small box in a free spot, later filled with exactly 4 / 5 points
            while True:
                c = rng.uniform(lo_room + 0.1, hi_room - 0.1)
                s = np.full(3, 0.05)
                if not np.any(np.all(np.abs(pts - c) <= 0.05, axis=1)):
                    break
        special.append((kind, len(centers)))
        centers.append(c)
        sizes.append(s)
        cls.append(int(rng.integers(0, NC)))
        assign.append(int(rng.integers(0, M)))
    centers, sizes = np.array(centers), np.array(sizes)
    slot = 0
    for kind, j in special:
        if kind in ("four", "five"):
            n = 4 if kind == "four" else 5
            pts[slot:slot + n] = centers[j] + rng.uniform(-0.4, 0.4, (n, 3)) * np.abs(sizes[j])
            slot += n
    perm = rng.permutation(K)
    centers, sizes = centers[perm], sizes[perm]
    cls, assign = np.array(cls)[perm], np.array(assign)[perm]
    corners = corners_of(centers, sizes)
    # keep points out of Delaunay's tolerance band around every face (re-draw the few that fall in it)
    lo, hi = corners.min(1), corners.max(1)
    for _ in range(100):
        bad = np.zeros(len(pts), bool)
        for kk in range(K):
            near = np.all((pts >= lo[kk] - 1e-5) & (pts <= hi[kk] + 1e-5), axis=1)
            inner = np.all((pts > lo[kk] + 1e-5) & (pts < hi[kk] - 1e-5), axis=1)
            bad |= near & ~inner
        if not bad.any():
            break
        pts[bad] = rng.uniform(lo_room, hi_room, (int(bad.sum()), 3))
    else:
        raise AssertionError("points keep landing on box faces")
    pts = pts.astype(np.float32)
    p64 = pts.astype(np.float64)
    for kk in range(K):
        near = np.all((p64 >= lo[kk] - 1e-5) & (p64 <= hi[kk] + 1e-5), axis=1)
        inner = np.all((p64 > lo[kk] + 1e-5) & (p64 < hi[kk] - 1e-5), axis=1)
        assert not (near & ~inner).any(), "a point lies within 1e-5 of a box face"
    height = (pts[:, 2:3] - np.percentile(pts[:, 2], 0.99)).astype(np.float32)
    pc = np.concatenate([pts, height], 1)
    # objectness: probabilities well apart from each other and from conf_thresh
    probs = rng.permutation(np.linspace(0.01, 0.99, K)) + rng.uniform(-2e-4, 2e-4, K)
    probs[:K // 8] = rng.uniform(0.001, 0.04, K // 8)   # some below conf_thresh
    x0 = rng.normal(0, 1, K).astype(np.float32)
    x1 = (x0 + np.log(probs / (1 - probs))).astype(np.float32)
    obj = np.stack([x0, x1], 1)
    scores = rng.normal(0, 1.5, (K, NC)).astype(np.float32)
    scores[np.arange(K), cls] += 4.0
    sem_cls = scores.argmax(1).astype(np.int64)
    gt = corners_of(base_c, base_s).astype(np.float32)
    return pc, corners, obj, sem_cls, scores, gt, assign.astype(np.int64)


def install_stubs():
    ed = types.ModuleType("easydict")

    class EasyDict(dict):
        def __getattr__(self, k):
            try:
                return self[k]
            except KeyError:
                raise AttributeError(k)

        def __setattr__(self, k, v):
            self[k] = v

    ed.EasyDict = EasyDict
    sys.modules["easydict"] = ed
    ply = types.ModuleType("plyfile")
    ply.PlyData = ply.PlyElement = object
    sys.modules["plyfile"] = ply
    sys.modules["trimesh"] = types.ModuleType("trimesh")
    mpl, plt = types.ModuleType("matplotlib"), types.ModuleType("matplotlib.pyplot")
    plt.cm = types.SimpleNamespace(jet=None)
    mpl.pyplot = plt
    sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, plt


def main():
    install_stubs()
    os.chdir(REF)
    sys.path.insert(0, REF)
    import torch
    from lib.ap_helper import parse_predictions, softmax
    from data.scannet.model_util_scannet import extract_pc_in_box3d
    from utils.box_util import box3d_iou_batch_tensor

    torch.Tensor.cuda = lambda self, *a, **k: self   # box3d_iou_batch_tensor's zeros(...).cuda() on a CPU-only box
    rng = np.random.default_rng(2024)
    DC = types.SimpleNamespace(num_class=NC)
    out = {}

    def scenes(B, N, K):
        cols = list(zip(*[make_scene(rng, N, K) for _ in range(B)]))
        return [np.stack(c) for c in cols]

    inputs = {"main": scenes(3, 3000, 256), "k512": scenes(2, 4000, 512)}
    variants = {"main": ("main", True, False), "k512": ("k512", True, False), "nocls": ("main", False, False),
                "oldtype": ("main", True, True), "oldnocls": ("main", False, True)}
    for name, (src, cls_nms, old_type) in variants.items():
        pc, corners, obj, sem_cls, scores, gt, assign = inputs[src]
        B, K = sem_cls.shape
        cfg = {"remove_empty_box": True, "use_3d_nms": True, "nms_iou": 0.25, "use_old_type_nms": old_type,
               "cls_nms": cls_nms, "per_class_proposal": True, "conf_thresh": 0.05, "dataset_config": DC}
        ep = {"center": torch.zeros(B, K, 3), "bbox_corner": torch.from_numpy(corners), "sem_cls": torch.from_numpy(sem_cls),
              "sem_cls_scores": torch.from_numpy(scores), "point_clouds": torch.from_numpy(pc),
              "objectness_scores": torch.from_numpy(obj)}
        bpmc = parse_predictions(ep, cfg)
        pred_mask = ep["pred_mask"]
        obj_prob = softmax(obj)[:, :, 1]
        conf = softmax(scores) * obj_prob[:, :, None]
        valid = (pred_mask == 1) & (obj_prob > cfg["conf_thresh"])
        rows = []   # (scene, class, proposal, conf) of batch_pred_map_cls in order
        for i, lst in enumerate(bpmc):
            for (c, box, cf) in lst:
                j = int(np.nonzero(np.all(corners[i] == box, axis=(1, 2)))[0][0])
                assert cf == conf[i, j, c] and valid[i, j]
                rows.append((i, c, j, float(cf)))
        assert len(rows) == NC * int(valid.sum())
        for i in range(B):
            p = np.sort(obj_prob[i].astype(np.float64))
            assert np.all(np.diff(p) > 1e-6 * p[1:]), "obj_prob values too close"
            assert np.all(np.abs(obj_prob[i] - 0.05) > 1e-6), "obj_prob next to conf_thresh"
        if src == name:
            count = np.zeros((B, K), np.int32)
            for i in range(B):
                for j in range(K):
                    count[i, j] = len(extract_pc_in_box3d(pc[i, :, 0:3], corners[i, j])[0])
            gt_t, oa_t = torch.from_numpy(gt), torch.from_numpy(assign)
            assigned = torch.gather(gt_t, 1, oa_t.view(B, K, 1, 1).repeat(1, 1, 8, 3))
            ious = box3d_iou_batch_tensor(assigned.view(-1, 8, 3), torch.from_numpy(corners).view(-1, 8, 3)).view(B, K).numpy()
            good = ious > 0.5
            print(f"{name}: counts 4 -> {int((count == 4).sum())}, 5 -> {int((count == 5).sum())}, 0 -> {int((count == 0).sum())}; "
                  f"good IoU {int(good.sum())} / {B * K}")
            assert (count == 4).any() and (count == 5).any() and (count == 0).any()
            assert good.any() and (~good).any()
            out.update({f"{name}/point_clouds": pc, f"{name}/bbox_corner": corners, f"{name}/objectness_scores": obj,
                        f"{name}/sem_cls": sem_cls, f"{name}/sem_cls_scores": scores, f"{name}/gt_box_corner_label": gt,
                        f"{name}/object_assignment": assign, f"{name}/point_count": count, f"{name}/ious": ious,
                        f"{name}/good": good})
        kept = int(pred_mask.sum())
        print(f"{name}: kept {kept} of {pred_mask.size} (non-empty {int((out[f'{src}/point_count'] >= 5).sum())})")
        out.update({f"{name}/pred_mask": pred_mask.astype(np.uint8), f"{name}/obj_prob": obj_prob, f"{name}/conf": conf,
                    f"{name}/valid": valid, f"{name}/pred_map_cls": np.array([r[:3] for r in rows], np.int64).reshape(-1, 3),
                    f"{name}/pred_map_conf": np.array([r[3] for r in rows], np.float32)})
    path = os.path.join(HERE, "postprocess_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
