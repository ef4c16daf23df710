"""numpy restatement of the evaluation post-processing (spacap3d_amd/postprocess.py, csrc/postprocess.hip), used by
tests/test_postprocess_cpu.py (against the reference's recorded outputs) and tests/test_postprocess_gpu.py (against the
device).  Written from the algorithms' definitions, not from the reference's code."""
import numpy as np


def closed_box_counts(xyz, corners, chunk=64):
    """xyz (N,3) f32, corners (K,8,3) f64 -> i32 (K,): points with lo <= p <= hi in every axis, compared in f64."""
    p = xyz.astype(np.float64)
    lo, hi = corners.min(1), corners.max(1)
    out = np.zeros(len(corners), np.int32)
    for s in range(0, len(corners), chunk):
        inside = (p[None] >= lo[s:s + chunk, None]) & (p[None] <= hi[s:s + chunk, None])
        out[s:s + chunk] = inside.all(-1).sum(1)
    return out


def exp_cr(x):
    """f32 exp, correctly rounded (via f64), as the kernel computes it."""
    return np.exp(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def objectness_prob(logits):
    """(..., 2) f32 -> (...) f32: exp(x - max) / sum, second column."""
    x = np.asarray(logits, np.float32)
    m = np.maximum(x[..., 0], x[..., 1])
    e0, e1 = exp_cr(x[..., 0] - m), exp_cr(x[..., 1] - m)
    return (e1 / (e0 + e1)).astype(np.float32)


def class_softmax(scores):
    """(..., NC) f32 softmax with numpy's pairwise-summation order (8 accumulators, then the tail; NC <= 128)."""
    s = np.asarray(scores, np.float32)
    e = exp_cr(s - s.max(-1, keepdims=True))
    n = s.shape[-1]
    if n < 8:
        tot = np.zeros(s.shape[:-1], np.float32)
        for j in range(n):
            tot = tot + e[..., j]
    else:
        acc = [e[..., q].copy() for q in range(8)]
        j = 8
        while j < n - n % 8:
            for q in range(8):
                acc[q] = acc[q] + e[..., j + q]
            j += 8
        tot = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))
        for jj in range(j, n):
            tot = tot + e[..., jj]
    return e / tot[..., None]


def nms_keep(corners, prob, cls, active, thr=0.25, cls_nms=True, old_type=False):
    """Greedy suppression over the active boxes of one scene -> bool (K,) keep mask.  Visiting order: prob descending,
    equal probabilities higher index first.  Overlap of the visited box i with a later box j, in f64:
    inter / (area_i + area_j - inter [+ 1e-8 with cls_nms]), or inter / area_j (old_type); times (class_i == class_j)
    with cls_nms; j is dropped when the overlap exceeds thr."""
    lo, hi = corners.min(1), corners.max(1)
    area = (hi[:, 0] - lo[:, 0]) * (hi[:, 1] - lo[:, 1]) * (hi[:, 2] - lo[:, 2])
    idx = np.nonzero(active)[0]
    order = idx[np.lexsort((-idx, -np.asarray(prob, np.float64)[idx]))]
    keep = np.zeros(len(corners), bool)
    alive = list(order)
    while alive:
        i, rest = alive[0], np.array(alive[1:], np.int64)
        keep[i] = True
        if len(rest) == 0:
            break
        ext = [np.maximum(0.0, np.minimum(hi[i, d], hi[rest, d]) - np.maximum(lo[i, d], lo[rest, d])) for d in range(3)]
        inter = ext[0] * ext[1] * ext[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            if old_type:
                ov = inter / area[rest]
            elif cls_nms:
                ov = inter / (area[i] + area[rest] - inter + 1e-8)
            else:
                ov = inter / (area[i] + area[rest] - inter)
        if cls_nms:
            ov = ov * (cls[rest] == cls[i])
        alive = list(rest[~(ov > thr)])
    return keep


def assigned_iou(gt_corners, assignment, corners):
    """IoU of each box (K,8,3) f64 with its assigned ground-truth box gt_corners[assignment] (M,8,3), the ground-truth
    volume computed in the labels' own precision (f32 labels: an f32 product), everything else in f64."""
    g = gt_corners[assignment]
    glo, ghi = g.min(1), g.max(1)
    lo, hi = corners.min(1), corners.max(1)
    ext = [np.maximum(np.minimum(ghi[:, d].astype(np.float64), hi[:, d]) - np.maximum(glo[:, d].astype(np.float64), lo[:, d]),
                      0.0) for d in range(3)]
    inter = ext[0] * ext[1] * ext[2]
    vg = ((ghi[:, 0] - glo[:, 0]) * (ghi[:, 1] - glo[:, 1]) * (ghi[:, 2] - glo[:, 2])).astype(np.float64)
    vb = (hi[:, 0] - lo[:, 0]) * (hi[:, 1] - lo[:, 1]) * (hi[:, 2] - lo[:, 2])
    return inter / (vg + vb - inter + 1e-8)


def postprocess(pc, corners, logits, sem_cls, scores=None, nms_iou=0.25, cls_nms=True, old_type=False,
                remove_empty_box=True, min_points=5, conf_thresh=0.05, obj_prob=None):
    """The whole of detection_postprocess on host arrays.  ``obj_prob``: use these probabilities for the ordering instead
    of restating them (compares the suppression alone)."""
    B, K = sem_cls.shape
    prob = objectness_prob(logits) if obj_prob is None else np.asarray(obj_prob, np.float32)
    count = np.stack([closed_box_counts(pc[b, :, :3], corners[b]) for b in range(B)])
    nonempty = count >= min_points if remove_empty_box else np.ones((B, K), bool)
    pred = np.stack([nms_keep(corners[b], prob[b], sem_cls[b], nonempty[b], nms_iou, cls_nms, old_type) for b in range(B)])
    out = {"obj_prob": prob, "point_count": count, "nonempty_mask": nonempty, "pred_mask": pred,
           "valid": pred & (prob > np.float32(conf_thresh))}
    if scores is not None:
        out["conf"] = class_softmax(scores) * prob[..., None]
    return out


def ulp_diff(a, b):
    """|a - b| in units of the last place (f32 arrays of the same sign)."""
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)
