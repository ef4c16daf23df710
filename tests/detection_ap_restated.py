"""numpy restatement of the detection mAP / AR (spacap3d_amd/detection_ap.py, csrc/detection_ap.hip), used by
tests/test_detection_ap_cpu.py (against the reference's recorded results, tests/golden/detection_ap_ref.npz) and by
tests/test_detection_ap_gpu.py for shapes the fixture does not hold.  It follows the device decomposition -- TP / FP flags
per (scene, class) slab, a stable global sort, then the curve -- with the arithmetic of utils/box_util.py:122-133 (box3d_iou)
and utils/eval_det.py:21-52, 148-156 (voc_ap, rec / prec)."""
import numpy as np

EXISTS = 0x80


def iou_matrix(pred, gt):
    """box3d_iou of every (prediction, ground-truth) pair: pred (n,8,3), gt (G,8,3) f64 -> (n,G) f64, elementwise the
    operations of utils/box_util.py:122-133 in their order."""
    lo1, hi1 = pred.min(1)[:, None, :], pred.max(1)[:, None, :]
    lo2, hi2 = gt.min(1)[None, :, :], gt.max(1)[None, :, :]
    A, B = np.maximum(lo1, lo2), np.minimum(hi1, hi2)
    e = np.maximum(B - A, 0)
    inter = e[..., 0] * e[..., 1] * e[..., 2]
    v1 = (hi1[..., 0] - lo1[..., 0]) * (hi1[..., 1] - lo1[..., 1]) * (hi1[..., 2] - lo1[..., 2])
    v2 = (hi2[..., 0] - lo2[..., 0]) * (hi2[..., 1] - lo2[..., 1]) * (hi2[..., 2] - lo2[..., 2])
    return inter / (v1 + v2 - inter + 1e-8)


def match(corners, valid, gt, gt_cls, gt_mask, thresholds, NC, conf=None, obj_prob=None, sem_cls=None):
    """One batch -> (score f32, flags u8, index i16) slabs (B,NC,K) in the kernel's layout, npos i64 (NC,) and ovmax f64
    (B,NC,K) by proposal (-inf without a record or ground truth).  Order inside a (scene, class): score descending as f32,
    equal scores lower proposal first."""
    B, K = valid.shape
    corners = corners.astype(np.float64)
    gt = gt.astype(np.float64)
    score = np.full((B, NC, K), -np.inf, np.float32)
    flags = np.zeros((B, NC, K), np.uint8)
    index = np.zeros((B, NC, K), np.int16)
    ovmax_all = np.full((B, NC, K), -np.inf)
    npos = np.zeros(NC, np.int64)
    for b in range(B):
        live = gt_mask[b] == 1
        for c in range(NC):
            g = np.nonzero(live & (gt_cls[b] == c))[0]
            npos[c] += len(g)
            ex = valid[b].astype(bool)
            if conf is not None:
                s = conf[b, :, c].astype(np.float32)
            else:
                ex = ex & (sem_cls[b] == c)
                s = obj_prob[b].astype(np.float32)
            rec = np.nonzero(ex)[0]
            rec = rec[np.argsort(-s[rec], kind="stable")]          # ascending index among equal scores
            n = len(rec)
            rest = np.nonzero(~ex)[0]
            index[b, c] = np.concatenate([rec, rest])
            score[b, c, :n] = s[rec]
            f = np.full(n, EXISTS, np.uint8)
            if n and len(g):
                iou = iou_matrix(corners[b, rec], gt[b, g])
                cmp = np.where(np.isnan(iou), -np.inf, iou)          # `iou > ovmax` is never true for NaN
                jmax = cmp.argmax(1)                                  # first maximum
                ovmax = cmp[np.arange(n), jmax]
                ovmax_all[b, c, rec] = ovmax
                for t, thr in enumerate(thresholds):
                    taken = np.zeros(len(g), bool)
                    for d in range(n):
                        if ovmax[d] > thr and not taken[jmax[d]]:
                            taken[jmax[d]] = True
                            f[d] |= 1 << t
            flags[b, c, :n] = f
    return score, flags, index, npos, ovmax_all


def sort_run(slabs, NC):
    """[(score, flags, ...)] per step -> per class the run's score / flags in evaluation order (stable, descending) and
    the record counts."""
    score = np.concatenate([s[0].transpose(1, 0, 2).reshape(NC, -1) for s in slabs], 1)
    flags = np.concatenate([s[1].transpose(1, 0, 2).reshape(NC, -1) for s in slabs], 1)
    order = np.argsort(-score, axis=1, kind="stable")
    score, flags = np.take_along_axis(score, order, 1), np.take_along_axis(flags, order, 1)
    return score, flags, (flags >= EXISTS).sum(1)


def curve(tp_flags, npos):
    """utils/eval_det.py:148-156 + voc_ap (use_07_metric=False) for one class and threshold: tp_flags bool (n,) in
    evaluation order -> rec, prec, ap."""
    tp = np.cumsum(tp_flags.astype(np.float64))
    fp = np.cumsum((~tp_flags).astype(np.float64))
    rec = tp / float(npos + 1e-8)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return rec, prec, np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def metrics(slabs, npos, NC, T, class2type_map=None):
    """The run's result dicts (one per threshold, the reference's keys) and per (class, threshold) the rec / prec arrays."""
    _, flags, count = sort_run(slabs, NC)
    name = (lambda c: class2type_map[c]) if class2type_map else str
    classes = [c for c in range(NC) if count[c] > 0 or npos[c] > 0]
    out, curves = [], {}
    for t in range(T):
        ap, rc = {}, {}
        for c in classes:
            if count[c] == 0:
                ap[c], rc[c] = 0, 0
                continue
            rec, prec, a = curve((flags[c, :count[c]] >> t & 1).astype(bool), npos[c])
            curves[c, t] = (rec, prec)
            ap[c], rc[c] = a, rec[-1]
        d = {"%s Average Precision" % name(c): ap[c] for c in classes}
        d["mAP"] = np.mean(list(ap.values()))
        d.update({"%s Recall" % name(c): rc[c] for c in classes})
        d["AR"] = np.mean(list(rc.values()))
        out.append(d)
    return out, curves
