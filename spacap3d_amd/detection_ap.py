"""Detection mAP / AR on the device (csrc/detection_ap.hip): the reference's ``APCalculator`` (lib/ap_helper.py:195-250)
with ``eval_det_cls`` / ``voc_ap`` (utils/eval_det.py:21-52, 74-158).

The reference keeps Python lists of (class, corners, score) tuples per scene and, at the end, walks every prediction of a
class in confidence order in a host loop, one ``box3d_iou`` call per ground-truth box.  Here ``DetectionAP.step`` is one
launch per batch on the current stream (TP / FP flags for all IoU thresholds at once, final per batch because a match only
depends on the better-ranked predictions of the same class in the same scene) and ``compute_metrics`` is one stable
``torch.sort`` per evaluation, one launch for the precision / recall curves and their VOC areas, and one device-to-host copy
of the per-class results.  No Python loop runs over predictions or scenes.

Ordering rules (the reference's ``np.argsort(-confidence)`` leaves ties unspecified): scores compare as f32, descending;
equal scores of a class order by earlier ``step`` call, then lower scene of the batch, then lower proposal index.  Scores
are expected to be numbers (a NaN score ranks last inside its scene; its place in the global order is unspecified).

CPU tensors raise ``RuntimeError("... CPU not supported")``: there is no host fallback.  ``parse_groundtruths`` is the
host-side drop-in for callers that still want the reference's lists.
"""
import ctypes

import numpy as np
import torch

from ._eval_util import MAX_PROPOSALS, gpu, mask_u8, ptr
from ._native import check, lib

MAX_GT, MAX_CLASSES, MAX_THRESHOLDS = 256, 128, 4
EXISTS = 0x80   # SPACAP_AP_EXISTS of include/spacap_hip.h


def parse_groundtruths(end_points, config_dict=None):
    """Drop-in for lib/ap_helper.py:163-192: per scene the list of (class int, corners (8,3) in the labels' dtype) of the
    slots whose ``box_label_mask`` equals 1; stored under ``end_points['batch_gt_map_cls']`` and returned.  Host code: one
    device-to-host copy per tensor."""
    mask = end_points["box_label_mask"].detach().cpu().numpy()
    cls = end_points["sem_cls_label"].detach().cpu().numpy()
    corners = end_points["gt_box_corner_label"].detach().cpu().numpy()
    out = [[(int(cls[i, j]), corners[i, j]) for j in range(corners.shape[1]) if mask[i, j] == 1]
           for i in range(cls.shape[0])]
    end_points["batch_gt_map_cls"] = out
    return out


class DetectionAP:
    """``DetectionAP(num_class, iou_thresholds=(0.25, 0.5), class2type_map=None, per_class_proposal=True)``.

    ``step(post, end_points)`` accumulates a batch; ``compute_metrics()`` returns one dict per threshold with the
    reference's keys (``'<name> Average Precision'``, ``'mAP'``, ``'<name> Recall'``, ``'AR'``; ``<name>`` from
    ``class2type_map`` or ``str(class)``); ``reset()`` starts over.  The means run over every class that has a prediction
    or a ground-truth box, as the reference's ``ap`` dict does.

    One deliberate difference: a class with ground truth and no prediction gets AP 0 and recall 0.  The reference's
    ``eval_det_multiprocessing`` (utils/eval_det.py:242-250) indexes its pool results by the position of the class among
    ALL classes although it only submitted those with predictions, so after such a class every later class reads a
    neighbour's result (or raises IndexError).  That misalignment is not reproduced.
    """

    def __init__(self, num_class, iou_thresholds=(0.25, 0.5), class2type_map=None, per_class_proposal=True):
        th = [float(t) for t in (iou_thresholds if np.ndim(iou_thresholds) else (iou_thresholds,))]
        if not 1 <= len(th) <= MAX_THRESHOLDS:
            raise RuntimeError(f"detection_ap: {len(th)} IoU thresholds, supported 1..{MAX_THRESHOLDS}")
        if not 1 <= int(num_class) <= MAX_CLASSES:
            raise RuntimeError(f"detection_ap: num_class={num_class}, supported 1..{MAX_CLASSES}")
        self.num_class = int(num_class)
        self.iou_thresholds = tuple(th)
        self._thr = (ctypes.c_double * len(th))(*th)
        self.class2type_map = class2type_map
        self.per_class_proposal = bool(per_class_proposal)
        self.reset()

    def reset(self):
        self.slabs = []      # per step: (score f32, flags u8, index i16), each (B, NC, K), in rank order per (scene, class)
        self.npos = None     # i32 (NC,) on the device: ground-truth boxes per class so far

    def step(self, post, end_points):
        """``post``: the dict of ``detection_postprocess`` (``valid``, and ``conf`` with per_class_proposal, else
        ``obj_prob``); ``end_points``: ``bbox_corner`` (B,K,8,3), ``sem_cls`` (B,K), ``gt_box_corner_label`` (B,M,8,3),
        ``sem_cls_label`` (B,M), ``box_label_mask`` (B,M).  One launch on the current stream, no host synchronisation;
        batches may differ in B.  Returns the batch's slab (score, flags, index)."""
        corners = gpu("detection_ap", end_points["bbox_corner"], "bbox_corner")
        dev = corners.device
        valid = gpu("detection_ap", post["valid"], "valid")
        gt = gpu("detection_ap", end_points["gt_box_corner_label"], "gt_box_corner_label")
        gt_cls = gpu("detection_ap", end_points["sem_cls_label"], "sem_cls_label")
        gt_mask = gpu("detection_ap", end_points["box_label_mask"], "box_label_mask")
        if corners.dim() != 4 or tuple(corners.shape[2:]) != (8, 3):
            raise RuntimeError(f"detection_ap: bbox_corner must be (B, K, 8, 3), got {tuple(corners.shape)}")
        B, K = corners.shape[:2]
        M = gt.shape[1]
        NC = self.num_class
        if tuple(gt.shape) != (B, M, 8, 3) or tuple(gt_cls.shape) != (B, M) or tuple(gt_mask.shape) != (B, M):
            raise RuntimeError(f"detection_ap: labels must be (B, M, 8, 3), (B, M), (B, M) with B={B}, got "
                               f"{tuple(gt.shape)}, {tuple(gt_cls.shape)}, {tuple(gt_mask.shape)}")
        if tuple(valid.shape) != (B, K):
            raise RuntimeError(f"detection_ap: valid must be (B, K) = ({B}, {K}), got {tuple(valid.shape)}")
        conf = obj_prob = sem_cls = None
        if self.per_class_proposal:
            conf = gpu("detection_ap", post["conf"], "conf").float().contiguous()
            if tuple(conf.shape) != (B, K, NC):
                raise RuntimeError(f"detection_ap: conf must be (B, K, num_class) = ({B}, {K}, {NC}), got {tuple(conf.shape)}")
        else:
            obj_prob = gpu("detection_ap", post["obj_prob"], "obj_prob").float().contiguous()
            sem_cls = gpu("detection_ap", end_points["sem_cls"], "sem_cls").long().contiguous()
            if tuple(obj_prob.shape) != (B, K) or tuple(sem_cls.shape) != (B, K):
                raise RuntimeError(f"detection_ap: obj_prob and sem_cls must be (B, K) = ({B}, {K})")
        corners = corners.double().contiguous()
        valid = mask_u8(valid)
        gt = gt.double().contiguous()                 # BBGT.astype(float)
        gt_cls = gt_cls.long().contiguous()
        gt_mask = (gt_mask == 1).to(torch.uint8).contiguous()
        with torch.cuda.device(dev):
            if self.npos is None:
                self.npos = torch.zeros(NC, dtype=torch.int32, device=dev)
            score = torch.empty(B, NC, K, dtype=torch.float32, device=dev)
            flags = torch.empty(B, NC, K, dtype=torch.uint8, device=dev)
            index = torch.empty(B, NC, K, dtype=torch.int16, device=dev)
            check(lib.spacap_detection_match_f32(corners.data_ptr(), valid.data_ptr(), ptr(conf), ptr(obj_prob), ptr(sem_cls),
                                                 B, K, NC, gt.data_ptr(), gt_cls.data_ptr(), gt_mask.data_ptr(), M, self._thr,
                                                 len(self.iou_thresholds), score.data_ptr(), flags.data_ptr(),
                                                 index.data_ptr(), self.npos.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream), "spacap_detection_match_f32")
        slab = (score, flags, index)
        if B:
            self.slabs.append(slab)
        return slab

    def sorted_records(self):
        """Per class the records of the whole run in evaluation order, on the device: ``score`` f32 (NC, L), ``flags`` u8
        (NC, L) and ``count`` i64 (NC,) -- the first ``count[c]`` entries of row c are records (the rest is the slabs'
        unused tail, score -inf)."""
        NC = self.num_class
        # (scenes of all steps, NC, K) -> (NC, scenes * K): concatenation order = step, scene, rank inside the slab; the
        # stable sort keeps it among equal scores.  Slabs of different K are laid side by side per scene.
        score = torch.cat([s.permute(1, 0, 2).reshape(NC, -1) for s, _, _ in self.slabs], 1)
        flags = torch.cat([f.permute(1, 0, 2).reshape(NC, -1) for _, f, _ in self.slabs], 1)
        score, order = torch.sort(score, dim=1, descending=True, stable=True)
        flags = torch.gather(flags, 1, order).contiguous()
        count = (flags >= EXISTS).sum(1)
        return score, flags, count

    def curves(self):
        """The device results of the run: dict with ``ap`` / ``last_rec`` f64 (NC, T), ``rec`` / ``prec`` f64 (NC, T, L) (zero behind a row's ``count[c]`` records),
        ``count`` i64 (NC,), ``npos`` i32 (NC,), ``score`` / ``flags`` (NC, L) (see ``sorted_records``)."""
        return self._run(True)

    def _run(self, with_curves):
        if not self.slabs:
            raise RuntimeError("detection_ap: compute_metrics() before any step()")
        NC, T = self.num_class, len(self.iou_thresholds)
        score, flags, count = self.sorted_records()
        dev = flags.device
        L = flags.shape[1]
        with torch.cuda.device(dev):
            ap = torch.empty(NC, T, dtype=torch.float64, device=dev)
            last = torch.empty(NC, T, dtype=torch.float64, device=dev)
            rec = prec = None
            if with_curves:
                rec = torch.zeros(NC, T, L, dtype=torch.float64, device=dev)     # the kernel writes the first count[c] of a row
                prec = torch.zeros(NC, T, L, dtype=torch.float64, device=dev)
            check(lib.spacap_ap_curve_f64(flags.data_ptr(), L, count.data_ptr(), self.npos.data_ptr(), NC, T, ptr(rec),
                                          ptr(prec), ap.data_ptr(), last.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream), "spacap_ap_curve_f64")
        return {"ap": ap, "last_rec": last, "rec": rec, "prec": prec, "count": count, "npos": self.npos, "score": score,
                "flags": flags}

    def compute_metrics(self):
        """One dict per IoU threshold, in the order of ``iou_thresholds``, with the keys and values of the reference's
        ``APCalculator(thresh, class2type_map).compute_metrics()`` (see the class docstring for the one difference)."""
        NC, T = self.num_class, len(self.iou_thresholds)
        r = self._run(False)
        small = torch.cat([r["ap"].reshape(-1), r["last_rec"].reshape(-1), r["count"].double(), r["npos"].double()])
        host = small.cpu().numpy()                   # the one device-to-host copy
        ap, last = host[:NC * T].reshape(NC, T), host[NC * T:2 * NC * T].reshape(NC, T)
        count, npos = host[2 * NC * T:2 * NC * T + NC], host[2 * NC * T + NC:]
        classes = [c for c in range(NC) if count[c] > 0 or npos[c] > 0]
        name = (lambda c: self.class2type_map[c]) if self.class2type_map else str
        out = []
        for t in range(T):
            d = {}
            aps = [float(ap[c, t]) if count[c] > 0 else 0 for c in classes]
            recs = [float(last[c, t]) if count[c] > 0 else 0 for c in classes]
            for c, v in zip(classes, aps):
                d["%s Average Precision" % name(c)] = v
            d["mAP"] = float(np.mean(aps)) if classes else float("nan")
            for c, v in zip(classes, recs):
                d["%s Recall" % name(c)] = v
            d["AR"] = float(np.mean(recs)) if classes else float("nan")
            out.append(d)
        return out
