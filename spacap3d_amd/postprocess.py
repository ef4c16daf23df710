"""Evaluation post-processing on the device: empty-box removal, class-aware 3D NMS and the IoU against the assigned
ground-truth box (csrc/postprocess.hip).

The reference runs this on the host for every evaluation batch: ``parse_predictions`` (lib/ap_helper.py:45-160; a scipy
Delaunay hull per proposal tested against every point, then a numpy NMS per scene) and the IoU / mask block of
``feed_scene_cap`` (lib/eval_helper.py:146-177).  Here it is two launches and no host synchronisation:

* ``detection_postprocess``  -- the device tensors (capturable in a graph);
* ``caption_eval_masks``     -- the masks and IoUs ``feed_scene_cap`` builds;
* ``parse_predictions``      -- drop-in for the reference's function (same signature, same outputs), one device-to-host
  copy of the compact results.

Only ``use_3d_nms=True`` is implemented (the 2D bird's-eye NMS raises ``NotImplementedError``).  CPU tensors raise
``RuntimeError("... CPU not supported")``: there is no host fallback.
"""
import numpy as np
import torch

from ._eval_util import MAX_PROPOSALS, gpu, ptr, to_host
from ._native import check, lib

REMOVE_EMPTY, CLS_NMS, OLD_TYPE, GT_F32 = 1, 2, 4, 8   # SPACAP_PP_* of include/spacap_hip.h


def post_kwargs(config_dict):
    """The keyword arguments of ``detection_postprocess`` for a reference POST_DICT (scripts/eval.py:201-210)."""
    if not config_dict.get("use_3d_nms", True):
        raise NotImplementedError("postprocess: use_3d_nms=False (2D bird's-eye NMS) is not implemented")
    kw = {}
    for src, dst in (("remove_empty_box", "remove_empty_box"), ("nms_iou", "nms_iou"), ("use_old_type_nms", "old_type"),
                     ("cls_nms", "cls_nms"), ("conf_thresh", "conf_thresh"), ("min_points", "min_points")):
        if src in config_dict:
            kw[dst] = config_dict[src]
    return kw


def _run(point_clouds, bbox_corner, objectness_scores, sem_cls, sem_cls_scores, nms_iou, cls_nms, old_type,
         remove_empty_box, min_points, conf_thresh, gt_corners=None, object_assignment=None, min_iou=0.5):
    pc = gpu("postprocess", point_clouds, "point_clouds")
    dev = pc.device
    for name, t in (("bbox_corner", bbox_corner), ("objectness_scores", objectness_scores), ("sem_cls", sem_cls)):
        gpu("postprocess", t, name)
        if t.device != dev:
            raise RuntimeError(f"postprocess: {name} must be on {dev}")
    if pc.dim() != 3 or pc.shape[2] < 3:
        raise RuntimeError(f"postprocess: point_clouds must be (B, N, C >= 3), got {tuple(pc.shape)}")
    B, N, C = pc.shape
    K = bbox_corner.shape[1]
    if tuple(bbox_corner.shape) != (B, K, 8, 3):
        raise RuntimeError(f"postprocess: bbox_corner must be (B, K, 8, 3), got {tuple(bbox_corner.shape)}")
    if not 1 <= K <= MAX_PROPOSALS:
        raise RuntimeError(f"postprocess: K={K} proposals, supported 1..{MAX_PROPOSALS}")
    pc = pc.float().contiguous()
    corners = bbox_corner.double().contiguous()
    obj = objectness_scores.float().contiguous()
    cls = sem_cls.long().contiguous()
    scores = None if sem_cls_scores is None else gpu("postprocess", sem_cls_scores, "sem_cls_scores").float().contiguous()
    NC = 0 if scores is None else scores.shape[-1]
    flags = (REMOVE_EMPTY if remove_empty_box else 0) | (CLS_NMS if cls_nms else 0) | (OLD_TYPE if old_type else 0)
    gt = oa = None
    M = 0
    if gt_corners is not None:
        gpu("postprocess", gt_corners, "gt_box_corner_label")
        gpu("postprocess", object_assignment, "object_assignment")
        if gt_corners.dtype == torch.float32:
            flags |= GT_F32
        gt = gt_corners.double().contiguous()   # widened once; the f32 volume is restated in the kernel (GT_F32)
        M = gt.shape[1]
        oa = object_assignment.long().contiguous()

    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        ws = torch.empty(int(lib.spacap_points_in_box_workspace_bytes(B, N, K)), dtype=torch.uint8, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        obj_prob = torch.empty(B, K, **f32)
        count = torch.empty(B, K, dtype=torch.int32, device=dev)
        nonempty, pred, valid = (torch.empty(B, K, **u8) for _ in range(3))
        conf = None if scores is None else torch.empty(B, K, NC, **f32)
        iou = good = None
        if gt is not None:
            iou = torch.empty(B, K, dtype=torch.float64, device=dev)
            good = torch.empty(B, K, **u8)
        check(lib.spacap_points_in_box_f32(pc.data_ptr(), B, N, C, corners.data_ptr(), K, ws.data_ptr(), ws.numel(), stream),
              "spacap_points_in_box_f32")
        check(lib.spacap_detection_nms_f32(obj.data_ptr(), cls.data_ptr(), ptr(scores), NC, corners.data_ptr(), ws.data_ptr(),
                                           B, N, K, ptr(gt), M, ptr(oa), flags, int(min_points), float(nms_iou),
                                           float(conf_thresh), float(min_iou), obj_prob.data_ptr(), count.data_ptr(),
                                           nonempty.data_ptr(), pred.data_ptr(), ptr(conf), valid.data_ptr(), ptr(iou),
                                           ptr(good), stream), "spacap_detection_nms_f32")
    out = {"obj_prob": obj_prob, "point_count": count, "nonempty_mask": nonempty.view(torch.bool),
           "pred_mask": pred.view(torch.bool), "conf": conf, "valid": valid.view(torch.bool)}
    if gt is not None:
        out["iou"], out["good"] = iou, good.view(torch.bool)
    return out


def detection_postprocess(point_clouds, bbox_corner, objectness_scores, sem_cls, sem_cls_scores=None, *, nms_iou=0.25,
                          cls_nms=True, old_type=False, remove_empty_box=True, min_points=5, conf_thresh=0.05):
    """lib/ap_helper.py:61-148 (use_3d_nms) on the device.  point_clouds (B,N,C) f32 (xyz = channels 0..2), bbox_corner
    (B,K,8,3) f64, objectness_scores (B,K,2), sem_cls (B,K) int, sem_cls_scores (B,K,NC) or None; K <= 512.  Returns device
    tensors: ``obj_prob`` f32 (B,K), ``point_count`` i32 (B,K), ``nonempty_mask`` / ``pred_mask`` / ``valid`` bool (B,K)
    (valid = pred_mask & obj_prob > conf_thresh) and ``conf`` f32 (B,K,NC) = softmax(sem_cls_scores) * obj_prob (None
    without class scores).  A scene whose boxes are all empty gets an all-False pred_mask (the reference asserts).  No host
    synchronisation: the call can be captured in a graph."""
    return _run(point_clouds, bbox_corner, objectness_scores, sem_cls, sem_cls_scores, nms_iou, cls_nms, old_type,
                remove_empty_box, min_points, conf_thresh)


def caption_eval_masks(data_dict, min_iou=0.5, **post):
    """The masks ``feed_scene_cap`` builds (lib/eval_helper.py:146-177) from the dict after
    ``get_scene_cap_loss(..., detection=True, caption=False)``: ``nms_masks`` i64 (B,K) = pred_mask * bbox_mask,
    ``ious`` f64 (B,K) = box3d_iou_batch_tensor(assigned gt corners, bbox_corner), ``good_bbox_masks`` bool = ious > min_iou
    and ``detected_object_ids`` = scene_object_ids gathered by object_assignment.  ``post``: keyword arguments of
    ``detection_postprocess`` (defaults = the reference's POST_DICT)."""
    d = data_dict
    r = _run(d["point_clouds"], d["bbox_corner"], d["objectness_scores"], d["sem_cls"], None,
             post.get("nms_iou", 0.25), post.get("cls_nms", True), post.get("old_type", False),
             post.get("remove_empty_box", True), post.get("min_points", 5), post.get("conf_thresh", 0.05),
             gt_corners=d["gt_box_corner_label"], object_assignment=d["object_assignment"], min_iou=min_iou)
    oa = d["object_assignment"]
    return {"nms_masks": r["pred_mask"].long() * d["bbox_mask"].long(), "ious": r["iou"], "good_bbox_masks": r["good"],
            "detected_object_ids": torch.gather(d["scene_object_ids"], 1, oa)}


def parse_predictions(end_points, config_dict):
    """Drop-in for lib/ap_helper.py:45-160 with ``use_3d_nms=True``: writes ``end_points['pred_mask']`` (numpy float64
    (B,K)) and returns / stores ``batch_pred_map_cls`` -- per scene a list of (class, corners (8,3) f64, confidence)
    tuples, per class for ``per_class_proposal`` (classes 0 .. dataset_config.num_class - 1), else one tuple per box with
    its predicted class.  Raises AssertionError when a scene keeps no box (the reference's ``assert len(pick) > 0``)."""
    kw = post_kwargs(config_dict)
    per_class = config_dict.get("per_class_proposal", True)
    r = detection_postprocess(end_points["point_clouds"], end_points["bbox_corner"], end_points["objectness_scores"],
                              end_points["sem_cls"], end_points["sem_cls_scores"] if per_class else None, **kw)
    B, K = r["pred_mask"].shape
    # one device-to-host copy of everything the lists are built from
    host = to_host([r["pred_mask"].to(torch.uint8), r["valid"].to(torch.uint8), r["obj_prob"],
                    end_points["sem_cls"].long(), end_points["bbox_corner"].double()] + ([r["conf"]] if per_class else []))
    pred, valid, obj_prob, sem_cls, corners = host[:5]
    pred_mask = pred.astype(np.float64)
    end_points["pred_mask"] = pred_mask
    for i in range(B):
        assert pred[i].any(), f"scene {i}: every proposal box is empty (NMS keeps nothing)"
    batch_pred_map_cls = []
    for i in range(B):
        keep = np.nonzero(valid[i])[0]
        if per_class:
            conf = host[5]
            cur = []
            for ii in range(config_dict["dataset_config"].num_class):
                cur += [(ii, corners[i, j], conf[i, j, ii]) for j in keep]
            batch_pred_map_cls.append(cur)
        else:
            batch_pred_map_cls.append([(int(sem_cls[i, j]), corners[i, j], obj_prob[i, j]) for j in keep])
    end_points["batch_pred_map_cls"] = batch_pred_map_cls
    return batch_pred_map_cls
