"""Generates tests/golden/detection_ap_ref.npz by RUNNING THE REFERENCE'S OWN evaluation in this container:
``parse_groundtruths`` and ``APCalculator.step`` / ``compute_metrics`` (lib/ap_helper.py:163-250) for the IoU thresholds 0.25
and 0.5, and ``eval_det_multiprocessing`` (utils/eval_det.py:207-253, what compute_metrics calls) once more per threshold for
the per-class ``rec`` / ``prec`` arrays of ``eval_det_cls``.  Nothing of the reference is copied; the stubs are those of
make_fixtures_postprocess.py.

Cases (keys ``<case>/...``; results ``<case>/t<i>/keys|values`` = the result dict in order, ``<case>/t<i>/rec_<class>`` /
``prec_<class>``):
  main    the ``main`` inputs of postprocess_ref.npz (3 scenes, K = 256, 16 ground-truth boxes; the reference's valid / conf
          and its batch_pred_map_cls order) with class labels (the majority class of the valid proposals assigned to a box)
          and a mask that drops three slots per scene, fed as TWO step calls (2 + 1 scenes); per_class_proposal=True;
  small   B = 2, K = 64, M = 128: live label slots interleaved with masked-out ones (mask 0 and mask 2: only == 1 counts;
          some masked-out slots are copies of live boxes), three boxes of one class in scene 0, pairs of predictions whose
          best match is the same box, classes with predictions and no ground truth, scene 1 without a valid box;
  small1  the small inputs with per_class_proposal=False (a box is a prediction of its own class, scored by obj_prob).
The prediction lists are built from valid / conf / obj_prob exactly as parse_predictions builds them (lib/ap_helper.py:
150-158).  Asserted while generating: no two scores of a class are equal over a case; no ovmax within 1e-9 of a threshold;
no two ground-truth IoUs of a prediction tie for a positive maximum (a prediction that overlaps nothing has all-zero IoUs:
its jmax is never used); TPs and FPs at both thresholds; a prediction that is a TP at 0.25 and an FP at 0.5; every class
with ground truth has a prediction (the reference's pool-result misalignment, utils/eval_det.py:242-250, must not enter);
and the numpy restatement (tests/detection_ap_restated.py) reproduces the reference.

Run:  python tests/golden/make_fixtures_ap.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_fixtures_postprocess import NC, REF, corners_of, install_stubs  # noqa: E402
import detection_ap_restated as R  # noqa: E402

THRESHOLDS = (0.25, 0.5)


def main_case():
    fix = np.load(os.path.join(HERE, "postprocess_ref.npz"))
    d = {k: fix["main/" + k] for k in ("bbox_corner", "valid", "conf", "obj_prob", "sem_cls", "gt_box_corner_label",
                                        "object_assignment", "pred_map_cls", "pred_map_conf")}
    B, M = d["gt_box_corner_label"].shape[:2]
    rng = np.random.default_rng(7)
    gt_cls = np.zeros((B, M), np.int64)
    mask = np.ones((B, M), np.float32)
    for b in range(B):
        for m in range(M):
            sel = d["valid"][b] & (d["object_assignment"][b] == m)
            gt_cls[b, m] = np.bincount(d["sem_cls"][b][sel], minlength=NC).argmax() if sel.any() else rng.integers(0, NC)
        mask[b, rng.choice(M, 3, replace=False)] = 0
    # the reference's own list order (scene, class, proposal), recorded by make_fixtures_postprocess.py
    pred = [[] for _ in range(B)]
    for (i, c, j), cf in zip(d["pred_map_cls"], d["pred_map_conf"]):
        assert cf == d["conf"][i, j, c]
        pred[i].append((int(c), d["bbox_corner"][i, j], cf))
    inputs = {"bbox_corner": d["bbox_corner"], "valid": d["valid"], "conf": d["conf"], "obj_prob": d["obj_prob"],
              "sem_cls": d["sem_cls"], "gt_box_corner_label": d["gt_box_corner_label"], "sem_cls_label": gt_cls,
              "box_label_mask": mask}
    return inputs, pred, [2, 1], True


def small_case():
    rng = np.random.default_rng(11)
    B, K, M = 2, 64, 128
    live = {0: [3, 4, 7, 10, 20, 21, 50, 127], 1: [0, 64, 65, 100]}
    cls_of = {0: [5, 5, 5, 2, 9, 9, 14, 0], 1: [5, 2, 9, 14]}
    gt = np.zeros((B, M, 8, 3), np.float32)
    gt_cls = rng.integers(0, NC, (B, M)).astype(np.int64)
    mask = np.where(rng.random((B, M)) < 0.5, 0.0, 2.0).astype(np.float32)      # neither value is ground truth
    gt[:] = corners_of(rng.uniform(-3, 3, (B * M, 3)), rng.uniform(0.3, 1.0, (B * M, 3))).reshape(B, M, 8, 3)
    centers, sizes = {}, {}
    for b in range(B):
        for n, (m, c) in enumerate(zip(live[b], cls_of[b])):
            ctr, sz = np.array([-3.0 + 0.9 * n, 1.5 * b, 0.5]), rng.uniform(0.5, 0.8, 3)   # the three class-5 boxes are neighbours
            centers[b, m], sizes[b, m] = ctr, sz
            gt[b, m] = corners_of(ctr[None], sz[None])[0]
            gt_cls[b, m], mask[b, m] = c, 1.0
            # a masked-out copy of the live box and class right behind it: a reader that ignores the mask double counts
            if m + 1 < M and m + 1 not in live[b]:
                gt[b, m + 1], gt_cls[b, m + 1] = gt[b, m], c
    # scene 0 predictions: per live box several jittered copies (IoU from ~0.9 down to ~0.2), then strays
    ctr_p, sz_p, cls_p = [], [], []
    for n, (m, c) in enumerate(zip(live[0], cls_of[0])):
        for jit in (0.02, 0.05, 0.12, 0.2, 0.3, 0.45):
            ctr_p.append(centers[0, m] + rng.uniform(-1, 1, 3) * jit * sizes[0, m])
            sz_p.append(sizes[0, m] * (1 + rng.uniform(-1, 1, 3) * jit))
            cls_p.append(c if rng.random() < 0.8 else int(rng.integers(0, NC)))
    while len(ctr_p) < K:
        ctr_p.append(rng.uniform(-3, 3, 3))
        sz_p.append(rng.uniform(0.2, 0.9, 3))
        cls_p.append(int(rng.choice([11, 16, 5, 2])))          # 11 and 16 have no ground truth anywhere
    perm = rng.permutation(K)
    c0 = corners_of(np.array(ctr_p)[perm], np.array(sz_p)[perm])
    corners = np.stack([c0, corners_of(rng.uniform(-3, 3, (K, 3)), rng.uniform(0.3, 1.0, (K, 3)))])
    sem_cls = np.stack([np.array(cls_p)[perm], rng.integers(0, NC, K)]).astype(np.int64)
    obj_prob = rng.permutation(np.linspace(0.06, 0.99, B * K)).reshape(B, K).astype(np.float32)
    valid = np.ones((B, K), bool)
    valid[0, rng.choice(K, 9, replace=False)] = False
    valid[1] = False                                            # scene 1: no valid box
    sm = rng.normal(0, 1.5, (B, K, NC))
    sm[np.arange(B)[:, None], np.arange(K)[None], sem_cls] += 3.0
    sm = np.exp(sm - sm.max(-1, keepdims=True))
    conf = (sm / sm.sum(-1, keepdims=True) * obj_prob[..., None]).astype(np.float32)
    inputs = {"bbox_corner": corners, "valid": valid, "conf": conf, "obj_prob": obj_prob, "sem_cls": sem_cls,
              "gt_box_corner_label": gt, "sem_cls_label": gt_cls, "box_label_mask": mask}
    return inputs


def pred_lists(inp, per_class):
    """lib/ap_helper.py:150-158 on the recorded valid / conf / obj_prob."""
    out = []
    for i in range(len(inp["valid"])):
        keep = np.nonzero(inp["valid"][i])[0]
        if per_class:
            cur = []
            for ii in range(NC):
                cur += [(ii, inp["bbox_corner"][i, j], inp["conf"][i, j, ii]) for j in keep]
            out.append(cur)
        else:
            out.append([(inp["sem_cls"][i, j].item(), inp["bbox_corner"][i, j], inp["obj_prob"][i, j]) for j in keep])
    return out


def run_case(name, inp, pred, steps, per_class, out):
    import torch
    from lib.ap_helper import APCalculator, parse_groundtruths
    from utils.eval_det import eval_det_multiprocessing, get_iou_obb

    B = len(inp["valid"])
    calcs = [APCalculator(t, None) for t in THRESHOLDS]
    i0 = 0
    for n in steps:                                             # unequal batches
        ep = {k: torch.from_numpy(inp[k][i0:i0 + n]) for k in ("gt_box_corner_label", "sem_cls_label", "box_label_mask")}
        gts = parse_groundtruths(ep, {})
        for calc in calcs:
            calc.step(pred[i0:i0 + n], gts)
        i0 += n
    assert i0 == B
    # what the device path computes, restated: the generator's own assertions and a parity check
    kw = dict(conf=inp["conf"]) if per_class else dict(obj_prob=inp["obj_prob"], sem_cls=inp["sem_cls"])
    score, flags, index, npos, ovmax = R.match(inp["bbox_corner"], inp["valid"], inp["gt_box_corner_label"],
                                               inp["sem_cls_label"], inp["box_label_mask"], THRESHOLDS, NC, **kw)
    ex = flags >= R.EXISTS
    for c in range(NC):
        s = score[:, c][ex[:, c]]
        assert len(np.unique(s)) == len(s), f"{name}: equal scores in class {c}"
        assert not (npos[c] > 0 and len(s) == 0), f"{name}: class {c} has ground truth and no prediction"
    fin = ovmax[np.isfinite(ovmax)]
    for t in THRESHOLDS:
        assert np.all(np.abs(fin - t) > 1e-9), f"{name}: ovmax next to {t}"
    gt64 = inp["gt_box_corner_label"].astype(np.float64)
    for b in range(B):
        for c in range(NC):
            g = np.nonzero((inp["box_label_mask"][b] == 1) & (inp["sem_cls_label"][b] == c))[0]
            rec = index[b, c][ex[b, c]]
            if len(g) > 1 and len(rec):
                iou = np.sort(R.iou_matrix(inp["bbox_corner"][b, rec].astype(np.float64), gt64[b, g]), 1)
                assert np.all((iou[:, -1] > iou[:, -2]) | (iou[:, -1] == 0)), f"{name}: tied maximum IoU"
    tp = [(flags >> t & 1).astype(bool) for t in range(2)]
    for t in range(2):
        assert (tp[t] & ex).any() and (~tp[t] & ex).any(), f"{name}: no TP or no FP at {THRESHOLDS[t]}"
    assert (tp[0] & ~tp[1] & ex).any(), f"{name}: no prediction that is a TP at 0.25 and an FP at 0.5"
    restated, curves = R.metrics([(score, flags)], npos, NC, 2)

    out.update({f"{name}/{k}": v for k, v in inp.items()})
    out[f"{name}/steps"] = np.array(steps, np.int64)
    out[f"{name}/per_class_proposal"] = np.array(per_class)
    for ti, calc in enumerate(calcs):
        ret = calc.compute_metrics()
        rec, prec, ap = eval_det_multiprocessing(calc.pred_map_cls, calc.gt_map_cls, ovthresh=THRESHOLDS[ti],
                                                 get_iou_func=get_iou_obb)
        out[f"{name}/t{ti}/keys"] = np.array(list(ret.keys()))
        out[f"{name}/t{ti}/values"] = np.array([float(v) for v in ret.values()], np.float64)
        assert list(ret.keys()) == list(restated[ti].keys()), (name, list(ret.keys()), list(restated[ti].keys()))
        for k, v in ret.items():
            assert abs(float(v) - float(restated[ti][k])) <= 1e-12, (name, k, v, restated[ti][k])
        for c in sorted(ap):
            assert ret["%d Average Precision" % c] == ap[c]
            out[f"{name}/t{ti}/rec_{c}"] = np.asarray(rec[c], np.float64)
            out[f"{name}/t{ti}/prec_{c}"] = np.asarray(prec[c], np.float64)
            np.testing.assert_array_equal(rec[c], curves[c, ti][0])
            np.testing.assert_array_equal(prec[c], curves[c, ti][1])
        print(f"{name} @{THRESHOLDS[ti]}: mAP {ret['mAP']:.6f} AR {ret['AR']:.6f}, {len(ap)} classes, "
              f"{int((tp[ti] & ex).sum())} TP / {int(ex.sum())} records, npos {int(npos.sum())}")


def main():
    install_stubs()
    os.chdir(REF)
    sys.path.insert(0, REF)
    out = {}
    inp, pred, steps, per_class = main_case()
    run_case("main", inp, pred, steps, per_class, out)
    small = small_case()
    run_case("small", small, pred_lists(small, True), [2], True, out)
    run_case("small1", small, pred_lists(small, False), [2], False, out)
    path = os.path.join(HERE, "detection_ap_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
