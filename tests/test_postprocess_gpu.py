"""Evaluation post-processing on the MI355X (spacap3d_amd/postprocess.py, csrc/postprocess.hip) against the reference's
recorded outputs (tests/golden/postprocess_ref.npz) and the numpy restatement (tests/postprocess_restated.py)."""
import os

import numpy as np
import pytest
import torch

import postprocess_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "postprocess_ref.npz"))
VARIANTS = {"main": ("main", True, False), "k512": ("k512", True, False), "nocls": ("main", False, False),
            "oldtype": ("main", True, True), "oldnocls": ("main", False, True)}
POST_DICT = {"remove_empty_box": True, "use_3d_nms": True, "nms_iou": 0.25, "use_old_type_nms": False, "cls_nms": True,
             "per_class_proposal": True, "conf_thresh": 0.05}


def _fix(prefix):
    return {k.split("/", 1)[1]: FIX[k] for k in FIX.files if k.startswith(prefix + "/")}


def _dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items()}


def _run(t, **kw):
    from spacap3d_amd.postprocess import detection_postprocess
    out = detection_postprocess(t["point_clouds"], t["bbox_corner"], t["objectness_scores"], t["sem_cls"],
                                t.get("sem_cls_scores"), **kw)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def _check_against_restatement(h, got, **kw):
    ref = R.postprocess(h["point_clouds"], h["bbox_corner"], h["objectness_scores"], h["sem_cls"], h.get("sem_cls_scores"),
                        obj_prob=got["obj_prob"], **kw)
    assert R.ulp_diff(got["obj_prob"], R.objectness_prob(h["objectness_scores"])).max() <= 1
    np.testing.assert_array_equal(got["point_count"], ref["point_count"])
    for k in ("nonempty_mask", "pred_mask", "valid"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    if got["conf"] is not None:
        assert R.ulp_diff(got["conf"], R.class_softmax(h["sem_cls_scores"]) * got["obj_prob"][..., None]).max() <= 1
    return ref


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_fixture_parity(name):
    src, cls_nms, old_type = VARIANTS[name]
    h, ref = _fix(src), _fix(name)
    got = _run(_dev(h), cls_nms=cls_nms, old_type=old_type)
    np.testing.assert_array_equal(got["point_count"], h["point_count"])
    np.testing.assert_array_equal(got["nonempty_mask"], h["point_count"] >= 5)
    np.testing.assert_array_equal(got["pred_mask"], ref["pred_mask"].astype(bool))
    np.testing.assert_array_equal(got["valid"], ref["valid"])
    # numpy's float32 exp is up to 2 ulp off (the kernel's is correctly rounded): see test_postprocess_cpu.py
    assert R.ulp_diff(got["obj_prob"], ref["obj_prob"]).max() <= 4
    assert R.ulp_diff(got["conf"], ref["conf"]).max() <= 16
    _check_against_restatement(h, got, cls_nms=cls_nms, old_type=old_type)


@pytest.mark.parametrize("src", ["main", "k512"])
def test_caption_eval_masks_iou_bit_exact(src):
    from spacap3d_amd.postprocess import caption_eval_masks
    h = _fix(src)
    d = _dev(h)
    B, K = h["sem_cls"].shape
    d["bbox_mask"] = torch.from_numpy(h["objectness_scores"].argmax(-1)).to(DEV)
    d["scene_object_ids"] = torch.arange(100, 100 + h["gt_box_corner_label"].shape[1], device=DEV).repeat(B, 1)
    out = caption_eval_masks(d)
    torch.cuda.synchronize()
    assert out["ious"].dtype == torch.float64 and out["nms_masks"].dtype == torch.int64
    np.testing.assert_array_equal(out["ious"].cpu().numpy(), h["ious"])
    np.testing.assert_array_equal(out["good_bbox_masks"].cpu().numpy(), h["good"])
    want = _fix(src)["pred_mask"].astype(np.int64) * h["objectness_scores"].argmax(-1)
    np.testing.assert_array_equal(out["nms_masks"].cpu().numpy(), want)
    np.testing.assert_array_equal(out["detected_object_ids"].cpu().numpy(), 100 + h["object_assignment"])


def synthetic_scenes(B, N, K, NC=18, seed=0, C=4):
    """Random clouds with clusters of near-duplicate boxes (half of them one class per cluster)."""
    rng = np.random.default_rng(seed)
    pc = np.concatenate([rng.uniform([-4, -4, 0], [4, 4, 3], (B, N, 3)), rng.normal(size=(B, N, C - 3))], 2).astype(np.float32)
    nA = (K + 3) // 4
    anchor = pc[np.arange(B)[:, None], rng.integers(0, N, (B, nA)), :3].astype(np.float64)
    ctr = np.repeat(anchor, 4, 1)[:, :K] + rng.normal(0, 0.05, (B, K, 3))
    size = np.repeat(rng.uniform(0.2, 1.2, (B, nA, 3)), 4, 1)[:, :K] * rng.uniform(0.85, 1.15, (B, K, 3))
    signs = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    corners = ctr[:, :, None] + signs * (size[:, :, None] / 2)
    scores = rng.normal(0, 2, (B, K, NC)).astype(np.float32)
    same = np.repeat(rng.integers(0, NC, (B, nA)), 4, 1)[:, :K]
    scores[np.arange(B)[:, None], np.arange(K)[None], same] += 3.0 * (rng.random((B, K)) < 0.5)
    return {"point_clouds": pc, "bbox_corner": np.ascontiguousarray(corners),
            "objectness_scores": rng.normal(0, 2, (B, K, 2)).astype(np.float32),
            "sem_cls": scores.argmax(-1).astype(np.int64), "sem_cls_scores": scores}


@pytest.mark.parametrize("B,N,K", [(8, 40000, 256), (4, 80000, 512), (1, 5000, 100), (2, 3000, 37)])
def test_matches_restatement_at_model_sizes(B, N, K):
    """cfg2 (8 x 40 000 points, 256 proposals), cfg5 (512 proposals, 80 000 points), B = 1, K not a multiple of 64."""
    h = synthetic_scenes(B, N, K, seed=B + K)
    got = _run(_dev(h))
    ref = _check_against_restatement(h, got)
    assert 0 < ref["pred_mask"].sum() < ref["nonempty_mask"].sum()


def test_scene_with_every_box_empty():
    h = synthetic_scenes(3, 4000, 128, seed=5)
    h["bbox_corner"][1, :, :, 2] += 100.0          # scene 1: every box above the cloud
    got = _run(_dev(h))
    assert not got["nonempty_mask"][1].any() and not got["pred_mask"][1].any() and not got["valid"][1].any()
    assert (got["point_count"][1] == 0).all()
    _check_against_restatement(h, got)
    from spacap3d_amd.postprocess import parse_predictions
    with pytest.raises(AssertionError):
        parse_predictions(_dev(h), dict(POST_DICT, dataset_config=type("DC", (), {"num_class": 18})))


def test_graph_capture_replays_the_same_masks():
    from spacap3d_amd.postprocess import detection_postprocess
    h = synthetic_scenes(8, 40000, 256, seed=11)
    t = _dev(h)
    args = (t["point_clouds"], t["bbox_corner"], t["objectness_scores"], t["sem_cls"], t["sem_cls_scores"])
    eager = _run(t)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        detection_postprocess(*args)               # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = detection_postprocess(*args)
    for k in static:
        if static[k] is not None:
            static[k].zero_()
    g.replay()
    torch.cuda.synchronize()
    for k, v in static.items():
        if v is not None:
            np.testing.assert_array_equal(v.cpu().numpy(), eager[k], err_msg=k)


def test_evaluator_writes_post_tensors():
    from spacap3d_amd.engine import Evaluator, synthetic_batch
    from spacap3d_amd.spacapnet import build_default
    torch.manual_seed(0)
    model = build_default(vocab_size=200, num_proposal=64, N=2, d_ff=256).to(DEV).eval()
    batches = [synthetic_batch(2, 4096, DEV, seed=s, vocab=200) for s in (1, 2)]
    ev = Evaluator(model, postprocess=dict(POST_DICT, dataset_config=None))
    outs = [ev(b, next_data=batches[i + 1] if i + 1 < len(batches) else None) for i, b in enumerate(batches)]
    torch.cuda.synchronize()
    for out in outs:
        keys = {"post_obj_prob", "post_point_count", "post_nonempty_mask", "post_pred_mask", "post_valid", "post_conf"}
        assert keys <= set(out) and all(isinstance(out[k], torch.Tensor) for k in keys)
        h = {k: out[k].detach().cpu().numpy() for k in ("point_clouds", "bbox_corner", "objectness_scores", "sem_cls",
                                                         "sem_cls_scores")}
        got = {k[5:]: out[k].cpu().numpy() for k in keys}
        _check_against_restatement(h, got)
    plain = Evaluator(model)(synthetic_batch(2, 4096, DEV, seed=1, vocab=200))
    assert not any(k.startswith("post_") for k in plain)


def test_parse_predictions_structure_and_types():
    from spacap3d_amd.postprocess import parse_predictions
    h, ref = _fix("main"), _fix("main")
    t = _dev(h)
    B, K = h["sem_cls"].shape
    DC = type("DC", (), {"num_class": 18})
    ep = {k: t[k] for k in ("point_clouds", "bbox_corner", "objectness_scores", "sem_cls", "sem_cls_scores")}
    ep["center"] = torch.zeros(B, K, 3, device=DEV)
    lists = parse_predictions(ep, dict(POST_DICT, dataset_config=DC))
    assert ep["batch_pred_map_cls"] is lists and len(lists) == B
    assert isinstance(ep["pred_mask"], np.ndarray) and ep["pred_mask"].dtype == np.float64 and ep["pred_mask"].shape == (B, K)
    np.testing.assert_array_equal(ep["pred_mask"], ref["pred_mask"].astype(np.float64))
    rows = [(i, c, int(np.nonzero(np.all(h["bbox_corner"][i] == box, axis=(1, 2)))[0][0])) for i, lst in enumerate(lists)
            for c, box, _ in lst]
    np.testing.assert_array_equal(np.array(rows), ref["pred_map_cls"])
    confs = np.array([cf for lst in lists for _, _, cf in lst], np.float32)
    assert R.ulp_diff(confs, ref["pred_map_conf"]).max() <= 16
    c, box, cf = lists[0][0]
    assert type(c) is int and box.shape == (8, 3) and box.dtype == np.float64 and isinstance(cf, np.float32)
    single = parse_predictions(dict(ep), dict(POST_DICT, dataset_config=DC, per_class_proposal=False))
    assert len(single[0]) == int(ref["valid"][0].sum())
    c, box, p = single[0][0]
    assert type(c) is int and box.shape == (8, 3) and isinstance(p, np.float32)
