"""No-GPU checks of the evaluation post-processing (spacap3d_amd/postprocess.py): the numpy restatement of its three
algorithms (tests/postprocess_restated.py) reproduces the reference's recorded outputs (tests/golden/postprocess_ref.npz,
made by tests/golden/make_fixtures_postprocess.py from lib/ap_helper.py parse_predictions, the scipy hull test and
box3d_iou_batch_tensor), the new C entry points reject bad arguments without touching a device, and the Python layer
refuses what it does not implement."""
import os

import numpy as np
import pytest
import torch

import postprocess_restated as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "postprocess_ref.npz"))
VARIANTS = {"main": ("main", True, False), "k512": ("k512", True, False), "nocls": ("main", False, False),
            "oldtype": ("main", True, True), "oldnocls": ("main", False, True)}


def _inputs(src):
    return {k.split("/", 1)[1]: FIX[k] for k in FIX.files if k.startswith(src + "/")}


@pytest.mark.parametrize("src", ["main", "k512"])
def test_closed_box_count_is_the_hull_count(src):
    d = _inputs(src)
    got = np.stack([R.closed_box_counts(d["point_clouds"][b, :, :3], d["bbox_corner"][b]) for b in range(len(d["sem_cls"]))])
    np.testing.assert_array_equal(got, d["point_count"])
    assert (got == 4).any() and (got == 5).any() and (got == 0).any()


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_restated_nms_reproduces_parse_predictions(name):
    src, cls_nms, old_type = VARIANTS[name]
    d, ref = _inputs(src), _inputs(name)
    out = R.postprocess(d["point_clouds"], d["bbox_corner"], d["objectness_scores"], d["sem_cls"], d["sem_cls_scores"],
                        cls_nms=cls_nms, old_type=old_type, obj_prob=ref["obj_prob"])
    np.testing.assert_array_equal(out["pred_mask"], ref["pred_mask"].astype(bool))
    np.testing.assert_array_equal(out["valid"], ref["valid"])
    assert 0 < out["pred_mask"].sum() < out["nonempty_mask"].sum()     # suppression happened


@pytest.mark.parametrize("src", ["main", "k512"])
def test_restated_iou_is_bit_exact(src):
    d = _inputs(src)
    got = np.stack([R.assigned_iou(d["gt_box_corner_label"][b], d["object_assignment"][b], d["bbox_corner"][b])
                    for b in range(len(d["sem_cls"]))])
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, d["ious"])
    assert (got > 0.5).any() and (got <= 0.5).any()


def test_restated_softmaxes_within_numpy_exp_error():
    """The restatement (and the kernel) use a correctly rounded exp; numpy's float32 exp is off by up to 2 ulp, which
    bounds the agreement: obj_prob within 4 ulp, conf within 16 ulp."""
    for src in ("main", "k512"):
        d = _inputs(src)
        p = R.objectness_prob(d["objectness_scores"])
        assert R.ulp_diff(p, d["obj_prob"]).max() <= 4
        c = R.class_softmax(d["sem_cls_scores"]) * p[..., None]
        assert R.ulp_diff(c, d["conf"]).max() <= 16


def test_entry_points_reject_bad_arguments_without_a_device():
    from spacap3d_amd._native import lib
    assert lib.spacap_points_in_box_workspace_bytes(8, 40000, 256) == 8 * 40 * 256 * 4
    assert lib.spacap_points_in_box_f32(None, 1, 0, 3, None, 4, None, 0, None) == -1            # N < 1
    assert b"bad sizes" in lib.spacap_last_error()
    assert lib.spacap_points_in_box_f32(None, 1, 100, 3, None, 513, None, 0, None) == -1        # K > 512
    assert lib.spacap_points_in_box_f32(None, 2, 100, 3, None, 64, None, 0, None) == -1         # null pointers
    assert b"null" in lib.spacap_last_error()
    assert lib.spacap_points_in_box_f32(None, 0, 100, 3, None, 64, None, 0, None) == 0          # empty batch: no-op
    args = lambda B, N, K, NC=0: (None, None, None, NC, None, None, B, N, K, None, 0, None, 3, 5, 0.25, 0.05, 0.5) + (None,) * 9
    assert lib.spacap_detection_nms_f32(*args(1, 100, 513)) == -1
    assert b"K <= 512" in lib.spacap_last_error()
    assert lib.spacap_detection_nms_f32(*args(1, 0, 64)) == -1
    assert lib.spacap_detection_nms_f32(*args(2, 100, 64)) == -1
    assert b"null" in lib.spacap_last_error()
    assert lib.spacap_detection_nms_f32(*args(0, 100, 64)) == 0


def test_python_layer_refuses_cpu_tensors_and_2d_nms():
    from spacap3d_amd import postprocess as P
    d = _inputs("main")
    t = {k: torch.from_numpy(v) for k, v in d.items()}
    with pytest.raises(RuntimeError, match="CPU not supported"):
        P.detection_postprocess(t["point_clouds"], t["bbox_corner"], t["objectness_scores"], t["sem_cls"])
    ep = {"point_clouds": t["point_clouds"], "bbox_corner": t["bbox_corner"], "objectness_scores": t["objectness_scores"],
          "sem_cls": t["sem_cls"], "sem_cls_scores": t["sem_cls_scores"]}
    with pytest.raises(NotImplementedError):
        P.parse_predictions(ep, {"use_3d_nms": False, "remove_empty_box": True, "nms_iou": 0.25})
