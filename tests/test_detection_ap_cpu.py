"""No-GPU checks of the detection mAP / AR (spacap3d_amd/detection_ap.py): the numpy restatement
(tests/detection_ap_restated.py) reproduces the reference's recorded results (tests/golden/detection_ap_ref.npz, made by
tests/golden/make_fixtures_ap.py from lib/ap_helper.py APCalculator), the C entry points reject bad arguments without
touching a device, the Python layer refuses CPU tensors, and the new symbols are declared and exported."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import detection_ap_restated as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "detection_ap_ref.npz"))
CASES = ("main", "small", "small1")
THRESHOLDS = (0.25, 0.5)
NC = 18
INPUTS = ("bbox_corner", "valid", "conf", "obj_prob", "sem_cls", "gt_box_corner_label", "sem_cls_label", "box_label_mask")


def case(name):
    d = {k: FIX[f"{name}/{k}"] for k in INPUTS}
    return d, [int(n) for n in FIX[f"{name}/steps"]], bool(FIX[f"{name}/per_class_proposal"])


def reference(name, t):
    """The reference's result dict at threshold index t and its per-class (rec, prec)."""
    ret = dict(zip((str(k) for k in FIX[f"{name}/t{t}/keys"]), FIX[f"{name}/t{t}/values"]))
    curves = {int(k.rsplit("_", 1)[1]): (FIX[k], FIX[k.replace("/rec_", "/prec_")]) for k in FIX.files
              if k.startswith(f"{name}/t{t}/rec_")}
    return ret, curves


def restated_run(name, thresholds=THRESHOLDS):
    d, steps, per_class = case(name)
    slabs, npos, i0 = [], np.zeros(NC, np.int64), 0
    for n in steps:
        s = slice(i0, i0 + n)
        kw = dict(conf=d["conf"][s]) if per_class else dict(obj_prob=d["obj_prob"][s], sem_cls=d["sem_cls"][s])
        score, flags, index, np_b, _ = R.match(d["bbox_corner"][s], d["valid"][s], d["gt_box_corner_label"][s],
                                               d["sem_cls_label"][s], d["box_label_mask"][s], thresholds, NC, **kw)
        slabs.append((score, flags, index))
        npos += np_b
        i0 += n
    return slabs, npos


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    slabs, npos = restated_run(name)
    got, curves = R.metrics(slabs, npos, NC, 2)
    for t in range(2):
        ref, ref_curves = reference(name, t)
        assert list(got[t].keys()) == list(ref.keys())
        for k, v in ref.items():
            assert abs(float(got[t][k]) - v) <= 1e-10, (k, got[t][k], v)
        assert ref_curves
        for c, (rec, prec) in ref_curves.items():
            np.testing.assert_array_equal(curves[c, t][0], rec)
            np.testing.assert_array_equal(curves[c, t][1], prec)


def test_fixture_holds_the_cases_it_is_for():
    for name in CASES:
        slabs, _ = restated_run(name)
        flags = np.concatenate([s[1].reshape(-1) for s in slabs])
        ex = flags >= R.EXISTS
        tp25, tp50 = (flags & 1).astype(bool), (flags & 2).astype(bool)
        assert (tp25 & ex).any() and (~tp25 & ex).any() and (tp50 & ex).any() and (~tp50 & ex).any()
        assert (tp25 & ~tp50).any()
    d, steps, _ = case("main")
    assert steps == [2, 1] and d["valid"].shape == (3, 256)
    d, _, _ = case("small")
    assert d["valid"].shape == (2, 64) and d["box_label_mask"].shape == (2, 128) and not d["valid"][1].any()
    assert set(np.unique(d["box_label_mask"])) == {0.0, 1.0, 2.0}


def test_entry_points_reject_bad_arguments_without_a_device():
    from spacap3d_amd._native import lib
    thr = (ctypes.c_double * 4)(0.25, 0.5, 0.6, 0.7)
    m = lambda B=1, K=64, NC=18, M=16, T=2, th=thr: lib.spacap_detection_match_f32(
        None, None, None, None, None, B, K, NC, None, None, None, M, th, T, None, None, None, None, None)
    for bad in (dict(K=0), dict(K=513), dict(M=0), dict(M=257), dict(NC=0), dict(NC=129), dict(T=0), dict(T=5), dict(B=-1)):
        assert m(**bad) == -1, bad
        assert b"bad sizes" in lib.spacap_last_error()
    assert m(th=None) == -1 and b"null" in lib.spacap_last_error()
    assert m() == -1 and b"null" in lib.spacap_last_error()          # sizes fine, pointers missing
    assert m(B=0) == 0                                                # empty batch: no-op
    c = lambda L=100, NC=18, T=2: lib.spacap_ap_curve_f64(None, L, None, None, NC, T, None, None, None, None, None)
    for bad in (dict(L=0), dict(NC=0), dict(NC=129), dict(T=0), dict(T=5)):
        assert c(**bad) == -1, bad
        assert b"bad sizes" in lib.spacap_last_error()
    assert c() == -1 and b"null" in lib.spacap_last_error()


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    from spacap3d_amd.detection_ap import DetectionAP
    d, _, _ = case("small")
    t = {k: torch.from_numpy(v) for k, v in d.items()}
    for per_class in (True, False):
        with pytest.raises(RuntimeError, match="CPU not supported"):
            DetectionAP(NC, per_class_proposal=per_class).step(t, t)
    with pytest.raises(RuntimeError, match="thresholds"):
        DetectionAP(NC, iou_thresholds=(0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(RuntimeError, match="num_class"):
        DetectionAP(129)
    with pytest.raises(RuntimeError, match="before any step"):
        DetectionAP(NC).compute_metrics()
    from spacap3d_amd.engine import Evaluator
    with pytest.raises(ValueError):
        Evaluator(None, detection_ap=DetectionAP(NC))


def test_parse_groundtruths_lists():
    from spacap3d_amd.detection_ap import parse_groundtruths
    d, _, _ = case("small")
    ep = {k: torch.from_numpy(d[k]) for k in ("gt_box_corner_label", "sem_cls_label", "box_label_mask")}
    out = parse_groundtruths(ep, {})
    assert ep["batch_gt_map_cls"] is out and len(out) == 2
    for i, lst in enumerate(out):
        live = np.nonzero(d["box_label_mask"][i] == 1)[0]
        assert [c for c, _ in lst] == [int(d["sem_cls_label"][i, j]) for j in live]
        assert all(type(c) is int and box.dtype == np.float32 and box.shape == (8, 3) for c, box in lst)
        np.testing.assert_array_equal(np.stack([box for _, box in lst]), d["gt_box_corner_label"][i, live])


def test_symbols_are_declared_and_exported():
    from spacap3d_amd import _native
    header = open(os.path.join(os.path.dirname(HERE), "include", "spacap_hip.h")).read()
    for name in ("spacap_detection_match_f32", "spacap_ap_curve_f64"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _native.SIGNATURES and hasattr(_native.lib, name)
    assert "#define SPACAP_AP_EXISTS 0x80" in header
    from spacap3d_amd import detection_ap
    assert detection_ap.EXISTS == 0x80 == R.EXISTS
