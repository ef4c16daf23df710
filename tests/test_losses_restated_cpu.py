"""tests/losses_restated.py is right, and its inputs are fit for the device test, checked without a device.  For every row of
its tables:
  * the restatement against spacap3d_amd/loss_helper.py's unfused composition on CPU tensors (``start_detection_losses``,
    ``compute_relation_loss`` and ``compute_cap_loss`` take that path by themselves there): the integer outputs from a float32
    run, equal wherever the minimum is unique, the lowest index where rows are tied; values and gradients from a float64
    autograd run, to 1e-10 of the largest reference entry (two float64 computations of one formula: derived, not measured);
  * (a) no proposal within 1e-6 of an objectness threshold, apart from the two placed exactly on them: about 30 ulp at 0.3 - 0.6,
    room for a device square root one ulp off without hiding a wrong comparison;
  * (b) the row has the positives it claims;
  * (c) the float32 composition, measured against the float64 restatement, stays under every bar of
    tests/test_losses_edges_gpu.py; its share of each bar is printed (``LOSSES-RESTATED ...``, pytest -s).
A row that misses a condition gets another seed or other inputs, never another bar.

In the float64 run only what carries a value is float64.  The aggregated vote positions and the box centres stay float32, so
that the composition takes its decisions on float32 distances as it does in training; the 0/1 flags stay float32 as well, as
the composition itself casts them (``.float()``).  The objectness weights are the float32 constants, held in float64."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import losses_restated as R
from spacap3d_amd import loss_helper as LH

ACC_ULP = 2.0 ** -23      # an accuracy is one float32 division of two exact counts in the composition
_name = lambda c: c.name if hasattr(c, "name") else "-".join(map(str, c))


def _det_run(x, dtype, monkeypatch):
    """loss_helper's composition on the inputs x: (losses (8,), label, mask, assignment, d net, d center, d vote_xyz)"""
    val = lambda a: torch.tensor(a).to(dtype)
    raw = lambda a: torch.tensor(a)
    NH, NS = x.NH, x.NS
    B, K, _ = x.net.shape
    net, cen, vote = (val(a).requires_grad_(True) for a in (x.net, x.center, x.vote_xyz))
    o_hr, o_ss = 5 + NH, 5 + 2 * NH
    o_sr, o_sem = o_ss + NS, o_ss + 4 * NS
    d = {"seed_xyz": val(x.seed_xyz), "vote_xyz": vote, "seed_inds": raw(x.seed_inds), "vote_label": val(x.vote_label),
         "vote_label_mask": raw(x.vote_mask), "aggregated_vote_xyz": raw(x.agg_xyz), "center_label": raw(x.gt_center),
         "box_label_mask": raw(x.box_mask), "center": cen, "objectness_scores": net[..., 0:2],
         "heading_scores": net[..., 5:o_hr], "heading_residuals_normalized": net[..., o_hr:o_ss],
         "size_scores": net[..., o_ss:o_sr], "size_residuals_normalized": net[..., o_sr:o_sem].reshape(B, K, NS, 3),
         "sem_cls_scores": net[..., o_sem:], "heading_class_label": raw(x.heading_cls_label),
         "heading_residual_label": val(x.heading_res_label), "size_class_label": raw(x.size_cls_label),
         "size_residual_label": val(x.size_res_label), "sem_cls_label": raw(x.sem_cls_label)}
    monkeypatch.setitem(LH._CONST, ("objectness_w", "cpu"), torch.tensor(R.OBJ_W, dtype=torch.float32).to(dtype))
    LH.start_detection_losses(d, NH, NS, x.mean_size)
    t = d["_detection_losses"]
    losses = torch.stack([t[0], t[1], t[5], t[6], t[7], t[8], t[9], t[10]])
    assert losses.dtype == dtype
    (losses * torch.tensor(R.DET_UPSTREAM, dtype=dtype)).sum().backward()
    grads = [g.grad if g.grad is not None else torch.zeros_like(g) for g in (net, cen, vote)]
    return [losses.detach().numpy(), t[2].numpy(), t[3].numpy(), t[4].numpy()] + [g.numpy() for g in grads]


@pytest.mark.parametrize("case", R.DET_CASES, ids=_name)
def test_detection_restatement_and_the_conditions_of_its_row(case, monkeypatch):
    x, want = R.detection_inputs(case), R.detection_reference(case)
    B, K, M = case.B, case.K, case.M
    assert x.net.shape == (B, K, 5 + 2 * case.NH + 4 * case.NS + case.NC) and x.gt_center.shape == (B, M, 3)
    assert x.seed_xyz.shape == (B, case.NSEED, 3) and x.vote_label.shape == (B, case.N, 9)
    # (a) the thresholds
    hits = R.threshold_hits(want.eu, x.near, x.far, 1e-6)
    assert hits == (2 if case.kind == "exact-thresholds" else 0)
    # (b) the positives
    pos, masked = int(want.obj_label.sum()), int(want.obj_mask.sum())
    if case.positives == "some":
        assert 0 < pos < B * K and pos < masked
    elif case.positives == "none":
        assert pos == 0 and masked > 0
    else:
        assert pos == 0 and masked == 0
    assert np.isfinite(want.losses).all()
    # float32 composition: the integer outputs
    l32, lab, msk, oa, gn32, gc32, gv32 = _det_run(x, torch.float32, monkeypatch)
    assert np.array_equal(lab, want.obj_label) and np.array_equal(msk, want.obj_mask) and msk.dtype == want.obj_mask.dtype
    unique = ~R.tied(want.d_agg, 2)
    assert np.array_equal(oa[unique], want.assignment[unique])
    lowest = (want.d_agg == want.d_agg.min(2, keepdims=True)).argmax(2)
    assert np.array_equal(want.assignment, lowest)
    # float64 composition: values and gradients
    l64, lab64, msk64, oa64, gn64, gc64, gv64 = _det_run(x, torch.float64, monkeypatch)
    assert np.array_equal(lab64, lab) and np.array_equal(msk64, msk) and np.array_equal(oa64, oa)
    f64 = {"losses": R.figure(l64, want.losses), "dnet": R.figure(gn64, want.dnet), "dcenter": R.figure(gc64, want.dcenter),
           "dvote": R.figure(gv64, want.dvote)}
    # (c) float32 done right inside the device bars
    f32 = {"losses": R.excess(l32, want.losses, R.DET_LOSS_RTOL, R.DET_LOSS_ATOL), "dnet": R.figure(gn32, want.dnet),
           "dcenter": R.figure(gc32, want.dcenter), "dvote": R.figure(gv32, want.dvote)}
    print(f"LOSSES-RESTATED det {case.name} staged={int(R.staged(K, M, case.NH, case.NS, case.NC))} hits={hits} pos={pos}/{B * K} "
          f"masked={masked} f64: " + " ".join(f"{k}={v:.2e}" for k, v in f64.items())
          + " | f32 losses (of the bar)=%.3f" % f32["losses"] + " ".join(f" {k}={f32[k]:.2e}" for k in ("dnet", "dcenter", "dvote")))
    assert all(v < R.F64_BAR for v in f64.values()), f64
    assert f32["losses"] <= 1.0 and all(f32[k] < R.DET_GRAD_BAR for k in ("dnet", "dcenter", "dvote")), f32
    # what the row is there for
    if case.kind == "scene0-no-valid-box":
        assert x.box_mask[0].sum() == 0 and x.box_mask[1].sum() > 0 and (want.assignment[0] == 0).all()
    if case.kind == "none-near":          # (the centre loss keeps its box -> proposal term)
        assert (want.losses[3:8] == 0.0).all() and (want.dnet[..., 5:] == 0.0).all() and want.losses[2] > 0 and want.losses[1] > 0
    if case.kind == "all-grey":
        assert want.losses[1] == 0.0 and (want.dnet[..., 0:2] == 0.0).all()
    if case.kind == "dup-boxes":
        assert (x.gt_center[:, 5] == x.gt_center[:, 2]).all() and (x.sem_cls_label[:, 5] != x.sem_cls_label[:, 2]).all()
        assert (want.assignment[:, :8] == 2).all() and not (want.assignment == 5).any() and (want.obj_label[:, :8] == 1).all()
    if case.kind == "dup-proposals":
        assert (x.center[:, 4] == x.center[:, 9]).all() and (want.i2[:, 1] == 4).all() and (x.box_mask[:, 1] == 1).all()
        assert R.tied(want.d_center, 1)[:, 1].all()
    if case.kind == "exact-thresholds":
        assert want.eu[0, 0] == np.float32(x.near) and want.eu[0, 1] == np.float32(x.far)
        assert (want.obj_label[0, :2] == 0).all() and (want.obj_mask[0, :2] == 0).all() and (want.assignment[0, :2] == 0).all()
    if case.kind == "same-votes":
        assert (want.pick == 0).all()
    if case.kind == "scene1-no-vote-mask":
        assert (want.dvote[1] == 0.0).all() and np.abs(want.dvote[0]).max() > 0


def test_detection_table_sits_on_the_dispatch_edges():
    """The rows are where the host code of spacap_det_losses_fwd_f32 / _bwd_f32 forks."""
    by = R.DET_BY_NAME
    st = lambda c: R.staged(c.K, c.M, c.NH, c.NS, c.NC)
    # 4 * (12 M + 6 K + 3 NS + 4) + 4 K CH <= 150 * 1024 at M = 128, NS = 18, CH = 97: 6 376 + 412 K <= 153 600
    assert R.K_EDGE == 357 == (150 * 1024 - 6376) // 412
    assert by["K-last-staged"].K == 357 and st(by["K-last-staged"]) and by["K-first-unstaged"].K == 358 and not st(by["K-first-unstaged"])
    assert not st(by["K512"]) and not st(by["K41-NC1000"]) and st(by["K41"]) and st(by["K257"])
    odd = by["K41-NC1000"]
    assert (odd.K * (5 + 2 * odd.NH + 4 * odd.NS + odd.NC)) % 2 == 1 and (by["K41"].K * 97) % 4 == 1
    assert all(R.lds_bytes(c.K, c.M, c.NS) <= 60000 for c in R.DET_CASES) and R.lds_bytes(2400, 128, 18) > 60000
    assert by["M129"].M == 1024 // 8 + 1 and by["M256"].M == 256 and by["K257"].K == 1024 // 4 + 1
    big = by["B12-K512"]
    assert big.B * big.K * (97 + 3) + big.B * big.NSEED * 3 > 2048 * 256      # det_scale_kernel strides
    assert all(R.n_valid(c, b) > 128 for c in (by["M129"], by["M256"]) for b in (0,)) and len(set(R.DET_UPSTREAM)) == 8
    assert len({c.name for c in R.DET_CASES}) == len(R.DET_CASES)


def test_exact_offsets_land_on_the_thresholds():
    for thr, known in ((R.NEAR, 0.29999834299087524), (R.FAR, 0.599999189376831)):
        for x in (R.exact_offset(thr), np.float32(known)):
            assert R.euclid32(np.float32(x) * np.float32(x)) == np.float32(thr)
            assert not (R.euclid32(np.float32(x) * np.float32(x)) < np.float32(thr))
    eu = np.asarray([0.3, 0.3 + 2e-6, 0.6 - 5e-7, 0.45], np.float32)
    assert R.threshold_hits(eu, 0.3, 0.6, 1e-6) == 2


# ---- relation loss -----------------------------------------------------------------------------------------------------------
def _rel_run(x, dtype):
    pred = torch.tensor(x.pred).to(dtype).requires_grad_(True)
    d = {"relation_pred": pred, "object_assignment": torch.tensor(x.assignment), "box_label_mask_int": torch.tensor(x.box_mask_int),
         "objectness_label": torch.tensor(x.obj_label), "x_label": torch.tensor(x.x_label), "y_label": torch.tensor(x.y_label),
         "z_label": torch.tensor(x.z_label)}
    r = LH.compute_relation_loss(d)
    sum(r[f"{a}_loss"] * g for a, g in zip("xyz", R.REL_UPSTREAM)).backward()
    out = np.asarray([float(r[k].detach()) for k in ("x_loss", "y_loss", "z_loss", "x_acc", "y_acc", "z_acc")])
    return out, pred.grad.numpy()


@pytest.mark.parametrize("case", R.REL_CASES, ids=_name)
def test_relation_restatement_and_the_conditions_of_its_row(case):
    x, want = R.relation_inputs(case), R.relation_reference(case)
    B, K = case.B, case.K
    if case.select == "all":
        assert want.n_pairs == B * K * K
    elif case.select == "none":
        assert want.n_pairs == 0 and (want.out[:6] == 0.0).all() and want.out[6] == 1.0 and (want.dpred == 0.0).all()
    else:
        assert 4 * B <= want.n_pairs < B * K * K
    assert want.out[6] == 1.0 / max(want.n_pairs, 1)
    o64, g64 = _rel_run(x, torch.float64)
    o32, g32 = _rel_run(x, torch.float32)
    f64 = max(R.figure(o64[:3], want.out[:3]), R.figure(g64, want.dpred))
    assert R.figure(o64[3:], want.out[3:6]) <= ACC_ULP      # the composition counts hits in float32 whatever the scores' type
    f32 = (R.excess(o32, want.out[:6], R.REL_LOSS_RTOL, R.REL_LOSS_ATOL), R.excess(g32, want.dpred, R.REL_GRAD_RTOL, R.REL_GRAD_ATOL))
    print(f"LOSSES-RESTATED rel {case.name} pairs={want.n_pairs} f64={f64:.2e} | f32 (of the bar) out={f32[0]:.3f} dpred={f32[1]:.3f}")
    assert f64 < R.F64_BAR
    assert f32[0] <= 1.0 and f32[1] <= 1.0
    # the planted ties are selected pairs, and hits only by the first maximum
    if case.select != "none":
        for b in range(B):
            for (vals, first), (i, j) in zip(R._REL_TIES, ((0, 0), (0, 1), (1, 0), (1, 1))):
                assert tuple(x.pred[b, i, j, 0:3]) == vals and x.x_label[b, x.assignment[b, i], x.assignment[b, j]] == first
                assert x.obj_label[b, i] == x.obj_label[b, j] == 1 and int(np.argmax(vals)) == first
    assert (K * K) % 256 != 0 or case.name == "2-256-64"


def test_relation_table_reaches_the_grid_cap():
    c = {c.name: c for c in R.REL_CASES}["2-256-64"]
    assert (c.B * c.K * c.K * 9 + 255) // 256 > 4096
    assert all((o.B * o.K * o.K * 9 + 255) // 256 <= 4096 for o in R.REL_CASES if o is not c)


# ---- caption head --------------------------------------------------------------------------------------------------------------
def _cap_run(x, want, dtype):
    logits = torch.tensor(x.logits).to(dtype).requires_grad_(True)
    W = x.logits.shape[1]
    ids = torch.tensor(x.lang_ids).clone()
    ids[:, 1:W + 1] = torch.tensor(want.target)      # F.cross_entropy refuses an id >= V; the kernel ignores it like the pad id
    lang_cap = F.log_softmax(logits, dim=-1)
    loss, acc = LH.compute_cap_loss({"lang_cap": lang_cap, "lang_ids": ids, "good_bbox_masks": torch.tensor(x.good)})
    (loss * R.CAP_UPSTREAM).backward()
    return lang_cap.detach().numpy(), float(loss.detach()), float(acc.detach()), logits.grad.numpy()


def cap_figures(logp, loss, acc, grad, want):
    """each as its share of its bar (at most 1 inside)"""
    scale = max(float(np.abs(want.dlogits).max()), 1e-6)
    return {"logp": float(np.abs(logp - want.logp).max()) / R.CAP_LOGP_ABS,
            "loss": abs(loss - want.loss) / (R.CAP_LOSS_REL * max(1.0, abs(want.loss))),
            "acc": abs(acc - want.acc) / R.CAP_ACC_ABS,
            "dlogits": float(np.abs(grad - want.dlogits).max()) / (R.CAP_GRAD_REL * scale + R.CAP_GRAD_ABS)}


@pytest.mark.parametrize("case", R.CAP_CASES, ids=_name)
def test_caption_restatement_and_the_conditions_of_its_row(case):
    x, want = R.caption_inputs(case), R.caption_reference(case)
    B, W, V = case.B, case.W, case.V
    assert x.lang_ids.shape[1] >= W + 1 and (case.V != 1000 or x.lang_ids.shape[1] > W + 1)
    raw = x.lang_ids[:, 1:W + 1]
    assert (raw == V).sum() == 1 and (raw == R.CAP_FAR_ID).sum() == 1 and (want.target < V).all()
    assert (want.target[(raw >= V)] == 0).all()
    assert want.n_valid == (0 if case.good == "none" else want.n_valid) and (want.n_valid > 0) == (case.good != "none")
    # the planted rows: equal maxima, and the target decides between a hit and a miss
    assert x.logits[0, 0].argmax() == want.target[0, 0]
    for w, (lo, hi), t in R.cap_ties(V):
        row = x.logits[0, w]
        assert row[lo] == row[hi] == row.max() and (row == row.max()).sum() == 2 and want.target[0, w] == t and lo < hi
    assert len(R.cap_ties(V)) >= 1
    a64 = _cap_run(x, want, torch.float64)
    a32 = _cap_run(x, want, torch.float32)
    f64 = max(R.figure(a64[0], want.logp), abs(a64[1] - want.loss) / max(abs(want.loss), 1e-300) if want.loss else abs(a64[1]),
              R.figure(a64[3], want.dlogits))
    assert abs(a64[2] - want.acc) <= ACC_ULP * want.acc     # (hits counted in float32 there, whatever the logits' type)
    f32 = cap_figures(*a32, want)
    print(f"LOSSES-RESTATED cap {_name(case)} valid={want.n_valid} f64={f64:.2e} | f32 (of the bar) "
          + " ".join(f"{k}={v:.3f}" for k, v in f32.items()))
    assert f64 < R.F64_BAR
    assert all(v <= 1.0 for v in f32.values()), f32
    if case.good == "none":
        assert want.loss == 0.0 and want.acc == 0.0 and (want.dlogits == 0.0).all()


def test_the_measures_treat_zero_exactly():
    z = np.zeros(3)
    assert R.figure(z, z) == 0.0 and R.figure(z + 1e-30, z) == math.inf and R.figure(-z, z) == 0.0
    assert R.excess([1.0 + 3e-5], [1.0], 2e-5, 1e-6) > 1.0 > R.excess([1.0 + 1e-5], [1.0], 2e-5, 1e-6)
    assert R.zero_where_reference_is([0.0, -0.0, 3.0], [0.0, 0.0, 1.0]) and not R.zero_where_reference_is([1e-30, 1.0], [0.0, 1.0])
