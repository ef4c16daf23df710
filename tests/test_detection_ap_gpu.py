"""Detection mAP / AR on the MI355X (spacap3d_amd/detection_ap.py, csrc/detection_ap.hip) against the reference's recorded
results (tests/golden/detection_ap_ref.npz) and the numpy restatement (tests/detection_ap_restated.py).

Exactness: flags, order and scores are compared exactly; rec / prec bit for bit (one IEEE division of exact integers each);
the areas within 1e-10 absolute -- a sum of at most ~1e5 non-negative f64 terms totalling <= 1 differs between summation
orders by at most n * eps ~ 1e-11."""
import numpy as np
import pytest
import torch

import detection_ap_restated as R
from test_detection_ap_cpu import NC, THRESHOLDS, case, reference, restated_run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AP_TOL = 1e-10
LABELS = ("gt_box_corner_label", "sem_cls_label", "box_label_mask")


def _dev(d, s=slice(None)):
    return {k: torch.from_numpy(np.ascontiguousarray(v[s])).to(DEV) for k, v in d.items()}


def _run(d, steps, per_class, nc=NC, thresholds=THRESHOLDS, ap=None):
    from spacap3d_amd.detection_ap import DetectionAP
    ap = ap or DetectionAP(nc, iou_thresholds=thresholds, per_class_proposal=per_class)
    i0 = 0
    for n in steps:
        t = _dev(d, slice(i0, i0 + n))
        ap.step(t, t)
        i0 += n
    return ap


def _restated(d, steps, per_class, nc, thresholds):
    slabs, npos, i0 = [], np.zeros(nc, np.int64), 0
    for n in steps:
        s = slice(i0, i0 + n)
        kw = dict(conf=d["conf"][s]) if per_class else dict(obj_prob=d["obj_prob"][s], sem_cls=d["sem_cls"][s])
        out = R.match(d["bbox_corner"][s], d["valid"][s], d["gt_box_corner_label"][s], d["sem_cls_label"][s],
                      d["box_label_mask"][s], thresholds, nc, **kw)
        slabs.append(out[:3])
        npos += out[3]
        i0 += n
    return slabs, npos


def _check(ap, slabs, npos, nc, T):
    """Slabs, global order, curves and result dicts of a DetectionAP against the restatement; returns the dicts."""
    assert len(ap.slabs) == len(slabs)
    for got, want in zip(ap.slabs, slabs):
        for g, w, what in zip(got, want, ("score", "flags", "index")):
            np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=what)
    np.testing.assert_array_equal(ap.npos.cpu().numpy(), npos)
    r = {k: v.cpu().numpy() for k, v in ap.curves().items()}
    score, flags, count = R.sort_run(slabs, nc)
    np.testing.assert_array_equal(r["count"], count)
    np.testing.assert_array_equal(r["flags"], flags)
    np.testing.assert_array_equal(r["score"], score)
    want, curves = R.metrics(slabs, npos, nc, T)
    for (c, t), (rec, prec) in curves.items():
        n = count[c]
        assert r["rec"][c, t, :n].tobytes() == rec.tobytes(), (c, t)
        assert r["prec"][c, t, :n].tobytes() == prec.tobytes(), (c, t)
        assert r["last_rec"][c, t] == rec[-1]
    got = ap.compute_metrics()
    assert len(got) == T
    for t in range(T):
        assert list(got[t].keys()) == list(want[t].keys())
        for k, v in want[t].items():
            print(f"threshold {t} {k}: {got[t][k]!r} vs {float(v)!r}")
            assert abs(got[t][k] - float(v)) <= AP_TOL, (t, k, got[t][k], v)
    return got, r, count


@pytest.mark.parametrize("name", ["main", "small", "small1"])
def test_fixture_parity(name):
    d, steps, per_class = case(name)
    ap = _run(d, steps, per_class)
    slabs, npos = restated_run(name)
    got, r, count = _check(ap, slabs, npos, NC, 2)
    for t in range(2):
        ref, ref_curves = reference(name, t)
        assert list(got[t].keys()) == list(ref.keys())
        for k, v in ref.items():
            assert abs(got[t][k] - v) <= AP_TOL, (t, k, got[t][k], v)
        for c, (rec, prec) in ref_curves.items():
            assert count[c] == len(rec)
            assert r["rec"][c, t, :len(rec)].tobytes() == rec.tobytes(), (c, t)
            assert r["prec"][c, t, :len(rec)].tobytes() == prec.tobytes(), (c, t)


def synthetic(B, K, M, nc, seed, quant=None, one_class=False, live=0.7):
    """Ground-truth boxes with random classes and mask, proposals jittered around them; ``quant``: scores rounded to
    multiples of 1 / quant (many equal scores: the tie rules decide the order)."""
    rng = np.random.default_rng(seed)
    signs = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    gc, gs = rng.uniform(-3, 3, (B, M, 3)), rng.uniform(0.3, 1.0, (B, M, 3))
    gt = (gc[:, :, None] + signs * gs[:, :, None] / 2).astype(np.float32)
    gt_cls = np.zeros((B, M), np.int64) if one_class else rng.integers(0, nc, (B, M))
    mask = (rng.random((B, M)) < live).astype(np.float32)
    pick = rng.integers(0, M, (B, K))
    jit = rng.uniform(0.0, 0.4, (B, K, 1))
    bi = np.arange(B)[:, None]
    pc = gc[bi, pick] + rng.uniform(-1, 1, (B, K, 3)) * jit * gs[bi, pick]
    ps = gs[bi, pick] * (1 + rng.uniform(-1, 1, (B, K, 3)) * jit)
    sem = np.where(rng.random((B, K)) < 0.7, gt_cls[bi, pick], rng.integers(0, nc, (B, K))).astype(np.int64)
    conf, obj = rng.random((B, K, nc), np.float32), rng.random((B, K), np.float32)
    if quant:
        conf, obj = np.round(conf * quant) / quant, np.round(obj * quant) / quant
    return {"bbox_corner": pc[:, :, None] + signs * ps[:, :, None] / 2, "valid": rng.random((B, K)) < 0.85,
            "conf": conf.astype(np.float32), "obj_prob": obj.astype(np.float32), "sem_cls": sem,
            "gt_box_corner_label": gt, "sem_cls_label": gt_cls, "box_label_mask": mask}


SHAPES = {   # B, K, M, NC, thresholds, per_class, steps, generator options
    "k512_m256": (1, 512, 256, 18, (0.25, 0.5), True, [1], {}),
    "k512_m256_one_class_all_live": (2, 512, 256, 2, (0.25, 0.5), True, [2], dict(one_class=True, live=1.1)),
    "k1_m1": (3, 1, 1, 2, (0.25, 0.5), True, [2, 1], dict(live=1.1)),
    "t1": (2, 100, 37, 18, (0.3,), True, [1, 1], {}),
    "t4_ties": (4, 70, 20, 5, (0.1, 0.25, 0.5, 0.75), True, [1, 2, 1], dict(quant=16)),
    "single_class_ties": (4, 200, 64, 18, (0.25, 0.5), False, [3, 1], dict(quant=32)),
    "nc128": (1, 33, 256, 128, (0.25, 0.5), False, [1], {}),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_matches_restatement(name):
    B, K, M, nc, thr, per_class, steps, opt = SHAPES[name]
    d = synthetic(B, K, M, nc, seed=len(name) + K, **opt)
    ap = _run(d, steps, per_class, nc, thr)
    slabs, npos = _restated(d, steps, per_class, nc, thr)
    flags = np.concatenate([s[1].reshape(-1) for s in slabs])
    if K > 1:
        assert (flags & 1).any() and (flags == R.EXISTS).any()       # TPs and FPs
    _check(ap, slabs, npos, nc, len(thr))


@pytest.mark.parametrize("per_class", [True, False])
def test_rank_order_with_special_scores_and_k_not_a_multiple_of_four(per_class):
    """The order inside a (scene, class) for scores that only the comparison rules tell apart -- NaN, both infinities, both
    zeros, a denormal, repeated values -- among valid and not-valid proposals alike, at a K whose last group of four
    proposals is incomplete.  Slabs and npos equal the restatement exactly."""
    B, K, M, nc, thr = 2, 37, 5, 3, (0.25, 0.5)
    pool = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, 0.5, 0.5, 0.25, 0.25, 0.75], np.float32)
    assert pool[5] != 0 and np.abs(pool[5]) < np.finfo(np.float32).tiny
    d = synthetic(B, K, M, nc, seed=7, live=1.1)
    b, k, c = np.arange(B)[:, None, None], np.arange(K)[None, :, None], np.arange(nc)[None, None, :]
    d["conf"] = pool[(k + 2 * c + b) % len(pool)]
    d["obj_prob"] = pool[(k + b)[:, :, 0] % len(pool)]
    d["valid"] = ((k // len(pool) + b) % 2 == 0)[:, :, 0]            # every pool value sits in valid and not-valid proposals
    d["sem_cls"] = d["sem_cls"] % 2                                  # single-class mode: long lists, and a class without records
    for s in (d["obj_prob"], d["conf"][:, :, 0]):
        for v in pool.view(np.uint32):
            hit = s.view(np.uint32) == v
            assert (hit & d["valid"]).any() and (hit & ~d["valid"]).any()
    ap = _run(d, [B], per_class, nc, thr)
    slabs, npos = _restated(d, [B], per_class, nc, thr)
    assert (slabs[0][1] & 3).any() and (slabs[0][1] == R.EXISTS).any() and (slabs[0][1] == 0).any()
    for g, w, what in zip(ap.slabs[0], slabs[0], ("score", "flags", "index")):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=what)                 # (NaN equals NaN)
    np.testing.assert_array_equal(np.signbit(ap.slabs[0][0].cpu().numpy()), np.signbit(slabs[0][0]), err_msg="sign of zero")
    np.testing.assert_array_equal(ap.npos.cpu().numpy(), npos)


def test_one_batch_equals_split_steps_and_reset_starts_over():
    d = synthetic(5, 128, 32, 18, seed=3, quant=64)
    whole = _run(d, [5], True)
    split = _run(d, [2, 1, 2], True)
    a, b = whole.curves(), split.curves()
    for k in ("ap", "last_rec", "rec", "prec", "count", "npos", "score", "flags"):
        np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), err_msg=k)
    m = whole.compute_metrics()
    assert m == split.compute_metrics()
    # reset(): a different run afterwards equals a fresh object's
    d2 = synthetic(2, 128, 32, 18, seed=4)
    whole.reset()
    assert whole.slabs == [] and whole.npos is None
    again = _run(d2, [2], True, ap=whole).compute_metrics()
    assert again == _run(d2, [2], True).compute_metrics() and again != m


def test_graph_capture_of_postprocess_and_step_replays_the_same_slab():
    from spacap3d_amd.detection_ap import DetectionAP
    from spacap3d_amd.postprocess import detection_postprocess
    from test_postprocess_gpu import synthetic_scenes
    h = synthetic_scenes(4, 20000, 256, seed=11)
    t = _dev(h)
    lab = _dev({k: synthetic(4, 256, 64, 18, seed=12)[k] for k in LABELS})
    lab["gt_box_corner_label"][:, :40] = t["bbox_corner"][:, 100:140].float()      # some proposals hit a box
    ep = dict(lab, bbox_corner=t["bbox_corner"], sem_cls=t["sem_cls"])
    args = (t["point_clouds"], t["bbox_corner"], t["objectness_scores"], t["sem_cls"], t["sem_cls_scores"])
    eager = DetectionAP(18)
    want = [x.cpu().numpy() for x in eager.step(detection_postprocess(*args), ep)]
    assert (want[1] & 3).any() and (want[1] == R.EXISTS).any()
    ap = DetectionAP(18)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ap.step(detection_postprocess(*args), ep)             # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = ap.step(detection_postprocess(*args), ep)
    for x in static:
        x.zero_()
    g.replay()
    torch.cuda.synchronize()
    for x, w, what in zip(static, want, ("score", "flags", "index")):
        np.testing.assert_array_equal(x.cpu().numpy(), w, err_msg=what)


def test_evaluator_accumulates_like_step_by_hand():
    from spacap3d_amd.detection_ap import DetectionAP
    from spacap3d_amd.engine import Evaluator, synthetic_batch
    from spacap3d_amd.spacapnet import build_default
    from test_postprocess_gpu import POST_DICT
    torch.manual_seed(0)
    model = build_default(vocab_size=200, num_proposal=64, N=2, d_ff=256).to(DEV).eval()
    batches = [synthetic_batch(2, 4096, DEV, seed=s, vocab=200) for s in (1, 2)]
    for i, b in enumerate(batches):
        M = b["sem_cls_label"].shape[1]
        b["gt_box_corner_label"] = torch.from_numpy(synthetic(2, 64, M, 18, seed=20 + i)["gt_box_corner_label"]).to(DEV)
    ap = DetectionAP(18)
    ev = Evaluator(model, postprocess=dict(POST_DICT, dataset_config=None), detection_ap=ap)
    outs = [ev(b, next_data=batches[i + 1] if i + 1 < len(batches) else None) for i, b in enumerate(batches)]
    assert len(ap.slabs) == 2
    hand = DetectionAP(18)
    for out, b in zip(outs, batches):
        assert out["sem_cls_scores"].shape[-1] == 18
        hand.step({"valid": out["post_valid"], "conf": out["post_conf"]},
                  {"bbox_corner": out["bbox_corner"], "sem_cls": out["sem_cls"], **{k: b[k] for k in LABELS}})
    for got, want in zip(ap.slabs, hand.slabs):
        for g, w in zip(got, want):
            assert torch.equal(g, w)
    assert torch.equal(ap.npos, hand.npos) and int(ap.npos.sum()) == int(sum((b["box_label_mask"] == 1).sum() for b in batches))
    m = ap.compute_metrics()
    assert m == hand.compute_metrics() and len(m) == 2 and "mAP" in m[0] and "AR" in m[1]
    plain = Evaluator(model, postprocess=dict(POST_DICT, dataset_config=None))
    assert plain.detection_ap is None
