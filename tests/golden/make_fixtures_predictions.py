"""Generates tests/golden/predictions_ref.npz by RUNNING THE REFERENCE'S OWN code in this container: ``parse_predictions``
(lib/ap_helper.py:45-160) with ``per_class_proposal=False`` -- per scene the list of (class, corners, obj_prob) of the boxes
that survive the empty-box test, the class-aware 3D NMS and the confidence threshold -- and ``decode_caption``
(lib/eval_helper.py:46-57) for every kept proposal against a small synthetic ``idx2word``.  Nothing of the reference is
copied; the stubs are those of make_fixtures_postprocess.py / make_fixtures_caption.py.

Words: ids 0..3 are pad_ / unk / sos / eos, every other id i is the word ``w<i>`` (tests/caption_eval_restated.py).

Per case ``<case>/...``, the inputs of spacap3d_amd.predictions.dense_caption_predictions
  valid u8 (B,K)            the reference's pred_mask == 1 and obj_prob > conf_thresh
  obj_prob f32 (B,K)        the reference's softmax(objectness_scores)[..., 1]
  objectness_scores f32 (B,K,2), sem_cls i64 (B,K), bbox_corner f64 (B,K,8,3), tokens i64 (B,K,L)
(the point clouds are not kept: they only decide ``valid``, which is recorded), and the reference's results
  ref_scene, ref_proposal, ref_cls (n,), ref_score f32 (n,), ref_corners f64 (n,8,3)   the tuples of batch_pred_map_cls in
                            its order (scene, proposal ascending); ref_proposal = where the tuple's corners sit in bbox_corner
  ref_caption (n,)          decode_caption's string of that proposal
Cases (sos = 2, eos = 3, 18 classes, 50 words):
  k5     B=2, K=5,   L=1    (eos at position 0 = last; no eos)
  k64    B=3, K=64,  L=31   scene 0 ordinary; scene 1 every objectness below conf_thresh: nothing kept; scene 2 exact score
                            ties (duplicate logits): three kept boxes sharing one score, a kept and an empty (dropped) box
                            sharing another, and pairs inside clusters, where the NMS may drop one of them
  k65    B=2, K=65,  L=62
  k512   B=2, K=512, L=12
In scene 0 of every case the first kept proposals get eos at position 0, eos only at the last position, and no eos.
Asserted while generating: every scene but k64's scene 1 keeps a box; scene 2 of k64 holds a tie between kept boxes and one
between a kept and a dropped box; the numpy restatement (tests/dense_caption_restated.py) reproduces the kept sets, classes,
scores (bit-equal f32), corners (bit-equal f64) and strings.

Run:  python tests/golden/make_fixtures_predictions.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_fixtures_postprocess import NC, REF, corners_of, install_stubs  # noqa: E402
import caption_eval_restated as R  # noqa: E402
import dense_caption_restated as D  # noqa: E402

SOS, EOS, V = R.SOS, R.EOS, 50
CONF = 0.05
M = 8


def make_scene(rng, N, K, mode):
    """Eight separated objects with points inside, K proposals: jittered copies of an object's box (the NMS suppresses
    inside such a cluster), lone boxes anywhere, boxes above the cloud (empty).  mode: "plain", "empty" (every objectness
    below conf_thresh) or "ties" (duplicate logits)."""
    base_c = np.array([[x, y, 0.6] for y in (-1.0, 1.0) for x in (-2.25, -0.75, 0.75, 2.25)]) + rng.uniform(-0.1, 0.1, (M, 3))
    base_s = rng.uniform(0.5, 0.9, (M, 3))
    base_cls = rng.permutation(NC)[:M]
    per = N // 2 // M
    pts = [rng.uniform([-3.5, -2.2, 0.0], [3.5, 2.2, 2.5], (N - per * M, 3))]
    for m in range(M):
        pts.append(base_c[m] + rng.uniform(-0.5, 0.5, (per, 3)) * base_s[m])
    pts = np.concatenate(pts).astype(np.float32)
    centers, sizes, cls, role = [], [], [], []
    for k in range(K):
        m = k % M
        u = rng.random()
        if k < min(M, K - 2) or u < 0.55:                 # the first round: one box per object, so something is kept
            jit = 0.0 if k < M else rng.uniform(0.02, 0.2)
            centers.append(base_c[m] + rng.normal(0, 1, 3) * jit * base_s[m] * 0.3)
            sizes.append(base_s[m] * rng.uniform(1 - jit, 1 + jit, 3))
            cls.append(int(base_cls[m]) if rng.random() < 0.7 or k < M else int(rng.integers(0, NC)))
            role.append("obj")
        elif u < 0.8 and k < K - 1:
            centers.append(rng.uniform([-3.0, -2.0, 0.3], [3.0, 2.0, 2.0]))
            sizes.append(rng.uniform(0.2, 0.8, 3))
            cls.append(int(rng.integers(0, NC)))
            role.append("lone")
        else:                                             # (the last proposal always: K = 5 holds one too)
            centers.append(rng.uniform([-3.0, -2.0, 6.0], [3.0, 2.0, 8.0]))
            sizes.append(rng.uniform(0.2, 0.6, 3))
            cls.append(int(rng.integers(0, NC)))
            role.append("out")
    corners = corners_of(np.array(centers), np.array(sizes))
    probs = rng.permutation(np.linspace(0.06, 0.99, K)) + rng.uniform(-1e-4, 1e-4, K)
    low = rng.random(K) < 0.12
    low[:min(M, K - 2)] = False
    probs[low] = rng.uniform(0.001, 0.04, int(low.sum()))
    if mode == "empty":
        probs = rng.uniform(0.001, 0.04, K)
    x0 = rng.normal(0, 1, K).astype(np.float32)
    x1 = (x0 + np.log(probs / (1 - probs))).astype(np.float32)
    obj = np.stack([x0, x1], 1)
    if mode == "ties":
        out = [k for k in range(K) if role[k] == "out"]
        assert len(out) >= 2
        hi = np.array([rng.normal(), 0.0], np.float32)
        hi[1] = hi[0] + np.float32(4.0)
        obj[0], obj[1], obj[2] = hi, hi, hi               # three of the first round (three objects, three classes): all kept
        obj[out[0]] = obj[3]                              # a kept box and an empty one
        obj[out[1]] = obj[3]
        for k in range(M, K - 1, 5):                      # pairs inside the clusters
            if role[k] == "obj" and role[k + 1] != "out":
                obj[k + 1] = obj[k]
    scores = rng.normal(0, 1.5, (K, NC)).astype(np.float32)
    scores[np.arange(K), cls] += 4.0
    sem_cls = scores.argmax(1).astype(np.int64)
    height = (pts[:, 2:3] - np.percentile(pts[:, 2], 0.99)).astype(np.float32)
    return np.concatenate([pts, height], 1), corners, obj, sem_cls, scores


def main():
    install_stubs()
    os.chdir(REF)
    sys.path.insert(0, REF)
    import torch
    import data.scannet.model_util_scannet as mus
    mus.ScannetDatasetConfig = lambda: types.SimpleNamespace(num_class=NC)     # its constructor reads a ScanNet label file
    from lib.ap_helper import parse_predictions, softmax
    from lib.eval_helper import decode_caption

    rng = np.random.default_rng(77)
    idx2word = {str(i): R.word(i) for i in range(V)}
    DC = types.SimpleNamespace(num_class=NC)
    cfg = {"remove_empty_box": True, "use_3d_nms": True, "nms_iou": 0.25, "use_old_type_nms": False, "cls_nms": True,
           "per_class_proposal": False, "conf_thresh": CONF, "dataset_config": DC}
    cases = {"k5": (5, 1, 600, ("plain", "plain")), "k64": (64, 31, 1500, ("plain", "empty", "ties")),
             "k65": (65, 62, 1500, ("plain", "plain")), "k512": (512, 12, 2000, ("plain", "plain"))}
    out = {}
    for name, (K, L, N, modes) in cases.items():
        B = len(modes)
        pc, corners, obj, sem_cls, scores = (np.stack(c) for c in zip(*[make_scene(rng, N, K, m) for m in modes]))
        ep = {"center": torch.zeros(B, K, 3), "bbox_corner": torch.from_numpy(corners), "sem_cls": torch.from_numpy(sem_cls),
              "sem_cls_scores": torch.from_numpy(scores), "point_clouds": torch.from_numpy(pc),
              "objectness_scores": torch.from_numpy(obj)}
        lists = parse_predictions(ep, cfg)
        obj_prob = softmax(obj)[:, :, 1]
        assert obj_prob.dtype == np.float32
        valid = (ep["pred_mask"] == 1) & (obj_prob > CONF)
        for b in range(B):
            p = obj_prob[b][np.abs(obj_prob[b] - CONF) < 1e-6]
            assert p.size == 0, "obj_prob next to conf_thresh"

        tokens = rng.integers(4, V, (B, K, L)).astype(np.int64)
        for b, k in np.ndindex(B, K):
            if rng.random() < 0.7:
                tokens[b, k, int(rng.integers(0, L))] = EOS      # one eos somewhere; what follows is junk (more words)
        kept0 = np.nonzero(valid[0])[0]
        assert len(kept0) >= 3 or (K == 5 and len(kept0) >= 2)
        tokens[0, kept0[0]] = rng.integers(4, V, L)
        tokens[0, kept0[0], 0] = EOS                             # eos at position 0
        tokens[0, kept0[1]] = rng.integers(4, V, L)              # no eos
        if len(kept0) >= 3:
            tokens[0, kept0[2]] = rng.integers(4, V, L)
            tokens[0, kept0[2], L - 1] = EOS                     # eos only at the last position

        rows = []
        for b, lst in enumerate(lists):
            js = np.nonzero(valid[b])[0]
            assert len(lst) == len(js)
            for j, (c, box, p) in zip(js, lst):                  # the list comprehension runs over j ascending
                assert np.array_equal(box, corners[b, j]) and isinstance(p, np.float32) and p == obj_prob[b, j]
                assert c == int(sem_cls[b, j])
                rows.append((b, int(j), int(c), p, np.array(box), decode_caption(torch.from_numpy(tokens[b, j]), idx2word)))
        kept = [int(valid[b].sum()) for b in range(B)]
        print(f"{name}: B={B} K={K} L={L}: kept {kept}, non-empty by the NMS mask {[int(x) for x in ep['pred_mask'].sum(1)]}")
        for b, m in enumerate(modes):
            assert (kept[b] == 0) == (m == "empty"), (name, b, kept[b])
            if m == "empty":
                assert ep["pred_mask"][b].sum() > 0              # dropped by the threshold, not by the reference's assert
            if m == "ties":
                p, v = obj_prob[b], valid[b]
                kk = sum(1 for i in range(K) for j in range(i + 1, K) if p[i] == p[j] and v[i] and v[j])
                kd = sum(1 for i in range(K) for j in range(K) if p[i] == p[j] and v[i] and not v[j])
                print(f"   ties: {kk} kept-kept pairs, {kd} kept-dropped pairs")
                assert kk >= 3 and kd >= 2

        got = D.select(valid, obj_prob, sem_cls, corners, tokens, SOS, EOS)
        for b in range(B):
            ref = {r[1]: r for r in rows if r[0] == b}
            recs = D.records(got, b)
            assert sorted(r[0] for r in recs) == sorted(ref)
            for j, c, p, box, text in recs:
                assert c == ref[j][2] and p.tobytes() == ref[j][3].tobytes() and box.tobytes() == ref[j][4].tobytes()
                assert text == ref[j][5], (text, ref[j][5])
        out.update({f"{name}/valid": valid.astype(np.uint8), f"{name}/obj_prob": obj_prob, f"{name}/objectness_scores": obj,
                    f"{name}/sem_cls": sem_cls, f"{name}/bbox_corner": corners, f"{name}/tokens": tokens,
                    f"{name}/ref_scene": np.array([r[0] for r in rows], np.int64),
                    f"{name}/ref_proposal": np.array([r[1] for r in rows], np.int64),
                    f"{name}/ref_cls": np.array([r[2] for r in rows], np.int64),
                    f"{name}/ref_score": np.array([r[3] for r in rows], np.float32),
                    f"{name}/ref_corners": np.array([r[4] for r in rows], np.float64).reshape(-1, 8, 3),
                    f"{name}/ref_caption": np.array([r[5] for r in rows])})
    path = os.path.join(HERE, "predictions_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
