"""Dense-caption predictions on the MI355X (spacap3d_amd/predictions.py, csrc/predictions.hip) against the numpy restatement
(tests/dense_caption_restated.py) and the reference's recorded results (tests/golden/predictions_ref.npz: lib/ap_helper.py's
parse_predictions with per_class_proposal=False and lib/eval_helper.py's decode_caption).

Exactness: the kernel only compares, ranks and copies, so every output array is compared with ``array_equal``, padding
included; scores and corners are bit copies of the inputs."""
import numpy as np
import pytest
import torch

import dense_caption_restated as D
from caption_eval_restated import EOS, SOS, word
from test_predictions_cpu import CASES, EMPTY, FIX, inputs, reference_rows, restated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDX2WORD = {str(i): word(i) for i in range(50)}


def _dev(h, scenes=None):
    """(post, out) dicts of device tensors from a fixture case's inputs (``scenes``: a list of scene indices)."""
    pick = (lambda a: a) if scenes is None else (lambda a: np.ascontiguousarray(a[scenes]))
    t = {k: torch.from_numpy(pick(v)).to(DEV) for k, v in h.items()}
    return ({"valid": t["valid"].bool(), "obj_prob": t["obj_prob"]},
            {"bbox_corner": t["bbox_corner"], "sem_cls": t["sem_cls"], "lang_cap": t["tokens"]})


def _host(pred):
    return {k: v.cpu().numpy() for k, v in pred.items()}


def _assert_equal(got, want, scenes=None):
    assert set(got) == set(D.KEYS)
    for k in D.KEYS:
        w = want[k] if scenes is None else want[k][scenes]
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, k
        np.testing.assert_array_equal(got[k], w, err_msg=k)


@pytest.mark.parametrize("case", CASES)
def test_kernel_equals_the_restatement(case):
    from spacap3d_amd.predictions import dense_caption_predictions
    post, out = _dev(inputs(case))
    _assert_equal(_host(dense_caption_predictions(post, out, SOS, EOS)), restated(case))
    if case == "k64":       # scores instead of tokens: argmax(-1) first; an integer mask instead of a bool one
        out["lang_cap"] = torch.nn.functional.one_hot(out["lang_cap"], 50).float()
        post["valid"] = post["valid"].long() * 3
        _assert_equal(_host(dense_caption_predictions(post, out, SOS, EOS)), restated(case))


def test_nan_scores_and_zero_signs():
    from spacap3d_amd.predictions import dense_caption_predictions
    valid = np.ones((1, 6), np.uint8)
    valid[0, 4] = 0
    h = {"valid": valid, "obj_prob": np.array([[0.5, np.nan, -0.0, 0.9, 0.99, 0.0]], np.float32), "sem_cls": np.arange(6)[None],
         "bbox_corner": np.random.default_rng(0).normal(size=(1, 6, 8, 3)), "tokens": np.full((1, 6, 2), 7)}
    want = D.select(h["valid"], h["obj_prob"], h["sem_cls"], h["bbox_corner"], h["tokens"], SOS, EOS)
    got = _host(dense_caption_predictions(*_dev(h), SOS, EOS))
    assert list(got["index"][0]) == [3, 0, 2, 5, 1, -1]
    for k in D.KEYS:
        assert got[k].tobytes() == want[k].tobytes(), k          # (bytes: the NaN and the -0 are copied as they are)


def test_second_call_into_the_same_buffers_leaves_nothing_stale():
    from spacap3d_amd.predictions import dense_caption_predictions
    case, empty = EMPTY
    pred = dense_caption_predictions(*_dev(inputs(case), [0]), SOS, EOS)
    first = _host(pred)
    assert first["count"][0] >= 20 and first["tokens"][0, :20].any() and first["corners"][0, :20].any()
    ptrs = {k: v.data_ptr() for k, v in pred.items()}
    again = dense_caption_predictions(*_dev(inputs(case), [empty]), SOS, EOS, into=pred)
    assert {k: v.data_ptr() for k, v in again.items()} == ptrs
    got = _host(pred)
    assert got["count"][0] == 0 and (got["index"] == -1).all()
    for k in ("score", "cls", "corners", "tokens", "length"):
        assert not got[k].any(), k
    _assert_equal(got, restated(case), [empty])


def test_graph_capture_replays_on_two_inputs():
    from spacap3d_amd.predictions import dense_caption_predictions
    case = "k64"
    post, out = _dev(inputs(case))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dense_caption_predictions(post, out, SOS, EOS)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pred = dense_caption_predictions(post, out, SOS, EOS)
    g.replay()
    torch.cuda.synchronize()
    _assert_equal(_host(pred), restated(case))
    rolled = [1, 2, 0]                                           # the same scenes in another order: every block's input changes
    post2, out2 = _dev(inputs(case), rolled)
    for dst, src in ((post, post2), (out, out2)):
        for k in dst:
            dst[k].copy_(src[k])
    g.replay()
    torch.cuda.synchronize()
    _assert_equal(_host(pred), restated(case), rolled)


@pytest.mark.parametrize("case", CASES)
def test_records_equal_the_reference(case):
    from spacap3d_amd.predictions import dense_caption_predictions, to_records
    names = {c: "class%d" % c for c in range(18)}
    pred = dense_caption_predictions(*_dev(inputs(case)), SOS, EOS)
    scenes = to_records(pred, idx2word=IDX2WORD, class2type=names)
    assert len(scenes) == FIX[f"{case}/valid"].shape[0]
    for b, recs in enumerate(scenes):
        ref = reference_rows(case, b)
        assert sorted(r["proposal"] for r in recs) == sorted(ref)
        assert (recs == []) == ((case, b) == EMPTY)
        for r in recs:
            c, p, box, text = ref[r["proposal"]]
            assert r["caption"] == text and r["sem_cls"] == c and r["class_name"] == names[c]
            assert r["score"] == float(p) and r["corners"].shape == (8, 3) and r["corners"].tobytes() == box.tobytes()
            assert r["tokens"][0] == SOS and r["tokens"][-1] == EOS and " ".join(word(t) for t in r["tokens"]) == text
        assert [r["score"] for r in recs] == sorted((r["score"] for r in recs), reverse=True)
    bare = to_records(pred)
    assert all("caption" not in r and "class_name" not in r for recs in bare for r in recs)
    assert [len(x) for x in bare] == [len(x) for x in scenes]


def test_evaluator_stores_predictions_without_labels():
    from spacap3d_amd.engine import Evaluator, synthetic_batch
    from spacap3d_amd.predictions import dense_caption_predictions, to_records
    from spacap3d_amd.spacapnet import build_default
    from test_postprocess_gpu import POST_DICT
    torch.manual_seed(0)
    K = 64
    model = build_default(vocab_size=200, num_proposal=K, N=2, d_ff=256).to(DEV).eval()
    post = dict(POST_DICT, dataset_config=None)
    batches = [{"point_clouds": synthetic_batch(2, 4096, DEV, seed=s, vocab=200)["point_clouds"]} for s in (1, 2)]
    ev = Evaluator(model, postprocess=post, predictions=(SOS, EOS))
    outs = [ev(b, next_data=batches[i + 1] if i + 1 < len(batches) else None) for i, b in enumerate(batches)]
    torch.cuda.synchronize()
    for out in outs:
        keys = ["pred_" + k for k in D.KEYS]
        assert all(isinstance(out.get(k), torch.Tensor) for k in keys)
        direct = dense_caption_predictions({"valid": out["post_valid"], "obj_prob": out["post_obj_prob"]}, out, SOS, EOS)
        for k in D.KEYS:
            assert torch.equal(out["pred_" + k], direct[k]), k
        L = out["lang_cap"].shape[2]
        assert out["pred_tokens"].shape == (2, K, L + 2) and out["pred_corners"].shape == (2, K, 8, 3)
        count = out["pred_count"].cpu().numpy()
        print("kept per scene:", count.tolist())
        np.testing.assert_array_equal(count, out["post_valid"].sum(1).cpu().numpy())
        assert [len(x) for x in to_records({k: out["pred_" + k] for k in D.KEYS})] == count.tolist()
    plain = Evaluator(model, postprocess=post)(dict(batches[0]))
    assert not any(k.startswith("pred_") for k in plain)


def test_error_paths():
    from spacap3d_amd.engine import Evaluator
    from spacap3d_amd.predictions import dense_caption_predictions, to_records
    post, out = _dev(inputs("k5"))
    pred = dense_caption_predictions(post, out, SOS, EOS)
    cpu = lambda d: {k: v.cpu() for k, v in d.items()}
    with pytest.raises(RuntimeError, match=r"predictions: .*: CPU not supported"):
        dense_caption_predictions(cpu(post), out, SOS, EOS)
    with pytest.raises(RuntimeError, match=r"predictions: .*: CPU not supported"):
        dense_caption_predictions(post, cpu(out), SOS, EOS)
    with pytest.raises(RuntimeError, match=r"predictions: .*: CPU not supported"):
        to_records(cpu(pred))
    z = lambda *s, dt=torch.int64: torch.zeros(*s, dtype=dt, device=DEV)
    big = ({"valid": z(1, 513, dt=torch.bool), "obj_prob": z(1, 513, dt=torch.float32)},
           {"bbox_corner": z(1, 513, 8, 3, dt=torch.float64), "sem_cls": z(1, 513), "lang_cap": z(1, 513, 4)})
    with pytest.raises(RuntimeError, match="K=513"):
        dense_caption_predictions(*big, SOS, EOS)
    with pytest.raises(RuntimeError, match="L=63"):
        dense_caption_predictions(post, dict(out, lang_cap=z(2, 5, 63)), SOS, EOS)
    with pytest.raises(RuntimeError, match="bbox_corner must be"):
        dense_caption_predictions(post, dict(out, bbox_corner=z(2, 5, 8, dt=torch.float64)), SOS, EOS)
    with pytest.raises(RuntimeError, match="into"):
        dense_caption_predictions(post, out, SOS, EOS, into=dict(pred, count=z(3, dt=torch.int32)))
    with pytest.raises(ValueError, match="predictions needs postprocess"):
        Evaluator(None, predictions=(SOS, EOS))
