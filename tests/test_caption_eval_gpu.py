"""Caption metrics on the MI355X (spacap3d_amd/caption_eval.py, csrc/caption_eval.hip) against the reference's recorded
results (tests/golden/caption_eval_ref.npz: lib/capeval's Bleu / Cider / Rouge and lib/eval_helper.py's feed_scene_cap).

Exactness: candidate tokens and lengths and every BLEU integer are compared exactly; ROUGE-L per key bit for bit (a chain of
IEEE divisions, two multiplies and an add in the reference's order, compiled without contraction); CIDEr per key and both
means within 1e-9 absolute (scores are <= 10, each fewer than ~2 000 f64 operations on values <= ~500 plus a device exp: an
error budget of about 1e-12, while one misplaced n-gram moves a score by more than 1e-4); BLEU-1..4 within 1e-12 (identical
integers: only the host's pow / exp could differ).  The largest differences are printed."""
import numpy as np
import pytest
import torch

import caption_eval_restated as R
from test_caption_eval_cpu import FIX, SCORE_CASES, SELECT_INPUTS, corpus_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CIDER_TOL = 1e-9
BLEU_TOL = 1e-12


def _eval(case, key_of=None):
    from spacap3d_amd.caption_eval import CaptionCorpus, CaptionEval
    corpus, w2i = corpus_of(case)
    if key_of is None:
        key_of = np.arange(len(corpus), dtype=np.int32)[None]
    return CaptionEval(CaptionCorpus(corpus, w2i, key_of=key_of), R.SOS, R.EOS)


def _select_batch(s):
    d = {k: torch.from_numpy(np.ascontiguousarray(FIX[f"select/{k}"][s])).to(DEV) for k in SELECT_INPUTS}
    d["lang_cap"] = d["tokens"]
    return d


def _table(ce):
    return ce.cand_tok.cpu().numpy(), ce.cand_len.cpu().numpy()


def test_select_two_steps_equal_feed_scene_cap():
    ce = _eval("select", FIX["select/key_table"])
    for s, suffix in ((0, "_step1"), (1, "")):
        d = _select_batch(s)
        ce.step(d, masks=d)
        tok, ln = _table(ce)
        np.testing.assert_array_equal(tok, FIX[f"select/cand_tok{suffix}"])
        np.testing.assert_array_equal(ln, FIX[f"select/cand_len{suffix}"])
    words = ce.candidates({str(i): R.word(i) for i in range(int(FIX["select/vocab"]))})
    assert list(words) == [str(k) for k in FIX["select/keys"]]
    for i, k in enumerate(words):
        assert words[k] == [R.sentence(FIX["select/cand_tok"][i, :FIX["select/cand_len"][i]])]
    # logits instead of tokens: argmax(-1) first, as lib/eval_helper.py:124-128
    ce.reset()
    for s in (0, 1):
        d = _select_batch(s)
        d["lang_cap"] = torch.nn.functional.one_hot(d["tokens"], int(FIX["select/vocab"])).float()
        ce.step(d, masks=d)
    np.testing.assert_array_equal(_table(ce)[0], FIX["select/cand_tok"])
    ce.reset()
    tok, ln = _table(ce)
    assert (ln == 2).all() and (tok[:, :2] == [R.SOS, R.EOS]).all() and not tok[:, 2:].any()


def test_graph_captured_step_replays_on_the_second_batch():
    ce = _eval("select", FIX["select/key_table"])
    static = _select_batch(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ce.step(static, masks=static)                   # the first batch, eagerly, on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ce.step(static, masks=static)
    np.testing.assert_array_equal(_table(ce)[0], FIX["select/cand_tok_step1"])      # capturing ran nothing
    for k, v in _select_batch(1).items():
        static[k].copy_(v)
    g.replay()
    torch.cuda.synchronize()
    tok, ln = _table(ce)
    np.testing.assert_array_equal(tok, FIX["select/cand_tok"])
    np.testing.assert_array_equal(ln, FIX["select/cand_len"])
    g.replay()                                          # the same batch again: later stamps, the same winners
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_table(ce)[0], FIX["select/cand_tok"])
    assert int(ce.counter[0]) == 3 * 2 * 64              # one eager call and two replays


@pytest.mark.parametrize("case", SCORE_CASES)
def test_scores_equal_the_reference(case):
    ce = _eval(case)
    ce.set_candidates(torch.from_numpy(FIX[f"{case}/cand_tok"]).to(DEV), torch.from_numpy(FIX[f"{case}/cand_len"]).to(DEV))
    r = {k: v.cpu().numpy() for k, v in ce.scores().items()}
    np.testing.assert_array_equal(r["bleu"], FIX[f"{case}/bleu_comp"])
    bad = np.nonzero(r["rouge"] != FIX[f"{case}/rouge_scores"])[0]
    assert r["rouge"].tobytes() == FIX[f"{case}/rouge_scores"].tobytes(), (bad, r["rouge"][bad], FIX[f"{case}/rouge_scores"][bad])
    dc = np.abs(r["cider"] - FIX[f"{case}/cider_scores"])
    print(f"{case}: largest per-key CIDEr difference {dc.max():.3e} at key {int(dc.argmax())}")
    assert dc.max() <= CIDER_TOL
    m = ce.compute_metrics()
    assert m["cider_scores"].tobytes() == r["cider"].tobytes() and m["rouge_scores"].tobytes() == r["rouge"].tobytes()
    print(f"{case}: CIDEr {m['cider']!r} vs {float(FIX[f'{case}/cider'])!r}, ROUGE {m['rouge']!r} vs {float(FIX[f'{case}/rouge'])!r}, "
          f"BLEU difference {max(abs(a - b) for a, b in zip(m['bleu'], FIX[f'{case}/bleu'])):.3e}")
    assert abs(m["cider"] - float(FIX[f"{case}/cider"])) <= CIDER_TOL
    assert abs(m["rouge"] - float(FIX[f"{case}/rouge"])) <= CIDER_TOL
    assert len(m["bleu"]) == 4 and all(abs(a - b) <= BLEU_TOL for a, b in zip(m["bleu"], FIX[f"{case}/bleu"]))


class _LabelledForward(torch.nn.Module):
    """The forward followed by what ``get_scene_cap_loss(..., detection=True, caption=False)`` adds in the reference: labels
    that depend on THIS forward's proposals.  (Which votes become proposals is a chaotic function of the network's outputs
    -- detector.ProposalModule.forward -- so labels taken from an earlier forward of the same batch need not fit the boxes
    of a later one.)  Proposal k is assigned ground-truth box k: its own box for even k (IoU 1), that box moved 100 m away
    for odd k (IoU 0)."""

    def __init__(self, model, M):
        super().__init__()
        self.model, self.M = model, M

    def forward(self, d, is_eval=True):
        out = self.model(d, is_eval=is_eval)
        B, K = out["bbox_mask"].shape
        gt = torch.zeros(B, self.M, 8, 3, device=out["bbox_corner"].device)
        gt[:, :K] = out["bbox_corner"].float()
        gt[:, 1:K:2] += 100.0
        out["gt_box_corner_label"] = gt
        out["object_assignment"] = torch.arange(K, device=gt.device).expand(B, K).contiguous()
        return out


def test_evaluator_accumulates_like_step_by_hand():
    from spacap3d_amd.engine import Evaluator, synthetic_batch
    from spacap3d_amd.postprocess import caption_eval_masks, post_kwargs
    from spacap3d_amd.spacapnet import build_default
    from test_postprocess_gpu import POST_DICT
    torch.manual_seed(0)
    K = 64
    model = build_default(vocab_size=200, num_proposal=K, N=2, d_ff=256).to(DEV).eval()
    with torch.no_grad():                                # an objectness head that says "object": bbox_mask = 1 whatever the
        head = model.proposal.proposal[-1]               # untrained features are, so the NMS alone decides nms_masks
        head.bias[0] -= 4.0
        head.bias[1] += 4.0
    post = dict(POST_DICT, dataset_config=None)
    batches = [synthetic_batch(2, 4096, DEV, seed=s, vocab=200) for s in (1, 2)]
    M = batches[0]["sem_cls_label"].shape[1]
    assert M >= K
    for i, b in enumerate(batches):                      # object ids 0..9 in turn (3 is coprime to 10): every row of the key
        ids = (3 * torch.arange(M, device=DEV)) % 10     # table is reached, the -1 entries included
        b["scene_object_ids"] = torch.stack([ids, (ids + 1) % 10])
        b["dataset_idx"] = torch.tensor([[i], [i + 1]], device=DEV)
    plain = Evaluator(model, postprocess=post)
    ce = _eval("select", FIX["select/key_table"])
    ev = Evaluator(_LabelledForward(model, M), postprocess=post, caption_eval=ce)
    outs = [ev(b, next_data=batches[i + 1] if i + 1 < len(batches) else None) for i, b in enumerate(batches)]
    hand = _eval("select", FIX["select/key_table"])
    for out, b in zip(outs, batches):
        d = {**b, **out}
        hand.step(d, masks=caption_eval_masks(d, min_iou=0.5, **post_kwargs(post)))
    assert int((hand.stamp > 0).sum()) >= 2              # the run wrote candidates
    assert torch.equal(ce.cand_tok, hand.cand_tok) and torch.equal(ce.cand_len, hand.cand_len)
    assert torch.equal(ce.stamp, hand.stamp) and int(ce.counter[0]) == 2 * 2 * K
    m = ce.compute_metrics()
    assert len(m["bleu"]) == 4 and m["cider_scores"].shape == (8,) and np.isfinite(m["rouge"])
    with pytest.raises(KeyError, match="object_assignment"):      # the bare forward adds no labels
        Evaluator(model, postprocess=post, caption_eval=ce)(batches[0])
    assert plain.caption_eval is None


def test_cpu_tensors_raise():
    ce = _eval("select", FIX["select/key_table"])
    d = _select_batch(0)
    ce.step(d, masks=d)
    cpu = {k: v.cpu() for k, v in d.items()}
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ce.step(cpu, masks=cpu)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ce.step(d, masks=cpu)
