"""No-GPU checks of the mixed rewards and the mixed caption loss of self-critical training: the numpy
restatement (tests/reward_mix_restated.py) reproduces what the reference's own ``BleuScorer`` and ``Rouge`` recorded per caption
row (tests/golden/caption_reward_ref.npz, made by tests/golden/make_fixtures_reward.py), the restated gradient of the mixed loss
equals a central difference, the case tables hold what they are for, the C entry points refuse bad arguments without touching a
device, and the Python layer refuses bad settings and CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import caption_eval_restated as R
import losses_restated as LR
import reward_mix_restated as RM
import self_critical_restated as SC
from test_caption_eval_cpu import FIX, corpus_of

HERE = os.path.dirname(os.path.abspath(__file__))
REC = np.load(os.path.join(HERE, "golden", "caption_reward_ref.npz"))


@pytest.mark.parametrize("name", RM.ROW_SET_NAMES)
def test_restated_scores_reproduce_the_reference(name):
    """Integers first: the key rows and the ten BLEU components exactly; ROUGE to the byte; BLEU-4 within 1e-12 (the same
    formula in the same float64)."""
    tokens, didx, oid, table, want_key, case = RM.row_set(FIX, name)
    got = RM.rewards(SC.Corpus(R.refs_of(FIX, case)), tokens, 1, didx, oid, table, R.SOS, R.EOS, (1.0, 2.0, 1.0))
    np.testing.assert_array_equal(got.key, REC[f"{name}/key"])
    np.testing.assert_array_equal(got.key, want_key)
    np.testing.assert_array_equal(got.bleu_comp, REC[f"{name}/bleu_comp"])
    assert got.scores[:, 2].tobytes() == REC[f"{name}/rouge"].tobytes()
    err = float(np.abs(got.scores[:, 1] - REC[f"{name}/bleu4"]).max())
    print(f"{name}: {len(tokens)} rows, largest |restated BLEU-4 - recorded| = {err:.3e}")
    assert err <= 1e-12
    lost = got.key < 0
    assert not got.scores[lost].any() and not got.bleu_comp[lost].any() and not got.reward[lost].any()
    assert got.reward.tobytes() == ((1.0 * got.scores[:, 0] + 2.0 * got.scores[:, 1]) + 1.0 * got.scores[:, 2]).tobytes()
    # CIDEr is section 7j's: the restatement of that section gives the same bits
    old = SC.rewards(SC.Corpus(R.refs_of(FIX, case)), tokens, 1, didx, oid, table, R.SOS, R.EOS)
    assert old.cider.tobytes() == got.scores[:, 0].tobytes()
    np.testing.assert_array_equal(old.tf_tok, got.tf_tok)


def test_a_zero_weight_is_not_computed():
    tokens, didx, oid, table, _, case = RM.row_set(FIX, "hand")
    corpus = SC.Corpus(R.refs_of(FIX, case))
    full = RM.rewards(corpus, tokens, 1, didx, oid, table, R.SOS, R.EOS, (1.0, 1.0, 1.0))
    for w in ((1.0, 0.0, 0.0), (0.0, 3.0, 0.0), (0.0, 0.0, 0.5), (2.0, 0.0, 0.25)):
        got = RM.rewards(corpus, tokens, 1, didx, oid, table, R.SOS, R.EOS, w)
        for i in range(3):
            if w[i] == 0:
                assert not got.scores[:, i].any() and not np.signbit(got.scores[:, i]).any()
            else:
                assert got.scores[:, i].tobytes() == full.scores[:, i].tobytes()
        assert got.bleu_comp.any() == (w[1] != 0)
    one = RM.rewards(corpus, tokens, 1, didx, oid, table, R.SOS, R.EOS, (1.0, 0.0, 0.0))
    assert one.reward.tobytes() == one.scores[:, 0].tobytes()                    # weights (1, 0, 0): the reward IS CIDEr-D


def test_the_recorded_rows_hold_what_they_are_for():
    comp = np.concatenate([REC[f"{n}/bleu_comp"] for n in RM.ROW_SET_NAMES])
    key = np.concatenate([REC[f"{n}/key"] for n in RM.ROW_SET_NAMES])
    rouge = np.concatenate([REC[f"{n}/rouge"] for n in RM.ROW_SET_NAMES])
    bleu4 = np.concatenate([REC[f"{n}/bleu4"] for n in RM.ROW_SET_NAMES])
    keyed = key >= 0
    assert 300 < len(key) < 1000 and (~keyed).any() and not comp[~keyed].any()
    assert (comp[keyed, 0] < comp[keyed, 1]).any()                                # brevity penalty
    assert ((comp[:, 0] == 2) & (comp[:, 4] == 0) & (comp[:, 5] == 0) & keyed).any()   # sos eos
    assert (comp[:, 0] == R.LMAX).any()                                           # the 64-token caption
    assert ((rouge > 0) & (rouge < 1)).any() and (bleu4[keyed] > 0).all() and (bleu4 <= 1.0).all()
    # the hand-made rows, one property each (tests/reward_mix_restated.py: HAND_ROWS)
    h = REC["hand/bleu_comp"]
    assert list(h[0, :2]) == [6, 5]                                               # the tie goes to the shorter reference
    assert list(h[1, 2:6]) == [6, 5, 4, 3] and h[1, 6] < 6 and h[1, 7] < 5      # clipped below the caption's own counts
    assert list(h[2]) == [2, 7, 2, 1, 0, 0, 2, 0, 0, 0]                           # sos eos: its one bigram is in no reference
    assert h[3, 0] < h[3, 1] and 0 < REC["hand/rouge"][4] < 1 and REC["hand/key"][5] == -1


def _small_case():
    B0, Rn, S, W, V = 2, 4, 2, 4, 6
    rng = np.random.default_rng(11)
    logits = rng.normal(0.0, 2.0, (B0 + Rn, W, V))
    ids = np.zeros((B0, W + 1), np.int64)
    ids[0] = [2, 3, 0, 4, 1]                                # an interior pad id
    ids[1] = [2, 5, V, SC.FAR_ID, 0]                        # ids out of range: ignored
    words = rng.integers(0, V, (Rn, W)).astype(np.int64)
    words[2, 1] = V
    length = np.asarray([1, W, 3, 2], np.int32)
    return logits, ids, words, length, rng.uniform(0.0, 3.0, Rn), rng.uniform(0.0, 3.0, Rn // S), S


@pytest.mark.parametrize("baseline", ("greedy", "samples"))
def test_restated_gradient_equals_a_central_difference(baseline):
    """The project's bound for this check (tests/test_self_critical_cpu.py): 1e-6 of the largest entry."""
    logits, ids, words, length, reward, base, S = _small_case()
    base = base if baseline == "greedy" else None
    good, count, w_xe = np.asarray([True, True]), np.asarray([True, True]), 0.5
    f = lambda x: RM.loss(x, ids, good, words, length, reward, base, count, S, w_xe).loss
    ref = RM.loss(logits, ids, good, words, length, reward, base, count, S, w_xe, gout=1.0)
    h = 1e-6
    num = np.zeros_like(logits)
    for i in np.ndindex(*logits.shape):
        up, dn = logits.copy(), logits.copy()
        up[i] += h
        dn[i] -= h
        num[i] = (f(up) - f(dn)) / (2 * h)
    fig = float(np.abs(ref.dlogits - num).max() / np.abs(num).max())
    print(f"{baseline}: largest |gradient - central difference| / largest entry = {fig:.3e}")
    assert fig <= 1e-6
    assert ref.loss == ref.l_rl + w_xe * ref.l_xe and ref.l_xe > 0 and np.abs(ref.dlogits[:2]).max() > 0
    assert not ref.dlogits[0, 1].any() and not ref.dlogits[1, 1:].any()          # pad and out-of-range targets
    # the parts are the two existing restatements
    assert ref.l_rl == SC.loss(logits[2:], words, length, reward, base, count, S).loss
    assert ref.l_xe == LR.caption(LR.CapInputs(logits[:2], ids, good), 1.0).loss
    # no good scene: the cross-entropy term and its gradient vanish, nothing is NaN
    none = RM.loss(logits, ids, np.zeros(2, bool), words, length, reward, base, count, S, w_xe)
    assert none.l_xe == 0.0 and none.loss == none.l_rl and not none.dlogits[:2].any() and np.isfinite(none.inv_xe)
    # weight 0: the loss is section 7j's and the ground-truth rows get no gradient
    zero = RM.loss(logits, ids, good, words, length, reward, base, count, S, 0.0)
    assert zero.loss == zero.l_rl and not zero.dlogits[:2].any() and zero.l_xe == ref.l_xe
    # ground-truth rows of fewer word positions than the pass: what is padded behind them counts for nothing
    cut = RM.loss(logits, ids, good, words, length, reward, base, count, S, w_xe, xe_positions=2)
    assert cut.l_xe == LR.caption(LR.CapInputs(logits[:2, :2], ids, good), 1.0).loss and cut.l_xe != ref.l_xe
    assert not cut.dlogits[:2, 2:].any() and cut.dlogits[0, 0].any() and cut.inv_xe == 1.0 / LR._den(4.0)
    assert np.array_equal(cut.dlogits[2:], ref.dlogits[2:])
    # no ground-truth rows at all
    bare = RM.loss(logits[2:], None, np.zeros(0, bool), words, length, reward, base, count, S, w_xe)
    assert bare.loss == ref.l_rl and bare.l_xe == 0.0 and np.array_equal(bare.dlogits, ref.dlogits[2:])


def test_loss_cases_hold_what_they_are_for():
    cases = RM.LOSS_CASES
    assert len(cases) == len(RM.LOSS_SHAPES) * 3 * 3 * 3 * 2
    assert {c.V for c in cases} >= {2, 255, 256, 257, 1000, 3001} and {c.B0 for c in cases} >= {0, 65} and max(c.R for c in cases) > 64
    assert {c.w_xe for c in cases} == {0.0, 0.5, 1.0}
    for shape in RM.LOSS_SHAPES:
        B0, Rn, S, W, V = shape
        x = RM.loss_inputs(RM.MixCase(*shape, "all", "all", 0.5, "greedy"))
        assert x.logits.shape == (B0 + Rn, W, V) and x.length.min() == 1 and x.length.max() == W
        assert x.words[Rn - 1, 0] == V and (W < 2 or x.words[Rn - 1, 1] == SC.FAR_ID)
        if not B0:
            assert x.lang_ids is None
            continue
        t = x.lang_ids[:, 1:W + 1]
        assert x.lang_ids.shape[1] >= W + 1 and (t[0] != 0).sum() >= W - 1 and t[B0 - 1, 0] == V and (W < 2 or t[B0 - 1, 1] == SC.FAR_ID)
        if W >= 3:
            assert t[0, 1] == 0 and t[0, 2] != 0                                # an interior pad id
        assert ((t[1:] != 0).sum(1) <= 1).any() or B0 < 3                        # a row of one word
    big = RM.MixCase(3, 9, 3, 7, 257, "some", "some", 0.5, "greedy")
    x, ref = RM.loss_inputs(big), RM.loss_reference(big)
    assert ref.acc_xe > 0 and ref.l_xe > 0 and ref.n_good == 2 and not ref.dlogits[1].any() and not x.good[1]
    assert not ref.dlogits[3 + 3:3 + 6].any() and not x.count[1]


def test_entry_points_reject_bad_arguments_without_a_device():
    from spacap3d_amd._native import lib
    off = (ctypes.c_int64 * 5)(0, 1, 2, 3, 4)
    name = b"spacap_caption_reward_mix_f64"

    def rw(rows=2, rps=1, L=31, items=1, nobj=1, nkeys=1, sos=2, eos=3, n_tok=1, n_ref=1, w=(1.0, 1.0, 1.0)):
        return lib.spacap_caption_reward_mix_f64(None, rows, rps, L, None, None, None, items, nobj, nkeys, sos, eos, None, n_tok, None,
                                                 None, n_ref, None, None, None, off, 0.0, w[0], w[1], w[2], None, None, None, None,
                                                 None, None, None, None, None)
    for bad in (dict(rows=-1), dict(rps=0), dict(rows=3, rps=2), dict(L=0), dict(L=63), dict(items=0), dict(nobj=0), dict(nkeys=0),
                dict(sos=-1), dict(eos=65536), dict(n_tok=-1), dict(n_ref=-1)):
        assert rw(**bad) == -1, bad
        assert name in lib.spacap_last_error() and b"bad sizes" in lib.spacap_last_error()
    for w in ((-1.0, 1.0, 1.0), (1.0, float("nan"), 0.0), (0.0, 0.0, float("inf"))):
        assert rw(w=w) == -1, w
        assert name in lib.spacap_last_error() and b"bad weights" in lib.spacap_last_error()
    assert rw() == -1 and name + b": null" in lib.spacap_last_error()
    assert rw(rows=0) == 0 and rw(rows=0, L=62) == 0

    one = ctypes.c_void_p(8)       # a non-null baseline for the size checks (nothing is launched, nothing dereferenced)
    name = b"spacap_mixed_cap_loss_fwd_f32"

    def fw(B0=2, R=6, S=3, W=5, V=7, ts=6, w=0.5, base=one, W0=5):
        return lib.spacap_mixed_cap_loss_fwd_f32(None, None, ts, None, B0, W0, None, None, None, base, None, R, S, W, V, w, None, None,
                                                 None, None, None, None)
    for bad in (dict(B0=-1), dict(R=-1), dict(S=0), dict(R=7), dict(W=0), dict(V=1), dict(ts=4), dict(W0=0), dict(W0=6),
                dict(B0=1 << 19, R=1 << 19, S=1, W=1 << 12, W0=1), dict(S=1, base=None)):
        assert fw(**bad) == -1, bad
        assert name in lib.spacap_last_error() and b"bad sizes" in lib.spacap_last_error()
    for w in (-0.5, float("nan"), float("inf")):
        assert fw(w=w) == -1 and name in lib.spacap_last_error() and b"bad weight" in lib.spacap_last_error()
    assert fw() == -1 and name + b": null" in lib.spacap_last_error()
    assert fw(B0=0, R=0) == 0 and fw(B0=0, R=0, ts=0, W0=0) == 0                  # (out is null: nothing to zero)
    assert fw(W0=3, ts=3) == -1 and name + b": null" in lib.spacap_last_error()   # narrower ground-truth rows pass the size checks
    name = b"spacap_mixed_cap_loss_bwd_f32"

    def bw(B0=2, R=6, W=5, V=7, ts=6, w=0.5, W0=5):
        return lib.spacap_mixed_cap_loss_bwd_f32(None, None, ts, None, B0, W0, None, None, None, None, None, None, R, W, V, w, None, None)
    for bad in (dict(B0=-1), dict(R=-1), dict(W=0), dict(V=1), dict(ts=4), dict(W0=0), dict(W0=6),
                dict(B0=1 << 19, R=1 << 19, W=1 << 12, W0=1)):
        assert bw(**bad) == -1, bad
        assert name in lib.spacap_last_error() and b"bad sizes" in lib.spacap_last_error()
    assert bw(w=-1.0) == -1 and b"bad weight" in lib.spacap_last_error()
    assert bw() == -1 and name + b": null" in lib.spacap_last_error()
    assert bw(B0=0, R=0) == 0


def test_symbols_are_declared_and_exported():
    from spacap3d_amd import _native
    header = open(os.path.join(os.path.dirname(HERE), "include", "spacap_hip.h")).read()
    for name in ("spacap_caption_reward_mix_f64", "spacap_mixed_cap_loss_fwd_f32", "spacap_mixed_cap_loss_bwd_f32"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _native.SIGNATURES and hasattr(_native.lib, name)


def _corpus():
    from spacap3d_amd.caption_eval import CaptionCorpus
    corpus, w2i = corpus_of("select")
    return CaptionCorpus(corpus, w2i, key_of=FIX["select/key_table"])


def test_self_critical_settings_and_refusals():
    from spacap3d_amd.fused_losses import mixed_caption_loss
    from spacap3d_amd.self_critical import REWARD_TERMS, SelfCritical
    c = _corpus()
    assert REWARD_TERMS == RM.TERMS
    sc = SelfCritical(c, R.SOS, R.EOS)
    assert sc.reward_weights == (1.0, 0.0, 0.0) and sc.xe_weight == 0.0 and not sc.mixed          # the defaults: section 7j
    assert not SelfCritical(c, R.SOS, R.EOS, reward={"cider": 1}).mixed
    for reward, want in (("bleu4", (0.0, 1.0, 0.0)), ("rouge", (0.0, 0.0, 1.0)), ({"cider": 1, "bleu4": 2, "rouge": 1}, (1.0, 2.0, 1.0)),
                         ({"rouge": 0.5}, (0.0, 0.0, 0.5)), ({"cider": 2.0}, (2.0, 0.0, 0.0))):
        got = SelfCritical(c, R.SOS, R.EOS, reward=reward)
        assert got.reward_weights == want and got.mixed
    assert SelfCritical(c, R.SOS, R.EOS, xe_weight=0.5).mixed and SelfCritical(c, R.SOS, R.EOS, xe_weight=0.5).xe_weight == 0.5
    for bad in ("meteor", "", None, 3, {}, {"meteor": 1.0}, {"cider": -1.0}, {"cider": 0.0, "bleu4": 0}, {"rouge": float("nan")},
                {"bleu4": float("inf")}, {"cider": "much"}, ["cider"]):
        with pytest.raises(ValueError, match="self_critical: reward"):
            SelfCritical(c, R.SOS, R.EOS, reward=bad)
    for bad in (-0.5, float("nan"), float("inf"), "half"):
        with pytest.raises(ValueError, match="self_critical: xe_weight"):
            SelfCritical(c, R.SOS, R.EOS, xe_weight=bad)
    mix = SelfCritical(c, R.SOS, R.EOS, reward={"cider": 1, "bleu4": 2, "rouge": 1})
    z = torch.zeros(2, dtype=torch.long)
    for s, kw in ((sc, dict(terms=True)), (mix, {}), (mix, dict(terms=True))):
        with pytest.raises(RuntimeError, match="CPU not supported"):
            s.rewards(torch.zeros(2, 31, dtype=torch.long), z, z, **kw)
    with pytest.raises(RuntimeError, match="mixed_caption_loss: CPU not supported"):
        mixed_caption_loss(torch.zeros(3, 3, 5), torch.zeros(1, 4, dtype=torch.long), torch.ones(1, dtype=torch.bool),
                           torch.zeros(2, 3, dtype=torch.long), torch.ones(2, dtype=torch.int32), torch.zeros(2, dtype=torch.float64),
                           torch.zeros(2, dtype=torch.float64), torch.ones(2, dtype=torch.bool), 1, 0.5)


def test_forward_train_refuses_cpu_tensors_with_the_mixed_settings():
    from spacap3d_amd.self_critical import SelfCritical
    from spacap3d_amd.spacapnet import build_default
    torch.manual_seed(0)
    cap = build_default(vocab_size=40, num_proposal=8, N=1, d_ff=128).caption.train()
    ep = {"aggregated_vote_features": torch.zeros(1, 8, 128), "aggregated_vote_xyz": torch.zeros(1, 8, 3), "center": torch.zeros(1, 8, 3),
          "pred_size": torch.ones(1, 8, 3), "bbox_mask": torch.ones(1, 8, dtype=torch.long), "ref_center_label": torch.zeros(1, 3),
          "lang_label": torch.ones(1, 33, dtype=torch.long), "lang_ids": torch.ones(1, 32, dtype=torch.long),
          "object_id": torch.zeros(1, dtype=torch.long), "dataset_idx": torch.zeros(1, dtype=torch.long)}
    cap.self_critical = SelfCritical(_corpus(), R.SOS, R.EOS, num_samples=2, reward={"bleu4": 1.0}, xe_weight=0.5)
    with pytest.raises(RuntimeError, match="self_critical.*not supported"):
        cap.forward_train(dict(ep))
