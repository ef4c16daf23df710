"""Mixed rewards and the mixed caption loss of self-critical training restated in numpy float64: the
specification ``spacap_caption_reward_mix_f64`` (csrc/caption_reward.hip), ``spacap_mixed_cap_loss_fwd_f32`` / ``_bwd_f32``
(csrc/scst_loss.hip) and the training forward with ``SelfCritical(reward=..., xe_weight=...)`` are held to.  Not a test module:
tests/test_reward_mix_cpu.py anchors the scores to the reference's own ``BleuScorer`` and ``Rouge`` (tests/golden/
caption_reward_ref.npz, made by tests/golden/make_fixtures_reward.py) and the gradient to a central difference,
tests/test_reward_mix_gpu.py runs the tables below through the kernels.

Scores of a row's caption (``self_critical_restated.caption_row``: sos, the words through the first eos, an eos appended when
there was none) against the references of its scene's key row:
  cider   ``self_critical_restated.Corpus.cider``: CIDEr-D x 10;
  bleu4   the sentence-level BLEU-4 the reference's scorer appends to bleu_list[3] (lib/capeval/bleu/bleu_scorer.py:232-240)
          from the ten components testlen, closest reflen (min over (|l - testlen|, l)), guess[k] = max(testlen - k, 0),
          correct[k] clipped by the maximum over the references: prod_{k<4} (correct_k + 1e-15) / (guess_k + 1e-9) to the power
          1/4, times exp(1 - 1 / ratio) when ratio = (testlen + 1e-15) / (reflen + 1e-9) < 1;
  rouge   ``Rouge.calc_score`` (lib/capeval/rouge/rouge.py:45-75, beta 1.2);
  reward  ((w_cider cider) + (w_bleu bleu4)) + (w_rouge rouge) in that order; a term of weight exactly 0 is not computed, reads
          +0.0 and adds +0.0 (its components read 0 as well).
A row without a key row: zeros everywhere, key -1.

Mixed loss over logits (B0 + R, W, V): rows 0 .. B0-1 teacher-forced ground-truth captions, one per scene, rows B0 .. the
R = G S drawn captions of G groups.
  L_rl = ``self_critical_restated.loss`` over rows B0 .. (section 7j, unchanged);
  L_xe = sum_b good_b sum_{t < W0: tgt_bt != 0} -logp[b, t, tgt_bt] / (W0 sum_b good_b + 1e-6), tgt = lang_ids[:, 1 : W0 + 1],
         an id outside [0, V) ignored like the pad id 0: ``losses_restated.caption`` (compute_cap_loss, lib/loss_helper.py:
         212-219, whose sum of good_bbox_masks runs over the (scene, word) rows) on the ground-truth rows' own W0 <= W word
         positions -- what the pass pads behind them counts for nothing; accuracy = first-arg-max hits over the counted
         positions (:226-233);
  loss = L_rl + w_xe L_xe.
Gradient: sample rows as section 7j; ground-truth rows g w_xe good_b / (W0 sum good + 1e-6) (softmax - onehot) at counted
positions; zero everywhere else."""
import collections
import functools
import math

import numpy as np

import caption_eval_restated as R
import losses_restated as LR
import self_critical_restated as SC

F32, F64 = np.float32, np.float64
TERMS = ("cider", "bleu4", "rouge")


# ---- the three scores ------------------------------------------------------------------------------------------------------
def bleu_components(cand, refs):
    """testlen, closest reflen, guess[4], correct[4] (``caption_eval_restated.bleu_components``; no references: reflen 0)"""
    if not refs:
        return [len(cand), 0] + [max(0, len(cand) - n) for n in range(4)] + [0] * 4
    return R.bleu_components(cand, refs)


def bleu4(comp):
    """bleu_list[3] of one sentence from its ten components, in the scorer's order of operations"""
    testlen, reflen, guess, correct = int(comp[0]), int(comp[1]), comp[2:6], comp[6:10]
    bleu = 1.0
    for k in range(4):
        bleu *= (float(correct[k]) + 1e-15) / (float(guess[k]) + 1e-9)
    bleu = bleu ** (1.0 / 4)
    ratio = (testlen + 1e-15) / (reflen + 1e-9)
    if ratio < 1:
        bleu *= math.exp(1 - 1 / ratio)
    return bleu


def rouge(cand, refs):
    return R.rouge(cand, refs) if refs else 0.0


MixRewards = collections.namedtuple("MixRewards", "reward scores bleu_comp key length tf_tok")


def rewards(corpus, tokens, rows_per_scene, dataset_idx, object_id, key_table, sos, eos, weights=(1.0, 1.0, 1.0)):
    """what spacap_caption_reward_mix_f64 writes for ``tokens`` (rows, L): ``scores`` (rows, 3) in the order of TERMS"""
    tokens = np.asarray(tokens)
    rows, L = tokens.shape
    w = [float(x) for x in weights]
    scores, comp = np.zeros((rows, 3)), np.zeros((rows, 10), np.int32)
    reward, key = np.zeros(rows), np.full(rows, -1, np.int32)
    length, tf = np.zeros(rows, np.int32), np.zeros((rows, L + 2), np.int64)
    for r in range(rows):
        b = r // rows_per_scene
        key[r] = SC.key_row(np.reshape(dataset_idx, -1)[b], np.reshape(object_id, -1)[b], key_table, corpus.nkeys)
        cap, length[r], tf[r] = SC.caption_row(tokens[r], sos, eos)
        if key[r] < 0:
            continue
        refs = corpus.refs[int(key[r])]
        if w[0] != 0:
            scores[r, 0] = corpus.cider(cap, int(key[r]))
        if w[1] != 0:
            comp[r] = bleu_components(cap, refs)
            scores[r, 1] = bleu4(comp[r])
        if w[2] != 0:
            scores[r, 2] = rouge(cap, refs)
        reward[r] = combine(scores[r], w)
    return MixRewards(reward, scores, comp, key, length, tf)


def combine(scores, weights):
    """((w_cider cider) + (w_bleu bleu4)) + (w_rouge rouge), float64, a zero weight adding +0.0; ``scores`` (..., 3)"""
    s = np.asarray(scores, F64)
    t = [F64(w) * s[..., i] if w != 0 else np.zeros(s.shape[:-1]) for i, w in enumerate(weights)]
    return (t[0] + t[1]) + t[2]


# ---- the mixed loss --------------------------------------------------------------------------------------------------------
MixLoss = collections.namedtuple("MixLoss", "loss l_rl l_xe acc_rl acc_xe dlogits rl xe labs inv_rl inv_xe n_good")


def loss(logits, lang_ids, good, words, length, reward, baseline, count, S, w_xe, gout=1.0, xe_positions=None):
    """Everything spacap_mixed_cap_loss_fwd_f32 / _bwd_f32 return, in float64.  ``logits`` (B0 + R, W, V) with B0 =
    len(``lang_ids``) (None: 0), ``xe_positions`` = W0 (None: W); ``rl`` is ``self_critical_restated.loss`` of the sample rows,
    ``xe`` ``losses_restated.caption`` of the ground-truth rows' W0 positions (None without any); ``labs`` the scale the loss's
    rounding errors are measured against."""
    logits = np.asarray(logits)
    B0 = 0 if lang_ids is None else len(lang_ids)
    rl = SC.loss(logits[B0:], words, length, reward, baseline, count, S, gout)
    W0 = logits.shape[1] if xe_positions is None else int(xe_positions)
    xe = LR.caption(LR.CapInputs(logits[:B0, :W0], np.asarray(lang_ids), np.asarray(good).astype(bool)), 1.0) if B0 else None
    return _compose(rl, xe, None if xe is None else int(np.asarray(good).astype(bool).sum()), w_xe, gout)


def _compose(rl, xe, n_good, w_xe, gout):
    """``rl`` = self_critical_restated.loss of the sample rows at upstream ``gout``, ``xe`` = losses_restated.caption of the
    ground-truth rows at upstream 1 (None: no such rows)"""
    if xe is None:
        return MixLoss(rl.loss, rl.loss, 0.0, rl.acc, 0.0, rl.dlogits, rl, None, rl.labs, rl.inv_den, 1.0 / LR._den(0.0), 0)
    l_xe, W0, W = float(xe.loss), xe.dlogits.shape[1], rl.dlogits.shape[1]
    d = np.concatenate([np.pad((gout * w_xe) * xe.dlogits, ((0, 0), (0, W - W0), (0, 0))), rl.dlogits], 0)
    # (the cross-entropy is a sum of terms of one sign: its own scale)
    return MixLoss(rl.loss + w_xe * l_xe, rl.loss, l_xe, rl.acc, float(xe.acc), d, rl, xe, rl.labs + w_xe * abs(l_xe), rl.inv_den,
                   1.0 / LR._den(float(n_good * W0)), n_good)


# ---- the loss cases of tests/test_reward_mix_gpu.py --------------------------------------------------------------------------
# (B0, R, S, W, V): self_critical_restated.LOSS_SHAPES with B0 ground-truth rows in front -- V on both sides of the 256-thread
# stride, 65 + 130 rows (more than the 64 lanes of the final kernel on either side), and B0 = 0.
LOSS_SHAPES = ((3, 9, 3, 5, 2), (2, 6, 2, 7, 255), (3, 9, 3, 5, 256), (3, 9, 3, 7, 257), (2, 6, 2, 31, 1000), (3, 15, 5, 31, 3001),
               (65, 130, 2, 3, 255), (0, 9, 3, 5, 256))
MODES = ("all", "some", "none")
W_XE = (0.0, 0.5, 1.0)
MixCase = collections.namedtuple("MixCase", "B0 R S W V good count w_xe baseline")
LOSS_CASES = tuple(MixCase(*s, g, c, w, b) for s in LOSS_SHAPES for g in MODES for c in MODES for w in W_XE
                   for b in ("greedy", "samples"))
MixInputs = collections.namedtuple("MixInputs", "logits lang_ids good words length reward baseline count")
LOSS_UPSTREAM = SC.LOSS_UPSTREAM


def _pick(mode, n):
    return {"all": np.ones(n, bool), "some": np.arange(n) % 2 == 0, "none": np.zeros(n, bool)}[mode]


@functools.lru_cache(maxsize=None)
def _shape_inputs(B0, Rn, S, W, V):
    """The arrays of a shape that do not depend on good / count / w_xe / baseline, built once.  The sample rows are
    self_critical_restated.loss_inputs' (lengths 1 and W, planted arg-max ties, word ids V and 2^40 + 7, a scene of advantage
    exactly 0); the ground-truth rows carry targets with interior pad ids, a full row and a row of one word, ids V and 2^40 + 7,
    planted ties whose target is the first tied column, and a planted hit."""
    x = SC.loss_inputs(SC.LossCase(Rn, S, W, V, "all", "greedy"))
    rng = np.random.default_rng(9000 + 17 * B0 + 3 * W + V)
    head = rng.normal(0.0, 3.0, (B0, W, V)).astype(F32)
    ids = np.zeros((B0, W + 2), np.int64)              # W + 1 is the least width; one more column is never read
    if B0:
        ids[:, 0] = min(2, V - 1)
        for b in range(B0):
            n = W if b == 0 else (1 if b == 1 else int(rng.integers(1, W + 1)))
            ids[b, 1:1 + n] = rng.integers(1, V, n)    # word ids; 0 pads the rest
        ids[:, W + 1] = 1                              # (behind the W targets: must not be read as one)
        if W >= 3:
            ids[0, 2] = 0                              # an interior pad id: ignored, the words behind it still count
        top = lambda b, t: F32(head[b, t].max() + F32(2.0))
        head[0, 0, ids[0, 1]] = top(0, 0)              # the maximum at the target: a hit
        for t, cols, first in LR.cap_ties(V):          # equal maxima: the first index is the arg-max
            if t < W and not (t == 1 and W >= 3):      # (position 1 holds the interior pad)
                head[0, t, list(cols)] = top(0, t)
                ids[0, t + 1] = first
        last = B0 - 1
        ids[last, 1] = V                               # out of range: ignored like the pad id
        if W > 1:
            ids[last, 2] = LR.CAP_FAR_ID
    logits = np.concatenate([head, x.logits], 0)
    for a in (logits, ids):
        a.setflags(write=False)
    return logits, ids, x


@functools.lru_cache(maxsize=None)
def loss_inputs(case):
    logits, ids, x = _shape_inputs(case.B0, case.R, case.S, case.W, case.V)
    out = MixInputs(logits, ids if case.B0 else None, _pick(case.good, case.B0), x.words, x.length, x.reward,
                    x.baseline if case.baseline == "greedy" else None, _pick(case.count, case.R // case.S))
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


# The two parts of a case's reference depend on few of its fields -- the sample rows' on (shape, count, baseline), the
# ground-truth rows' on (shape, good) -- and are shared among the cases that agree in them, never modified.  The caches are
# small: LOSS_CASES runs shape by shape, and the float64 images of the large shapes are not kept.
@functools.lru_cache(maxsize=8)
def _rl_part(shape, count, baseline):
    B0, Rn, S = shape[:3]
    x = loss_inputs(MixCase(*shape, "all", count, 0.0, baseline))
    return SC.loss(x.logits[B0:], x.words, x.length, x.reward, x.baseline, x.count, S, LOSS_UPSTREAM)


@functools.lru_cache(maxsize=4)
def _xe_part(shape, good):
    B0 = shape[0]
    x = loss_inputs(MixCase(*shape, good, "all", 0.0, "greedy"))
    return LR.caption(LR.CapInputs(x.logits[:B0], x.lang_ids, x.good), 1.0) if B0 else None


def loss_reference(case):
    shape = tuple(case[:5])
    return _compose(_rl_part(shape, case.count, case.baseline), _xe_part(shape, case.good), int(_pick(case.good, case.B0).sum()),
                    case.w_xe, LOSS_UPSTREAM)


# ---- the reward rows of the fixture and of the two test modules --------------------------------------------------------------
ROW_SETS = (("edge", "edge", False), ("edge_extra", "edge", True), ("random", "random", False), ("random_extra", "random", True))

# Hand-made rows on the `edge` corpus, for what the rows built back from its candidates may miss: (decoded words, key).  Words
# a .. f are ids 10 .. 15 (tests/golden/make_fixtures_caption.py: edge_case).
HAND_ROWS = (
    ((10, 11, 12, 13, R.EOS), 3),          # six tokens against references of 5 and 7: a tie in the closest length (5 wins)
    ((10, 10, 10, 10, R.EOS), 4),          # a a a a against a a: unigram and bigram counts clipped
    ((R.EOS,), 1),                         # sos eos: guess[2] = guess[3] = 0
    ((10, 11, R.EOS), 1),                  # shorter than every reference: brevity penalty
    ((14, 13, 12, 11, 10, R.EOS), 14),     # reordered: ROUGE strictly between 0 and 1
    ((10, 11, 12), -1),                    # no key row
)


def hand_rows(fix):
    """(tokens (rows, 62), dataset_idx, object_id, key_table, want_key) of HAND_ROWS: junk words (never eos) behind the eos"""
    nkeys, vocab = len(fix["edge/cand_len"]), int(fix["edge/vocab"])
    rng = np.random.default_rng(77)
    tokens = np.stack([np.asarray(list(w) + [int(j) for j in rng.integers(4, vocab, SC.L_WORDS - len(w))], np.int64) for w, _ in HAND_ROWS])
    n_obj = (nkeys + 1) // 2 + 1
    table = np.full((2, n_obj), -1, np.int32)
    for k in range(nkeys):
        table[k % 2, k // 2] = k
    want = np.asarray([k for _, k in HAND_ROWS], np.int32)
    didx = np.where(want >= 0, want % 2, 0).astype(np.int64)
    oid = np.where(want >= 0, want // 2, n_obj - 1).astype(np.int64)               # behind a -1 entry
    return tokens, didx, oid, table, want


def row_set(fix, name):
    """(tokens, dataset_idx, object_id, key_table, want_key, case) of a recorded row set: ROW_SETS' rows are
    ``self_critical_restated.fixture_rows``', the rows tests/test_self_critical_cpu.py builds; ``hand`` are HAND_ROWS."""
    if name == "hand":
        return hand_rows(fix) + ("edge",)
    case, extra = {n: (c, e) for n, c, e in ROW_SETS}[name]
    return SC.fixture_rows(fix, case, extra=extra)[:5] + (case,)


ROW_SET_NAMES = tuple(n for n, _, _ in ROW_SETS) + ("hand",)
