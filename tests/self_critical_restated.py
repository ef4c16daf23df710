"""Self-critical caption training restated in numpy float64: the specification the kernels of
csrc/caption_reward.hip and csrc/scst_loss.hip and ``TransformerDecoderModel._self_critical_train`` are held to.  The
reference has no self-critical training; these semantics are the project's own.  Not a test module:
tests/test_self_critical_cpu.py anchors the rewards to the reference's recorded CIDEr (tests/golden/caption_eval_ref.npz) and
the gradient to a central difference, tests/test_self_critical_gpu.py runs the tables below through the kernels.

Rows.  A batch has B scenes with one referred object each and S samples per scene; row r = b S + s.  The scene's corpus key row
is key_table[dataset_idx[b]][object_id[b]]; an index outside its table or an entry outside 0..nkeys-1 gives no row.  Scene b
counts (c_b = 1) when its matched proposal is good and it has a key row.

Caption of a row: sos, the decoded words through the first eos, an eos appended when there was none (decode_caption).
length_r = the decoded words through the first eos (n_words: none).  tf_tok = sos, those words, zeros behind them, n_words + 2
columns.

Reward R_r: CIDEr-D (n = 4, sigma = 6, x 10, / references) of the caption against the references of the scene's key row with
the corpus' document frequencies; 0 without a key row.

Advantage (float64, rounded to float32 once): A_r = c_b (R_r - base_b) with base_b the greedy caption's reward, or
A_r = c_b (R_r - sum_{s' != s} R_{b,s'} / (S - 1)).

Loss = - sum_r A_r sum_{t < length_r} logp[r, t, w_rt] / (sum_r c_b length_r + 1e-6), logp the log-softmax of the teacher-forced
logits; a word id outside [0, V) contributes nothing.  Gradient: g (-A_r inv_den) ([v == w_rt] - softmax) for t < length_r,
zero elsewhere.  Reported with it: the share of counted positions (c_b, t < length_r) whose first arg-max is the drawn word, the
mean reward and mean baseline over the counting rows, and per row sum_{t < length} logp."""
import collections
import functools

import numpy as np

import caption_eval_restated as R
import losses_restated as LR

F32, F64 = np.float32, np.float64
FAR_ID = LR.CAP_FAR_ID


# ---- rows, captions, rewards -----------------------------------------------------------------------------------------------
def key_row(dataset_idx, object_id, key_table, nkeys):
    """the key row of a scene, or -1 (caption_row's rule, csrc/caption_eval.hip)"""
    item, oid = int(dataset_idx), int(object_id)
    if not (0 <= item < key_table.shape[0] and 0 <= oid < key_table.shape[1]):
        return -1
    row = int(key_table[item, oid])
    return row if 0 <= row < nkeys else -1


def caption_row(tokens, sos, eos):
    """(caption, length, tf_tok) of one row of decoded words"""
    n = len(tokens)
    cap = R.decode(tokens, sos, eos)
    hit = [i for i, t in enumerate(tokens) if int(t) == eos]
    length = hit[0] + 1 if hit else n
    tf = np.zeros(n + 2, np.int64)
    tf[0] = sos
    tf[1:1 + length] = [int(t) for t in tokens[:length]]
    return cap, length, tf


class Corpus:
    """The references per key row with their document frequencies, computed once."""

    def __init__(self, refs_per_key):
        self.refs = refs_per_key
        self.nkeys = len(refs_per_key)
        self.df = R.doc_freq(refs_per_key)
        self.log_nkeys = np.log(float(self.nkeys))
        self._vec = {}

    def vec_of(self, s):
        """cider_scorer.py's counts2vec: per n the tf-idf vector, its norm, and `length` = the number of bigrams"""
        vec, norm, length = [{} for _ in range(4)], [0.0] * 4, 0
        for g, tf in R.ngrams(s).items():
            n = len(g) - 1
            vec[n][g] = float(tf) * (self.log_nkeys - np.log(max(1.0, self.df.get(g, 0.0))))
            norm[n] += pow(vec[n][g], 2)
            if n == 1:
                length += tf
        return vec, [np.sqrt(x) for x in norm], length

    def ref_vecs(self, key):
        if key not in self._vec:
            self._vec[key] = [self.vec_of(r) for r in self.refs[key]]
        return self._vec[key]

    def cider(self, cand, key, sigma=6.0):
        """CIDEr-D x 10 of one caption against the references of key row ``key`` (caption_eval_restated.cider for one candidate)"""
        vh, nh, lh = self.vec_of(cand)
        score = np.zeros(4)
        refs = self.ref_vecs(key)
        for vr, nr, lr in refs:
            delta = float(lh - lr)
            val = np.zeros(4)
            for n in range(4):
                for g, x in vh[n].items():
                    y = vr[n].get(g, 0.0)
                    val[n] += min(x, y) * y
                if nh[n] != 0 and nr[n] != 0:
                    val[n] /= nh[n] * nr[n]
                val[n] *= np.e ** (-(delta ** 2) / (2 * sigma ** 2))
            score += val
        s = np.mean(score)
        if refs:
            s /= len(refs)
        return s * 10.0


Rewards = collections.namedtuple("Rewards", "cider key length tf_tok")


def rewards(corpus, tokens, rows_per_scene, dataset_idx, object_id, key_table, sos, eos):
    """what spacap_caption_reward_f64 writes for ``tokens`` (rows, L)"""
    tokens = np.asarray(tokens)
    rows, L = tokens.shape
    cider, key = np.zeros(rows), np.full(rows, -1, np.int32)
    length, tf = np.zeros(rows, np.int32), np.zeros((rows, L + 2), np.int64)
    for r in range(rows):
        b = r // rows_per_scene
        key[r] = key_row(np.reshape(dataset_idx, -1)[b], np.reshape(object_id, -1)[b], key_table, corpus.nkeys)
        cap, length[r], tf[r] = caption_row(tokens[r], sos, eos)
        if key[r] >= 0:
            cider[r] = corpus.cider(cap, int(key[r]))
    return Rewards(cider, key, length, tf)


# ---- advantage and loss ----------------------------------------------------------------------------------------------------
def advantage(reward, baseline, count, S):
    """(A float64 (R,), base float64 (R,)): ``baseline`` (B,) or None for leave-one-out"""
    reward = np.asarray(reward, F64)
    B = len(reward) // S
    r2 = reward.reshape(B, S)
    if baseline is None:
        base = np.empty((B, S))
        for s in range(S):
            o = np.zeros(B)
            for s2 in range(S):          # in sample order, as the kernel adds them
                if s2 != s:
                    o = o + r2[:, s2]
            base[:, s] = o / float(S - 1)
    else:
        base = np.repeat(np.asarray(baseline, F64)[:, None], S, 1)
    c = np.asarray(count).astype(bool)[:, None]
    return np.where(c, r2 - base, 0.0).reshape(-1), base.reshape(-1)


LossRef = collections.namedtuple("LossRef", "loss acc adv adv32 rowlogp dlogits labs inv_den n_scenes mean_reward mean_baseline logp")


def loss(logits, words, length, reward, baseline, count, S, gout=1.0):
    """Everything spacap_scst_loss_fwd_f32 / _bwd_f32 return, in float64 on the given logits (any float dtype).  ``labs`` is the
    loss with |A_r| in place of A_r and |logp|: the scale its rounding errors are measured against (the signed sum cancels)."""
    s = np.asarray(logits, F64)
    Rn, W, V = s.shape
    words = np.asarray(words, np.int64)
    length = np.clip(np.asarray(length, np.int64), 0, W)
    cnt = np.repeat(np.asarray(count).astype(bool), S)
    A64, base = advantage(reward, baseline, count, S)
    A = A64.astype(F32).astype(F64)                              # rounded to float32 once
    m = s.max(-1, keepdims=True)
    lse = m + np.log(np.exp(s - m).sum(-1, keepdims=True))
    logp_all = s - lse
    ok = (words >= 0) & (words < V)
    w = np.where(ok, words, 0)
    lp = np.where(ok, np.take_along_axis(logp_all, w[..., None], -1)[..., 0], 0.0)          # (R, W)
    live = np.arange(W)[None, :] < length[:, None]
    rowlogp = (lp * live).sum(1)
    den = LR._den(float((length * cnt).sum()))
    value = -(A * rowlogp).sum() / den
    labs = (np.abs(A) * (np.abs(lp) * live).sum(1)).sum() / den
    counted = live & cnt[:, None]
    hits = (np.asarray(logits).argmax(-1) == words) & counted                               # first maximum, in the logits' own dtype
    acc = hits.sum() / max(float(counted.sum()), 1.0)
    coef = gout * (-A / den)
    onehot = np.zeros_like(s)
    np.put_along_axis(onehot, w[..., None], ok[..., None].astype(F64), -1)
    d = coef[:, None, None] * (onehot - np.exp(logp_all)) * (live & ok)[..., None]
    nrow = max(int(cnt.sum()), 1)
    return LossRef(value, acc, A64, A, rowlogp, d, labs, 1.0 / den, int(cnt.sum()) // S,
                   float((np.asarray(reward, F64) * cnt).sum() / nrow), float((base * cnt).sum() / nrow), lp)


# ---- the loss cases of tests/test_self_critical_gpu.py ---------------------------------------------------------------------
# (R, S, W, V): V on both sides of the 256-thread stride of scst_rows_kernel / scst_bwd_kernel, three scenes or more (one that
# counts with advantages, one that may not count, one whose samples all equal the baseline), and 130 rows: more than the 64
# lanes of scst_final_kernel.
LOSS_SHAPES = ((9, 3, 5, 2), (6, 2, 7, 255), (9, 3, 5, 256), (9, 3, 7, 257), (6, 2, 31, 1000), (15, 5, 31, 3001), (130, 2, 3, 255))
LossCase = collections.namedtuple("LossCase", "R S W V count baseline")
LOSS_CASES = tuple(LossCase(*s, c, b) for s in LOSS_SHAPES for c in ("all", "some", "none") for b in ("greedy", "samples"))
LossInputs = collections.namedtuple("LossInputs", "logits words length reward baseline count")
LOSS_UPSTREAM = 1.7
ZERO_SCENE = 2        # the scene whose samples all equal the baseline: advantage exactly 0


@functools.lru_cache(maxsize=None)
def loss_inputs(case):
    Rn, S, W, V = case.R, case.S, case.W, case.V
    B = Rn // S
    rng = np.random.default_rng(7000 + 13 * Rn + 3 * W + V)
    logits = rng.normal(0.0, 3.0, (Rn, W, V)).astype(F32)
    words = rng.integers(0, V, (Rn, W))
    length = rng.integers(1, W + 1, Rn)
    length[0], length[1], length[Rn - 1] = 1, W, W                # the shortest, the longest
    top = lambda r, t: F32(logits[r, t].max() + F32(2.0))
    logits[0, 0, words[0, 0]] = top(0, 0)                          # the maximum at the drawn word: a hit
    for t, cols, first in LR.cap_ties(V):                          # equal maxima: the first index is the arg-max
        if t < W:
            logits[1, t, list(cols)] = top(1, t)
            words[1, t] = first
    words[Rn - 1, 0] = V                                           # out of range: contributes nothing
    if W > 1:
        words[Rn - 1, 1] = FAR_ID
    reward = rng.uniform(0.0, 3.0, Rn)
    baseline = rng.uniform(0.0, 3.0, B)
    reward[ZERO_SCENE * S:(ZERO_SCENE + 1) * S] = 1.25             # equal samples: the leave-one-out mean is 1.25 exactly
    baseline[ZERO_SCENE] = 1.25
    count = {"all": np.ones(B, bool), "some": np.arange(B) % 2 == 0, "none": np.zeros(B, bool)}[case.count]
    out = LossInputs(logits, words.astype(np.int64), length.astype(np.int32), reward, baseline if case.baseline == "greedy" else None,
                     count)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def loss_reference(case):
    x = loss_inputs(case)
    return loss(x.logits, x.words, x.length, x.reward, x.baseline, x.count, case.S, LOSS_UPSTREAM)


# ---- the reward rows of the two test modules ---------------------------------------------------------------------------------
L_WORDS = 62          # decoded words per row: L + 2 = 64 tokens, the kernels' most


def raw_row(cand, rng, vocab, eos):
    """A candidate of the fixture (sos ... eos, up to 64 tokens) turned back into L_WORDS decoded words: the candidate without its
    sos, ending with its eos when that fits, junk words (never eos) behind the eos."""
    body = [int(t) for t in cand[1:]]
    if len(body) > L_WORDS:
        body = body[:L_WORDS]                    # the 64-token candidate: 62 words, its eos is the one decode_caption appends
        assert eos not in body
    junk = rng.integers(4, vocab, L_WORDS - len(body))
    return np.asarray(body + [int(j) for j in junk], np.int64)


def fixture_rows(fix, case, extra=False):
    """(tokens (rows, 62), dataset_idx, object_id, key_table, want_key, perm): row i carries candidate perm[i] of the fixture case
    and is pointed at that candidate's key.  ``extra``: every key is used 0 to 3 times, some rows get an object id outside the
    table or one behind a -1 entry (under a quarter of the rows), one row starts with eos (the placeholder [sos, eos])."""
    cand_tok, cand_len = fix[f"{case}/cand_tok"], fix[f"{case}/cand_len"]
    nkeys, vocab = len(cand_len), int(fix[f"{case}/vocab"])
    rng = np.random.default_rng(100 + nkeys)
    perm = rng.permutation(nkeys)
    if extra:
        uses = rng.integers(0, 4, nkeys)
        uses[cand_len == cand_len.max()] |= 1    # the longest candidate (edge: 64 tokens) is among the rows
        ph = int(np.flatnonzero(cand_len == 2)[0])
        uses[ph] = min(uses[ph], 2)              # (the placeholder's key gets one more row below)
        perm = np.concatenate([np.repeat(np.arange(nkeys), uses), [ph]])
        rng.shuffle(perm[:-1])
    rows = len(perm)
    tokens = np.stack([raw_row(cand_tok[k, :cand_len[k]], rng, vocab, R.EOS) for k in perm])
    # the key table: two dataset items; item 0 holds the even keys at column key // 2, item 1 the odd ones; column n_obj - 1 is -1
    n_obj = (nkeys + 1) // 2 + 1
    table = np.full((2, n_obj), -1, np.int32)
    for k in range(nkeys):
        table[k % 2, k // 2] = k
    didx, oid, want = perm % 2, perm // 2, perm.astype(np.int32).copy()
    if extra:
        lost = rng.permutation(rows - 1)[:max(2, rows // 6)]
        for j, r in enumerate(lost):
            want[r] = -1
            if j % 4 == 0:
                oid[r] = n_obj - 1               # behind a -1 entry
            elif j % 4 == 1:
                oid[r] = n_obj + 3               # outside the table
            elif j % 4 == 2:
                oid[r] = -1
            else:
                didx[r] = 2                      # no such dataset item
    return tokens, didx.astype(np.int64), oid.astype(np.int64), table, want, perm
