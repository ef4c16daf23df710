"""Numpy / plain-Python restatement over word IDS of what spacap3d_amd/caption_eval.py computes on the device: the
candidate selection of feed_scene_cap (lib/eval_helper.py:178-222 with decode_caption and check_candidates), the BLEU
components (bleu_scorer.py:60-84), ROUGE-L (rouge.py:45-75) and CIDEr-D (cider_scorer.py:93-181).  Sentences are int
sequences; a reference word outside the vocabulary is any id the candidates never use.  Sums run in the reference's own
order (dicts keep insertion order), so the values are the reference's to the last bit or two.
tests/golden/make_fixtures_caption.py asserts that against the reference's recorded output."""
import math

import numpy as np

LMAX = 64


def decode(tokens, sos, eos):
    out = [sos]
    for t in tokens:
        out.append(int(t))
        if int(t) == eos:
            break
    if eos not in out:
        out.append(eos)
    return out


def new_table(nkeys, sos, eos):
    tok = np.zeros((nkeys, LMAX), np.int32)
    tok[:, 0], tok[:, 1] = sos, eos
    return tok, np.full(nkeys, 2, np.int32)


def select(table, tokens, nms_masks, good, dataset_idx, scene_object_ids, object_assignment, key_table, sos, eos):
    """One batch in the reference's loop order; ``table`` = (cand_tok, cand_len) updated in place (last write wins)."""
    tok, ln = table
    B, K = nms_masks.shape
    for b in range(B):
        item = int(np.reshape(dataset_idx, -1)[b])
        for k in range(K):
            if nms_masks[b, k] != 1 or not good[b, k]:
                continue
            oa = int(object_assignment[b, k])
            if not (0 <= item < key_table.shape[0] and 0 <= oa < scene_object_ids.shape[1]):
                continue
            oid = int(scene_object_ids[b, oa])
            row = int(key_table[item, oid]) if 0 <= oid < key_table.shape[1] else -1
            if row < 0:
                continue
            cap = decode(tokens[b, k], sos, eos)
            tok[row] = 0
            tok[row, :len(cap)] = cap
            ln[row] = len(cap)
    return table


def ngrams(s):
    """n-gram -> count for n = 1..4, in the insertion order of precook (by n, then by position)."""
    c = {}
    for n in range(1, 5):
        for i in range(len(s) - n + 1):
            g = tuple(int(x) for x in s[i:i + n])
            c[g] = c.get(g, 0) + 1
    return c


def bleu_components(cand, refs):
    """(testlen, reflen, guess[4], correct[4]) as ten ints; reflen = the closest length, ties to the shorter."""
    testlen = len(cand)
    reflen = min((abs(len(r) - testlen), len(r)) for r in refs)[1]
    maxc = {}
    for r in refs:
        for g, c in ngrams(r).items():
            maxc[g] = max(maxc.get(g, 0), c)
    correct = [0] * 4
    for g, c in ngrams(cand).items():
        correct[len(g) - 1] += min(maxc.get(g, 0), c)
    return [testlen, reflen] + [max(0, testlen - n) for n in range(4)] + correct


def corpus_bleu(totals):
    testlen, reflen, guess, correct = totals[0], totals[1], totals[2:6], totals[6:10]
    out, prod = [], 1.0
    for k in range(4):
        prod *= float(correct[k] + 1e-15) / (guess[k] + 1e-9)
        out.append(prod ** (1.0 / (k + 1)))
    ratio = (testlen + 1e-15) / (reflen + 1e-9)
    if ratio < 1:
        out = [b * math.exp(1 - 1 / ratio) for b in out]
    return out


def lcs(a, b):
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[-1]


def rouge(cand, refs, beta=1.2):
    prec = max(lcs(r, cand) / float(len(cand)) for r in refs)
    rec = max(lcs(r, cand) / float(len(r)) for r in refs)
    if prec != 0 and rec != 0:
        return ((1 + beta ** 2) * prec * rec) / float(rec + beta ** 2 * prec)
    return 0.0


def doc_freq(refs_per_key):
    df = {}
    for refs in refs_per_key:
        for g in set(g for r in refs for g in ngrams(r)):
            df[g] = df.get(g, 0) + 1
    return df


def cider(cands, refs_per_key, sigma=6.0):
    """Per-key CIDEr-D scores (x 10), the reference's ``length`` quirk (the number of bigrams) included."""
    df = doc_freq(refs_per_key)
    ref_len = np.log(float(len(refs_per_key)))

    def vec_of(s):
        vec, norm, length = [{} for _ in range(4)], [0.0] * 4, 0
        for g, tf in ngrams(s).items():
            n = len(g) - 1
            vec[n][g] = float(tf) * (ref_len - np.log(max(1.0, df.get(g, 0.0))))
            norm[n] += pow(vec[n][g], 2)
            if n == 1:
                length += tf
        return vec, [np.sqrt(x) for x in norm], length

    out = []
    for cand, refs in zip(cands, refs_per_key):
        vh, nh, lh = vec_of(cand)
        score = np.zeros(4)
        for r in refs:
            vr, nr, lr = vec_of(r)
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
        s /= len(refs)
        s *= 10.0
        out.append(s)
    return np.array(out)


def score_all(cand_tok, cand_len, refs_per_key):
    """-> dict with bleu_comp i64 (NKEYS,10), bleu [4], rouge_scores, rouge, cider_scores, cider."""
    cands = [[int(t) for t in cand_tok[i, :cand_len[i]]] for i in range(len(cand_len))]
    comp = np.array([bleu_components(c, r) for c, r in zip(cands, refs_per_key)], np.int64)
    rg = np.array([rouge(c, r) for c, r in zip(cands, refs_per_key)])
    cd = cider(cands, refs_per_key)
    return {"bleu_comp": comp, "bleu": corpus_bleu([int(x) for x in comp.sum(0)]), "rouge_scores": rg,
            "rouge": float(np.mean(rg)), "cider_scores": cd, "cider": float(np.mean(cd))}


# ---- the fixture's id <-> word convention --------------------------------------------------------------------------------
SPECIAL = {0: "pad_", 1: "unk", 2: "sos", 3: "eos"}
UNK, SOS, EOS = 1, 2, 3


def word(i):
    """ids 0..3 are pad_ / unk / sos / eos, every other id i is the word ``w<i>`` (ids >= the vocabulary size: words
    outside the vocabulary)."""
    return SPECIAL.get(int(i), "w%d" % int(i))


def vocabulary(V):
    return {word(i): i for i in range(V)}


def sentence(ids):
    return " ".join(word(i) for i in ids)


def refs_of(fix, case):
    """The references of a fixture case as lists of id lists per key."""
    tok, ln, nref = fix[f"{case}/ref_tok"], fix[f"{case}/ref_len"], fix[f"{case}/key_nref"]
    out, r, o = [], 0, 0
    for n in nref:
        cur = []
        for _ in range(int(n)):
            cur.append([int(t) for t in tok[o:o + ln[r]]])
            o += int(ln[r])
            r += 1
        out.append(cur)
    return out
