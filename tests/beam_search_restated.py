"""The beam-search contract, restated in plain numpy float64 with no shortcut: every candidate of every
hypothesis is enumerated and sorted.  Not a test module; tests/test_beam_search*.py compare the kernels of
csrc/caption_decode.hip and spacap3d_amd/beam_search.py against it.

Each sequence keeps W hypotheses (score, last word, finished, length); at the start hypothesis 0 has score 0 and the others
-inf (dead).  One selection: a live unfinished hypothesis j offers (score_j + logp_j[v], j, v) for EVERY word v, a finished one
exactly (score_j, j, eos), a dead one nothing; the W best are kept in the order score descending, then smaller j, then smaller
v.  A kept hypothesis is finished when its parent was or v == eos; its length is the parent's plus one unless the parent was
finished.  After n_words selections the winner maximises score / length ** alpha (alpha = 0: the score), the smaller slot on
ties; the tokens come from backtracking the (parent, word) trace, so eos repeats after the first eos."""
import numpy as np


def beam_search_restated(step_logp, R, W, n_words, sos, eos, alpha=0.0):
    """``step_logp(s, r, j, last_word, tokens)`` -> the (V,) log-probabilities of word s of hypothesis j of sequence r, whose
    newest word is ``last_word`` (``sos`` at s = 0) and whose words so far are ``tokens``.  Returns a dict of numpy arrays:
    ys (R, n_words), score (R,), beams (R, W, n_words), scores (R, W), lengths (R, W), finished (R, W), parent / word
    (n_words, R, W) and gap (n_words, R) = the W-th kept score minus the best one not kept (inf when there is none)."""
    out = {"ys": np.zeros((R, n_words), np.int64), "score": np.zeros(R), "beams": np.zeros((R, W, n_words), np.int64),
           "scores": np.zeros((R, W)), "lengths": np.zeros((R, W), np.int64), "finished": np.zeros((R, W), bool),
           "parent": np.zeros((n_words, R, W), np.int64), "word": np.zeros((n_words, R, W), np.int64),
           "gap": np.full((n_words, R), np.inf)}
    for r in range(R):
        hyps = [{"score": 0.0 if j == 0 else -np.inf, "word": sos, "fin": False, "len": 0, "toks": []} for j in range(W)]
        for s in range(n_words):
            cands = []
            for j, h in enumerate(hyps):
                if h["score"] == -np.inf:
                    continue
                if h["fin"]:
                    cands.append((h["score"], j, eos))
                    continue
                lp = np.asarray(step_logp(s, r, j, h["word"], list(h["toks"])), np.float64)
                cands.extend((h["score"] + float(lp[v]), j, v) for v in range(lp.shape[0]))
            cands.sort(key=lambda c: (-c[0], c[1], c[2]))
            assert len(cands) >= W
            if len(cands) > W:
                out["gap"][s, r] = cands[W - 1][0] - cands[W][0]
            new = []
            for w, (sc, j, v) in enumerate(cands[:W]):
                p = hyps[j]
                new.append({"score": sc, "word": v, "fin": p["fin"] or v == eos, "len": p["len"] + (0 if p["fin"] else 1),
                            "toks": p["toks"] + [v]})
                out["parent"][s, r, w], out["word"][s, r, w] = j, v
            hyps = new
        norm = [h["score"] if alpha == 0.0 else h["score"] / float(max(h["len"], 1)) ** alpha for h in hyps]
        best = max(range(W), key=lambda w: (norm[w], -w))
        for w, h in enumerate(hyps):
            # backtracking the trace gives the same words as the lists carried along
            slot, toks = w, []
            for s in range(n_words - 1, -1, -1):
                toks.append(out["word"][s, r, slot])
                slot = out["parent"][s, r, slot]
            assert toks[::-1] == h["toks"]
            out["beams"][r, w], out["scores"][r, w], out["lengths"][r, w], out["finished"][r, w] = h["toks"], h["score"], h["len"], h["fin"]
        out["ys"][r], out["score"][r] = hyps[best]["toks"], hyps[best]["score"]
    return out
