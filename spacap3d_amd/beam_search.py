"""Beam search over any step function: the generic path beside ``caption_decode.beam_decode`` (late guide, other head counts,
the CPU oracle backend).  The reference decodes greedily only (models/transformer_captioner.py:402-453); the semantics are
the project's own and ``tests/beam_search_restated.py`` restates them:

Each of R sequences keeps W hypotheses (score, last word, finished, length); before the first selection hypothesis 0 has
score 0 and the others -inf (dead).  A selection offers ``score_j + logp_j[v]`` for every word v of every live unfinished
hypothesis j, exactly one ``(score_j, j, eos)`` for a finished j and nothing for a dead j, and keeps the W best: score
descending, then the smaller j, then the smaller v.  A new hypothesis is finished when its parent was or v == eos; its length
is the parent's plus one unless the parent was finished.  After ``n_words`` selections the winner maximises
``score / length ** length_penalty`` (0: the score), the smaller slot on ties; its words come from backtracking, eos
repeating after the first eos.
"""
import torch

NEG_INF = float("-inf")


def select_top(cand, W):
    """The W best entries of every row of ``cand`` (R, N): values descending, equal values in ascending index order.
    ``torch.topk`` gives the values; it does not promise an order among equal ones, so the indices are found explicitly:
    slot i takes the (n + 1)-th entry equal to its value, n = the number of earlier slots holding the same value."""
    vals = torch.topk(cand, W, dim=1).values
    idx = torch.empty(cand.shape[0], W, dtype=torch.long, device=cand.device)
    for i in range(W):
        eq = cand == vals[:, i:i + 1]
        n = (vals[:, :i] == vals[:, i:i + 1]).sum(1, keepdim=True)
        hit = eq & (eq.cumsum(1, dtype=torch.int32) == n + 1)
        idx[:, i] = hit.to(torch.uint8).argmax(1)
    return vals, idx


@torch.no_grad()
def beam_search(step_fn, R, W, n_words, sos, eos, length_penalty=0.0, device=None, constraints=None):
    """``step_fn(s, words, parents)`` returns the (R W, V) log-probabilities of word s of every hypothesis (row r W + w):
    ``words`` (R W,) int64 are the newest words (``sos`` at s = 0) and ``parents`` (R W,) int64 the ROW each hypothesis
    continues (None at s = 0: all W rows of a sequence are the same start) -- a cached decoder reorders its caches with
    ``index_select(0, parents)``.  Returns a dict: ``ys`` (R, n_words) int64 and ``score`` (R,) float32 of the winners,
    ``beams`` (R, W, n_words), ``scores`` (R, W), ``lengths`` (R, W) of all final hypotheses, the trace ``parent`` /
    ``word`` (n_words, R, W) and ``gap`` (n_words, R): the W-th kept score minus the best one not kept (inf when none).
    ``constraints``: a ``decode_constraints.DecodeConstraints``.  ``step_fn`` must then return the
    LOGITS -- the repetition penalty depends on their sign --; they are constrained over each hypothesis' own history, kept
    here through the parent selections, and the log-softmax is taken of the result."""
    from . import decode_constraints as dc
    W, n_words, sos, eos = int(W), int(n_words), int(sos), int(eos)
    cons = dc.resolve(constraints)
    hist = None
    words = torch.full((R * W,), sos, dtype=torch.long, device=device)
    parents = None
    score = fin = length = None
    tr_parent, tr_word, gaps = [], [], []
    for s in range(n_words):
        logp = step_fn(s, words, parents).float()
        dev, V = logp.device, logp.shape[1]
        if W > V:
            raise ValueError(f"beam_search: beam width {W} exceeds the vocabulary size {V}")
        if cons is not None:
            if hist is None:
                cons.check("beam_search", V, n_words, eos)
                hist = torch.zeros(R * W, n_words, dtype=torch.long, device=dev)
            logp = torch.log_softmax(dc.apply(cons, logp, hist, s, eos), 1)
        if score is None:
            score = torch.full((R, W), NEG_INF, dtype=torch.float32, device=dev)
            score[:, 0] = 0.0
            fin = torch.zeros(R, W, dtype=torch.bool, device=dev)
            length = torch.zeros(R, W, dtype=torch.long, device=dev)
        cand = score.unsqueeze(-1) + logp.view(R, W, V)               # a dead hypothesis offers -inf everywhere
        once = torch.full_like(cand, NEG_INF)
        once[..., eos] = score                                        # a finished one: itself, once
        cand = torch.where(fin.unsqueeze(-1), once, cand).view(R, W * V)
        k = min(W + 1, W * V)
        top = torch.topk(cand, k, dim=1).values
        gaps.append(top[:, W - 1] - top[:, W] if k > W else torch.full((R,), float("inf"), device=dev))
        vals, idx = select_top(cand, W)
        parent, word = idx // V, idx % V
        pf = fin.gather(1, parent)
        fin = pf | (word == eos)
        length = length.gather(1, parent) + (~pf).long()
        score = vals
        tr_parent.append(parent)
        tr_word.append(word)
        words = word.reshape(-1)
        parents = (torch.arange(R, device=dev).unsqueeze(1) * W + parent).reshape(-1)
        if hist is not None:
            hist = hist.index_select(0, parents)
            hist[:, s] = words
    alpha = float(length_penalty)
    norm = score.double() if alpha == 0.0 else score.double() / length.clamp(min=1).double() ** alpha
    best = norm.argmax(1, keepdim=True)                               # (the first maximum: the smaller slot on ties)
    beams = torch.empty(R, W, n_words, dtype=torch.long, device=score.device)
    slot = torch.arange(W, device=score.device).unsqueeze(0).expand(R, W)
    for s in range(n_words - 1, -1, -1):
        beams[:, :, s] = tr_word[s].gather(1, slot)
        slot = tr_parent[s].gather(1, slot)
    return {"ys": beams.gather(1, best.unsqueeze(-1).expand(R, 1, n_words)).squeeze(1), "score": score.gather(1, best).squeeze(1),
            "beams": beams, "scores": score, "lengths": length, "parent": torch.stack(tr_parent), "word": torch.stack(tr_word),
            "gap": torch.stack(gaps)}
