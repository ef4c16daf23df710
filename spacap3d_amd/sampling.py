"""Sampled decoding over any step function: the generic path beside ``caption_decode.sample_decode`` (late guide, other head
counts, the CPU oracle backend).  The reference decodes greedily only (models/transformer_captioner.py:402-453); the semantics
are the project's own and ``tests/sampling_restated.py`` restates them:

Row rho = r S + s is sample s of sequence r.  At step i the row draws ``argmax_v z_v``, ``z_v = logit_v * (1 / tau) + g_v``
(the larger z, among equal z the smaller v), with Gumbel noise ``g_v = -log(-log u)``, ``u = ((h >> 9) + 0.5) 2^-23`` and h the
dropout keep mask's hash (csrc/dropout.hpp) of the flat index ``(rho n_words + i) V + v``: the draw is distributed as
``softmax(logit / tau)``.  With ``top_k`` = k >= 1 the candidates are the row's k most probable words (log-probability
descending, the smaller word first) and z is formed from their log-probabilities -- the logits minus one constant per row --
with the noise of their word id.  ``logp = logit_word - logsumexp(logit)`` whatever tau and k are; ``score`` sums it through the
row's first eos, ``length`` is the position of that eos plus one (``n_words``: none), and behind it the row emits eos.

Nucleus sampling, ``top_p`` = p in (0, 1) (``tests/nucleus_restated.py``): with ``q = softmax(logit / tau)`` -- the tempered
distribution -- and ``A_v`` the sum of ``q_u`` over the words with ``logit_u > logit_v``, the mass strictly more probable than v,
the nucleus is ``{v : A_v < p}``.  Words with equal logits enter or stay out together, the most probable word is always in, and
no sort order or tie rule takes part.  The row draws the first maximum of the same ``z_v`` over the nucleus, so a row whose
unrestricted draw lies in its nucleus draws that word; ``logp`` stays the untempered, untruncated one.  ``None`` or 1.0 is the
unrestricted path.  One restriction at a time: ``top_p`` < 1 together with ``top_k`` >= 1 is refused.
"""
import math

import torch

_M32 = 0xFFFFFFFF
_GOLDEN = 0x9E3779B97F4A7C15 - (1 << 64)      # the seed's 64-bit golden-ratio constant as a two's-complement int64


def check_arguments(who, num_samples, temperature, top_k, V=None, top_p=None):
    """The argument rules of every entry to sampled decoding, in one place: S >= 1, tau finite and positive, ``top_k`` in
    0..8 and at most the vocabulary size V (where known), ``top_p`` None or in (0, 1] and below 1 only with ``top_k`` = 0.
    Raises ValueError naming ``who``."""
    if num_samples < 1:
        raise ValueError(f"{who}: num_samples {num_samples} < 1")
    if not (math.isfinite(temperature) and temperature > 0.0):
        raise ValueError(f"{who}: temperature {temperature} must be finite and positive")
    if not 0 <= top_k <= 8 or (V is not None and top_k > V):
        raise ValueError(f"{who}: top_k {top_k} unsupported (0 <= top_k <= 8 and top_k <= vocabulary size{'' if V is None else ' ' + str(V)})")
    if top_p is not None:
        if not 0.0 < top_p <= 1.0:                                 # (NaN fails both compares)
            raise ValueError(f"{who}: top_p {top_p} must lie in (0, 1]")
        if top_p < 1.0 and top_k >= 1:
            raise ValueError(f"{who}: top_p {top_p} and top_k {top_k}: one restriction at a time")


def nucleus_of(top_p):
    """The p of a nucleus restriction, or None where ``top_p`` (None or 1.0) asks for the unrestricted path"""
    return None if top_p is None or float(top_p) == 1.0 else float(top_p)


def nucleus_mask(logits, tau, p):
    """(N, V) bool: word v of a row is in when the words with a larger logit hold less than p of softmax(logits / tau).  The
    mass is summed in float64 along the logits in descending order; a run of equal logits takes the mass in front of the run."""
    srt, order = torch.sort(logits.double(), dim=1, descending=True)
    q = torch.softmax(srt * (1.0 / tau), dim=1)
    above = torch.cumsum(q, 1) - q
    starts = torch.ones_like(srt, dtype=torch.bool)
    starts[:, 1:] = srt[:, 1:] != srt[:, :-1]
    above = torch.cummax(torch.where(starts, above, torch.zeros_like(above)), 1).values      # (`above` never decreases along a row)
    return torch.zeros_like(starts).scatter_(1, order, above < p)


def seed_words(seed, seed_dev=None, device=None):
    """(lo, hi) int64 tensors holding the two 32-bit halves of ``seed + seed_dev * golden`` (mod 2^64): ``make_seed`` of
    csrc/dropout.hpp.  ``seed_dev``: a one-element int64 tensor (``attention.rng_state``) or None; it is read on its device."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    s = torch.tensor(s - (1 << 64) if s >= 1 << 63 else s, dtype=torch.int64, device=device)
    if seed_dev is not None:
        s = s + seed_dev.reshape(()).to(s.device) * _GOLDEN        # int64 arithmetic wraps as the device's uint64 does
    return s & _M32, (s >> 32) & _M32


def hash32(idx, lo, hi):
    """``hash32`` of csrc/dropout.hpp on an int64 tensor of flat indices (below 2^63): uint32 arithmetic carried in int64,
    masked after every step that can leave 32 bits."""
    h = (idx & _M32) ^ lo
    h = (h + (((idx >> 32) & _M32) ^ hi) * 0x9E3779B1) & _M32
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def gumbel_noise(idx, lo, hi):
    """g = -log(-log u) in float32, u = ((hash >> 9) + 0.5) 2^-23 (exact in float32, in [2^-24, 1 - 2^-24])"""
    u = ((hash32(idx, lo, hi) >> 9).to(torch.float32) + 0.5) * (2.0 ** -23)
    return -torch.log(-torch.log(u))


def _first_max(z, words):
    """Per row of z (N, C) with word ids ``words`` (N, C): the largest z, among equal z the smaller word; and the gap to the
    second-largest z (inf with one candidate).  Returns (column, gap)."""
    top = torch.topk(z, min(2, z.shape[1]), dim=1).values
    gap = top[:, 0] - top[:, 1] if top.shape[1] > 1 else torch.full_like(top[:, 0], float("inf"))
    big = torch.full_like(words, torch.iinfo(torch.int64).max)
    col = torch.where(z == top[:, :1], words, big).argmin(1)
    return col, gap


@torch.no_grad()
def sample(step_fn, R, S, n_words, sos, eos, temperature=1.0, top_k=0, seed=0, seed_dev=None, device=None, top_p=None, constraints=None):
    """``step_fn(i, words)`` returns the (R S, V) logits (before log-softmax) of word i of every row; ``words`` (R S,) int64
    are the newest words (``sos`` at i = 0).  Returns a dict: ``ys`` (R, S, n_words) int64, ``score`` (R, S) float32,
    ``length`` (R, S) int32 and ``gap`` (n_words, R S) float32: per row and step the best z minus the second-best one among
    the candidates (inf with one candidate; recorded for finished rows too).  ``top_p``: the nucleus restriction of the module's
    docstring (None or 1.0: none).  ``constraints``: a ``decode_constraints.DecodeConstraints``: the
    logits of every step are constrained over the row's own history before anything else sees them."""
    from . import decode_constraints as dc
    from .beam_search import select_top
    cons = dc.resolve(constraints)
    hist = None
    R, S, n_words, sos, eos, k, tau = int(R), int(S), int(n_words), int(sos), int(eos), int(top_k), float(temperature)
    N = R * S
    words = torch.full((N,), sos, dtype=torch.long, device=device)
    ys, gaps = [], []
    score = fin = length = lo = hi = rho = None
    for i in range(n_words):
        logits = step_fn(i, words).float()
        dev, V = logits.device, logits.shape[1]
        if score is None:
            check_arguments("sample", S, tau, k, V, top_p)
            score = torch.zeros(N, dtype=torch.float32, device=dev)
            fin = torch.zeros(N, dtype=torch.bool, device=dev)
            length = torch.zeros(N, dtype=torch.int32, device=dev)
            lo, hi = seed_words(seed, seed_dev, dev)
            rho = torch.arange(N, dtype=torch.int64, device=dev)
            if cons is not None:
                cons.check("sample", V, n_words, eos)
                hist = torch.zeros(N, n_words, dtype=torch.long, device=dev)
        if cons is not None:
            logits = dc.apply(cons, logits, hist, i, eos)
        logp = logits - torch.logsumexp(logits, 1, keepdim=True)
        base = ((rho * n_words + i) * V).unsqueeze(1)                  # the noise index of word 0 of every row at this step
        if k == 0:
            cand = torch.arange(V, dtype=torch.int64, device=dev).unsqueeze(0).expand(N, V)
            z = logits * (1.0 / tau) + gumbel_noise(base + cand, lo, hi)
            if nucleus_of(top_p) is not None:
                z = torch.where(nucleus_mask(logits, tau, nucleus_of(top_p)), z, torch.full_like(z, float("-inf")))
        else:
            vals, cand = select_top(logp, k)
            z = vals * (1.0 / tau) + gumbel_noise(base + cand, lo, hi)
        col, gap = _first_max(z, cand)
        word = cand.gather(1, col.unsqueeze(1)).squeeze(1)
        lp = logp.gather(1, word.unsqueeze(1)).squeeze(1)
        word = torch.where(fin, torch.full_like(word, eos), word)
        score = torch.where(fin, score, score + lp)
        length = torch.where(fin, length, torch.full_like(length, i + 1))
        fin = fin | (word == eos)
        ys.append(word)
        gaps.append(gap)
        if hist is not None:
            hist[:, i] = word
        words = word
    return {"ys": torch.stack(ys, 1).view(R, S, n_words), "score": score.view(R, S), "length": length.view(R, S),
            "gap": torch.stack(gaps)}
