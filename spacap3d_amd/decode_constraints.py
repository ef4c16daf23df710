"""Constrained caption decoding (restated by ``tests/decode_constraints_restated.py``): a minimum length,
a no-repeat n-gram rule, a fixed set of bad words and a repetition penalty, for the greedy decoder, the beam search and the
sampler alike.  The reference decodes greedily without constraints; the semantics are the project's own:

A decoding row is a sequence, a beam hypothesis or a sample, and ``y_0 .. y_{i-1}`` are the words it has generated so far
(neither ``sos`` nor the object indicator; a beam hypothesis' history is its own ancestry).  Before anything else looks at the
logits z (fp32, V words) of step i they become z':

1. ``repetition_penalty`` theta >= 1: for every distinct word v of the history ``z_v / theta`` if ``z_v > 0`` else
   ``z_v * theta`` -- one fp32 operation.
2. Bans, ``z_v = -inf``, for every v in ``bad_words``, for ``eos`` while ``i < min_length``, and with ``no_repeat_ngram`` =
   n >= 1 for every v for which ``(y_{i-n+1}, .., y_{i-1}, v)`` equals some ``(y_j, .., y_{j+n-1})`` of the history
   (n = 1: every used word; nothing while ``i < n - 1``).

The greedy arg-max, the beam's ``log_softmax`` and the sampler's softmax, top-k set, nucleus and reported log-probability all
see z'.  A beam hypothesis or sample that has finished keeps emitting eos with a frozen score: no constraint applies to it.
The fused decoders (``caption_decode``) apply the same rule inside their word-selection kernels; ``apply`` is the rule in
torch operations for every path that is not fused.
"""
import math

import torch

MAX_BAD_WORDS = 64


class DecodeConstraints:
    """The four settings; every one is off at its default.  ``check`` holds them against a decoding call."""

    def __init__(self, min_length=0, no_repeat_ngram=0, repetition_penalty=1.0, bad_words=()):
        self.min_length, self.no_repeat_ngram = int(min_length), int(no_repeat_ngram)
        self.repetition_penalty = float(repetition_penalty)
        self.bad_words = tuple(sorted({int(w) for w in bad_words}))
        if self.min_length < 0:
            raise ValueError(f"DecodeConstraints: min_length {self.min_length} < 0")
        if self.no_repeat_ngram < 0:
            raise ValueError(f"DecodeConstraints: no_repeat_ngram {self.no_repeat_ngram} < 0")
        if not (math.isfinite(self.repetition_penalty) and self.repetition_penalty >= 1.0):
            raise ValueError(f"DecodeConstraints: repetition_penalty {self.repetition_penalty} must be finite and >= 1")
        if len(self.bad_words) > MAX_BAD_WORDS:
            raise ValueError(f"DecodeConstraints: {len(self.bad_words)} bad words, at most {MAX_BAD_WORDS}")

    def active(self):
        return self.min_length > 0 or self.no_repeat_ngram > 0 or self.repetition_penalty != 1.0 or len(self.bad_words) > 0

    def check(self, who, V, n_words, eos):
        """Raises ValueError naming ``who`` where the settings cannot hold for a vocabulary of V words and captions of
        ``n_words`` words: a row must always keep a finite logit."""
        bad = [w for w in self.bad_words if not 0 <= w < V]
        if bad:
            raise ValueError(f"{who}: bad_words {bad} outside the vocabulary 0..{V - 1}")
        if not 0 <= int(eos) < V:
            raise ValueError(f"{who}: eos {eos} outside the vocabulary 0..{V - 1}")
        if int(eos) in self.bad_words:
            raise ValueError(f"{who}: eos ({eos}) must not be a bad word")
        if len(self.bad_words) + n_words + 1 >= V:
            raise ValueError(f"{who}: {len(self.bad_words)} bad words + {n_words} words + eos could leave a row of {V} words "
                             "without an allowed one")
        if self.min_length > n_words - 1:
            raise ValueError(f"{who}: min_length {self.min_length} > n_words - 1 = {n_words - 1}")
        return self

    def __repr__(self):
        return (f"DecodeConstraints(min_length={self.min_length}, no_repeat_ngram={self.no_repeat_ngram}, "
                f"repetition_penalty={self.repetition_penalty}, bad_words={self.bad_words})")


def resolve(constraints):
    """None, a ``DecodeConstraints`` or a dict of its arguments -> a ``DecodeConstraints`` that is active, or None"""
    if constraints is None:
        return None
    c = constraints if isinstance(constraints, DecodeConstraints) else DecodeConstraints(**constraints)
    return c if c.active() else None


def banned_and_seen(c, history, step, eos, V):
    """(banned, seen) bool (N, V) for the histories ``history`` (N, >= step) int64, of which columns 0 .. step - 1 count."""
    N, dev = history.shape[0], history.device
    h = history[:, :step]
    seen = torch.zeros(N, V, dtype=torch.bool, device=dev)
    banned = torch.zeros(N, V, dtype=torch.bool, device=dev)
    if step > 0:
        seen.scatter_(1, h, True)
    if c.bad_words:
        banned[:, list(c.bad_words)] = True
    if step < c.min_length:
        banned[:, int(eos)] = True
    n = c.no_repeat_ngram
    if n >= 1 and step >= n:                 # (a history of n - 1 words holds no n-gram yet)
        # the n-grams of the history end at j = n - 1 .. step - 1: (y_{j-n+1} .. y_{j-1}) against the last n - 1 words
        ends = h[:, n - 1:]                                                     # (N, step - n + 1): the word a match bans
        hit = torch.ones_like(ends, dtype=torch.bool)
        for k in range(1, n):
            hit &= h[:, n - 1 - k:step - k] == h[:, step - k:step - k + 1]
        banned |= torch.zeros(N, V, dtype=torch.int32, device=dev).scatter_add_(1, ends, hit.int()) > 0     # (nothing read back)
    return banned, seen


def apply(c, logits, history, step, eos):
    """z' (N, V) float32 of the logits z (N, V) of step ``step`` for rows with the histories ``history`` (N, >= step) int64."""
    z = logits.float()
    banned, seen = banned_and_seen(c, history, step, eos, z.shape[1])
    if c.repetition_penalty != 1.0:
        # a float32 tensor, not a Python scalar: a device may divide by a scalar as a product with its reciprocal, which is
        # another rounding than the one float32 division the rule and the fused kernels do
        theta = torch.full((), c.repetition_penalty, dtype=torch.float32, device=z.device)
        z = torch.where(seen, torch.where(z > 0, z / theta, z * theta), z)
    return z.masked_fill(banned, float("-inf"))
