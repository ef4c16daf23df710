"""Numpy / plain-Python restatement of what spacap3d_amd/predictions.py computes on the device (csrc/predictions.hip): per
scene the proposals with ``valid`` set, ordered by ``obj_prob`` descending compared as f32 (equal scores: lower proposal
index first, -0 == +0; NaN behind every number), each with its class, score, corners and the caption of ``decode_caption``
(lib/eval_helper.py:46-57) over word ids.  Every output array has the kernel's shape, dtype and padding (``index`` -1 and
everything else zero behind ``count``), so a comparison is ``array_equal`` per array.
tests/golden/make_fixtures_predictions.py asserts it against the reference's recorded output."""
import math

import numpy as np

from caption_eval_restated import decode, sentence  # noqa: F401  (decode_caption's rule; the fixture's id <-> word map)

KEYS = ("count", "index", "score", "cls", "corners", "tokens", "length")


def order(valid, obj_prob):
    """The kept proposals of ONE scene in rank order."""
    kept = [k for k in range(len(valid)) if valid[k]]
    p = np.asarray(obj_prob, np.float32)
    return sorted(kept, key=lambda k: (1, 0.0, k) if math.isnan(p[k]) else (0, -float(p[k]), k))


def select(valid, obj_prob, sem_cls, corners, tokens, sos, eos):
    """valid (B,K), obj_prob f32 (B,K), sem_cls int (B,K), corners f64 (B,K,8,3), tokens int (B,K,L) -> the kernel's seven
    arrays."""
    B, K, L = tokens.shape
    out = {"count": np.zeros(B, np.int32), "index": np.full((B, K), -1, np.int32), "score": np.zeros((B, K), np.float32),
           "cls": np.zeros((B, K), np.int32), "corners": np.zeros((B, K, 8, 3), np.float64),
           "tokens": np.zeros((B, K, L + 2), np.int32), "length": np.zeros((B, K), np.int32)}
    for b in range(B):
        ranked = order(valid[b], obj_prob[b])
        out["count"][b] = len(ranked)
        for r, k in enumerate(ranked):
            out["index"][b, r] = k
            out["score"][b, r] = np.float32(obj_prob[b, k])
            out["cls"][b, r] = int(sem_cls[b, k])
            out["corners"][b, r] = corners[b, k]
            cap = decode(tokens[b, k], sos, eos)
            out["tokens"][b, r, :len(cap)] = cap
            out["length"][b, r] = len(cap)
    return out


def records(out, scene):
    """[(proposal, class, score f32, corners, "sos ... eos")] of one scene from ``select``'s arrays (or the device's, copied
    to the host), in rank order."""
    return [(int(out["index"][scene, r]), int(out["cls"][scene, r]), out["score"][scene, r], out["corners"][scene, r],
             sentence(out["tokens"][scene, r, :out["length"][scene, r]])) for r in range(int(out["count"][scene]))]
