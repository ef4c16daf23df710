"""Dense-caption predictions on the device (csrc/predictions.hip): for every scene the boxes that survive post-processing,
ranked by objectness, each with its class, score, corners and caption -- the model's actual output, no ground truth needed.

A caller of the reference gets these from ``parse_predictions`` with ``per_class_proposal=False`` (lib/ap_helper.py:145-158,
which copies every proposal to the host and builds tuples) plus a ``decode_caption`` loop (lib/eval_helper.py:46-57, one
``.item()`` per token).  Here:

* ``dense_caption_predictions`` -- one launch on the current stream, no host synchronisation (capturable in a graph);
* ``to_records``                -- one device-to-host copy, then per scene a list of dicts.

Differences from the reference: the boxes of a scene come ranked (objectness descending, equal scores lower proposal first)
instead of in proposal order -- ``proposal`` names the original index; words are ids until ``to_records`` is given
``idx2word``; a scene that keeps nothing is an empty list, not an ``AssertionError``.

CPU tensors raise ``RuntimeError("... CPU not supported")``: there is no host fallback.
"""
import torch

from ._eval_util import MAX_PROPOSALS, gpu, mask_u8, to_host, word
from ._native import check, lib

MAX_TOKENS = 62      # L + 2 positions = one wave (csrc/predictions.hip)
KEYS = ("count", "index", "score", "cls", "corners", "tokens", "length")


def _aligned(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()


def dense_caption_predictions(post, out, sos, eos, into=None):
    """``post``: the dict of ``postprocess.detection_postprocess`` (``valid`` bool (B,K), ``obj_prob`` f32 (B,K)).  ``out``:
    ``bbox_corner`` (B,K,8,3), ``sem_cls`` (B,K) and ``lang_cap`` as (B,K,L) tokens or (B,K,L,V) scores (``argmax(-1)``
    first, lib/eval_helper.py:124-128); K <= 512, L <= 62.  ``sos`` / ``eos``: the two word ids.  ``into``: the dict of an
    earlier call with the same shapes, to write into its tensors again.

    Returns device tensors, every element written by the call: ``count`` i32 (B,) kept boxes per scene; by rank (objectness
    descending as f32, equal scores lower proposal first) ``index`` i32 (B,K) the proposal (-1 behind ``count``), ``score``
    f32 (B,K), ``cls`` i32 (B,K), ``corners`` f64 (B,K,8,3), ``tokens`` i32 (B,K,L+2) = sos, the words through the first eos,
    an eos appended when there was none, zeros, and ``length`` i32 (B,K) (sos and eos included); rows behind ``count`` are
    zero."""
    valid = gpu("predictions", post["valid"], "valid")
    dev = valid.device
    prob = gpu("predictions", post["obj_prob"], "obj_prob")
    corners = gpu("predictions", out["bbox_corner"], "bbox_corner")
    cls = gpu("predictions", out["sem_cls"], "sem_cls")
    cap = gpu("predictions", out["lang_cap"], "lang_cap")
    for name, t in (("obj_prob", prob), ("bbox_corner", corners), ("sem_cls", cls), ("lang_cap", cap)):
        if t.device != dev:
            raise RuntimeError(f"predictions: {name} must be on {dev}")
    if valid.dim() != 2:
        raise RuntimeError(f"predictions: valid must be (B, K), got {tuple(valid.shape)}")
    B, K = valid.shape
    if not 1 <= K <= MAX_PROPOSALS:
        raise RuntimeError(f"predictions: K={K} proposals, supported 1..{MAX_PROPOSALS}")
    if cap.dim() == 4:
        cap = cap.argmax(-1)
    if cap.dim() != 3 or tuple(cap.shape[:2]) != (B, K):
        raise RuntimeError(f"predictions: lang_cap must be (B, K, L) tokens or (B, K, L, V) scores with B={B}, K={K}, got "
                           f"{tuple(out['lang_cap'].shape)}")
    L = cap.shape[2]
    if not 1 <= L <= MAX_TOKENS:
        raise RuntimeError(f"predictions: L={L} tokens per caption, supported 1..{MAX_TOKENS}")
    if tuple(corners.shape) != (B, K, 8, 3):
        raise RuntimeError(f"predictions: bbox_corner must be (B, K, 8, 3), got {tuple(corners.shape)}")
    if tuple(prob.shape) != (B, K) or tuple(cls.shape) != (B, K):
        raise RuntimeError(f"predictions: obj_prob and sem_cls must be (B, K) with B={B}, K={K}, got {tuple(prob.shape)}, "
                           f"{tuple(cls.shape)}")
    sos, eos = int(sos), int(eos)
    if not (0 <= sos < 2 ** 31 and 0 <= eos < 2 ** 31):
        raise RuntimeError(f"predictions: sos={sos} / eos={eos} must be word ids (0 <= id < 2^31)")
    valid = mask_u8(valid)
    prob = prob.float().contiguous()
    cls = cls.long().contiguous()
    cap = cap.long().contiguous()
    corners = _aligned(corners.double().contiguous())
    shapes = {"count": ((B,), torch.int32), "index": ((B, K), torch.int32), "score": ((B, K), torch.float32),
              "cls": ((B, K), torch.int32), "corners": ((B, K, 8, 3), torch.float64), "tokens": ((B, K, L + 2), torch.int32),
              "length": ((B, K), torch.int32)}
    with torch.cuda.device(dev):
        if into is None:
            r = {k: torch.empty(s, dtype=dt, device=dev) for k, (s, dt) in shapes.items()}
        else:
            r = {k: gpu("predictions", into[k], k) for k in KEYS}
            for k, (s, dt) in shapes.items():
                if tuple(r[k].shape) != s or r[k].dtype != dt or r[k].device != dev or not r[k].is_contiguous() \
                        or (k == "corners" and r[k].data_ptr() % 16):
                    raise RuntimeError(f"predictions: into[{k!r}] must be a contiguous {dt} tensor of shape {s} on {dev}")
        check(lib.spacap_dense_caption_select(valid.data_ptr(), prob.data_ptr(), cls.data_ptr(), corners.data_ptr(),
                                              cap.data_ptr(), B, K, L, sos, eos, *(r[k].data_ptr() for k in KEYS),
                                              torch.cuda.current_stream(dev).cuda_stream), "spacap_dense_caption_select")
    return r


def to_records(pred, idx2word=None, class2type=None):
    """The dict of ``dense_caption_predictions`` as one list of dicts per scene, best box first: ``proposal`` (its index among
    the K proposals), ``score`` (float), ``sem_cls`` (int; ``class_name`` = ``class2type[sem_cls]`` when the map is given),
    ``corners`` ((8,3) f64 array), ``tokens`` (list of ints, sos .. eos) and, when ``idx2word`` is given (``str(id)`` or the
    int id -> word), ``caption`` = the string ``"sos ... eos"``.  A scene with nothing kept gives an empty list.  One
    device-to-host copy."""
    host = to_host({k: gpu("predictions", pred[k], k) for k in KEYS})
    scenes = []
    for b in range(host["count"].shape[0]):
        cur = []
        for r in range(int(host["count"][b])):
            c = int(host["cls"][b, r])
            toks = [int(t) for t in host["tokens"][b, r, :host["length"][b, r]]]
            rec = {"proposal": int(host["index"][b, r]), "score": float(host["score"][b, r]), "sem_cls": c,
                   "corners": host["corners"][b, r].copy(), "tokens": toks}
            if class2type is not None:
                rec["class_name"] = class2type[c]
            if idx2word is not None:
                rec["caption"] = " ".join(word(idx2word, t) for t in toks)
            cur.append(rec)
        scenes.append(cur)
    return scenes
