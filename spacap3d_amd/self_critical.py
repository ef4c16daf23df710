"""Self-critical caption training: CIDEr-D rewards of drawn captions and the settings of the training
forward that uses them.  The reference trains its captioner with teacher-forced cross-entropy only; fine-tuning on the CIDEr
reward is the project's own addition and ``tests/self_critical_restated.py`` restates its semantics.

``SelfCritical`` holds the corpus and the drawing parameters; set it as ``TransformerDecoderModel.self_critical`` (a plain
attribute, like ``num_samples``) and ``forward_train`` draws S captions per scene for the referred object's proposal, scores
them against the references of the object's corpus key (``rewards``: one launch, csrc/caption_reward.hip), teacher-forces its
own samples and leaves the reward-weighted loss (``fused_losses.self_critical_loss``) where the cross-entropy would be.  No
step reads a value back on the host.

With ``proposals="matched"`` the forward rewards up to ``max_proposals`` annotated objects of every
scene instead of the batch's one referred object: ``select`` (one launch, csrc/scst_select.hip) pairs every annotated object
that has references with its nearest proposal and keeps the nearest pairs; the samples, rewards and loss then run over the
B x ``max_proposals`` groups.

With ``reward=`` the reward is a weighted sum of CIDEr-D, sentence-level BLEU-4 and ROUGE-L from one launch, and with
``xe_weight=`` the loss gains the cross-entropy of the referred object's ground-truth caption, from the same teacher-forced
pass (``tests/reward_mix_restated.py`` restates both).  Both are off by default.

CPU tensors raise ``RuntimeError("... CPU not supported")``: there is no host fallback."""
import ctypes

import numpy as np

import torch

from ._eval_util import gpu
from ._native import check, lib
from .caption_eval import LMAX, MAX_IDS, CaptionCorpus
from .sampling import check_arguments

BASELINES = ("greedy", "samples")
PROPOSALS = ("referred", "matched")
MAX_PROPOSALS = 128        # groups per scene in the matched mode
MAX_OBJECTS = 256          # object slots per scene spacap_scst_select_f32 takes
REWARD_TERMS = ("cider", "bleu4", "rouge")   # the columns of the (rows, 3) scores, the order of the reward's sum


def reward_weights(reward):
    """``reward`` -- one of ``REWARD_TERMS`` or a dict over them -- as the three float weights (w_cider, w_bleu, w_rouge)."""
    if isinstance(reward, str):
        if reward not in REWARD_TERMS:
            raise ValueError(f"self_critical: reward {reward!r} unknown (one of {REWARD_TERMS}, or a dict of weights over them)")
        return tuple(1.0 if k == reward else 0.0 for k in REWARD_TERMS)
    if not isinstance(reward, dict) or not reward or any(k not in REWARD_TERMS for k in reward):
        raise ValueError(f"self_critical: reward must be one of {REWARD_TERMS} or a dict of weights over them, got {reward!r}")
    try:
        w = tuple(float(reward.get(k, 0.0)) for k in REWARD_TERMS)
    except (TypeError, ValueError):
        raise ValueError(f"self_critical: reward weights must be numbers, got {reward!r}") from None
    if not all(np.isfinite(x) and x >= 0.0 for x in w) or not any(w):
        raise ValueError(f"self_critical: reward weights must be finite, not negative and not all zero, got {reward!r}")
    return w


def select_pairs(who, corpus, max_proposals, near2, xyz, center_label, box_label_mask, scene_object_ids, dataset_idx, out=None):
    """The launch of ``spacap_scst_select_f32`` behind ``SelfCritical.select`` and ``dense_xe.DenseCaptionXE.select`` (arguments
    and results as stated there); ``who`` names the caller in the refusals, ``near2`` is the float32 square of the threshold."""
    xyz = gpu(who, xyz, "xyz")
    dev = xyz.device
    ctr = gpu(who, center_label, "center_label")
    msk = gpu(who, box_label_mask, "box_label_mask")
    ids = gpu(who, scene_object_ids, "scene_object_ids")
    idx = gpu(who, dataset_idx, "dataset_idx").reshape(-1)
    M = int(max_proposals)
    if xyz.dim() != 3 or xyz.shape[-1] != 3 or ctr.dim() != 3 or ctr.shape[-1] != 3 or ctr.shape[0] != xyz.shape[0] or \
            tuple(msk.shape) != tuple(ctr.shape[:2]) or tuple(ids.shape) != tuple(ctr.shape[:2]) or idx.numel() != xyz.shape[0]:
        raise RuntimeError(f"{who}: expected xyz (B,K,3), center_label (B,G,3), box_label_mask / scene_object_ids (B,G), "
                           f"dataset_idx (B,); got {tuple(xyz.shape)}, {tuple(ctr.shape)}, {tuple(msk.shape)}, {tuple(ids.shape)}, "
                           f"{tuple(idx.shape)}")
    B, K, G = xyz.shape[0], xyz.shape[1], ctr.shape[1]
    if any(t.device != dev for t in (ctr, msk, ids, idx)):
        raise RuntimeError(f"{who}: xyz lives on {dev}, the labels elsewhere")
    if not (K >= 1 and M <= G <= MAX_OBJECTS):
        raise RuntimeError(f"{who}: K={K} proposals, G={G} object slots, max_proposals={M}: supported K >= 1, "
                           f"max_proposals <= G <= {MAX_OBJECTS}")
    xyz, ctr, msk = (t.detach().float().contiguous() for t in (xyz, ctr, msk))
    ids, idx = ids.long().contiguous(), idx.long().contiguous()
    kt = corpus.on(dev)["key_table"]
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty(B, M, dtype=torch.int64, device=dev), torch.empty(B, M, dtype=torch.int64, device=dev),
                   torch.empty(B, M, dtype=torch.int32, device=dev), torch.empty(B, M, dtype=torch.int32, device=dev),
                   torch.empty(B, M, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
        want = (((B, M), torch.int64), ((B, M), torch.int64), ((B, M), torch.int32), ((B, M), torch.int32),
                ((B, M), torch.float32), ((B,), torch.int32))
        for t, (shape, dtype) in zip(out, want):
            if tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
                raise RuntimeError(f"{who}: out must be contiguous {want} on {dev}")
        prop, obj, slot_of, key, dist, n_sel = out
        check(lib.spacap_scst_select_f32(xyz.data_ptr(), ctr.data_ptr(), msk.data_ptr(), ids.data_ptr(), idx.data_ptr(),
                                         kt.data_ptr(), B, K, G, M, kt.shape[0], kt.shape[1], corpus.nkeys, float(near2),
                                         prop.data_ptr(), obj.data_ptr(), slot_of.data_ptr(), key.data_ptr(), dist.data_ptr(),
                                         n_sel.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "spacap_scst_select_f32")
    return prop, obj, slot_of, key, dist, n_sel


class SelfCritical:
    """``SelfCritical(corpus, sos, eos, num_samples=5, temperature=1.0, top_k=0, baseline="greedy", seed=None, top_p=None)``.

    ``corpus``: a ``CaptionCorpus`` (its key table maps ``(dataset_idx, object_id)`` to the references of the referred object).
    ``num_samples`` = S captions are drawn per scene from softmax(logits / ``temperature``), over the whole vocabulary or the
    ``top_k`` <= 8 most probable words, or -- ``top_p`` in (0, 1), with ``top_k`` = 0 -- the row's nucleus
    (``sampling.check_arguments``; ``sampling.py`` states the set).  ``baseline``: ``"greedy"`` -- the reward of the greedy
    caption of the same proposal -- or ``"samples"`` -- per sample the mean reward of the scene's other samples (S >= 2; no
    greedy decode runs).  ``seed``: an integer draws the same captions at every call, None new ones per call.

    ``proposals``: ``"referred"`` (the default) rewards the proposal nearest to the batch's referred object and reads neither
    of the next two arguments.  ``"matched"`` rewards up to ``max_proposals`` = M (1 .. 128) objects per scene: the annotated
    objects (``box_label_mask`` > 0) with a key row whose nearest proposal lies closer than ``near_threshold`` (> 0; the
    detector's NEAR_THRESHOLD by default) to their centre, nearest first (``select``).  The batch then carries ``center_label``
    (B,G,3), ``box_label_mask`` (B,G), ``scene_object_ids`` (B,G) and ``dataset_idx``; ``object_id`` is not read.

    ``reward`` and ``xe_weight``.  ``reward``: ``"cider"`` (the default), ``"bleu4"``, ``"rouge"`` or a
    dict of weights over those three names -- finite, not negative, not all zero --: the reward of a caption is
    ``w_cider CIDEr-D + w_bleu4 BLEU-4 + w_rouge ROUGE-L`` (sentence-level BLEU-4 and ROUGE-L as the reference's scorers compute
    them per caption), from one launch.  ``xe_weight`` >= 0: with a positive value the training forward adds ``xe_weight`` times
    the teacher-forced cross-entropy of the referred object's ground-truth caption (the loss of the plain training forward) to
    the reward-weighted loss; both come from ONE teacher-forced pass over B + R rows, and the batch then also carries
    ``lang_label`` and ``lang_ids``.  Anything else raises ``ValueError``."""

    def __init__(self, corpus, sos, eos, num_samples=5, temperature=1.0, top_k=0, baseline="greedy", seed=None,
                 proposals="referred", max_proposals=16, near_threshold=0.3, reward="cider", xe_weight=0.0, top_p=None):
        if not isinstance(corpus, CaptionCorpus):
            raise TypeError("self_critical: corpus must be a CaptionCorpus")
        if not (0 <= int(sos) < MAX_IDS and 0 <= int(eos) < MAX_IDS):
            raise ValueError("self_critical: sos / eos must be word ids below 65536")
        self.corpus = corpus
        self.sos, self.eos = int(sos), int(eos)
        self.num_samples, self.temperature, self.top_k = int(num_samples), float(temperature), int(top_k)
        self.top_p = None if top_p is None else float(top_p)
        check_arguments("self_critical", self.num_samples, self.temperature, self.top_k, top_p=self.top_p)
        if baseline not in BASELINES:
            raise ValueError(f"self_critical: baseline {baseline!r} unknown (one of {BASELINES})")
        if baseline == "samples" and self.num_samples < 2:
            raise ValueError(f"self_critical: baseline 'samples' compares a sample with the scene's other samples: num_samples "
                             f"{self.num_samples} < 2")
        self.baseline = baseline
        self.seed = None if seed is None else int(seed)
        self._df_off = (ctypes.c_int64 * 5)(*[int(x) for x in corpus.df_off])
        if proposals not in PROPOSALS:
            raise ValueError(f"self_critical: proposals {proposals!r} unknown (one of {PROPOSALS})")
        self.proposals = proposals
        if proposals == "matched":
            if not 1 <= int(max_proposals) <= MAX_PROPOSALS:
                raise ValueError(f"self_critical: max_proposals {max_proposals} outside 1 .. {MAX_PROPOSALS}")
            if not float(near_threshold) > 0.0:
                raise ValueError(f"self_critical: near_threshold {near_threshold} must be positive")
            self.max_proposals, self.near_threshold = int(max_proposals), float(near_threshold)
            self.near2 = float(np.float32(self.near_threshold) * np.float32(self.near_threshold))   # the fp32 product, once
        self.reward_weights = reward_weights(reward)
        try:
            self.xe_weight = float(xe_weight)
        except (TypeError, ValueError):
            raise ValueError(f"self_critical: xe_weight must be a number, got {xe_weight!r}") from None
        if not (np.isfinite(self.xe_weight) and self.xe_weight >= 0.0):
            raise ValueError(f"self_critical: xe_weight {xe_weight} must be finite and not negative")
        # the settings of DESIGN.md section 7l; with the defaults every call goes where it went before them
        self.mixed = self.reward_weights != (1.0, 0.0, 0.0) or self.xe_weight > 0.0

    def select(self, xyz, center_label, box_label_mask, scene_object_ids, dataset_idx, out=None):
        """The (proposal, object) pairs the matched mode rewards: ``xyz`` (B,K,3) proposal centres, ``center_label`` (B,G,3),
        ``box_label_mask`` (B,G), ``scene_object_ids`` (B,G), ``dataset_idx`` (B,) or (B,1); G >= ``max_proposals`` = M, G <= 256.
        Returns ``(prop (B,M) int64, obj (B,M) int64, slot_of (B,M) int32, key (B,M) int32, dist (B,M) float32, n_sel (B,)
        int32)`` -- per scene the qualifying objects in (distance, slot) order, -1 / +inf in the empty slots --, written into the
        six tensors of ``out`` when given.  One launch on the current stream, no host synchronisation."""
        if self.proposals != "matched":
            raise RuntimeError("self_critical: select() belongs to proposals='matched'")
        return select_pairs("self_critical", self.corpus, self.max_proposals, self.near2, xyz, center_label, box_label_mask,
                            scene_object_ids, dataset_idx, out)

    def rewards(self, tokens, dataset_idx, object_id, rows_per_scene=1, out=None, terms=False):
        """The reward of every drawn caption: ``tokens`` (rows, L) decoded words (any integer dtype), row r of scene
        r // ``rows_per_scene``; ``dataset_idx`` and ``object_id`` one entry per scene.  Returns ``(reward (rows,) float64, key
        (rows,) int32 (-1: the scene has no key row, reward 0), length (rows,) int32, tf_tok (rows, L + 2) int64)``, written into the four
        tensors of ``out`` when given (contiguous, of those shapes and dtypes).  One launch on the current stream, no host
        synchronisation.

        The reward is CIDEr-D by default; with the constructor's ``reward`` it is the weighted sum of CIDEr-D, sentence-level
        BLEU-4 and ROUGE-L (one launch all the same: ``spacap_caption_reward_mix_f64``; a term of weight 0 is not computed and
        reads 0).  ``terms=True`` returns two more tensors: ``scores (rows, 3) float64`` -- the columns of ``REWARD_TERMS``, a
        transposed view of a contiguous (3, rows) tensor -- and ``bleu_comp (rows, 10) int32`` (testlen, closest reflen, guess[4],
        correct[4]; zeros when BLEU-4 has weight 0).  ``out`` then holds six tensors, the fifth the contiguous (3, rows) one."""
        tokens = gpu("self_critical", tokens, "tokens")
        dev = tokens.device
        if tokens.dim() != 2:
            raise RuntimeError(f"self_critical: tokens must be (rows, L), got {tuple(tokens.shape)}")
        rows, L = tokens.shape
        rps = int(rows_per_scene)
        if L + 2 > LMAX or L < 1:
            raise RuntimeError(f"self_critical: L={L} words per caption, supported 1 .. {LMAX - 2}")
        idx = gpu("self_critical", dataset_idx, "dataset_idx").reshape(-1)
        oid = gpu("self_critical", object_id, "object_id").reshape(-1)
        if rps < 1 or rows % rps or idx.numel() * rps != rows or oid.numel() * rps != rows:
            raise RuntimeError(f"self_critical: {rows} rows at {rps} per scene need {rows // max(rps, 1)} entries of dataset_idx "
                               f"and object_id, got {idx.numel()} and {oid.numel()}")
        if idx.device != dev or oid.device != dev:
            raise RuntimeError(f"self_critical: tokens live on {dev}, dataset_idx / object_id on {idx.device} / {oid.device}")
        co = self.corpus
        c = co.on(dev)
        tokens, idx, oid = (t.long().contiguous() for t in (tokens, idx, oid))
        kt = c["key_table"]
        with torch.cuda.device(dev):
            n_out = 6 if terms else 4
            if out is None:
                out = (torch.empty(rows, dtype=torch.float64, device=dev), torch.empty(rows, dtype=torch.int32, device=dev),
                       torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, L + 2, dtype=torch.int64, device=dev))
                if terms:
                    out += (torch.empty(3, rows, dtype=torch.float64, device=dev), torch.empty(rows, 10, dtype=torch.int32, device=dev))
            want = (((rows,), torch.float64), ((rows,), torch.int32), ((rows,), torch.int32), ((rows, L + 2), torch.int64),
                    ((3, rows), torch.float64), ((rows, 10), torch.int32))[:n_out]
            if len(out) != n_out:
                raise RuntimeError(f"self_critical: out must hold {n_out} tensors: contiguous {want} on {dev}")
            for t, (shape, dtype) in zip(out, want):
                if tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
                    raise RuntimeError(f"self_critical: out must be contiguous {want} on {dev}")
            reward, key, length, tf_tok = out[:4]
            st = torch.cuda.current_stream(dev).cuda_stream
            if not terms and self.reward_weights == (1.0, 0.0, 0.0):
                check(lib.spacap_caption_reward_f64(tokens.data_ptr(), rows, rps, L, idx.data_ptr(), oid.data_ptr(), kt.data_ptr(),
                                                    kt.shape[0], kt.shape[1], co.nkeys, self.sos, self.eos, c["ref_tok"].data_ptr(),
                                                    c["ref_tok"].numel(), c["ref_off"].data_ptr(), c["ref_len"].data_ptr(),
                                                    c["ref_len"].numel(), c["key_ref_off"].data_ptr(), c["df_code"].data_ptr(),
                                                    c["df_idf"].data_ptr(), self._df_off, co.log_nkeys, reward.data_ptr(),
                                                    key.data_ptr(), length.data_ptr(), tf_tok.data_ptr(), st), "spacap_caption_reward_f64")
                return reward, key, length, tf_tok
            scores, comp = out[4:] if terms else (torch.empty(3, rows, dtype=torch.float64, device=dev),
                                                  torch.empty(rows, 10, dtype=torch.int32, device=dev))
            w = self.reward_weights
            check(lib.spacap_caption_reward_mix_f64(tokens.data_ptr(), rows, rps, L, idx.data_ptr(), oid.data_ptr(), kt.data_ptr(),
                                                    kt.shape[0], kt.shape[1], co.nkeys, self.sos, self.eos, c["ref_tok"].data_ptr(),
                                                    c["ref_tok"].numel(), c["ref_off"].data_ptr(), c["ref_len"].data_ptr(),
                                                    c["ref_len"].numel(), c["key_ref_off"].data_ptr(), c["df_code"].data_ptr(),
                                                    c["df_idf"].data_ptr(), self._df_off, co.log_nkeys, w[0], w[1], w[2],
                                                    scores[0].data_ptr(), key.data_ptr(), length.data_ptr(), tf_tok.data_ptr(),
                                                    scores[1].data_ptr(), scores[2].data_ptr(), reward.data_ptr(), comp.data_ptr(), st),
                  "spacap_caption_reward_mix_f64")
        if terms:
            return reward, key, length, tf_tok, scores.t(), comp
        return reward, key, length, tf_tok
