"""Self-critical caption training: CIDEr-D rewards of drawn captions and the settings of the training
forward that uses them.  The reference trains its captioner with teacher-forced cross-entropy only; fine-tuning on the CIDEr
reward is the project's own addition and ``tests/self_critical_restated.py`` restates its semantics.

``SelfCritical`` holds the corpus and the drawing parameters; set it as ``TransformerDecoderModel.self_critical`` (a plain
attribute, like ``num_samples``) and ``forward_train`` draws S captions per scene for the referred object's proposal, scores
them against the references of the object's corpus key (``rewards``: one launch, csrc/caption_reward.hip), teacher-forces its
own samples and leaves the reward-weighted loss (``fused_losses.self_critical_loss``) where the cross-entropy would be.  No
step reads a value back on the host.

CPU tensors raise ``RuntimeError("... CPU not supported")``: there is no host fallback."""
import ctypes

import torch

from ._eval_util import gpu
from ._native import check, lib
from .caption_eval import LMAX, MAX_IDS, CaptionCorpus
from .sampling import check_arguments

BASELINES = ("greedy", "samples")


class SelfCritical:
    """``SelfCritical(corpus, sos, eos, num_samples=5, temperature=1.0, top_k=0, baseline="greedy", seed=None)``.

    ``corpus``: a ``CaptionCorpus`` (its key table maps ``(dataset_idx, object_id)`` to the references of the referred object).
    ``num_samples`` = S captions are drawn per scene from softmax(logits / ``temperature``), over the whole vocabulary or the
    ``top_k`` <= 8 most probable words (``sampling.check_arguments``).  ``baseline``: ``"greedy"`` -- the reward of the greedy
    caption of the same proposal -- or ``"samples"`` -- per sample the mean reward of the scene's other samples (S >= 2; no
    greedy decode runs).  ``seed``: an integer draws the same captions at every call, None new ones per call."""

    def __init__(self, corpus, sos, eos, num_samples=5, temperature=1.0, top_k=0, baseline="greedy", seed=None):
        if not isinstance(corpus, CaptionCorpus):
            raise TypeError("self_critical: corpus must be a CaptionCorpus")
        if not (0 <= int(sos) < MAX_IDS and 0 <= int(eos) < MAX_IDS):
            raise ValueError("self_critical: sos / eos must be word ids below 65536")
        self.corpus = corpus
        self.sos, self.eos = int(sos), int(eos)
        self.num_samples, self.temperature, self.top_k = int(num_samples), float(temperature), int(top_k)
        check_arguments("self_critical", self.num_samples, self.temperature, self.top_k)
        if baseline not in BASELINES:
            raise ValueError(f"self_critical: baseline {baseline!r} unknown (one of {BASELINES})")
        if baseline == "samples" and self.num_samples < 2:
            raise ValueError(f"self_critical: baseline 'samples' compares a sample with the scene's other samples: num_samples "
                             f"{self.num_samples} < 2")
        self.baseline = baseline
        self.seed = None if seed is None else int(seed)
        self._df_off = (ctypes.c_int64 * 5)(*[int(x) for x in corpus.df_off])

    def rewards(self, tokens, dataset_idx, object_id, rows_per_scene=1, out=None):
        """CIDEr-D of every drawn caption: ``tokens`` (rows, L) decoded words (any integer dtype), row r of scene
        r // ``rows_per_scene``; ``dataset_idx`` and ``object_id`` one entry per scene.  Returns ``(cider (rows,) float64, key
        (rows,) int32 (-1: the scene has no key row, reward 0), length (rows,) int32, tf_tok (rows, L + 2) int64)``, written into the four
        tensors of ``out`` when given (contiguous, of those shapes and dtypes).  One launch on the current stream, no host
        synchronisation."""
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
            if out is None:
                out = (torch.empty(rows, dtype=torch.float64, device=dev), torch.empty(rows, dtype=torch.int32, device=dev),
                       torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, L + 2, dtype=torch.int64, device=dev))
            cider, key, length, tf_tok = out
            want = (((rows,), torch.float64), ((rows,), torch.int32), ((rows,), torch.int32), ((rows, L + 2), torch.int64))
            for t, (shape, dtype) in zip(out, want):
                if tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
                    raise RuntimeError(f"self_critical: out must be contiguous {want} on {dev}")
            check(lib.spacap_caption_reward_f64(tokens.data_ptr(), rows, rps, L, idx.data_ptr(), oid.data_ptr(), kt.data_ptr(),
                                                kt.shape[0], kt.shape[1], co.nkeys, self.sos, self.eos, c["ref_tok"].data_ptr(),
                                                c["ref_tok"].numel(), c["ref_off"].data_ptr(), c["ref_len"].data_ptr(),
                                                c["ref_len"].numel(), c["key_ref_off"].data_ptr(), c["df_code"].data_ptr(),
                                                c["df_idf"].data_ptr(), self._df_off, co.log_nkeys, cider.data_ptr(),
                                                key.data_ptr(), length.data_ptr(), tf_tok.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream), "spacap_caption_reward_f64")
        return cider, key, length, tf_tok
