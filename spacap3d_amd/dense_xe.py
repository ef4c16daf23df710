"""Cross-entropy caption training over every matched object of a scene: which reference sentences a
training step teaches, chosen and laid out as teacher-forcing rows on the device.  The reference supervises one caption per
scene, the referred object's; the mode is the project's own addition and ``tests/dense_xe_restated.py`` restates its semantics.

``DenseCaptionXE`` holds the corpus and the settings; set it as ``TransformerDecoderModel.dense_xe`` (a plain attribute, like
``self_critical``) and ``forward_train`` pairs up to ``max_proposals`` annotated objects of every scene with their nearest
proposals (``select``: the launch of the matched self-critical mode, csrc/scst_select.hip), draws ``refs_per_object`` of each
object's reference sentences and builds their token rows (``targets``: one launch, csrc/dense_xe.hip), and runs the decoder and
the plain caption loss over those B x ``max_proposals`` x ``refs_per_object`` rows.  No step reads a value back on the host.

CPU tensors raise ``RuntimeError("... CPU not supported")``: there is no host fallback."""
import numpy as np

import torch

from ._eval_util import gpu
from ._native import check, lib
from .caption_eval import MAX_IDS, CaptionCorpus
from .self_critical import MAX_PROPOSALS, select_pairs

MAX_REFS = 8               # rows per group spacap_dense_xe_targets_i64 takes
ROW_IDS = 32               # MAX_DES_LEN + 2: lang_ids' width (sos, 30 words, eos)


class DenseCaptionXE:
    """``DenseCaptionXE(corpus, sos, eos, unk, max_proposals=16, near_threshold=0.3, refs_per_object=1, seed=None)``.

    ``corpus``: a ``CaptionCorpus`` (its key table maps ``(dataset_idx, object_id)`` to an object's reference sentences).
    ``max_proposals`` = M (1 .. 128) objects per scene are taught: the annotated objects (``box_label_mask`` > 0) with a key row
    whose nearest proposal lies closer than ``near_threshold`` (> 0; the detector's NEAR_THRESHOLD by default) to their centre,
    nearest first.  ``refs_per_object`` = r (1 .. 8) reference sentences are drawn per object, distinct while the object has
    that many: a uniformly drawn first one and its successors in corpus order, cyclically.  ``unk`` replaces the words outside
    the vocabulary.  ``seed``: an integer draws the same sentences at every call, None new ones per call -- and, in a captured
    graph, after every ``attention.advance_rng``.  The batch carries ``center_label`` (B,G,3), ``box_label_mask`` (B,G),
    ``scene_object_ids`` (B,G) and ``dataset_idx``.  Anything else raises ``ValueError``."""

    def __init__(self, corpus, sos, eos, unk, max_proposals=16, near_threshold=0.3, refs_per_object=1, seed=None):
        if not isinstance(corpus, CaptionCorpus):
            raise TypeError("dense_xe: corpus must be a CaptionCorpus")
        if not all(0 <= int(w) < MAX_IDS for w in (sos, eos, unk)):
            raise ValueError("dense_xe: sos / eos / unk must be word ids below 65536")
        if not 1 <= int(max_proposals) <= MAX_PROPOSALS:
            raise ValueError(f"dense_xe: max_proposals {max_proposals} outside 1 .. {MAX_PROPOSALS}")
        if not float(near_threshold) > 0.0:
            raise ValueError(f"dense_xe: near_threshold {near_threshold} must be positive")
        if not 1 <= int(refs_per_object) <= MAX_REFS:
            raise ValueError(f"dense_xe: refs_per_object {refs_per_object} outside 1 .. {MAX_REFS}")
        self.corpus = corpus
        self.sos, self.eos, self.unk = int(sos), int(eos), int(unk)
        self.max_proposals, self.near_threshold = int(max_proposals), float(near_threshold)
        self.near2 = float(np.float32(self.near_threshold) * np.float32(self.near_threshold))   # the fp32 product, once
        self.refs_per_object = int(refs_per_object)
        self.seed = None if seed is None else int(seed)

    def select(self, xyz, center_label, box_label_mask, scene_object_ids, dataset_idx, out=None):
        """The (proposal, object) pairs the mode teaches: ``SelfCritical.select``'s arguments and results -- ``(prop (B,M) int64,
        obj (B,M) int64, slot_of (B,M) int32, key (B,M) int32, dist (B,M) float32, n_sel (B,) int32)``, the same launch."""
        return select_pairs("dense_xe", self.corpus, self.max_proposals, self.near2, xyz, center_label, box_label_mask,
                            scene_object_ids, dataset_idx, out)

    def targets(self, key, out=None):
        """The teacher-forcing rows of the selection's ``key`` (B, M) int32, r = ``refs_per_object`` per group: returns ``(tok
        (B M r, 33) int64 -- lang_label's layout: a leading 1, then the id row --, ids (B M r, 32) int64 -- lang_ids' layout: the
        sentence cut as the reference's dataset cuts it, words outside the vocabulary as ``unk``, zeros behind it --, ref (B M r,)
        int32 the reference's index in the corpus or -1, good (B M r,) uint8, length (B M r,) int32 the target words with eos)``,
        written into the five tensors of ``out`` when given (contiguous, of those shapes and dtypes).  A row without a reference
        -- an empty slot, an object with fewer than r sentences -- is the empty caption sos eos, good 0, length 0.  One launch on
        the current stream, no host synchronisation."""
        from .attention import _next_seed, rng_state
        key = gpu("dense_xe", key, "key")
        dev = key.device
        if key.dim() != 2 or key.dtype != torch.int32:
            raise RuntimeError(f"dense_xe: key must be (B, M) int32, got {tuple(key.shape)} {key.dtype}")
        B, M = key.shape
        r, T = self.refs_per_object, ROW_IDS
        R = B * M * r
        key = key.contiguous()
        co = self.corpus
        c = co.on(dev)
        if self.seed is None:
            seed_host, seed_dev = _next_seed(), rng_state(dev).data_ptr()
        else:
            seed_host, seed_dev = self.seed & 0xFFFFFFFFFFFFFFFF, None
        with torch.cuda.device(dev):
            if out is None:
                out = (torch.empty(R, T + 1, dtype=torch.int64, device=dev), torch.empty(R, T, dtype=torch.int64, device=dev),
                       torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.uint8, device=dev),
                       torch.empty(R, dtype=torch.int32, device=dev))
            want = (((R, T + 1), torch.int64), ((R, T), torch.int64), ((R,), torch.int32), ((R,), torch.uint8), ((R,), torch.int32))
            if len(out) != 5:
                raise RuntimeError(f"dense_xe: out must hold 5 tensors: contiguous {want} on {dev}")
            for t, (shape, dtype) in zip(out, want):
                if tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
                    raise RuntimeError(f"dense_xe: out must be contiguous {want} on {dev}")
            tok, ids, ref, good, length = out
            check(lib.spacap_dense_xe_targets_i64(key.data_ptr(), B, M, c["ref_tok"].data_ptr(), c["ref_tok"].numel(),
                                                  c["ref_off"].data_ptr(), c["ref_len"].data_ptr(), c["ref_len"].numel(),
                                                  c["key_ref_off"].data_ptr(), co.nkeys, co.n_vocab, self.unk, self.sos, self.eos, r, T,
                                                  seed_host, seed_dev, ids.data_ptr(), tok.data_ptr(), ref.data_ptr(), good.data_ptr(),
                                                  length.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                  "spacap_dense_xe_targets_i64")
        return tok, ids, ref, good, length
