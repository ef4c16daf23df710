"""Caption metrics on the device (csrc/caption_eval.hip): the candidate loop of the reference's ``feed_scene_cap``
(lib/eval_helper.py:178-222, with ``decode_caption``, ``check_candidates`` and ``organize_candidates``) and the ``Bleu(4)``,
``Cider()`` and ``Rouge()`` scorers that ``eval_cap`` runs at the end (lib/eval_helper.py:304-317).

The reference reads masks, object ids and up to 30 tokens per proposal with ``.item()`` in a Python loop and scores string
dicts on the host.  Once words are ids none of this is string processing: ``CaptionEval.step`` is two launches per batch on
the current stream (no host synchronisation; can be captured in a graph) that keep, per corpus key, the caption of the LAST
counting proposal in the reference's order (step, scene, proposal); ``compute_metrics`` is one launch (one wave per key) and
one device-to-host copy.

Differences from the reference: METEOR is absent (it needs a Java jar; ``candidates()`` returns the decoded strings for
whoever runs it elsewhere); the per-key ``bleu_list`` is not returned (nothing in scripts/eval.py reads it); words are ids.
A reference word outside ``word2idx`` gets a fresh id: it can never match a candidate token but still matches the same word
in another reference, which the document frequency needs.

CPU tensors raise ``RuntimeError("... CPU not supported")``: there is no host fallback.
"""
import ctypes

import numpy as np
import torch

from ._eval_util import gpu, mask_u8, word
from ._native import check, lib

LMAX = 64            # tokens per sentence (csrc/caption_eval.hip: one lane per token)
MAX_IDS = 1 << 16    # an n-gram is n x 16 bits


def ngram_tables(refs, key_of_ref, nkeys):
    """Document frequencies of cider_scorer.py:93-104 over id sentences: ``refs`` = list of int sequences, ``key_of_ref`` =
    the key row of each.  Returns (code u64, df i64, off i64[5]): per n = 1..4 the distinct n-gram codes (n x 16 bits, first
    word highest) ascending with the number of KEYS whose references hold the n-gram; table n = off[n-1]:off[n]."""
    codes, dfs, off = [], [], [0]
    lens = np.array([len(r) for r in refs], np.int64)
    flat = np.concatenate([np.asarray(r, np.uint64) for r in refs]) if len(refs) else np.zeros(0, np.uint64)
    start = np.concatenate([[0], np.cumsum(lens)])[:-1]
    pos_in = np.arange(len(flat)) - np.repeat(start, lens)          # position inside its sentence
    left = np.repeat(lens, lens) - pos_in                            # tokens from here to the sentence's end
    key = np.repeat(np.asarray(key_of_ref, np.int64), lens)
    code = np.zeros(len(flat), np.uint64)
    for n in range(1, 5):
        nxt = np.zeros(len(flat), np.uint64)
        m = max(len(flat) - (n - 1), 0)
        nxt[:m] = flat[n - 1:n - 1 + m]
        code = (code << np.uint64(16)) | nxt
        ok = left >= n
        c, k = code[ok], key[ok]
        order = np.lexsort((k, c))
        c, k = c[order], k[order]
        new_pair = np.ones(len(c), bool)
        new_pair[1:] = (c[1:] != c[:-1]) | (k[1:] != k[:-1])        # one count per (n-gram, key)
        uc, df = np.unique(c[new_pair], return_counts=True)
        codes.append(uc)
        dfs.append(df.astype(np.int64))
        off.append(off[-1] + len(uc))
    return np.concatenate(codes), np.concatenate(dfs), np.array(off, np.int64)


class CaptionCorpus:
    """``CaptionCorpus(corpus, word2idx, organized=None, key_of=None, scene_ids=None, device=None)``: one-time host setup.

    ``corpus``: the reference's ``{"scene|object_id|object_name": ["sos ... eos", ...]}`` of ``prepare_corpus``; sentences
    are split with ``str.split()``.  ``word2idx``: word -> id.  The key table maps ``(dataset_idx, object_id)`` to a key
    row or -1 (where the reference hits ``KeyError: continue`` or builds a key outside the corpus): pass it as ``key_of``
    (int array ``[n_dataset_items, max_object_id + 1]``) or have it built from ``organized`` (ScanRefer_filtered_organized
    .json: scene -> object id -> annotation id -> record with ``object_name``) and ``scene_ids`` (``scene_ids[dataset_idx]``
    = the scene of that dataset item, ``dataset.scanrefer[i]["scene_id"]``).  Raises ``ValueError`` for a reference longer
    than ``LMAX`` = 64 tokens and for an id space of 65 536 ids or more."""

    def __init__(self, corpus, word2idx, organized=None, key_of=None, scene_ids=None, device=None):
        self.keys = list(corpus.keys())
        self.nkeys = len(self.keys)
        if self.nkeys == 0:
            raise ValueError("caption_eval: empty corpus")
        ids = {w: int(i) for w, i in word2idx.items()}
        nxt = len(word2idx)
        self.n_vocab = nxt
        refs, key_of_ref, key_ref_off = [], [], [0]
        for row, key in enumerate(self.keys):
            for sent in corpus[key]:
                toks = []
                for w in sent.split():
                    i = ids.get(w)
                    if i is None:
                        i = ids[w] = nxt      # outside the vocabulary: matches only itself in other references
                        nxt += 1
                    toks.append(i)
                if len(toks) > LMAX:
                    raise ValueError(f"caption_eval: a reference of {key!r} has {len(toks)} tokens, supported <= {LMAX}")
                refs.append(toks)
                key_of_ref.append(row)
            key_ref_off.append(len(refs))
        self.n_ids = max(nxt, max(ids.values(), default=-1) + 1)
        if self.n_ids >= MAX_IDS or min(ids.values(), default=0) < 0:
            raise ValueError(f"caption_eval: {self.n_ids} word ids do not fit 16 bits (< {MAX_IDS})")
        self.ids = ids
        self.ref_tok = np.array([t for r in refs for t in r], np.int32)
        self.ref_len = np.array([len(r) for r in refs], np.int32)
        self.ref_off = (np.cumsum(np.concatenate([[0], self.ref_len]))[:-1]).astype(np.int32)
        self.key_ref_off = np.array(key_ref_off, np.int32)
        self.df_code, self.df, self.df_off = ngram_tables(refs, key_of_ref, self.nkeys)
        # the reference's own values: np.log of a Python float, per distinct document frequency
        self.log_nkeys = float(np.log(float(self.nkeys)))
        logs = {int(d): np.log(max(1.0, float(d))) for d in np.unique(self.df)}
        self.df_idf = np.array([self.log_nkeys - logs[int(d)] for d in self.df], np.float64)

        if key_of is not None:
            self.key_table = np.ascontiguousarray(np.asarray(key_of), dtype=np.int32)
            if self.key_table.ndim != 2 or self.key_table.size == 0:
                raise ValueError("caption_eval: key_of must be [n_dataset_items, max_object_id + 1]")
        elif organized is not None and scene_ids is not None:
            self.key_table = self.build_key_table(organized, scene_ids)
        else:
            raise ValueError("caption_eval: pass key_of, or organized and scene_ids")
        self._dev = {}
        if device is not None:
            self.on(device)

    def build_key_table(self, organized, scene_ids):
        row_of = {k: i for i, k in enumerate(self.keys)}
        per_scene = {}
        for scene in set(scene_ids):
            rows = {}
            for oid, anns in organized.get(scene, {}).items():
                ann = list(anns.keys())
                if not ann or not str(oid).lstrip("-").isdigit() or int(oid) < 0:
                    continue
                key = "{}|{}|{}".format(scene, oid, anns[ann[0]]["object_name"])
                if str(int(oid)) == str(oid) and key in row_of:     # the reference looks up str(int id)
                    rows[int(oid)] = row_of[key]
            per_scene[scene] = rows
        n_obj = max([o for r in per_scene.values() for o in r], default=0) + 1
        table = np.full((len(scene_ids), n_obj), -1, np.int32)
        for i, scene in enumerate(scene_ids):
            for oid, row in per_scene[scene].items():
                table[i, oid] = row
        return table

    def on(self, device):
        """The device copies (uploaded once per device)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("caption_eval: corpus: CPU not supported")
        d = self._dev.get(device)
        if d is None:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            d = {"ref_tok": up(self.ref_tok), "ref_off": up(self.ref_off), "ref_len": up(self.ref_len),
                 "key_ref_off": up(self.key_ref_off), "key_table": up(self.key_table),
                 "df_code": up(self.df_code.view(np.int64)), "df_idf": up(self.df_idf)}
            self._dev[device] = d
        return d


class CaptionEval:
    """``CaptionEval(corpus, sos, eos, min_iou=0.5)``: ``corpus`` a ``CaptionCorpus``, ``sos`` / ``eos`` the two word ids.

    ``step(data_dict, masks=None, **post)`` accumulates a batch, ``compute_metrics()`` returns ``{"bleu": [b1..b4],
    "cider": float, "rouge": float, "cider_scores": ndarray[NKEYS], "rouge_scores": ndarray[NKEYS]}`` (keys in corpus
    order), ``candidates(idx2word)`` the reference's candidates dict, ``reset()`` clears the run."""

    def __init__(self, corpus, sos, eos, min_iou=0.5):
        if not isinstance(corpus, CaptionCorpus):
            raise TypeError("caption_eval: corpus must be a CaptionCorpus")
        if not (0 <= int(sos) < MAX_IDS and 0 <= int(eos) < MAX_IDS):
            raise ValueError("caption_eval: sos / eos must be word ids below 65536")
        self.corpus = corpus
        self.sos, self.eos = int(sos), int(eos)
        self.min_iou = float(min_iou)
        self._df_off = (ctypes.c_int64 * 5)(*[int(x) for x in corpus.df_off])
        self.device = None
        self.reset()

    def reset(self):
        """Every key row back to the placeholder ``[sos, eos]`` (check_candidates), stamps and counter to zero."""
        self.cand_tok = self.cand_len = self.stamp = self.counter = None
        if self.device is not None:
            self._alloc(self.device)

    def _alloc(self, dev):
        n = self.corpus.nkeys
        with torch.cuda.device(dev):
            self.cand_tok = torch.zeros(n, LMAX, dtype=torch.int32, device=dev)
            self.cand_tok[:, 0] = self.sos
            self.cand_tok[:, 1] = self.eos
            self.cand_len = torch.full((n,), 2, dtype=torch.int32, device=dev)
            self.stamp = torch.zeros(n, dtype=torch.int64, device=dev)
            self.counter = torch.zeros(2, dtype=torch.int64, device=dev)
        self.device = dev

    def set_candidates(self, tokens, lengths):
        """Replaces the run's candidate table: ``tokens`` int (NKEYS, <= 64) and ``lengths`` int (NKEYS,) device tensors in
        corpus order (captions decoded elsewhere); later ``step`` calls overwrite the rows they hit."""
        tokens, lengths = gpu("caption_eval", tokens, "tokens"), gpu("caption_eval", lengths, "lengths")
        n = self.corpus.nkeys
        if tokens.dim() != 2 or tokens.shape[0] != n or tokens.shape[1] > LMAX or tuple(lengths.shape) != (n,):
            raise RuntimeError(f"caption_eval: candidates must be ({n}, <= {LMAX}) tokens and ({n},) lengths")
        self._alloc(tokens.device)
        self.cand_tok.zero_()
        self.cand_tok[:, :tokens.shape[1]] = tokens
        self.cand_len.copy_(lengths.clamp(0, tokens.shape[1]))

    def step(self, data_dict, masks=None, **post):
        """``data_dict``: ``lang_cap`` (tokens (B,K,L), or 4-D scores that get an ``argmax(-1)``, lib/eval_helper.py:124-128),
        ``dataset_idx`` (B,) or (B,1), ``scene_object_ids`` (B,M), ``object_assignment`` (B,K).  ``masks``: the dict of
        ``postprocess.caption_eval_masks`` (``nms_masks``, ``good_bbox_masks``); computed here from ``data_dict`` (with the
        ``detection_postprocess`` keyword arguments ``post``) when not given.  Two launches on the current stream, no host
        synchronisation; L + 2 <= 64."""
        cap = gpu("caption_eval", data_dict["lang_cap"], "lang_cap")
        dev = cap.device
        if masks is None:
            from .postprocess import caption_eval_masks
            masks = caption_eval_masks(data_dict, min_iou=self.min_iou, **post)
        if cap.dim() == 4:
            cap = cap.argmax(-1)
        if cap.dim() != 3:
            raise RuntimeError(f"caption_eval: lang_cap must be (B, K, L) tokens or (B, K, L, V) scores, got {tuple(cap.shape)}")
        B, K, L = cap.shape
        if L + 2 > LMAX:
            raise RuntimeError(f"caption_eval: L={L} tokens per caption, supported <= {LMAX - 2}")
        idx = gpu("caption_eval", data_dict["dataset_idx"], "dataset_idx").reshape(-1)
        ids = gpu("caption_eval", data_dict["scene_object_ids"], "scene_object_ids")
        oa = gpu("caption_eval", data_dict["object_assignment"], "object_assignment")
        nms = gpu("caption_eval", masks["nms_masks"], "nms_masks")
        good = gpu("caption_eval", masks["good_bbox_masks"], "good_bbox_masks")
        if idx.numel() != B or ids.dim() != 2 or ids.shape[0] != B or tuple(oa.shape) != (B, K) or tuple(nms.shape) != (B, K) \
                or tuple(good.shape) != (B, K):
            raise RuntimeError(f"caption_eval: expected dataset_idx (B,), scene_object_ids (B, M), object_assignment / masks "
                               f"(B, K) with B={B}, K={K}; got {tuple(idx.shape)}, {tuple(ids.shape)}, {tuple(oa.shape)}, "
                               f"{tuple(nms.shape)}, {tuple(good.shape)}")
        if self.device is None or self.cand_tok is None:
            self._alloc(dev)
        elif dev != self.device:
            raise RuntimeError(f"caption_eval: the run lives on {self.device}, got tensors on {dev}")
        c = self.corpus.on(dev)
        cap, idx, ids, oa, nms = (t.long().contiguous() for t in (cap, idx, ids, oa, nms))
        good = mask_u8(good)
        kt = c["key_table"]
        with torch.cuda.device(dev):
            check(lib.spacap_caption_select_i32(cap.data_ptr(), nms.data_ptr(), good.data_ptr(), idx.data_ptr(), ids.data_ptr(),
                                                oa.data_ptr(), B, K, L, max(ids.shape[1], 1), kt.data_ptr(), kt.shape[0],
                                                kt.shape[1], self.corpus.nkeys, self.sos, self.eos, self.stamp.data_ptr(),
                                                self.counter.data_ptr(), self.cand_tok.data_ptr(), self.cand_len.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream), "spacap_caption_select_i32")

    def scores(self):
        """The device results of the run: ``bleu`` i32 (NKEYS, 10) = testlen, reflen, guess[4], correct[4]; ``rouge`` and
        ``cider`` f64 (NKEYS,).  One launch."""
        if self.cand_tok is None:
            raise RuntimeError("caption_eval: compute_metrics() before any step()")
        dev, n, co = self.device, self.corpus.nkeys, self.corpus
        c = co.on(dev)
        with torch.cuda.device(dev):
            bleu = torch.empty(n, 10, dtype=torch.int32, device=dev)
            rouge = torch.empty(n, dtype=torch.float64, device=dev)
            cider = torch.empty(n, dtype=torch.float64, device=dev)
            check(lib.spacap_caption_score_f64(self.cand_tok.data_ptr(), self.cand_len.data_ptr(), n, c["ref_tok"].data_ptr(),
                                               c["ref_tok"].numel(), c["ref_off"].data_ptr(), c["ref_len"].data_ptr(),
                                               c["ref_len"].numel(), c["key_ref_off"].data_ptr(), c["df_code"].data_ptr(),
                                               c["df_idf"].data_ptr(), self._df_off, co.log_nkeys, bleu.data_ptr(),
                                               rouge.data_ptr(), cider.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                  "spacap_caption_score_f64")
        return {"bleu": bleu, "rouge": rouge, "cider": cider}

    def compute_metrics(self):
        r = self.scores()
        n = self.corpus.nkeys
        small = torch.cat([r["bleu"].sum(0, dtype=torch.int64).double(), r["cider"], r["rouge"]])   # totals < 2^53: exact
        host = small.cpu().numpy()                    # the one device-to-host copy
        totals = [int(v) for v in host[:10]]
        cider, rouge = host[10:10 + n].copy(), host[10 + n:].copy()
        return {"bleu": corpus_bleu(totals), "cider": float(np.mean(cider)), "rouge": float(np.mean(rouge)),
                "cider_scores": cider, "rouge_scores": rouge}

    def candidates(self, idx2word):
        """key -> ["sos ... eos"] for every corpus key in corpus order (check_candidates / organize_candidates applied);
        ``idx2word`` maps ``str(id)`` (the reference's vocabulary) or the int id to the word.  One device-to-host copy."""
        if self.cand_tok is None:
            return {k: ["{} {}".format(word(idx2word, self.sos), word(idx2word, self.eos))] for k in self.corpus.keys}
        host = torch.cat([self.cand_tok, self.cand_len[:, None]], 1).cpu().numpy()
        return {k: [" ".join(word(idx2word, int(t)) for t in host[i, :host[i, LMAX]])] for i, k in enumerate(self.corpus.keys)}


def corpus_bleu(totals):
    """BLEU-1..4 of bleu_scorer.py:245-257 from the ten corpus totals (testlen, reflen, guess[4], correct[4]) in Python
    floats: the geometric mean of the clipped precisions so far, times exp(1 - 1/ratio) when the candidates are shorter."""
    testlen, reflen = totals[0], totals[1]
    guess, correct = totals[2:6], totals[6:10]
    small, tiny = 1e-9, 1e-15
    out, prod = [], 1.0
    for k in range(4):
        prod *= float(correct[k] + tiny) / (guess[k] + small)
        out.append(prod ** (1.0 / (k + 1)))
    ratio = (testlen + tiny) / (reflen + small)
    if ratio < 1:
        import math
        out = [b * math.exp(1 - 1 / ratio) for b in out]
    return out
