"""Times of the caption metrics (spacap3d_amd/caption_eval.py, csrc/caption_eval.hip), one JSON line each, on a synthetic
ScanRefer-val-sized corpus (2 068 keys, 1 - 8 references each, 3 000 words):

* device time of ``CaptionEval.step`` (the two bookkeeping launches) per cfg2 batch (8 scenes x 256 proposals, L = 31) and of
  the scoring launch over all keys, HIP events around graph replays after a warm-up, median of 5 groups;
* ``compute_metrics()`` (scoring launch, totals, one device-to-host copy, host BLEU) as wall time between device
  synchronisations;
* with ``--reference DIR`` (no GPU needed): the reference's ``Bleu(4)``, ``Cider()`` and ``Rouge()`` on the SAME corpus and
  candidates as word strings, on this host's CPU -- the baseline.  DIR is a checkout of the reference.

Run:  timeout -k 10 300 python tools/bench_caption_eval.py [--iters 200] [--keys 2068]
      python tools/bench_caption_eval.py --reference DIR [--keys 2068]"""
import argparse
import json
import os
import sys
import time

import numpy as np

from _eval_bench import ROOT, enter_reference, replay_us

sys.path.insert(0, ROOT)
SOS, EOS, V, B, K, L = 2, 3, 3000, 8, 256, 31


def word(i):
    return {2: "sos", 3: "eos"}.get(int(i), "w%d" % int(i))


def make(nk, seed=3):
    """corpus and candidates as id lists: per key a base sentence, references and the candidate are noisy prefixes of it;
    20 % of the candidates are the placeholder."""
    rng = np.random.default_rng(seed)
    refs, cands = [], []
    for _ in range(nk):
        base = rng.integers(4, V, int(rng.integers(3, 31)))

        def noisy():
            t = base.copy()
            m = rng.random(len(t)) < 0.3
            t[m] = rng.integers(4, V, m.sum())
            return [SOS] + [int(x) for x in t[: int(rng.integers(1, len(t) + 1))]] + [EOS]

        refs.append([noisy() for _ in range(int(rng.integers(1, 9)))])
        cands.append([SOS, EOS] if rng.random() < 0.2 else noisy())
    return refs, cands


def strings(refs, cands):
    corpus = {"k%d" % i: [" ".join(word(t) for t in r) for r in rs] for i, rs in enumerate(refs)}
    cand = {"k%d" % i: [" ".join(word(t) for t in c)] for i, c in enumerate(cands)}
    return corpus, cand


def reference_baseline(ref_dir, nk):
    enter_reference(ref_dir)
    import lib.capeval.bleu.bleu as capbleu
    import lib.capeval.cider.cider as capcider
    import lib.capeval.rouge.rouge as caprouge
    corpus, cand = strings(*make(nk))
    out = {"what": "reference Bleu(4) / Cider() / Rouge() on the host", "keys": nk, "cpus": os.cpu_count()}
    for name, scorer in (("bleu", capbleu.Bleu(4)), ("cider", capcider.Cider()), ("rouge", caprouge.Rouge())):
        t0 = time.perf_counter()
        score, _ = scorer.compute_score(corpus, cand)
        out[f"seconds_{name}"] = round(time.perf_counter() - t0, 3)
        out[name] = [float(s) for s in score] if name == "bleu" else float(score)
    print(json.dumps(out), flush=True)


def device_times(iters, nk):
    import torch
    from spacap3d_amd.caption_eval import LMAX, CaptionCorpus, CaptionEval
    dev = "cuda:0"
    refs, cands = make(nk)
    corpus, _ = strings(refs, cands)
    w2i = {word(i): i for i in range(V)}
    n_items, n_obj = nk // 8 + 1, 8
    key_of = np.arange(n_items * n_obj).reshape(n_items, n_obj)
    key_of = np.where(key_of < nk, key_of, -1)
    t_setup = time.perf_counter()
    co = CaptionCorpus(corpus, w2i, key_of=key_of, device=dev)
    t_setup = time.perf_counter() - t_setup
    ce = CaptionEval(co, SOS, EOS)
    rng = np.random.default_rng(0)
    tokens = rng.integers(4, V, (B, K, L))
    tokens[np.arange(B)[:, None], np.arange(K)[None], rng.integers(2, L, (B, K))] = EOS
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = {"lang_cap": up(tokens), "dataset_idx": up(rng.integers(0, n_items, B)), "scene_object_ids": up(rng.integers(0, n_obj, (B, 128))),
         "object_assignment": up(rng.integers(0, 128, (B, K))), "nms_masks": up((rng.random((B, K)) < 0.3).astype(np.int64)),
         "good_bbox_masks": up(rng.random((B, K)) < 0.5)}
    step_us, _ = replay_us(lambda: ce.step(d, masks=d), iters, settle=20)
    print(json.dumps({"what": "CaptionEval.step", "B": B, "K": K, "L": L, "keys": nk, "device_us_per_batch": round(step_us, 2),
                      "iters": iters}), flush=True)
    tok = np.zeros((nk, LMAX), np.int32)
    for i, c in enumerate(cands):
        tok[i, :len(c)] = c
    ce.set_candidates(up(tok), up(np.array([len(c) for c in cands], np.int32)))
    score_us, _ = replay_us(ce.scores, iters, settle=20)
    print(json.dumps({"what": "scoring launch (spacap_caption_score_f64)", "keys": nk, "references": int(co.ref_len.size),
                      "device_us": round(score_us, 2), "iters": iters}), flush=True)
    ms = []
    for _ in range(7):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        m = ce.compute_metrics()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - w0) * 1e3)
    print(json.dumps({"what": "CaptionEval.compute_metrics", "keys": nk, "ms_first": round(ms[0], 3),
                      "ms_median_of_rest": round(float(np.median(ms[1:])), 3), "corpus_setup_s": round(t_setup, 3),
                      "bleu": m["bleu"], "cider": m["cider"], "rouge": m["rouge"]}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--keys", type=int, default=2068)
    p.add_argument("--reference", default=None, help="a checkout of the reference: time its three scorers on the host instead")
    a = p.parse_args()
    if a.reference:
        reference_baseline(os.path.abspath(a.reference), a.keys)
    else:
        device_times(a.iters, a.keys)


if __name__ == "__main__":
    main()
