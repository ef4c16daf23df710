"""Device time of the self-critical training pieces (DESIGN.md sections 7j and 7l) at cfg2's shape -- 8 scenes, S = 5 samples,
W = 31 words, V = 3 001 --, one JSON line each, in ONE run so that the numbers share a device state:

* the reward launch (``spacap_caption_reward_f64``) over the 40 drawn captions, 5 references of ~12 words per key; the same rows
  through ``spacap_caption_reward_mix_f64`` at weights (1, 0, 0) and with all three terms;
* the self-critical loss forward + backward (``spacap_scst_loss_fwd_f32`` / ``_bwd_f32``) beside the cross-entropy caption head
  (``spacap_cap_loss_fwd_f32`` / ``_bwd_f32``) at the same (rows, W, V) = (40, 31, 3 001): the yardstick, which moves one more
  (rows, W, V) image each way;
* the mixed loss pair (``spacap_mixed_cap_loss_fwd_f32`` / ``_bwd_f32``) over (8 + 40, 31, 3 001) beside what it replaces: the
  cross-entropy pair over the 8 ground-truth rows plus the self-critical pair over the 40 sample rows;
* one eager ``Trainer.step`` without ``self_critical``, with it, and with the mixed settings (synchronised eager calls: host work
  included; ``--step-iters 0`` skips them).

The kernels are warmed up, captured in a graph and replayed between two HIP events (no host work inside); median of five
groups.  Random inputs: no time depends on the values except the lengths (every row counts all W positions here: the most).

Run:  timeout -k 10 600 python tools/bench_self_critical.py [--iters 50] [--step-iters 5] [--points 40000]"""
import argparse
import json
import sys

import numpy as np

from _eval_bench import ROOT, eager_us, replay_us

sys.path.insert(0, ROOT)
B, S, W, V, K, LAYERS = 8, 5, 31, 3001, 256, 6


def corpus_for(cap, n_keys, rng):
    from spacap3d_amd.caption_eval import CaptionCorpus
    idx2word = {i: w for w, i in cap.word_to_idx.items()}
    corpus = {"k%d" % k: ["sos " + " ".join(idx2word[int(t)] for t in rng.integers(4, V, 12)) + " eos" for _ in range(5)]
              for k in range(n_keys)}
    table = np.full((n_keys, 4), -1, np.int32)
    table[:, 3] = np.arange(n_keys)
    return CaptionCorpus(corpus, cap.word_to_idx, key_of=table)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--step-iters", type=int, default=5)
    p.add_argument("--points", type=int, default=40000)
    a = p.parse_args()
    import torch
    from spacap3d_amd import synthetic
    from spacap3d_amd._native import check, lib
    from spacap3d_amd.engine import Trainer, synthetic_batch
    from spacap3d_amd.self_critical import SelfCritical
    from spacap3d_amd.spacapnet import build_default
    dev = "cuda:0"
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    model = build_default(vocab_size=V, num_proposal=K, N=LAYERS).to(dev).train()
    cap = model.caption
    sos, eos = cap.word_to_idx["sos"], cap.word_to_idx["eos"]
    sc = SelfCritical(corpus_for(cap, B, rng), sos, eos, num_samples=S)
    R = B * S
    shape = {"scenes": B, "S": S, "W": W, "V": V}

    # the reward launch
    tokens = torch.from_numpy(rng.integers(4, V, (R, W))).to(dev)
    didx, oid = torch.arange(B, device=dev), torch.full((B,), 3, device=dev)
    out = sc.rewards(tokens, didx, oid, S)
    us, _ = replay_us(lambda: sc.rewards(tokens, didx, oid, S, out=out), a.iters, settle=2)
    print(json.dumps(dict(shape, what="reward launch", rows=R, iters=a.iters, device_us=round(us, 2))), flush=True)
    for what, reward in (("mixed reward launch, weights (1, 0, 0)", {"cider": 1.0}),
                         ("mixed reward launch, all three terms", {"cider": 1.0, "bleu4": 1.0, "rouge": 1.0})):
        mx = SelfCritical(sc.corpus, sos, eos, num_samples=S, reward=reward)
        out6 = mx.rewards(tokens, didx, oid, S, terms=True)
        out6 = out6[:4] + (out6[4].t(), out6[5])
        us, _ = replay_us(lambda: mx.rewards(tokens, didx, oid, S, out=out6, terms=True), a.iters, settle=2)
        print(json.dumps(dict(shape, what=what, rows=R, iters=a.iters, device_us=round(us, 2))), flush=True)

    # the loss kernels beside the cross-entropy caption head at the same (rows, W, V)
    st = lambda: torch.cuda.current_stream().cuda_stream
    logits = torch.randn(R, W, V, device=dev)
    words = torch.from_numpy(rng.integers(1, V, (R, W + 1))).to(dev)
    length = torch.full((R,), W, dtype=torch.int32, device=dev)
    reward, base = torch.rand(R, dtype=torch.float64, device=dev), torch.rand(B, dtype=torch.float64, device=dev)
    ones = torch.ones(R, dtype=torch.uint8, device=dev)
    pair, hit = torch.empty(R, W, 2, device=dev), torch.empty(R, W, dtype=torch.uint8, device=dev)
    adv, rowlogp, o8 = torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty(8, device=dev)
    dlogits, logp = torch.empty_like(logits), torch.empty_like(logits)
    rowstat, o4, gl = torch.empty(R * W, 4, device=dev), torch.empty(4, device=dev), torch.ones(1, device=dev)
    wsc = words[:, :W].contiguous()

    def scst():
        check(lib.spacap_scst_loss_fwd_f32(logits.data_ptr(), wsc.data_ptr(), length.data_ptr(), reward.data_ptr(), base.data_ptr(),
                                           ones.data_ptr(), R, S, W, V, pair.data_ptr(), hit.data_ptr(), adv.data_ptr(), rowlogp.data_ptr(),
                                           o8.data_ptr(), st()), "spacap_scst_loss_fwd_f32")
        check(lib.spacap_scst_loss_bwd_f32(logits.data_ptr(), wsc.data_ptr(), length.data_ptr(), pair.data_ptr(), adv.data_ptr(),
                                           o8.data_ptr(), gl.data_ptr(), R, W, V, dlogits.data_ptr(), st()), "spacap_scst_loss_bwd_f32")

    def ce():
        check(lib.spacap_cap_loss_fwd_f32(logits.data_ptr(), words.data_ptr() + 8, ones.data_ptr(), R, W, V, W + 1, logp.data_ptr(),
                                          rowstat.data_ptr(), o4.data_ptr(), st()), "spacap_cap_loss_fwd_f32")
        check(lib.spacap_cap_loss_bwd_f32(logp.data_ptr(), words.data_ptr() + 8, ones.data_ptr(), o4.data_ptr(), gl.data_ptr(), R, W, V,
                                          W + 1, dlogits.data_ptr(), st()), "spacap_cap_loss_bwd_f32")

    us_ce, _ = replay_us(ce, a.iters, settle=2)
    us_sc, _ = replay_us(scst, a.iters, settle=2)
    print(json.dumps(dict(shape, what="cross-entropy caption head, forward + backward", rows=R, iters=a.iters,
                          device_us=round(us_ce, 2))), flush=True)
    print(json.dumps(dict(shape, what="self-critical loss, forward + backward", rows=R, iters=a.iters, device_us=round(us_sc, 2),
                          times_cross_entropy=round(us_sc / us_ce, 3))), flush=True)

    # the mixed pair over B ground-truth rows + R sample rows beside the two pairs it replaces
    N = B + R
    logits_n = torch.randn(N, W, V, device=dev)
    good = torch.ones(B, dtype=torch.uint8, device=dev)
    pair_n, hit_n = torch.empty(N, W, 2, device=dev), torch.empty(N, W, dtype=torch.uint8, device=dev)
    dlogits_n, o12 = torch.empty_like(logits_n), torch.empty(12, device=dev)
    tail = logits_n[B:]

    def mixed():
        check(lib.spacap_mixed_cap_loss_fwd_f32(logits_n.data_ptr(), words.data_ptr() + 8, W + 1, good.data_ptr(), B, W, wsc.data_ptr(),
                                                length.data_ptr(), reward.data_ptr(), base.data_ptr(), ones.data_ptr(), R, S, W, V, 0.5,
                                                pair_n.data_ptr(), hit_n.data_ptr(), adv.data_ptr(), rowlogp.data_ptr(), o12.data_ptr(),
                                                st()), "spacap_mixed_cap_loss_fwd_f32")
        check(lib.spacap_mixed_cap_loss_bwd_f32(logits_n.data_ptr(), words.data_ptr() + 8, W + 1, good.data_ptr(), B, W, wsc.data_ptr(),
                                                length.data_ptr(), pair_n.data_ptr(), adv.data_ptr(), o12.data_ptr(), gl.data_ptr(), R, W,
                                                V, 0.5, dlogits_n.data_ptr(), st()), "spacap_mixed_cap_loss_bwd_f32")

    def two_pairs():
        check(lib.spacap_cap_loss_fwd_f32(logits_n.data_ptr(), words.data_ptr() + 8, good.data_ptr(), B, W, V, W + 1, logp.data_ptr(),
                                          rowstat.data_ptr(), o4.data_ptr(), st()), "spacap_cap_loss_fwd_f32")
        check(lib.spacap_cap_loss_bwd_f32(logp.data_ptr(), words.data_ptr() + 8, good.data_ptr(), o4.data_ptr(), gl.data_ptr(), B, W, V,
                                          W + 1, dlogits_n.data_ptr(), st()), "spacap_cap_loss_bwd_f32")
        check(lib.spacap_scst_loss_fwd_f32(tail.data_ptr(), wsc.data_ptr(), length.data_ptr(), reward.data_ptr(), base.data_ptr(),
                                           ones.data_ptr(), R, S, W, V, pair.data_ptr(), hit.data_ptr(), adv.data_ptr(), rowlogp.data_ptr(),
                                           o8.data_ptr(), st()), "spacap_scst_loss_fwd_f32")
        check(lib.spacap_scst_loss_bwd_f32(tail.data_ptr(), wsc.data_ptr(), length.data_ptr(), pair.data_ptr(), adv.data_ptr(),
                                           o8.data_ptr(), gl.data_ptr(), R, W, V, dlogits_n[B:].data_ptr(), st()), "spacap_scst_loss_bwd_f32")

    us_two, _ = replay_us(two_pairs, a.iters, settle=2)
    us_mx, _ = replay_us(mixed, a.iters, settle=2)
    print(json.dumps(dict(shape, what="cross-entropy pair over 8 rows + self-critical pair over 40 rows", rows=N, iters=a.iters,
                          device_us=round(us_two, 2))), flush=True)
    print(json.dumps(dict(shape, what="mixed loss, forward + backward", rows=N, iters=a.iters, device_us=round(us_mx, 2),
                          times_two_pairs=round(us_mx / us_two, 3))), flush=True)
    if a.step_iters <= 0:
        return

    # one eager Trainer.step without the attribute, with it, and with the mixed settings
    data = synthetic_batch(B, a.points, dev, seed=0, vocab=V)
    data["dataset_idx"], data["object_id"] = didx, oid
    mixed_sc = SelfCritical(sc.corpus, sos, eos, num_samples=S, reward={"cider": 1.0, "bleu4": 1.0, "rouge": 1.0}, xe_weight=0.5)
    for name, attr in (("cross-entropy", None), ("self-critical", sc), ("self-critical, mixed reward + cross-entropy term", mixed_sc)):
        torch.manual_seed(0)
        m = build_default(vocab_size=V, num_proposal=K, N=LAYERS).to(dev).train()
        if attr is not None:
            m.caption.self_critical = attr
        tr = Trainer(m, synthetic.mean_size_arr().numpy())
        for _ in range(3):
            tr.step(data)
        us = eager_us(lambda: tr.step(data), a.step_iters)
        print(json.dumps(dict(shape, what="eager Trainer.step, " + name, points=a.points, iters=a.step_iters,
                              ms=round(us / 1e3, 3))), flush=True)
        del tr, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
