"""Device time of the pieces of self-critical training over every matched object of a scene at cfg2's
shape -- 8 scenes, K = 256 proposals, G = 128 object slots, M = 16 groups a scene, S = 5 samples, T = 33 token columns,
V = 3 001 --, one JSON line each, in ONE run so that the numbers share a device state:

* the selection launch (``spacap_scst_select_f32``), every scene with 32 annotated objects near a proposal;
* the row-indexed decoder input forward + backward (``spacap_caption_prep_rows_fwd_f32`` / ``_bwd_f32``) at 640 rows, beside
  what it replaces: the M S-fold ``repeat_interleave`` of xyz / src / memory, ``spacap_caption_prep_fwd_f32`` / ``_bwd_f32`` at
  640 rows and the sum of the 80 copies of the (K, D) gradient slab a scene that autograd's expand-backward does;
* one eager ``Trainer.step`` in referred and in matched mode (synchronised eager calls: host work included).

The kernels are warmed up, captured in a graph and replayed between two HIP events (no host work inside); median of five
groups.  Random inputs: no time depends on the values (empty groups run their rows like filled ones).

Run:  timeout -k 10 600 python tools/bench_scene_scst.py [--iters 50] [--step-iters 5] [--points 40000]"""
import argparse
import json
import sys

import numpy as np

from _eval_bench import ROOT, eager_us, replay_us

sys.path.insert(0, ROOT)
B, K, G, M, S, D, T, V, LAYERS, N_GT, ID0 = 8, 256, 128, 16, 5, 128, 33, 3001, 6, 32, 3


def corpus_for(cap, rng):
    """a key row for each of the N_GT annotated objects of every scene, 5 references of 12 words each"""
    from spacap3d_amd.caption_eval import CaptionCorpus
    idx2word = {i: w for w, i in cap.word_to_idx.items()}
    n = B * N_GT
    corpus = {"k%d" % k: ["sos " + " ".join(idx2word[int(t)] for t in rng.integers(4, V, 12)) + " eos" for _ in range(5)] for k in range(n)}
    table = np.full((B, G + ID0), -1, np.int32)
    table[:, ID0:ID0 + N_GT] = np.arange(n).reshape(B, N_GT)
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
    from spacap3d_amd.attention import rng_state
    from spacap3d_amd.engine import Trainer, synthetic_batch
    from spacap3d_amd.self_critical import SelfCritical
    from spacap3d_amd.spacapnet import build_default
    dev = "cuda:0"
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    model = build_default(vocab_size=V, num_proposal=K, N=LAYERS).to(dev).train()
    cap = model.caption
    sos, eos = cap.word_to_idx["sos"], cap.word_to_idx["eos"]
    corpus = corpus_for(cap, rng)
    mk = lambda mode: SelfCritical(corpus, sos, eos, num_samples=S, proposals=mode, max_proposals=M)
    sc = mk("matched")
    shape = {"scenes": B, "K": K, "G": G, "M": M, "S": S, "T": T, "V": V}
    R, L = B * M * S, T - 1

    # the selection launch: 32 objects a scene within 0.05 m of a proposal each
    xyz = torch.rand(B, K, 3, device=dev) * 5.0
    center = torch.zeros(B, G, 3, device=dev)
    center[:, :N_GT] = xyz[:, torch.randperm(K, device=dev)[:N_GT]] + 0.05 * torch.randn(B, N_GT, 3, device=dev)
    lmask = torch.zeros(B, G, device=dev)
    lmask[:, :N_GT] = 1
    ids, didx = (torch.arange(G, device=dev) + ID0).repeat(B, 1), torch.arange(B, device=dev)
    out = sc.select(xyz, center, lmask, ids, didx)
    us, _ = replay_us(lambda: sc.select(xyz, center, lmask, ids, didx, out=out), a.iters, settle=2)
    torch.cuda.synchronize()
    print(json.dumps(dict(shape, what="selection launch", filled=int(out[5].sum()), iters=a.iters, device_us=round(us, 2))), flush=True)

    # the row-indexed decoder input beside the copies and the nearest-centre kernel it replaces
    st = lambda: torch.cuda.current_stream().cuda_stream
    sdev = rng_state(torch.device(dev)).data_ptr()
    src, mem = torch.randn(B, K, D, device=dev), torch.randn(B, K, D, device=dev)
    prop = out[0].reshape(-1).clone()
    tok = torch.from_numpy(rng.integers(1, V, (R, T))).to(dev)
    emb, pe = cap.model.tgt_embed[0].lut.weight.detach().contiguous(), cap.model.tgt_embed[1].pe[0].contiguous()
    g = torch.randn(R, L, D, device=dev)
    x0, m8 = torch.empty(R, L, D, device=dev), torch.empty(R, L, L, dtype=torch.uint8, device=dev)
    d_rows, d_emb = torch.empty(B, K, D, device=dev), torch.empty(V, D, device=dev)
    p_drop, seed = 0.1, 12345

    def rows():
        check(lib.spacap_caption_prep_rows_fwd_f32(src.data_ptr(), mem.data_ptr(), prop.data_ptr(), tok.data_ptr(), emb.data_ptr(),
                                                   pe.data_ptr(), B, K, M, S, D, T, V, p_drop, seed, sdev, x0.data_ptr(), m8.data_ptr(),
                                                   st()), "spacap_caption_prep_rows_fwd_f32")
        check(lib.spacap_caption_prep_rows_bwd_f32(g.data_ptr(), tok.data_ptr(), prop.data_ptr(), B, K, M, S, D, T, V, p_drop, seed, sdev,
                                                   d_rows.data_ptr(), d_emb.data_ptr(), st()), "spacap_caption_prep_rows_bwd_f32")

    idx, dist, pred = torch.empty(R, dtype=torch.int64, device=dev), torch.empty(R, device=dev), torch.empty(1, device=dev)
    good, ticket = torch.empty(R, dtype=torch.bool, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    ref = xyz[torch.arange(B, device=dev).repeat_interleave(M * S), prop.clamp(min=0).repeat_interleave(S)].contiguous()

    def copies():
        xr, sr, mr = (t.repeat_interleave(M * S, 0) for t in (xyz, src, mem))
        check(lib.spacap_caption_prep_fwd_f32(xr.data_ptr(), ref.data_ptr(), sr.data_ptr(), mr.data_ptr(), tok.data_ptr(), emb.data_ptr(),
                                              pe.data_ptr(), R, K, D, T, V, p_drop, seed, sdev, x0.data_ptr(), m8.data_ptr(), idx.data_ptr(),
                                              dist.data_ptr(), good.data_ptr(), pred.data_ptr(), ticket.data_ptr(), st()),
              "spacap_caption_prep_fwd_f32")
        dr = torch.empty(R, K, D, device=dev)
        check(lib.spacap_caption_prep_bwd_f32(g.data_ptr(), tok.data_ptr(), idx.data_ptr(), R, K, D, T, V, p_drop, seed, sdev, dr.data_ptr(),
                                              d_emb.data_ptr(), st()), "spacap_caption_prep_bwd_f32")
        return dr.view(B, M * S, K, D).sum(1)

    us_rows, _ = replay_us(rows, a.iters, settle=2)
    us_copy, _ = replay_us(copies, a.iters, settle=2)
    print(json.dumps(dict(shape, what="row-indexed decoder input, forward + backward", rows=R, iters=a.iters,
                          device_us=round(us_rows, 2))), flush=True)
    print(json.dumps(dict(shape, what="M S-fold copies + nearest-centre decoder input, forward + backward + slab sum", rows=R,
                          iters=a.iters, device_us=round(us_copy, 2), times_row_indexed=round(us_copy / us_rows, 2))), flush=True)
    del g, x0, m8

    # one eager Trainer.step in both modes
    data = synthetic_batch(B, a.points, dev, seed=0, vocab=V)
    data["dataset_idx"], data["object_id"] = didx, torch.full((B,), ID0, device=dev)
    data["scene_object_ids"] = ids
    for name in ("referred", "matched"):
        torch.manual_seed(0)
        m = build_default(vocab_size=V, num_proposal=K, N=LAYERS).to(dev).train()
        m.caption.self_critical = mk(name)
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
