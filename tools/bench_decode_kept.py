"""Device time of caption decoding over the kept proposals only at cfg2's decode shape (8 scenes x 256
proposals, 31 words, V = 3 001, 6 decoder layers, d_ff 2 048), one JSON line each, in ONE run so that the numbers share a
device state:

* the yardstick: ``caption_decode.greedy_decode`` and ``caption_decode.beam_decode`` (W = 3, 5, 8) over all 2 048 rows, as the
  unmasked forward calls them;
* the masked path -- ``decode_select.select`` + ``gather``, the same decoder on the packed rows, ``scatter_words`` /
  ``scatter_values`` -- for random masks at kept fractions 1.0, 0.5, 0.25 and 0.125, the capacity equal to the count;
* the three new launches alone.

Each is warmed up, captured in a graph and replayed between two HIP events (no host work inside); median of five groups.
Random weights, rows and masks: the time does not depend on the values (no step reads anything back).  ``ffn`` names the
feed-forward kernel the row count selects (tf_layer.FFN_BF3_MIN_ROWS).

Run:  timeout -k 10 900 python tools/bench_decode_kept.py [--iters 5] [--widths 3,5,8] [--fractions 1.0,0.5,0.25,0.125]"""
import argparse
import json
import sys

from _eval_bench import ROOT, replay_us

sys.path.insert(0, ROOT)
B, K, V, LAYERS, N_WORDS = 8, 256, 3001, 6, 31


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--widths", default="3,5,8")
    p.add_argument("--fractions", default="1.0,0.5,0.25,0.125")
    a = p.parse_args()
    import torch
    from spacap3d_amd import caption_decode as cd
    from spacap3d_amd import decode_select as ds
    from spacap3d_amd import tf_layer
    from spacap3d_amd.spacapnet import build_default
    dev = "cuda:0"
    torch.manual_seed(0)
    cap = build_default(vocab_size=V, num_proposal=K, N=LAYERS).to(dev).eval().caption
    m = cap.model
    embed, pos = m.tgt_embed[0], m.tgt_embed[1]
    sos, eos = cap.word_to_idx["sos"], cap.word_to_idx["eos"]
    n = B * K
    obj, mem = torch.randn(n, 128, device=dev), torch.randn(n, 128, device=dev)
    indicator = obj + mem
    assert cd.decode_supported(m.decoder.layers, indicator, N_WORDS)
    widths = [1] + [int(w) for w in a.widths.split(",")]          # 1 = greedy_decode
    shape = {"proposals": n, "words": N_WORDS, "V": V, "layers": LAYERS, "iters": a.iters}
    ffn = lambda rows: "split-bf16" if tf_layer.FFN_BF3 and rows > tf_layer.FFN_BF3_MIN_ROWS else "fp32"  # noqa: E731

    def decode(ind, W):
        if W == 1:
            return (cd.greedy_decode(m.decoder, m.generator, embed, pos.pe, ind, sos, N_WORDS),)
        return cd.beam_decode(m.decoder, m.generator, embed, pos.pe, ind, sos, eos, N_WORDS, W)

    def masked(mask, capacity, W):
        rows, slot, _ = ds.select(mask, capacity)
        got = decode(ds.gather(obj, mem, rows), W)
        out = [ds.scatter_words(got[0], slot, eos)]
        if W > 1:
            out.append(ds.scatter_values(got[1], slot, 0.0))
        return out

    yard = {}
    with torch.no_grad():
        for W in widths:
            yard[W], _ = replay_us(lambda: decode(indicator, W), a.iters, settle=2)
            print(json.dumps(dict(shape, what="all rows", W=W, rows=n * W, ffn=ffn(n * W), device_ms=round(yard[W] / 1e3, 3),
                                  us_per_row=round(yard[W] / (n * W), 3))), flush=True)
            torch.cuda.empty_cache()
        g = torch.Generator().manual_seed(1)
        for frac in (float(f) for f in a.fractions.split(",")):
            count = max(1, int(round(frac * n)))
            mask = torch.zeros(n, dtype=torch.bool)
            mask[torch.randperm(n, generator=g)[:count]] = True
            mask = mask.view(B, K).to(dev)
            for W in widths:
                us, out = replay_us(lambda: masked(mask, count, W), a.iters, settle=2)
                print(json.dumps(dict(shape, what="kept rows", kept_fraction=frac, W=W, rows=count * W, ffn=ffn(count * W),
                                      device_ms=round(us / 1e3, 3), us_per_row=round(us / (count * W), 3),
                                      times_all_rows=round(us / yard[W], 3))), flush=True)
                del out
                torch.cuda.empty_cache()
        # the three new launches alone, at half the proposals kept
        count = n // 2
        mask = (torch.arange(n, device=dev) % 2 == 0).view(B, K)
        rows, slot, _ = ds.select(mask, count)
        ys = torch.zeros(count, N_WORDS, dtype=torch.long, device=dev)
        for what, fn in (("select", lambda: ds.select(mask, count)), ("gather", lambda: ds.gather(obj, mem, rows)),
                         ("scatter_words", lambda: ds.scatter_words(ys, slot, eos))):
            us, _ = replay_us(fn, 50, settle=2)
            print(json.dumps(dict(what=what, proposals=n, capacity=count, device_us=round(us, 2))), flush=True)


if __name__ == "__main__":
    main()
