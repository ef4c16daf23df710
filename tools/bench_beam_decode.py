"""Device time of caption decoding at cfg2's decode shape (8 scenes x 256 proposals = 2 048 sequences, 31 words, V = 3 001,
6 decoder layers, d_ff 2 048), one JSON line each, in ONE run so that the numbers share a device state:

* ``caption_decode.greedy_decode`` -- the yardstick: today's greedy loop;
* ``caption_decode.beam_decode`` for W = 1, 3, 5 (csrc/caption_decode.hip).

Each decode is warmed up, captured in a graph and replayed between two HIP events (no host work inside); median of five
groups.  Random weights and indicator rows: the time does not depend on the values (no step reads anything back).

Run:  timeout -k 10 600 python tools/bench_beam_decode.py [--iters 5] [--widths 1,3,5]"""
import argparse
import json
import sys

from _eval_bench import ROOT, replay_us

sys.path.insert(0, ROOT)
B, K, V, LAYERS, N_WORDS = 8, 256, 3001, 6, 31


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--widths", default="1,3,5")
    a = p.parse_args()
    import torch
    from spacap3d_amd import caption_decode
    from spacap3d_amd.spacapnet import build_default
    dev = "cuda:0"
    torch.manual_seed(0)
    cap = build_default(vocab_size=V, num_proposal=K, N=LAYERS).to(dev).eval().caption
    m = cap.model
    embed, pos = m.tgt_embed[0], m.tgt_embed[1]
    sos, eos = cap.word_to_idx["sos"], cap.word_to_idx["eos"]
    R = B * K
    indicator = torch.randn(R, 128, device=dev)
    assert caption_decode.decode_supported(m.decoder.layers, indicator, N_WORDS)
    shape = {"sequences": R, "words": N_WORDS, "V": V, "layers": LAYERS, "iters": a.iters}
    with torch.no_grad():
        us, ys = replay_us(lambda: caption_decode.greedy_decode(m.decoder, m.generator, embed, pos.pe, indicator, sos, N_WORDS), a.iters, settle=2)
        greedy = us
        print(json.dumps(dict(shape, what="greedy_decode", device_ms=round(us / 1e3, 3))), flush=True)
        for W in (int(w) for w in a.widths.split(",")):
            us, out = replay_us(lambda: caption_decode.beam_decode(m.decoder, m.generator, embed, pos.pe, indicator, sos, eos, N_WORDS, W),
                                a.iters, settle=2)
            same = float((out[0] == ys).float().mean())
            print(json.dumps(dict(shape, what="beam_decode", W=W, device_ms=round(us / 1e3, 3), times_greedy=round(us / greedy, 2),
                                  cache_GiB=round(12 * R * W * (N_WORDS + 1) * 512 / 2**30, 2), words_equal_to_greedy=round(same, 4))),
                  flush=True)
            del out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
