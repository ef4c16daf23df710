"""Device time of sampled caption decoding beside the greedy decoder at cfg2's decode shape (8 scenes x 256 proposals = 2 048
sequences, 31 words, V = 3 001, 6 decoder layers, d_ff 2 048), one JSON line each, in ONE run so that the numbers share a
device state:

* ``caption_decode.greedy_decode`` -- the yardstick;
* ``caption_decode.sample_decode`` at S = 1 with ``top_k`` = 0, with ``top_k`` = 8, and with ``top_p`` = 0.9 and 0.5;
* the word choice of one step alone for each: ``spacap_decode_word_f32``, ``spacap_sample_word_f32`` with ``top_k`` = 0 and
  with ``top_k`` = 8, ``spacap_sample_word_nucleus_f32`` with ``top_p`` = 0.9 and 0.5, on one set of decoder output rows.

Each is warmed up, captured in a graph and replayed between two HIP events (no host work inside); median of five groups.
Random weights and rows: the time does not depend on the values (no step reads anything back).

Run:  timeout -k 10 600 python tools/bench_sample_decode.py [--iters 5] [--word-iters 50]"""
import argparse
import json
import sys

from _eval_bench import ROOT, replay_us

sys.path.insert(0, ROOT)
B, K, V, LAYERS, N_WORDS = 8, 256, 3001, 6, 31


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--word-iters", type=int, default=50)
    a = p.parse_args()
    import torch
    from spacap3d_amd import caption_decode
    from spacap3d_amd._native import check, lib
    from spacap3d_amd.linear import bf3_pieces
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
    shape = {"sequences": R, "words": N_WORDS, "V": V, "layers": LAYERS}
    with torch.no_grad():
        greedy, _ = replay_us(lambda: caption_decode.greedy_decode(m.decoder, m.generator, embed, pos.pe, indicator, sos, N_WORDS), a.iters, settle=2)
        print(json.dumps(dict(shape, what="greedy_decode", iters=a.iters, device_ms=round(greedy / 1e3, 3))), flush=True)
        for k in (0, 8):
            us, _ = replay_us(lambda: caption_decode.sample_decode(m.decoder, m.generator, embed, pos.pe, indicator, sos, eos, N_WORDS, 1, 1.0,
                                                                   k, seed=1), a.iters, settle=2)
            print(json.dumps(dict(shape, what="sample_decode", S=1, top_k=k, iters=a.iters, device_ms=round(us / 1e3, 3),
                                  times_greedy=round(us / greedy, 3))), flush=True)
            torch.cuda.empty_cache()
        for top_p in (0.9, 0.5):
            us, _ = replay_us(lambda: caption_decode.sample_decode(m.decoder, m.generator, embed, pos.pe, indicator, sos, eos, N_WORDS, 1, 1.0,
                                                                   0, seed=1, top_p=top_p), a.iters, settle=2)
            print(json.dumps(dict(shape, what="sample_decode", S=1, top_p=top_p, iters=a.iters, device_ms=round(us / 1e3, 3),
                                  times_greedy=round(us / greedy, 3))), flush=True)
            torch.cuda.empty_cache()
        # the word choice alone
        Vv = m.generator.proj.weight.shape[0]
        x = torch.randn(R, 128, device=dev)
        Wp, bias, lut = bf3_pieces(m.generator.proj.weight.contiguous()), m.generator.proj.bias.contiguous(), embed.lut.weight.contiguous()
        pe_row = pos.pe[0, 5].contiguous()
        ys = torch.empty(R, N_WORDS, dtype=torch.long, device=dev)
        xw = torch.empty(R, 128, device=dev)
        score = torch.zeros(R, device=dev)
        length, fin = torch.zeros(R, dtype=torch.int32, device=dev), torch.zeros(R, dtype=torch.int32, device=dev)
        ws = torch.empty(max(int(lib.spacap_decode_word_workspace_bytes(R, Vv)), int(lib.spacap_sample_word_workspace_bytes(R, Vv, 0)),
                             int(lib.spacap_sample_word_workspace_bytes(R, Vv, 8)), int(lib.spacap_sample_word_nucleus_workspace_bytes(R, Vv))),
                         dtype=torch.uint8, device=dev)
        scale = float(embed.d_model) ** 0.5

        def word_greedy():
            check(lib.spacap_decode_word_f32(x.data_ptr(), Wp.data_ptr(), bias.data_ptr(), R, Vv, lut.data_ptr(), scale, pe_row.data_ptr(),
                                             ys.data_ptr(), N_WORDS, 5, xw.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  "spacap_decode_word_f32")

        def word_sample(k):
            check(lib.spacap_sample_word_f32(x.data_ptr(), Wp.data_ptr(), bias.data_ptr(), R, Vv, k, 1.0, 1, None, N_WORDS, 5, int(eos),
                                             lut.data_ptr(), scale, pe_row.data_ptr(), ys.data_ptr(), score.data_ptr(), length.data_ptr(),
                                             fin.data_ptr(), xw.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  "spacap_sample_word_f32")

        def word_nucleus(top_p):
            check(lib.spacap_sample_word_nucleus_f32(x.data_ptr(), Wp.data_ptr(), bias.data_ptr(), R, Vv, top_p, 1.0, 1, None, N_WORDS, 5,
                                                     int(eos), lut.data_ptr(), scale, pe_row.data_ptr(), ys.data_ptr(), score.data_ptr(),
                                                     length.data_ptr(), fin.data_ptr(), xw.data_ptr(), ws.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream), "spacap_sample_word_nucleus_f32")

        wg, _ = replay_us(word_greedy, a.word_iters, settle=2)
        print(json.dumps(dict(shape, what="word choice, greedy", iters=a.word_iters, device_us=round(wg, 2))), flush=True)
        for k in (0, 8):
            us, _ = replay_us(lambda: word_sample(k), a.word_iters, settle=2)
            print(json.dumps(dict(shape, what="word choice, sampled", top_k=k, iters=a.word_iters, device_us=round(us, 2),
                                  times_greedy=round(us / wg, 3))), flush=True)
        for top_p in (0.9, 0.5):
            fin.zero_()                                   # (rows that drew eos in an earlier replay stay live: the time is a live row's)
            us, _ = replay_us(lambda: word_nucleus(top_p), a.word_iters, settle=2)
            print(json.dumps(dict(shape, what="word choice, sampled", top_p=top_p, workspace_mb=round(ws.numel() / 2 ** 20, 1),
                                  iters=a.word_iters, device_us=round(us, 2), times_greedy=round(us / wg, 3))), flush=True)


if __name__ == "__main__":
    main()
