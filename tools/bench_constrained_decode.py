"""Device time of constrained caption decoding beside the unconstrained decoders at cfg2's decode shape
(8 scenes x 256 proposals = 2 048 sequences, 31 words, V = 3 001, 6 decoder layers, d_ff 2 048), one JSON line each, in ONE
run so that the numbers share a device state:

* ``caption_decode.greedy_decode``, ``beam_decode`` (W = 3) and ``sample_decode`` (S = 5, ``top_k`` = 0) as they are;
* the same three with the example constraints: bad_words = {0, sos, unk}, min_length = 4, no_repeat_ngram = 2; and once more
  with repetition_penalty = 1.2 on top;
* the whole inference forward (detector, encoder, decoder) at 8 scenes x 40 000 points in the three modes, without and with
  the example constraints;
* the word choice of one step alone, greedy and constrained greedy, and the launch that builds the bit images.

Each is warmed up, captured in a graph and replayed between two HIP events (no host work inside); median of five groups.
Random weights and rows: the time does not depend on the values (no step reads anything back).  ``--tree DIR`` measures the
package of another checkout (one without the feature reports the unconstrained rows only).

Run:  timeout -k 10 600 python tools/bench_constrained_decode.py [--iters 5] [--tree DIR]"""
import argparse
import inspect
import json
import sys

from _eval_bench import ROOT, replay_us

B, K, V, LAYERS, N_WORDS, W, S = 8, 256, 3001, 6, 31, 3, 5


def forward_ms(a, torch, has, example):
    """The whole inference forward -- ``engine.Evaluator(model, graph=True)`` on one batch of 8 scenes x 40 000 points x 256
    proposals: detector, encoder and decoder -- per decoding mode, without and with the example constraints.  Eager calls
    between two HIP events on an idle device, the median of ``--forward-iters``: the decoder's host work is included, as in
    the README's figure for greedy decoding."""
    from _eval_bench import eager_us
    from spacap3d_amd.engine import Evaluator, synthetic_batch
    from spacap3d_amd.spacapnet import build_default
    dev = "cuda:0"
    torch.manual_seed(0)
    model = build_default(vocab_size=V, num_proposal=K, N=LAYERS).to(dev).eval()
    cap = model.caption
    batch = {"point_clouds": synthetic_batch(B, 40000, dev, seed=0, vocab=V)["point_clouds"]}
    modes = {"greedy": {}, f"beam W={W}": dict(beam_size=W), f"sample S={S}": dict(sample=dict(num_samples=S, seed=1))}
    for what, kw in modes.items():
        for name, c in [("off", {})] + ([("example", dict(constraints=example))] if has else []):
            ev = Evaluator(model, graph=True, **kw, **c)
            for _ in range(3):
                ev(dict(batch))
            us = eager_us(lambda: ev(dict(batch)), a.forward_iters)
            print(json.dumps(dict(tree=a.tree, what="inference forward, " + what, constraints=name, scenes=B, points=40000, proposals=K,
                                  iters=a.forward_iters, ms=round(us / 1e3, 3))), flush=True)
            for k in ("beam_size", "num_samples", "temperature", "top_k", "top_p", "sample_seed", "min_length", "no_repeat_ngram",
                      "repetition_penalty", "bad_words"):
                cap.__dict__.pop(k, None)
            del ev
            torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--word-iters", type=int, default=50)
    p.add_argument("--forward-iters", type=int, default=20)
    p.add_argument("--tree", default=ROOT)
    a = p.parse_args()
    sys.path.insert(0, a.tree)
    import torch
    from spacap3d_amd import caption_decode as cd
    from spacap3d_amd.spacapnet import build_default
    dev = "cuda:0"
    torch.manual_seed(0)
    cap = build_default(vocab_size=V, num_proposal=K, N=LAYERS).to(dev).eval().caption
    m = cap.model
    embed, pos = m.tgt_embed[0], m.tgt_embed[1]
    sos, eos, unk = cap.word_to_idx["sos"], cap.word_to_idx["eos"], cap.word_to_idx["unk"]
    R = B * K
    indicator = torch.randn(R, 128, device=dev)
    assert cd.decode_supported(m.decoder.layers, indicator, N_WORDS)
    has = "constraints" in inspect.signature(cd.greedy_decode).parameters
    example = dict(bad_words=(0, sos, unk), min_length=4, no_repeat_ngram=2)
    sets = [("off", None)] + ([("example", example), ("example + penalty 1.2", dict(example, repetition_penalty=1.2))] if has else [])
    shape = {"tree": a.tree, "sequences": R, "words": N_WORDS, "V": V, "layers": LAYERS, "iters": a.iters}
    args = (m.decoder, m.generator, embed, pos.pe, indicator, sos)
    base = {}
    with torch.no_grad():
        for name, c in sets:
            kw = {} if c is None else dict(constraints=c)
            calls = {"greedy": lambda: cd.greedy_decode(*args, N_WORDS, **(dict(kw, eos=eos) if kw else {})),
                     f"beam W={W}": lambda: cd.beam_decode(*args, eos, N_WORDS, W, **kw),
                     f"sample S={S}": lambda: cd.sample_decode(*args, eos, N_WORDS, S, 1.0, 0, seed=1, **kw)}
            for what, fn in calls.items():
                us, _ = replay_us(fn, a.iters, settle=2)
                base.setdefault(what, us)
                print(json.dumps(dict(shape, what=what, constraints=name, device_ms=round(us / 1e3, 3),
                                      times_off=round(us / base[what], 3), times_greedy=round(us / base["greedy"], 3))), flush=True)
                torch.cuda.empty_cache()
        if not has:
            forward_ms(a, torch, has, example)
            return
        # the word choice of one step alone
        from spacap3d_amd._native import check, lib
        from spacap3d_amd.linear import bf3_pieces
        Vv = m.generator.proj.weight.shape[0]
        x = torch.randn(R, 128, device=dev)
        Wp, bias, lut = bf3_pieces(m.generator.proj.weight.contiguous()), m.generator.proj.bias.contiguous(), embed.lut.weight.contiguous()
        pe_row, scale = pos.pe[0, 5].contiguous(), float(embed.d_model) ** 0.5
        ys = torch.randint(4, Vv, (R, N_WORDS), device=dev)
        xw = torch.empty(R, 128, device=dev)
        ws = torch.empty(int(lib.spacap_decode_word_workspace_bytes(R, Vv)), dtype=torch.uint8, device=dev)
        con = cd._constrained("bench", example, R, Vv, N_WORDS, eos, dev)      # the images' buffer and the launch that fills it
        st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

        def word(constrained):
            if constrained:
                check(lib.spacap_decode_word_constrained_f32(x.data_ptr(), Wp.data_ptr(), bias.data_ptr(), R, Vv, con.bits, 1.2, lut.data_ptr(),
                                                             scale, pe_row.data_ptr(), ys.data_ptr(), N_WORDS, 20, xw.data_ptr(), ws.data_ptr(),
                                                             st()), "spacap_decode_word_constrained_f32")
            else:
                check(lib.spacap_decode_word_f32(x.data_ptr(), Wp.data_ptr(), bias.data_ptr(), R, Vv, lut.data_ptr(), scale, pe_row.data_ptr(),
                                                 ys.data_ptr(), N_WORDS, 20, xw.data_ptr(), ws.data_ptr(), st()), "spacap_decode_word_f32")

        for what, fn in (("word choice, greedy", lambda: word(False)), ("bit images, step 20", lambda: con.refresh(20, R, st(), ys=ys)),
                         ("word choice, constrained greedy", lambda: word(True))):
            us, _ = replay_us(fn, a.word_iters, settle=2)
            print(json.dumps(dict(what=what, sequences=R, V=Vv, iters=a.word_iters, device_us=round(us, 2))), flush=True)
        forward_ms(a, torch, has, example)


if __name__ == "__main__":
    main()
