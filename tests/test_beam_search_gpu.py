"""Beam-search decoding on the MI355X (csrc/caption_decode.hip, caption_decode.beam_decode, transformer_captioner.forward_eval)
against the float64 restatement of the contract (tests/beam_search_restated.py), the greedy decoder (a beam
of width 1) and the generic path (spacap3d_amd/beam_search.py).  The greedy decoder's own kernels and the step the two decoders
share: tests/test_caption_decode_gpu.py."""
import math

import numpy as np
import pytest
import torch

from beam_search_restated import beam_search_restated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEG = -1e9     # the log-probability of every word a hand-made list does not name (never kept: each list names W words)


@pytest.fixture(autouse=True, scope="module")
def _needs_a_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _lib():
    from spacap3d_amd._native import check, lib
    return lib, check, torch.cuda.current_stream().cuda_stream


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ---- 4. the W best log-probabilities of every row ------------------------------------------------------------------------------
TOPW_SHAPES = [(16, 64, 1), (37, 40, 3), (300, 1000, 5), (33, 3001, 8)]


def _topw(x, Wt, b, W):
    from spacap3d_amd.linear import bf3_pieces
    lib, check, st = _lib()
    rows, V = x.shape[0], Wt.shape[0]
    ws = torch.empty(int(lib.spacap_beam_topw_workspace_bytes(rows, V, W)), dtype=torch.uint8, device=DEV)
    lp = torch.full((rows, W), float("nan"), device=DEV)
    wd = torch.full((rows, W), -7, dtype=torch.int32, device=DEV)
    Wp = bf3_pieces(Wt)
    check(lib.spacap_beam_topw_f32(x.data_ptr(), Wp.data_ptr(), b.data_ptr(), rows, V, W, lp.data_ptr(), wd.data_ptr(), ws.data_ptr(), st),
          "spacap_beam_topw_f32")
    return lp.cpu().double().numpy(), wd.cpu().numpy().astype(np.int64)


def _logp64(x, Wt, b):
    logits = (x.double() @ Wt.double().t() + b.double()).cpu()
    return logits.numpy(), torch.log_softmax(logits, 1).numpy()


@pytest.mark.parametrize("rows,V,W", TOPW_SHAPES)
def test_top_w_words_of_integer_logits_are_exact(rows, V, W):
    """x, W, bias from {-2..2}: every piece product and every partial sum is an integer below 2^24, so the logits are exact
    integers with many ties -- the words must be the float64 top-W under the tie rule (the smaller word first) exactly, and
    logp = logit - lse within 1e-5 (one fp32 log and one sum of exp, each relative 1e-7, on magnitudes below 100)."""
    g = torch.Generator().manual_seed(rows + V)
    x = torch.randint(-2, 3, (rows, 128), generator=g).float().to(DEV)
    Wt = torch.randint(-2, 3, (V, 128), generator=g).float().to(DEV)
    b = torch.randint(-2, 3, (V,), generator=g).float().to(DEV)
    Wt[7] = Wt[3]
    b[7] = b[3]                                   # two identical words
    x[0] = 0.0                                    # a row whose logits are the bias: V / 5 words tie for every place
    lp, wd = _topw(x, Wt, b, W)
    logits, logp = _logp64(x, Wt, b)
    want = np.argsort(-logits, axis=1, kind="stable")[:, :W]          # stable: equal logits keep the smaller word first
    ties = int((np.sort(logits, 1)[:, ::-1][:, W - 1] == np.sort(logits, 1)[:, ::-1][:, min(W, V - 1)]).sum())
    print(f"rows with a tie across the cut: {ties} of {rows}; max |logit| {np.abs(logits).max():.0f}")
    assert np.array_equal(wd, want)
    err = np.abs(lp - np.take_along_axis(logp, want, 1)).max()
    print(f"max |logp - float64| = {err:.3g}")
    assert err < 1e-5


@pytest.mark.parametrize("rows,V,W", TOPW_SHAPES)
def test_top_w_words_of_gaussian_logits(rows, V, W):
    """Inputs as in test_decode_word_choice_without_logits.  Near-ties may swap places, so by order statistics: the i-th returned
    word's float64 log-probability is at least the i-th best one minus 1e-4 max|logit| (that test's bound for the same
    arithmetic), and every returned value is within that bound of its word's float64 value."""
    g = torch.Generator().manual_seed(rows + V)
    x = torch.randn(rows, 128, generator=g).to(DEV)
    Wt, b = (0.3 * torch.randn(V, 128, generator=g)).to(DEV), torch.randn(V, generator=g).to(DEV)
    lp, wd = _topw(x, Wt, b, W)
    logits, logp = _logp64(x, Wt, b)
    tol = 1e-4 * float(np.abs(logits).max())
    assert (wd >= 0).all() and (wd < V).all() and all(len(set(r)) == W for r in wd.tolist())
    mine = np.take_along_axis(logp, wd, 1)
    best = -np.sort(-logp, axis=1)[:, :W]
    print(f"worst place deficit {float((best - mine).max()):.3g}, worst value error {float(np.abs(lp - mine).max()):.3g}, bound {tol:.3g}")
    assert float((best - mine).max()) <= tol
    assert float(np.abs(lp - mine).max()) <= tol
    assert (np.diff(lp, axis=1) <= 0).all()


def test_top_w_refuses_a_width_it_cannot_run():
    lib, check, st = _lib()
    x, Wt, b = torch.zeros(16, 128, device=DEV), torch.zeros(3, 128, device=DEV), torch.zeros(3, device=DEV)
    from spacap3d_amd.linear import bf3_pieces
    Wp = bf3_pieces(Wt)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    lp = torch.full((16, 9), 5.0, device=DEV)
    wd = torch.full((16, 9), -7, dtype=torch.int32, device=DEV)
    for V, W in ((3, 4), (3, 9), (64, 9), (64, 0)):
        rc = lib.spacap_beam_topw_f32(x.data_ptr(), Wp.data_ptr(), b.data_ptr(), 16, V, W, lp.data_ptr(), wd.data_ptr(), ws.data_ptr(), st)
        assert rc != 0 and b"spacap_beam_topw_f32" in lib.spacap_last_error()
    torch.cuda.synchronize()
    assert bool((lp == 5.0).all()) and bool((wd == -7).all()) and bool((ws == 0).all())      # nothing was launched


# ---- 5. selection and backtracking on hand-made lists --------------------------------------------------------------------------
def _lists(R, W, V, n_words, eos, seed):
    """top-W lists [n_words][R W][W] with exactly representable log-probabilities (multiples of 1/4: equal scores abound),
    sorted as spacap_beam_topw_f32 sorts them.  Sequences r = 2 (mod 3) are never offered eos.  The first two steps of
    sequences 0 and 1 are made by hand (see the test)."""
    g = np.random.default_rng(seed)
    lp = np.zeros((n_words, R * W, W), np.float32)
    wd = np.zeros((n_words, R * W, W), np.int32)
    for s in range(n_words):
        for row in range(R * W):
            r = row // W
            words = g.choice(np.array([v for v in range(V) if v != eos or r % 3 != 2]), size=W, replace=False)
            vals = -g.integers(1, 7, size=W) / 4.0
            order = sorted(range(W), key=lambda i: (-vals[i], words[i]))
            lp[s, row], wd[s, row] = vals[order], words[order]
    return lp, wd


@pytest.mark.parametrize("R,W", [(3, 3), (70, 8)])
def test_selection_and_backtracking_equal_the_restatement(R, W):
    """spacap_beam_step_f32 n_words times, then spacap_beam_finish_f32 for alpha 0 and 0.7: state, ancestor table, trace, next
    input rows, winners and all hypotheses equal the restatement exactly.  Every output buffer is poisoned before the call
    that writes it, so an element the kernels skip shows.  Covered (asserted below on the restatement's own results): two
    dead hypotheses at the first step (always: only hypothesis 0 is alive), a finished hypothesis that stays best (sequence
    0), one that is displaced (sequence 1), equal scores across hypotheses (sequence 0, step 1), a sequence that never
    finishes (sequence 2)."""
    lib, check, st = _lib()
    V, n_words, eos, sos = 12, 6, 1, 0
    T = n_words + 1
    lp, wd = _lists(R, W, V, n_words, eos, seed=R)

    def put(s, row, head, tail=()):
        """A hand-made list: ``head``, then fillers at -4, -4.25, .. (words nobody named, never eos), then ``tail``."""
        used = {w for _, w in head + list(tail)} | {eos}
        fill = [(-4.0 - i / 4.0, w) for i, w in enumerate([v for v in range(V) if v not in used][:W - len(head) - len(tail)])]
        pairs = head + fill + list(tail)
        lp[s, row], wd[s, row] = [p for p, _ in pairs], [w for _, w in pairs]

    # sequence 0: eos is the best first word and stays best; at step 1 hypotheses 1 and 2 both reach -3.5 (the smaller parent first)
    put(0, 0, [(-0.25, eos), (-1.0, 5), (-1.5, 6)])
    put(1, 1, [(-2.0, 7), (-2.5, 8), (-3.0, 9)])
    put(1, 2, [(-2.0, 7), (-2.5, 8), (-3.0, 9)])
    # sequence 1: eos comes last at -9 and is displaced at step 1
    put(0, W, [(-0.25, 4), (-0.5, 5)], tail=[(-9.0, eos)])
    put(1, W, [(-0.25, 6), (-0.25, 7), (-1.0, 8)])
    put(1, W + 1, [(-0.25, 6), (-0.5, 7), (-1.0, 8)])
    dense = np.full((n_words, R * W, V), NEG)
    for s in range(n_words):
        np.put_along_axis(dense[s], wd[s].astype(np.int64), lp[s].astype(np.float64), 1)
    want = {a: beam_search_restated(lambda s, r, j, last, toks: dense[s, r * W + j], R, W, n_words, sos, eos, a) for a in (0.0, 0.7)}
    w0 = want[0.0]
    assert w0["finished"][0, 0] and (w0["beams"][0, 0] == eos).all() and w0["ys"][0, 0] == eos       # finished, stays best
    assert eos in w0["word"][0, 1] and eos not in w0["word"][1, 1]                                 # finished, displaced
    assert w0["parent"][1, 0].tolist()[:3] == [0, 1, 1] and (w0["gap"][1, 0] == 0 if W == 3 else w0["parent"][1, 0, 3] == 2)   # equal scores across beams
    assert eos not in w0["beams"][2] and not w0["finished"][2].any()                               # never finishes
    assert all(w["scores"].max() > NEG / 2 for w in want.values())

    g = torch.Generator().manual_seed(1)
    lut, pe = torch.randn(V, 128, generator=g).to(DEV), torch.randn(T, 128, generator=g).to(DEV)
    scale = math.sqrt(128.0)
    score = [torch.full((R, W), float("-inf"), device=DEV) for _ in range(2)]
    score[1][:, 0] = 0.0
    fin = [torch.zeros(R, W, dtype=torch.int32, device=DEV) for _ in range(2)]
    ln = [torch.zeros(R, W, dtype=torch.int32, device=DEV) for _ in range(2)]
    anc = [torch.arange(W, dtype=torch.int8, device=DEV).view(1, W, 1).expand(R, W, T).contiguous() for _ in range(2)]
    trp = torch.full((n_words, R, W), 0x55, dtype=torch.int8, device=DEV)
    trw = torch.full((n_words, R, W), -7, dtype=torch.int32, device=DEV)
    xn = torch.empty(R * W, 128, device=DEV)
    anc_want = np.broadcast_to(np.arange(W).reshape(1, W, 1), (R, W, T)).copy()
    for t in range(1, T):
        i0, i1 = t % 2, (t + 1) % 2
        score[i1].fill_(float("nan")), fin[i1].fill_(-7), ln[i1].fill_(-7), anc[i1].fill_(0x55), xn.fill_(float("nan"))
        tl, tw = torch.from_numpy(lp[t - 1]).to(DEV), torch.from_numpy(wd[t - 1]).to(DEV)
        check(lib.spacap_beam_step_f32(tl.data_ptr(), tw.data_ptr(), R, W, V, T, t, eos, score[i0].data_ptr(), fin[i0].data_ptr(),
                                       ln[i0].data_ptr(), score[i1].data_ptr(), fin[i1].data_ptr(), ln[i1].data_ptr(), anc[i0].data_ptr(),
                                       anc[i1].data_ptr(), trp.data_ptr(), trw.data_ptr(), lut.data_ptr(), scale, pe[t].data_ptr(),
                                       xn.data_ptr(), st), "spacap_beam_step_f32")
        par = w0["parent"][t - 1]
        new = np.broadcast_to(np.arange(W).reshape(1, W, 1), (R, W, T)).copy()           # positions behind t: the slot itself
        new[:, :, :t] = np.take_along_axis(anc_want, par[:, :, None], 1)[:, :, :t]
        new[:, :, t] = par
        anc_want = new
        assert np.array_equal(anc[i1].cpu().numpy(), anc_want), t
        word = torch.from_numpy(w0["word"][t - 1].reshape(-1)).to(DEV)
        assert torch.equal(xn, lut[word] * scale + pe[t]), t
    last = T % 2
    assert np.array_equal(trp.cpu().numpy(), w0["parent"]) and np.array_equal(trw.cpu().numpy(), w0["word"])
    assert np.array_equal(score[last].cpu().numpy(), w0["scores"].astype(np.float32))
    assert np.array_equal(fin[last].cpu().numpy(), w0["finished"].astype(np.int32))
    assert np.array_equal(ln[last].cpu().numpy(), w0["lengths"])
    for alpha, w in want.items():
        for give_all in (True, False):
            ys = torch.full((R, n_words), -7, dtype=torch.long, device=DEV)
            best = torch.full((R,), float("nan"), device=DEV)
            beams = torch.full((R, W, n_words), -7, dtype=torch.long, device=DEV)
            scs, lens = torch.full((R, W), float("nan"), device=DEV), torch.full((R, W), -7, dtype=torch.int32, device=DEV)
            ptr = (lambda t_: t_.data_ptr()) if give_all else (lambda t_: None)
            check(lib.spacap_beam_finish_f32(score[last].data_ptr(), ln[last].data_ptr(), trp.data_ptr(), trw.data_ptr(), R, W, n_words, alpha,
                                             ys.data_ptr(), best.data_ptr(), ptr(beams), ptr(scs), ptr(lens), st), "spacap_beam_finish_f32")
            assert np.array_equal(ys.cpu().numpy(), w["ys"]), alpha
            assert np.array_equal(best.cpu().numpy(), w["score"].astype(np.float32)), alpha
            if give_all:
                assert np.array_equal(beams.cpu().numpy(), w["beams"])
                assert np.array_equal(scs.cpu().numpy(), w["scores"].astype(np.float32)) and np.array_equal(lens.cpu().numpy(), w["lengths"])
    if R > 3:
        assert (want[0.0]["ys"] != want[0.7]["ys"]).any()      # the length penalty changes a winner somewhere


# ---- 6. attention through the ancestor table -------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,W,T", [(1, 1, 1), (2, 8, 5), (5, 3, 32)])   # one key and nothing cached; the widest table and a row stride that is not 32
def test_attention_reads_a_hypothesis_history_through_the_ancestor_table(R, W, T):
    lib, check, st = _lib()
    h, dk = 8, 16
    RW = R * W
    g = torch.Generator().manual_seed(3)
    ident = torch.arange(W, dtype=torch.int8, device=DEV).view(1, W, 1).expand(R, W, T).contiguous()
    kc, vc = torch.zeros(RW, T, 128, device=DEV), torch.zeros(RW, T, 128, device=DEV)
    kb, vb = torch.zeros(RW, T, 128, device=DEV), torch.zeros(RW, T, 128, device=DEV)
    kp, vp = torch.zeros(RW, T, 128, device=DEV), torch.zeros(RW, T, 128, device=DEV)
    out, outb, outp = (torch.empty(RW, 128, device=DEV) for _ in range(3))
    rows = []
    base = (torch.arange(R).view(R, 1, 1) * W)
    for t in range(T):
        qkv = torch.randn(RW, 384, generator=g).to(DEV)
        rows.append(qkv)
        check(lib.spacap_decode_attn_f32(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), RW, h, dk, T, t, 0.25, out.data_ptr(), st), "greedy")
        check(lib.spacap_decode_attn_beam_f32(qkv.data_ptr(), kb.data_ptr(), vb.data_ptr(), ident.data_ptr(), R, W, h, dk, T, t, 0.25,
                                              outb.data_ptr(), st), "beam, identity")
        assert torch.equal(out, outb) and torch.equal(kc, kb) and torch.equal(vc, vb), t     # identity ancestors: bit-equal
        anc = torch.randint(0, W, (R, W, T), generator=g).to(torch.int8)                     # a new table at every step
        anc_d = anc.to(DEV)
        check(lib.spacap_decode_attn_beam_f32(qkv.data_ptr(), kp.data_ptr(), vp.data_ptr(), anc_d.data_ptr(), R, W, h, dk, T, t, 0.25,
                                              outp.data_ptr(), st), "beam, permuted")
        allr = torch.stack(rows, 1).double().cpu()                                           # (RW, t + 1, 384)
        src = (base + anc.long()).view(RW, T)[:, :t + 1].clone()                             # the row that holds position p ...
        src[:, t] = torch.arange(RW)                                                         # ... position t: the row itself
        hist = allr[src, torch.arange(t + 1).view(1, -1)]                                    # (RW, t + 1, 384)
        q = allr[:, -1, :128].view(RW, h, 1, dk)
        k = hist[:, :, 128:256].view(RW, t + 1, h, dk).transpose(1, 2)
        v = hist[:, :, 256:].view(RW, t + 1, h, dk).transpose(1, 2)
        p = torch.softmax(q @ k.transpose(-1, -2) * 0.25, -1)
        want = (p @ v).transpose(1, 2).reshape(RW, 128)
        assert rel(outp, want) < 3e-6, t
        assert torch.equal(kp[:, t], qkv[:, 128:256]) and torch.equal(vp[:, t], qkv[:, 256:])
    rc = lib.spacap_decode_attn_beam_f32(qkv.data_ptr(), kp.data_ptr(), vp.data_ptr(), anc_d.data_ptr(), R, 9, h, dk, T, 0, 0.25, outp.data_ptr(), st)
    assert rc != 0 and b"W=9" in lib.spacap_last_error()


# ---- 7..9: the decoder -----------------------------------------------------------------------------------------------------------
SEED = 0      # weight seed of the model below; see test_fused_beam_search_against_the_generic_path (c)


@pytest.fixture(scope="module")
def scene():
    """The model of the decoder tests and one detector + encoder forward of two scenes of 4 096 points (shared, not modified)."""
    from spacap3d_amd.engine import synthetic_batch
    from spacap3d_amd.spacapnet import build_default
    torch.manual_seed(SEED)
    model = build_default(vocab_size=120, num_proposal=32, N=2, d_ff=256).to(DEV).eval()
    data = synthetic_batch(2, 4096, DEV, seed=1, vocab=120)
    with torch.no_grad():
        d = model(dict(data), is_eval=True)
    return model, data, d


def _through_first_eos(tokens, eos):
    """(R, n) bool: the positions up to and including each row's first eos (all of them where there is none)."""
    is_eos = tokens == eos
    before = torch.cumsum(is_eos.long(), 1) - is_eos.long()
    return before == 0


def test_width_one_is_the_greedy_decoder(scene, monkeypatch):
    """beam_decode(W = 1) against greedy_decode on the same inputs, word for word through each row's first eos (behind it a
    beam repeats eos; the greedy loop goes on).  Exact: the logit arithmetic is ONE definition (csrc/caption_decode.hip), the
    first-maximum order does not depend on how the vocabulary is sliced, and the other kernels are row-independent."""
    from spacap3d_amd import caption_decode
    model, data, d = scene
    seen = {}
    real = caption_decode.greedy_decode

    def spy(*a):
        seen["args"] = a
        return real(*a)

    monkeypatch.setattr(caption_decode, "greedy_decode", spy)
    with torch.no_grad():
        g = model.caption.forward_eval(dict(d))["lang_cap"]
    dec, gen, embed, pe, indicator, sos, n_words = seen["args"]
    eos = model.caption.word_to_idx["eos"]
    tr = {}
    ys, score = caption_decode.beam_decode(dec, gen, embed, pe, indicator, sos, eos, n_words, 1, trace=tr)
    g = g.reshape(-1, n_words)
    assert torch.equal(g, d["lang_cap"].reshape(-1, n_words)) and ys.shape == g.shape
    keep = _through_first_eos(g, eos)
    print(f"rows with an eos: {int((g == eos).any(1).sum())} of {g.shape[0]}")
    assert torch.equal(ys[keep], g[keep])
    assert bool((ys[~keep] == eos).all())
    assert bool((tr["parent"] == 0).all()) and torch.equal(tr["word"][:, :, 0].t().long(), ys)
    assert bool(torch.isfinite(score).all()) and bool((score <= 0).all())



SCORE_TOL = 4 * 1.81e-5    # (a): four times the largest deviation measured on the MI355X (1.81e-5, see the test); must stay below 1e-3


def _teacher_forced_score(model, d, tokens, eos):
    """Sum of the log-probabilities of ``tokens`` (B, K, n) through each row's first eos, from the UNCACHED decoder: the whole
    prefix in one pass (``self.model(...)`` + generator, the loop of ``forward_eval(use_cache=False)`` without the loop)."""
    from spacap3d_amd.transformer_captioner import subsequent_mask
    cap = model.caption
    obj = d["aggregated_vote_features"]
    if cap.token_proj is not None:
        obj = cap.token_proj(obj)
    B, K, _ = obj.shape
    src_pos = cap._src_pos(d)
    src_mask = d["bbox_mask"].unsqueeze(1)
    memory = cap.model.encode(obj, src_pos, src_mask)
    n = tokens.shape[-1]
    tok = tokens.reshape(B * K, n)
    ys = torch.cat([torch.full((B * K, 1), cap.word_to_idx["sos"], dtype=torch.long, device=tok.device), tok[:, :-1]], 1)
    out = cap.model(obj, ys, src_mask, subsequent_mask(n + 1, device=tok.device), obj.reshape(B * K, -1).unsqueeze(1),
                    src_pos=src_pos, memory=memory)
    logp = cap.model.generator(out[:, 1:, :]).double()                     # position 1 + i predicts word i
    picked = logp.gather(2, tok.unsqueeze(-1)).squeeze(-1)
    return (picked * _through_first_eos(tok, eos)).sum(1).view(B, K)


def _fused_generic_cpu(model, d, W):
    """forward_eval three ways on the detector outputs ``d``: fused (caption_decode.beam_decode), generic on the GPU, generic on the
    CPU oracle backend.  Returns the two GPU outputs, the three traces and the teacher-forced scores of the fused winners."""
    import copy
    from oracle.attention_ref import OracleBackend
    from spacap3d_amd import backend
    cap = model.caption
    eos = cap.word_to_idx["eos"]
    try:
        with torch.no_grad():
            cap.last_beam_trace = None
            fused = cap.forward_eval(dict(d), beam_size=W)
            tz = {k: v.cpu() for k, v in cap.last_beam_trace.items()}
            assert "gap" not in tz, "forward_eval did not take caption_decode.beam_decode"
            cap.beam_generic = True
            gen = cap.forward_eval(dict(d), beam_size=W)
            tg = {k: v.cpu() for k, v in cap.last_beam_trace.items()}
            cpu_cap = copy.deepcopy(cap).cpu()
            with backend.use_backend(OracleBackend()):
                cpu_cap.forward_eval({k: v.cpu() for k, v in d.items() if torch.is_tensor(v)}, beam_size=W)
            tc = {k: v.cpu() for k, v in cpu_cap.last_beam_trace.items()}
            tf_score = _teacher_forced_score(model, d, fused["lang_cap"], eos)
    finally:
        cap.__dict__.pop("beam_generic", None)
        cap.__dict__.pop("last_beam_trace", None)
    return fused, gen, tz, tg, tc, tf_score


def _differing(a, b):
    """[(sequence, first differing step)] of two (parent, word) traces (n_words, R, W)"""
    diff = ((a["parent"].long() != b["parent"].long()) | (a["word"].long() != b["word"].long())).any(-1)        # (n_words, R)
    return [(r, int(torch.nonzero(diff[:, r])[0])) for r in range(diff.shape[1]) if bool(diff[:, r].any())]


def test_fused_beam_search_against_the_generic_path(scene):
    """W = 3, forward_eval on the fused path (caption_decode.beam_decode) against the generic one (beam_search.beam_search over
    decode_incremental).
    (a) lang_cap_score equals the winner's words teacher-forced through the uncached decoder, summed through the first eos,
        within SCORE_TOL = 4 x the largest deviation measured on the MI355X (1.81e-5 on scores down to -80: fp32 accumulation
        of 31 terms; the factor is headroom for other seeds).
    (b) per sequence the (parent, word) traces agree at every step, or at the first differing step the generic path's gap
        between its W-th and (W+1)-th candidate is below SCORE_TOL (a near-tie either order of which is right).
    (c) at most 5 % of the sequences differ at all.  The weight seed (SEED) was chosen so that the generic path ALONE stays
        within that cap between fp32 on the GPU and fp32 on the CPU oracle backend; that is checked here first (measured on
        the MI355X with SEED = 0: 0 of 64 sequences differ there, and 0 of 64 between fused and generic)."""
    model, data, d = scene
    R = d["lang_cap"].shape[0] * d["lang_cap"].shape[1]
    fused, gen, tz, tg, tc, tf_score = _fused_generic_cpu(model, d, 3)
    assert fused["lang_cap"].shape == d["lang_cap"].shape and fused["lang_cap_score"].shape == d["lang_cap"].shape[:2]
    # (c) first: the generic path alone, GPU against the CPU oracle backend
    alone = _differing(tg, tc)
    print(f"generic GPU vs generic CPU: {len(alone)} of {R} sequences differ")
    assert len(alone) <= 0.05 * R
    # (a)
    dev_ = float((fused["lang_cap_score"].double() - tf_score).abs().max())
    print(f"largest |lang_cap_score - teacher-forced score| = {dev_:.3g} (scores down to {float(tf_score.min()):.1f})")
    assert SCORE_TOL < 1e-3 and dev_ <= SCORE_TOL
    # (b), (c)
    diff = _differing(tz, tg)
    print(f"fused vs generic: {len(diff)} of {R} sequences differ; gaps at the first differing step: "
          f"{[float(tg['gap'][s, r]) for r, s in diff]}")
    for r, s in diff:
        assert float(tg["gap"][s, r]) < SCORE_TOL, (r, s)
    assert len(diff) <= 0.05 * R
    if not diff:
        assert torch.equal(fused["lang_cap"], gen["lang_cap"])
        assert float((fused["lang_cap_score"] - gen["lang_cap_score"]).abs().max()) <= SCORE_TOL


def test_evaluator_pipeline_with_a_beam(scene):
    """Evaluator(..., beam_size=3) on two consecutive batches: lang_cap, lang_cap_score and the predictions built from them
    (pred_tokens = decode_caption of the kept proposals' lang_cap, by the restatement of tests/dense_caption_restated.py);
    beam_size=1 gives the captions of an Evaluator without the argument."""
    import dense_caption_restated as D
    from spacap3d_amd.engine import Evaluator, synthetic_batch
    from test_postprocess_gpu import POST_DICT
    model = scene[0]
    sos, eos = model.caption.word_to_idx["sos"], model.caption.word_to_idx["eos"]
    post = dict(POST_DICT, dataset_config=None)
    batches = [{"point_clouds": synthetic_batch(2, 4096, DEV, seed=s, vocab=120)["point_clouds"]} for s in (1, 2)]
    try:
        ev = Evaluator(model, graph=True, postprocess=post, predictions=(sos, eos), beam_size=3)
        outs = [ev(dict(b), next_data=batches[i + 1] if i + 1 < len(batches) else None) for i, b in enumerate(batches)]
        torch.cuda.synchronize()
        for out in outs:
            assert out["lang_cap"].shape == (2, 32, 31) and out["lang_cap"].dtype == torch.long
            assert out["lang_cap_score"].shape == (2, 32) and out["lang_cap_score"].dtype == torch.float32
            assert bool(torch.isfinite(out["lang_cap_score"]).all())
            h = {k: out[k].cpu().numpy() for k in ("post_valid", "post_obj_prob", "sem_cls", "bbox_corner", "lang_cap")}
            want = D.select(h["post_valid"], h["post_obj_prob"], h["sem_cls"], h["bbox_corner"], h["lang_cap"], sos, eos)
            np.testing.assert_array_equal(out["pred_tokens"].cpu().numpy(), want["tokens"])
            np.testing.assert_array_equal(out["pred_length"].cpu().numpy(), want["length"])
        one = Evaluator(model, postprocess=post, beam_size=1)(dict(batches[0]))
        assert model.caption.beam_size == 1 and "lang_cap_score" not in one
        del model.caption.beam_size                                    # back to the class default
        plain = Evaluator(model, postprocess=post)(dict(batches[0]))
        assert torch.equal(one["lang_cap"], plain["lang_cap"])
    finally:
        model.caption.__dict__.pop("beam_size", None)
        model.caption.__dict__.pop("length_penalty", None)
