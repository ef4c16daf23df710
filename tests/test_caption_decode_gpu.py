"""The caption decoders' own kernels and shared step on the MI355X (csrc/caption_decode.hip, spacap3d_amd/caption_decode.py): the
greedy decoder's attention over the cache and its word choice against float64 PyTorch, and the step that greedy_decode and
beam_decode share (sized by rows = sequences x hypotheses).  The beam search's kernels and semantics: tests/test_beam_search_gpu.py."""
import pytest
import torch

from test_beam_search_gpu import _through_first_eos, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True, scope="module")
def _needs_a_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _rand(*s, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*s, generator=g) * scale).to(DEV)


# ---- 1..3: the greedy decoder's kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,T", [(1, 1), (3, 5), (37, 32)])     # one key and nothing cached; a row stride that is not 32; several waves of rows
def test_decode_attention_step_over_the_cache(R, T):
    """spacap_decode_attn_f32: appending the new token's k, v and attending over positions 0..t equals the last row of causal
    attention over the whole prefix (what the reference recomputes at every word, models/transformer_captioner.py:435-438)."""
    from spacap3d_amd._native import check, lib
    h, dk = 8, 16
    kc, vc = torch.zeros(R, T, 128, device=DEV), torch.zeros(R, T, 128, device=DEV)
    out = torch.empty(R, 128, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for t in range(T):
        qkv = _rand(R, 384, seed=100 + t)
        rows.append(qkv)
        check(lib.spacap_decode_attn_f32(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), R, h, dk, T, t, 0.25, out.data_ptr(), st), "dec")
        allr = torch.stack(rows, 1).double()                                   # (R, t+1, 384)
        q = allr[:, -1, :128].view(R, h, 1, dk)
        k = allr[:, :, 128:256].view(R, t + 1, h, dk).transpose(1, 2)
        v = allr[:, :, 256:].view(R, t + 1, h, dk).transpose(1, 2)
        p = torch.softmax(q @ k.transpose(-1, -2) * 0.25, -1)
        want = (p @ v).transpose(1, 2).reshape(R, 128)
        assert rel(out, want) < 3e-6, t
        assert torch.equal(kc[:, t], qkv[:, 128:256]) and torch.equal(vc[:, t], qkv[:, 256:])


@pytest.mark.parametrize("R,V", [(2048, 3001), (37, 40), (16, 64), (300, 1000)])
def test_decode_word_choice_without_logits(R, V):
    """spacap_decode_word_f32 (csrc/caption_decode.hip: vocab_argmax_kernel + decode_next_kernel): the greedy word of every sequence
    = arg-max of x W^T + b (models/transformer_captioner.py:441-447 on the Generator of :93-100; first maximum on ties, as
    torch.max), written into the caption, and the next input row lut[word] sqrt(d) + pe.  Against float64 logits: the chosen
    word's logit is within fp32 rounding of the maximum (an exact tie in float64 picks the smaller index)."""
    import math
    from spacap3d_amd._native import check, lib
    g = torch.Generator().manual_seed(R + V)
    x = torch.randn(R, 128, generator=g).to(DEV)
    W, b = (0.3 * torch.randn(V, 128, generator=g)).to(DEV), torch.randn(V, generator=g).to(DEV)
    W[7] = W[3]
    b[7] = b[3]                                      # two identical words: the first one must win wherever they lead
    x[0] = 0.0
    b[3] = b[7] = 50.0                               # ... which they do for row 0 (all-zero input: logits = bias)
    lut, pe = torch.randn(V, 128, generator=g).to(DEV), torch.randn(128, generator=g).to(DEV)
    ys = torch.full((R, 5), -1, dtype=torch.long, device=DEV)
    xn = torch.empty(R, 128, device=DEV)
    ws = torch.empty(int(lib.spacap_decode_word_workspace_bytes(R, V)), dtype=torch.uint8, device=DEV)
    scale = math.sqrt(128.0)
    from spacap3d_amd.linear import bf3_pieces
    Wp = bf3_pieces(W)
    check(lib.spacap_decode_word_f32(x.data_ptr(), Wp.data_ptr(), b.data_ptr(), R, V, lut.data_ptr(), scale, pe.data_ptr(), ys.data_ptr(), 5, 2,
                                     xn.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream), "spacap_decode_word_f32")
    word = ys[:, 2]
    assert int(word[0]) == 3 and bool((ys[:, [0, 1, 3, 4]] == -1).all())
    logits = x.double() @ W.double().t() + b.double()
    best = logits.max(1).values
    chosen = logits.gather(1, word.view(-1, 1)).squeeze(1)
    assert float((best - chosen).max()) < 1e-4 * float(logits.abs().max())
    assert float((word == logits.argmax(1)).double().mean()) > 0.995
    assert torch.allclose(xn, lut[word] * scale + pe, rtol=0, atol=1e-5)


# ---- 4. the step the two decoders share is sized by rows = sequences x hypotheses -----------------------------------------------
@pytest.fixture(scope="module")
def one_layer():
    """A one-layer decoder (d_ff 128, vocabulary 40): (decoder, generator, embed, pe, sos, eos)"""
    from spacap3d_amd.spacapnet import build_default
    torch.manual_seed(0)
    cap = build_default(vocab_size=40, num_proposal=8, N=1, d_ff=128).to(DEV).eval().caption
    m = cap.model
    return m.decoder, m.generator, m.tgt_embed[0], m.tgt_embed[1].pe, cap.word_to_idx["sos"], cap.word_to_idx["eos"]


@pytest.fixture
def ffn_calls(monkeypatch):
    """Counts the calls of the two feed-forward entries (both still run)."""
    from spacap3d_amd import _native
    calls = {"spacap_tf_ffn_f32": 0, "spacap_tf_ffn_bf3_f32": 0}

    def spy(name, real):
        def through(*a):
            calls[name] += 1
            return real(*a)
        return through

    for name in calls:
        monkeypatch.setattr(_native.lib, name, spy(name, getattr(_native.lib, name)))
    return calls


N_WORDS_SHORT = 2      # three positions through one layer: three feed-forward launches per decoding call


def test_greedy_rows_below_the_split_bf16_threshold_take_the_fp32_feed_forward(one_layer, ffn_calls):
    from spacap3d_amd import caption_decode, tf_layer
    dec, gen, embed, pe, sos, eos = one_layer
    R = 260
    assert R <= tf_layer.FFN_BF3_MIN_ROWS
    ys = caption_decode.greedy_decode(dec, gen, embed, pe, _rand(R, 128, seed=5), sos, N_WORDS_SHORT)
    assert ys.shape == (R, N_WORDS_SHORT)
    assert ffn_calls == {"spacap_tf_ffn_f32": N_WORDS_SHORT + 1, "spacap_tf_ffn_bf3_f32": 0}


def test_beam_rows_count_the_hypotheses_for_the_feed_forward_choice(one_layer, ffn_calls):
    """260 sequences x 2 hypotheses = 520 rows, above FFN_BF3_MIN_ROWS: a step that sizes its buffers or picks the kernel from
    the sequences alone calls the fp32 entry (or writes out of its buffers)."""
    from spacap3d_amd import caption_decode, tf_layer
    dec, gen, embed, pe, sos, eos = one_layer
    R, W = 260, 2
    assert R <= tf_layer.FFN_BF3_MIN_ROWS < R * W
    ys, score = caption_decode.beam_decode(dec, gen, embed, pe, _rand(R, 128, seed=5), sos, eos, N_WORDS_SHORT, W)
    assert ys.shape == (R, N_WORDS_SHORT) and bool(torch.isfinite(score).all())
    assert ffn_calls == {"spacap_tf_ffn_f32": 0, "spacap_tf_ffn_bf3_f32": N_WORDS_SHORT + 1}


def test_width_one_equals_greedy_on_the_split_bf16_feed_forward(one_layer, ffn_calls):
    from spacap3d_amd import caption_decode, tf_layer
    dec, gen, embed, pe, sos, eos = one_layer
    R = 520
    assert R > tf_layer.FFN_BF3_MIN_ROWS
    indicator = _rand(R, 128, seed=6)
    g = caption_decode.greedy_decode(dec, gen, embed, pe, indicator, sos, N_WORDS_SHORT)
    assert ffn_calls == {"spacap_tf_ffn_f32": 0, "spacap_tf_ffn_bf3_f32": N_WORDS_SHORT + 1}
    ys, _ = caption_decode.beam_decode(dec, gen, embed, pe, indicator, sos, eos, N_WORDS_SHORT, 1)
    assert ffn_calls == {"spacap_tf_ffn_f32": 0, "spacap_tf_ffn_bf3_f32": 2 * (N_WORDS_SHORT + 1)}
    keep = _through_first_eos(g, eos)
    assert torch.equal(ys[keep], g[keep])
