"""Caption decoding on the device (csrc/caption_decode.hip): the greedy decoder, the beam search and sampled decoding over the
early-guide decoder stack, one token per row and step over pre-allocated key / value caches.  The layers themselves are the training
kernels of ``tf_layer`` with dropout off; what the two decoders share -- the per-call buffers and the launch sequence of one
position -- is ``_Stack``, written once: a beam of width 1 must choose the greedy words bit for bit
(tests/test_beam_search_gpu.py), and so must sampling with ``top_k`` = 1 (tests/test_sampling_gpu.py).  Each decoder keeps its
own word selection, the beam search its hypothesis state and the sampler its row state."""
import math

import torch

from . import tf_layer
from ._native import check, lib
from .tf_layer import D_MODEL, _new, _packed, _rows, refresh_ffn_pieces, stack_supported


def decode_supported(layers, x, n_words):
    """True when ``greedy_decode`` / ``beam_decode`` can run: everything ``tf_layer.stack_supported`` asks for, plus what
    ``spacap_decode_attn_f32`` requires (h = 8, d_k = 16, at most 32 cached positions) and one feed-forward width for the
    whole stack (one partial-sum buffer).  Anything else decodes through the cached per-operator path
    (``decode_incremental``)."""
    if not stack_supported(layers, x) or n_words + 1 > 32:
        return False
    dff = layers[0].feed_forward.w_1.out_features
    return all(l.self_attn.h == 8 and l.self_attn.d_k == 16 and l.feed_forward.w_1.out_features == dff for l in layers)


class _Stack:
    """The decoder stack ``dec`` for one decoding call over ``rows`` rows (sequences x hypotheses) and T positions: the per-call
    state, sized by ``rows`` as is the choice of the feed-forward kernel, and one position through the stack."""

    def __init__(self, dec, generator, embed, pe, rows, T, dev):
        self.dec, self.layers, self.rows, self.T, self.dev = dec, list(dec.layers), rows, T, dev
        layers = self.layers
        self.st = torch.cuda.current_stream(dev).cuda_stream
        self.packs = [_packed(l.self_attn)[:2] for l in layers]
        self.h, self.dk = layers[0].self_attn.h, layers[0].self_attn.d_k
        self.dff = layers[0].feed_forward.w_1.out_features
        self.S, self.scale, self.sqrt_d = self.dff // 128, 1.0 / math.sqrt(self.dk), math.sqrt(embed.d_model)
        self.lut, self.gw, self.gb = embed.lut.weight.contiguous(), generator.proj.weight.contiguous(), generator.proj.bias.contiguous()
        self.V, self.pe, self.pieces = self.gw.shape[0], pe, None
        if tf_layer.FFN_BF3 and rows > tf_layer.FFN_BF3_MIN_ROWS:
            refresh_ffn_pieces(layers)
            pieces = [tf_layer.ffn_pieces(l.feed_forward.w_1.weight, self.dff) for l in layers]
            self.pieces = pieces if all(e is not None for e in pieces) else None

    def allocate(self, on_cache_oom=None):
        """The key / value caches (rows, T, 128) of every layer -- ``on_cache_oom(error)`` answers a failure to allocate them --
        then the work buffers of one position, the vocabulary projection's pieces and the positions' sinusoid rows."""
        from .linear import bf3_pieces
        dev, rows, T = self.dev, self.rows, self.T
        try:
            self.kc = [_new(dev, rows, T, D_MODEL) for _ in self.layers]
            self.vc = [_new(dev, rows, T, D_MODEL) for _ in self.layers]
        except torch.cuda.OutOfMemoryError as e:
            if on_cache_oom is None:
                raise
            on_cache_oom(e)
        self.qkv = _new(dev, rows, 3 * D_MODEL)
        self.a, self.x1, self.x2, self.n2, self.n = (_new(dev, rows, D_MODEL) for _ in range(5))
        self.parts = _new(dev, self.S, rows, D_MODEL)
        self.gwp = bf3_pieces(self.gw)                  # the projection weight's three bf16 pieces, once per call
        self.pe_rows = self.pe[0, :self.T].contiguous()
        self.xw = _new(dev, rows, D_MODEL)              # the next step's input rows (written by the word / selection kernel)

    def sos_rows(self, sos):   # position 1 of every row: the start symbol
        return (self.lut[int(sos)] * self.sqrt_d + self.pe_rows[0]).expand(self.rows, D_MODEL).contiguous()

    def position(self, x, t, attn):
        """x (rows, 128), the input rows of position t -> n (rows, 128), the stack's output rows: the first LayerNorm + packed
        q|k|v, then per layer attention -> rows -> feed-forward (split-bf16 or fp32) -> rows.  ``attn(i, t)`` launches layer i's
        attention of ``qkv`` over ``kc[i]`` / ``vc[i]`` into ``a``: the one launch that differs between the two decoders."""
        layers, dec, R, dev, st = self.layers, self.dec, self.rows, self.dev, self.st
        packs, pieces, dff, S = self.packs, self.pieces, self.dff, self.S
        qkv, a, x1, x2, n2, n, parts = self.qkv, self.a, self.x1, self.x2, self.n2, self.n, self.parts
        n0 = layers[0].sublayer[0].norm
        _rows(0, R, dev, res=x, ln_a=n0.a_2, ln_b=n0.b_2, eps=n0.eps, w2=packs[0][0], bias2=packs[0][1], n2=3 * D_MODEL, out2=qkv)
        xres = x
        for i, l in enumerate(layers):
            sa, ff, nf = l.self_attn, l.feed_forward, l.sublayer[-1].norm
            attn(i, t)
            _rows(0, R, dev, a1=a, w1=sa.linears[-1].weight, bias1=sa.linears[-1].bias, k1=D_MODEL, res=xres, x_out=x1,
                  ln_a=nf.a_2, ln_b=nf.b_2, eps=nf.eps, n_out=n2)
            if pieces is not None:
                check(lib.spacap_tf_ffn_bf3_f32(0, n2.data_ptr(), pieces[i].data_ptr(), ff.w_1.bias.data_ptr(), None, R, dff, 0.0, 0,
                                                None, None, parts.data_ptr(), st), "spacap_tf_ffn_bf3_f32")
            else:
                check(lib.spacap_tf_ffn_f32(0, n2.data_ptr(), ff.w_1.weight.data_ptr(), ff.w_2.weight.data_ptr(),
                                            ff.w_1.bias.data_ptr(), None, R, dff, 0.0, 0, None, None, parts.data_ptr(), st),
                      "spacap_tf_ffn_f32")
            if i + 1 < len(layers):
                nn_ = layers[i + 1].sublayer[0].norm
                _rows(0, R, dev, a1=parts, nparts=S, bias1=ff.w_2.bias, res=x1, x_out=x2, ln_a=nn_.a_2, ln_b=nn_.b_2, eps=nn_.eps,
                      w2=packs[i + 1][0], bias2=packs[i + 1][1], n2=3 * D_MODEL, out2=qkv)
                xres = x2
            else:
                _rows(0, R, dev, a1=parts, nparts=S, bias1=ff.w_2.bias, res=x1, ln_a=dec.norm.a_2, ln_b=dec.norm.b_2,
                      eps=dec.norm.eps, n_out=n)
        return n


class _Constrained:
    """An active ``DecodeConstraints`` for one decoding call over ``rows`` rows: the rows' two bit images
    over the vocabulary and the launch that refreshes them before a step's word choice."""

    def __init__(self, who, c, rows, V, n_words, eos, dev):
        import ctypes
        if eos is None:
            raise ValueError(f"{who}: constraints need eos")
        c.check(who, V, n_words, eos)
        self.theta, self.eos, self.V, self.T = c.repetition_penalty, int(eos), V, n_words + 1
        self.min_length, self.ngram, self.n_bad = c.min_length, c.no_repeat_ngram, len(c.bad_words)
        self.bad = (ctypes.c_int32 * max(self.n_bad, 1))(*c.bad_words)
        self.images = torch.empty(int(lib.spacap_decode_constraints_bytes(rows, V)), dtype=torch.uint8, device=dev)
        self.bits = self.images.data_ptr()

    def refresh(self, step, R, st, ys=None, trace_word=None, anc=None, W=1):
        """the images of step ``step``: from the rows of ``ys`` (R, n_words), or a beam's trace and ancestor table"""
        check(lib.spacap_decode_constraints(None if ys is None else ys.data_ptr(), 0 if ys is None else ys.shape[1],
                                            None if trace_word is None else trace_word.data_ptr(), None if anc is None else anc.data_ptr(),
                                            R, W, self.T, self.V, step, self.eos, self.min_length, self.ngram, self.bad, self.n_bad,
                                            self.bits, st), "spacap_decode_constraints")


def _constrained(who, constraints, rows, V, n_words, eos, dev):
    from .decode_constraints import resolve
    c = resolve(constraints)
    return None if c is None else _Constrained(who, c, rows, V, n_words, eos, dev)


@torch.no_grad()
def greedy_decode(dec, generator, embed, pe, indicator, sos, n_words, eos=None, constraints=None):
    """Greedy decoding of R sequences through the early-guide decoder stack ``dec`` with pre-allocated key / value caches
    (models/transformer_captioner.py:402-453; the reference re-runs encoder and decoder prefix for every word).  Position 0
    is the object indicator token (R, 128), position 1 the start symbol, then every chosen word is fed back; one token per
    sequence per step, four launches per layer and step (the training kernels with dropout off + spacap_decode_attn_f32).
    The word choice of a step -- vocabulary projection + arg-max + the chosen word's embedding row -- is one library call
    (csrc/caption_decode.hip: vocab_argmax_kernel / decode_next_kernel: no logits in HBM, no BLAS call).
    ``constraints`` (a ``decode_constraints.DecodeConstraints`` or a dict of its arguments; needs ``eos``): the word choice
    over the constrained logits -- one more small launch per step builds the rows' bit images, and the
    constrained copy of the arg-max kernel tests two bits per logit.  None or nothing active: exactly the calls above.
    Returns the (R, n_words) int64 word ids."""
    R, dev = indicator.shape[0], indicator.device
    T = n_words + 1
    s = _Stack(dec, generator, embed, pe, R, T, dev)
    st, V = s.st, s.V
    con = _constrained("greedy_decode", constraints, R, V, n_words, eos, dev)

    def attn(i, t):
        check(lib.spacap_decode_attn_f32(s.qkv.data_ptr(), s.kc[i].data_ptr(), s.vc[i].data_ptr(), R, s.h, s.dk, T, t, s.scale,
                                         s.a.data_ptr(), st), "spacap_decode_attn_f32")

    with torch.cuda.device(dev):
        s.allocate()
        ys = torch.empty(R, n_words, dtype=torch.long, device=dev)
        ws = torch.empty(int(lib.spacap_decode_word_workspace_bytes(R, V)), dtype=torch.uint8, device=dev)
        x = indicator.contiguous()
        for t in range(T):
            if t == 1:
                x = s.sos_rows(sos)                         # every sequence starts with <sos>
            elif t > 1:
                x = s.xw
            n = s.position(x, t, attn)
            if t >= 1 and con is not None:
                con.refresh(t - 1, R, st, ys=ys)
                check(lib.spacap_decode_word_constrained_f32(n.data_ptr(), s.gwp.data_ptr(), s.gb.data_ptr(), R, V, con.bits, con.theta,
                                                             s.lut.data_ptr(), s.sqrt_d, s.pe_rows[min(t, T - 1)].data_ptr(), ys.data_ptr(),
                                                             n_words, t - 1, s.xw.data_ptr(), ws.data_ptr(), st),
                      "spacap_decode_word_constrained_f32")
            elif t >= 1:
                # ys[:, t - 1] = argmax_v (n W^T + b); xw = lut[word] sqrt(d) + pe[t]: the input of step t + 1
                check(lib.spacap_decode_word_f32(n.data_ptr(), s.gwp.data_ptr(), s.gb.data_ptr(), R, V, s.lut.data_ptr(), s.sqrt_d,
                                                 s.pe_rows[min(t, T - 1)].data_ptr(), ys.data_ptr(), n_words, t - 1, s.xw.data_ptr(),
                                                 ws.data_ptr(), st), "spacap_decode_word_f32")
    return ys


@torch.no_grad()
def beam_decode(dec, generator, embed, pe, indicator, sos, eos, n_words, beam_size, length_penalty=0.0, return_all=False, trace=None,
                constraints=None):
    """Beam-search decoding of R sequences with ``beam_size`` = W hypotheses each (1 <= W <= 8): the ``greedy_decode`` loop at
    R W rows (row r W + w = hypothesis w of sequence r) through the same row / feed-forward kernels -- they are
    row-independent -- with three kernels of csrc/caption_decode.hip in place of the greedy ones: attention that reads a
    hypothesis' history through an ancestor table (the key / value caches are never reordered), the W best log-probabilities
    of every row without the logits in HBM, and one selection per sequence; the trace is backtracked once at the end.  The
    semantics are DESIGN.md section 7e (the reference has no beam search); no step reads a value back on the host, so the
    call can be captured in a graph like the greedy loop.  Cache memory: 12 R W T 512 bytes for 6 layers.
    Returns ``(ys (R, n_words) int64, score (R,) float32)`` -- the winner's words (eos repeats after the first eos) and its
    sum of log-probabilities -- and with ``return_all`` also ``(beams (R, W, n_words) int64, scores (R, W), lengths (R, W))``.  ``trace``: a dict that
    receives the selections, ``parent`` int8 and ``word`` int32, each (n_words, R, W).  ``constraints``: as for
    ``greedy_decode``; a hypothesis' history is its own ancestry, read through the trace and the ancestor table."""
    R, dev = indicator.shape[0], indicator.device
    W = int(beam_size)
    T = n_words + 1
    V = generator.proj.weight.shape[0]
    if not 1 <= W <= 8 or W > V:
        raise ValueError(f"beam_decode: beam_size {W} unsupported (1 <= beam_size <= 8 and beam_size <= vocabulary size {V})")
    RW = R * W
    s = _Stack(dec, generator, embed, pe, RW, T, dev)
    st = s.st
    con = _constrained("beam_decode", constraints, RW, V, n_words, eos, dev)
    with torch.cuda.device(dev):
        def cache_oom(e):
            nl = len(s.layers)
            need = 2 * nl * RW * T * D_MODEL * 4
            raise RuntimeError(f"beam_decode: the key / value caches of {R} sequences x {W} hypotheses need {need / 2**30:.2f} GiB "
                               f"({nl} layers x 2 x {RW} rows x {T} positions x 512 B) and could not be allocated: "
                               "decode fewer scenes per call or lower beam_size") from e

        x = indicator.contiguous().repeat_interleave(W, 0)    # positions 0 and 1: the W rows of a sequence are identical
        s.allocate(on_cache_oom=cache_oom)
        ws = torch.empty(int(lib.spacap_beam_topw_workspace_bytes(RW, V, W)), dtype=torch.uint8, device=dev)
        top_lp = torch.empty(RW, W, dtype=torch.float32, device=dev)
        top_wd = torch.empty(RW, W, dtype=torch.int32, device=dev)
        # hypothesis state, double-buffered: before the first selection hypothesis 0 has score 0, the others are dead
        score = [torch.full((R, W), float("-inf"), dtype=torch.float32, device=dev) for _ in range(2)]
        score[1][:, 0] = 0.0                           # (the selection after position t reads buffer t % 2)
        fin = [torch.zeros(R, W, dtype=torch.int32, device=dev) for _ in range(2)]
        ln = [torch.zeros(R, W, dtype=torch.int32, device=dev) for _ in range(2)]
        anc = [torch.arange(W, dtype=torch.int8, device=dev).view(1, W, 1).expand(R, W, T).contiguous() for _ in range(2)]
        tr_parent = torch.empty(n_words, R, W, dtype=torch.int8, device=dev)
        tr_word = torch.empty(n_words, R, W, dtype=torch.int32, device=dev)

        def attn(i, t):
            check(lib.spacap_decode_attn_beam_f32(s.qkv.data_ptr(), s.kc[i].data_ptr(), s.vc[i].data_ptr(), anc[t % 2].data_ptr(), R, W,
                                                  s.h, s.dk, T, t, s.scale, s.a.data_ptr(), st), "spacap_decode_attn_beam_f32")

        for t in range(T):
            if t == 1:
                x = s.sos_rows(sos)                         # every hypothesis starts with <sos>
            elif t > 1:
                x = s.xw
            n = s.position(x, t, attn)
            if t >= 1:
                # the W best (log-probability, word) of every row, then one selection per sequence: state t % 2 -> (t + 1) % 2,
                # trace[t - 1], the ancestor table for position t + 1 and xw = lut[word] sqrt(d) + pe[t], the input of step t + 1
                i0, i1 = t % 2, (t + 1) % 2
                if con is None:
                    check(lib.spacap_beam_topw_f32(n.data_ptr(), s.gwp.data_ptr(), s.gb.data_ptr(), RW, V, W, top_lp.data_ptr(),
                                                   top_wd.data_ptr(), ws.data_ptr(), st), "spacap_beam_topw_f32")
                else:
                    con.refresh(t - 1, R, st, trace_word=tr_word, anc=anc[i0], W=W)
                    check(lib.spacap_beam_topw_constrained_f32(n.data_ptr(), s.gwp.data_ptr(), s.gb.data_ptr(), RW, V, W, con.bits, con.theta,
                                                               top_lp.data_ptr(), top_wd.data_ptr(), ws.data_ptr(), st),
                          "spacap_beam_topw_constrained_f32")
                check(lib.spacap_beam_step_f32(top_lp.data_ptr(), top_wd.data_ptr(), R, W, V, T, t, int(eos), score[i0].data_ptr(),
                                               fin[i0].data_ptr(), ln[i0].data_ptr(), score[i1].data_ptr(), fin[i1].data_ptr(),
                                               ln[i1].data_ptr(), anc[i0].data_ptr(), anc[i1].data_ptr(), tr_parent.data_ptr(),
                                               tr_word.data_ptr(), s.lut.data_ptr(), s.sqrt_d, s.pe_rows[min(t, T - 1)].data_ptr(),
                                               s.xw.data_ptr(), st), "spacap_beam_step_f32")
        last = T % 2                                    # the buffer the last selection (t = T - 1) wrote
        ys = torch.empty(R, n_words, dtype=torch.long, device=dev)
        best = torch.empty(R, dtype=torch.float32, device=dev)
        beams = scores = lengths = None
        if return_all:
            beams = torch.empty(R, W, n_words, dtype=torch.long, device=dev)
            scores = torch.empty(R, W, dtype=torch.float32, device=dev)
            lengths = torch.empty(R, W, dtype=torch.int32, device=dev)
        check(lib.spacap_beam_finish_f32(score[last].data_ptr(), ln[last].data_ptr(), tr_parent.data_ptr(), tr_word.data_ptr(), R, W, n_words,
                                         float(length_penalty), ys.data_ptr(), best.data_ptr(),
                                         beams.data_ptr() if return_all else None, scores.data_ptr() if return_all else None,
                                         lengths.data_ptr() if return_all else None, st), "spacap_beam_finish_f32")
    if trace is not None:
        trace["parent"], trace["word"] = tr_parent, tr_word
    return (ys, best, beams, scores, lengths) if return_all else (ys, best)


NUCLEUS_MAX_V = 16384     # spacap_sample_word_nucleus_f32 keeps a row in LDS, 8 bytes a word


@torch.no_grad()
def sample_decode(dec, generator, embed, pe, indicator, sos, eos, n_words, num_samples=1, temperature=1.0, top_k=0, seed=None,
                  top_p=None, constraints=None):
    """Sampled decoding of R sequences, ``num_samples`` = S captions each (the reference decodes greedily
    only): the ``greedy_decode`` loop at R S rows (row r S + s = sample s of sequence r; rows are independent, so the attention is
    the greedy one and there is no ancestor table) with ``spacap_sample_word_f32`` as the word choice: the Gumbel-max draw from
    softmax(logits / ``temperature``) over the whole vocabulary (``top_k`` = 0) or over the row's ``top_k`` <= 8 most probable
    words, the log-probability of the drawn word under the model's own distribution, and the row state -- no logits in HBM.
    ``seed``: an integer draws the same captions at every call; None takes the host word from ``attention._next_seed()`` and
    mixes in the device word ``attention.rng_state``, so a captured graph draws new captions after every ``advance_rng``.  No step
    reads a value back on the host.  Cache memory: 12 R S T 512 bytes for 6 layers.
    ``top_p`` in (0, 1): nucleus sampling instead (``spacap_sample_word_nucleus_f32``; the semantics are stated in
    ``sampling.py``) -- the draw is restricted to the words whose strictly more probable words hold less than ``top_p`` of the
    tempered distribution.  This mode alone keeps a step's logits in HBM, R S x (V rounded up to 64) floats, between its two
    launches.  None or 1.0 is the path above, bit for bit; ``top_p`` < 1 with ``top_k`` >= 1 is refused: one restriction at a time.
    ``constraints``: as for ``greedy_decode``; the softmax, the top-k set, the nucleus and the reported log-probability are
    those of the constrained logits (the nucleus mode patches its own image of the logits in place).
    Returns ``(ys (R, S, n_words) int64, score (R, S) float32, length (R, S) int32)``: the words (eos repeats after the first
    eos), the summed log-probabilities through the first eos, and the position of the first eos plus one (``n_words``: none);
    or None -- not taken -- for nucleus sampling over more than ``NUCLEUS_MAX_V`` words."""
    from .attention import _next_seed, rng_state
    from .sampling import check_arguments, nucleus_of
    R, dev = indicator.shape[0], indicator.device
    S, k, tau = int(num_samples), int(top_k), float(temperature)
    T = n_words + 1
    V = generator.proj.weight.shape[0]
    check_arguments("sample_decode", S, tau, k, V, top_p)
    p = nucleus_of(top_p)
    if p is not None and V > NUCLEUS_MAX_V:
        return None
    RS = R * S
    s = _Stack(dec, generator, embed, pe, RS, T, dev)
    st = s.st
    con = _constrained("sample_decode", constraints, RS, V, n_words, eos, dev)
    if seed is None:
        seed_host, seed_dev = _next_seed(), rng_state(dev).data_ptr()
    else:
        seed_host, seed_dev = int(seed) & 0xFFFFFFFFFFFFFFFF, None

    def attn(i, t):
        check(lib.spacap_decode_attn_f32(s.qkv.data_ptr(), s.kc[i].data_ptr(), s.vc[i].data_ptr(), RS, s.h, s.dk, T, t, s.scale,
                                         s.a.data_ptr(), st), "spacap_decode_attn_f32")

    with torch.cuda.device(dev):
        def cache_oom(e):
            nl = len(s.layers)
            need = 2 * nl * RS * T * D_MODEL * 4
            raise RuntimeError(f"sample_decode: the key / value caches of {R} sequences x {S} samples need {need / 2**30:.2f} GiB "
                               f"({nl} layers x 2 x {RS} rows x {T} positions x 512 B) and could not be allocated: "
                               "decode fewer scenes per call or lower num_samples") from e

        x = indicator.contiguous().repeat_interleave(S, 0) if S > 1 else indicator.contiguous()
        s.allocate(on_cache_oom=cache_oom)
        need = lib.spacap_sample_word_workspace_bytes(RS, V, k) if p is None else lib.spacap_sample_word_nucleus_workspace_bytes(RS, V)
        ws = torch.empty(int(need), dtype=torch.uint8, device=dev)
        ys = torch.empty(RS, n_words, dtype=torch.long, device=dev)
        score = torch.zeros(RS, dtype=torch.float32, device=dev)
        length = torch.zeros(RS, dtype=torch.int32, device=dev)
        fin = torch.zeros(RS, dtype=torch.int32, device=dev)
        for t in range(T):
            if t == 1:
                x = s.sos_rows(sos)                         # every row starts with <sos>
            elif t > 1:
                x = s.xw
            n = s.position(x, t, attn)
            if t >= 1 and con is not None:
                con.refresh(t - 1, RS, st, ys=ys)
                tail = (seed_host, seed_dev, n_words, t - 1, int(eos), con.bits, con.theta, s.lut.data_ptr(), s.sqrt_d,
                        s.pe_rows[min(t, T - 1)].data_ptr(), ys.data_ptr(), score.data_ptr(), length.data_ptr(), fin.data_ptr(),
                        s.xw.data_ptr(), ws.data_ptr(), st)
                if p is None:
                    check(lib.spacap_sample_word_constrained_f32(n.data_ptr(), s.gwp.data_ptr(), s.gb.data_ptr(), RS, V, k, 1.0 / tau, *tail),
                          "spacap_sample_word_constrained_f32")
                else:
                    check(lib.spacap_sample_word_nucleus_constrained_f32(n.data_ptr(), s.gwp.data_ptr(), s.gb.data_ptr(), RS, V, p, 1.0 / tau,
                                                                         *tail), "spacap_sample_word_nucleus_constrained_f32")
            elif t >= 1 and p is None:
                # word t - 1 of every row, its log-probability into the row's state, and xw = lut[word] sqrt(d) + pe[t]
                check(lib.spacap_sample_word_f32(n.data_ptr(), s.gwp.data_ptr(), s.gb.data_ptr(), RS, V, k, 1.0 / tau, seed_host, seed_dev,
                                                 n_words, t - 1, int(eos), s.lut.data_ptr(), s.sqrt_d,
                                                 s.pe_rows[min(t, T - 1)].data_ptr(), ys.data_ptr(), score.data_ptr(), length.data_ptr(),
                                                 fin.data_ptr(), s.xw.data_ptr(), ws.data_ptr(), st), "spacap_sample_word_f32")
            elif t >= 1:          # the same from the row's nucleus
                check(lib.spacap_sample_word_nucleus_f32(n.data_ptr(), s.gwp.data_ptr(), s.gb.data_ptr(), RS, V, p, 1.0 / tau, seed_host,
                                                         seed_dev, n_words, t - 1, int(eos), s.lut.data_ptr(), s.sqrt_d,
                                                         s.pe_rows[min(t, T - 1)].data_ptr(), ys.data_ptr(), score.data_ptr(),
                                                         length.data_ptr(), fin.data_ptr(), s.xw.data_ptr(), ws.data_ptr(), st),
                      "spacap_sample_word_nucleus_f32")
    return ys.view(R, S, n_words), score.view(R, S), length.view(R, S)
