"""Fused scaled-dot-product attention on libspacap_hip.so -- boundary B2 of SURVEY.md section 8b.

Replaces the four-kernel Python ``attention()`` of the reference
(models/transformer_captioner.py:27-37:  QK^T/sqrt(d_k) -> masked_fill(mask==0, -1e9) -> softmax ->
dropout -> PV) with one launch of ``spacap_mha_fwd_f32`` and one of ``spacap_mha_bwd_f32``.

``attention(query, key, value, mask, dropout_p, training, need_p)`` returns ``(out, p_attn)`` like the
reference: ``out`` is (B,h,Lq,d_k) (a transposed view of a dense (B,Lq,h,d_k) buffer, so the caller's
``x.transpose(1,2).contiguous()`` is free) and ``p_attn`` the post-dropout (B,h,Lq,Lk) matrix the
reference stores as ``self.attn`` -- or None when ``need_p`` is False, in which case the L x L matrix
never leaves registers.  Gradients flow to q, k, v from both outputs (the relation head consumes
``p_attn`` of the last encoder layer, models/transformer_captioner.py:392-394).
"""
import math

import torch
from torch.autograd import Function

from ._native import check, lib, sum_slabs


def _strides3(t):
    assert t.stride(3) == 1, "last (d_k) dimension must be contiguous"
    return t.stride(0), t.stride(1), t.stride(2)


def _prep_mask(mask, B, Lq, Lk):
    """reference masks: (B,1,1,Lk) int64 key mask or (B,1,Lq,Lk) bool -> uint8 (B,Lq|1,Lk)."""
    if mask is None:
        return None, 0, 0
    # the same mask object goes through every layer of a stack: convert it once (2 launches saved per layer)
    for ent in _MASK_CACHE:
        if ent[0] is mask and ent[1] == (mask._version, B, Lq, Lk):
            return ent[2]
    res = _prep_mask_uncached(mask, B, Lq, Lk)
    _MASK_CACHE.insert(0, (mask, (mask._version, B, Lq, Lk), res))
    del _MASK_CACHE[4:]
    return res


_MASK_CACHE = []


def _prep_mask_uncached(mask, B, Lq, Lk):
    m = mask
    if m.dim() == 4:
        assert m.size(1) == 1, "per-head masks are not used by the reference"
        m = m[:, 0]
    assert m.dim() == 3 and m.size(-1) == Lk and m.size(1) in (1, Lq)
    if m.dtype == torch.uint8 and m.size(0) == B and m.is_contiguous():   # already in the kernels' form (caption_prep)
        return m, m.stride(0), (0 if m.size(1) == 1 else m.stride(1))
    m = (m != 0).to(torch.uint8)
    if m.size(0) != B:
        m = m.expand(B, -1, -1)
    m = m.contiguous()
    return m, m.stride(0), (0 if m.size(1) == 1 else m.stride(1))


# ---- dropout randomness ----------------------------------------------------------------------------------
# The keep mask is a counter hash of (seed, element).  `seed` is a host integer drawn per call from a Python
# counter seeded by torch's CPU generator; it would be frozen inside a captured hipGraph, so a device-resident
# word (`_RNG_STATE[device]`, bumped once per training step by an in-graph add) is mixed in by the kernel.
_RNG_STATE = {}
_CALL_COUNTER = [None]


def rng_state(device):
    device = torch.device(device)     # ("cuda:0" and torch.device("cuda", 0) must name the same word)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    st = _RNG_STATE.get(device)
    if st is None:
        st = torch.zeros(1, dtype=torch.int64, device=device)
        _RNG_STATE[device] = st
    return st


def advance_rng(device):
    """Call once per step (captured into the step's graph): every attention call then sees new dropout masks."""
    rng_state(device).add_(1)


def _next_seed():
    if _CALL_COUNTER[0] is None:
        _CALL_COUNTER[0] = int(torch.randint(0, 2 ** 31, (1,), device="cpu").item()) << 20
    _CALL_COUNTER[0] += 1
    return _CALL_COUNTER[0]


def mha_args(q_ptr, k_ptr, v_ptr, q_strides, k_strides, v_strides, mask_u8, mask_sb, mask_sq, bias, B, h, Lq, Lk, dk, scale,
             dropout_p, seed, device):
    """The leading arguments spacap_mha_fwd_f32, spacap_mha_bwd_f32 and spacap_mha_bwd_delta_f32 share: the three operand
    pointers and their (scene, head, row) strides, mask, bias, sizes, scale, and the dropout triple (probability, host seed,
    the device's rng word -- passed only when something is dropped)."""
    bs = (bias.stride(0), bias.stride(1), bias.stride(2)) if bias is not None else (0, 0, 0)
    return (q_ptr, k_ptr, v_ptr, *q_strides, *k_strides, *v_strides,
            mask_u8.data_ptr() if mask_u8 is not None else None, mask_sb, mask_sq,
            bias.data_ptr() if bias is not None else None, *bs,
            B, h, Lq, Lk, dk, scale, float(dropout_p), int(seed),
            rng_state(device).data_ptr() if dropout_p > 0.0 else None)


class Operands:
    """Where the attention kernels read q, k, v -- three pointers and three (scene, head, row) stride triples -- and where their
    backward writes dq, dk, dv (``grads``): three tensors, or the three column blocks of one packed projection."""

    def __init__(self, ptrs, strides, B, h, Lq, Lk, dk, device, packed):
        self.ptrs, self.strides, self.device, self.packed = ptrs, strides, device, packed
        self.B, self.h, self.Lq, self.Lk, self.dk = B, h, Lq, Lk, dk
        self.scale = 1.0 / math.sqrt(dk)

    @staticmethod
    def separate(q, k, v):
        """q (B,h,Lq,d_k), k, v (B,h,Lk,d_k), last dimension dense."""
        B, h, Lq, dk = q.shape
        return Operands((q.data_ptr(), k.data_ptr(), v.data_ptr()), (_strides3(q), _strides3(k), _strides3(v)), B, h, Lq, k.shape[2],
                        dk, q.device, None)

    @staticmethod
    def packed(qkv, h):
        """qkv (B, L, 3*h*d_k) = [q | k | v], contiguous."""
        B, L, three_hd = qkv.shape
        hd = three_hd // 3
        base, es, strides = qkv.data_ptr(), qkv.element_size(), (L * three_hd, hd // h, three_hd)
        return Operands((base, base + hd * es, base + 2 * hd * es), (strides,) * 3, B, h, L, L, hd // h, qkv.device, qkv)

    def args(self, mask, bias, dropout_p, seed):
        """``mha_args`` of these operands; ``mask`` = (mask_u8, mask_sb, mask_sq) of ``_prep_mask``."""
        return mha_args(*self.ptrs, *self.strides, *mask, bias, self.B, self.h, self.Lq, self.Lk, self.dk, self.scale, dropout_p,
                        seed, self.device)

    def grads(self):
        """Fresh gradient buffers: (the tensors, their three pointers, the row stride of the packed layout or 0 for dense
        (B, L, h, d_k) ones)."""
        if self.packed is not None:
            dqkv = torch.empty_like(self.packed)
            gb, step = dqkv.data_ptr(), self.h * self.dk * dqkv.element_size()
            return (dqkv,), (gb, gb + step, gb + 2 * step), dqkv.shape[2]
        g = tuple(torch.empty(self.B, L, self.h, self.dk, dtype=torch.float32, device=self.device) for L in (self.Lq, self.Lk, self.Lk))
        return g, tuple(t.data_ptr() for t in g), 0


def mha_forward(o, mask, bias, dropout_p, seed, need_p):
    """One launch of spacap_mha_fwd_f32: (out (B,Lq,h,d_k), p (B,h,Lq,Lk) or None, the row statistics (B,h,Lq,2) = (max, sum))."""
    with torch.cuda.device(o.device):
        out = torch.empty(o.B, o.Lq, o.h, o.dk, dtype=torch.float32, device=o.device)
        p = torch.empty(o.B, o.h, o.Lq, o.Lk, dtype=torch.float32, device=o.device) if need_p else None
        lse = torch.empty(o.B, o.h, o.Lq, 2, dtype=torch.float32, device=o.device)
        check(lib.spacap_mha_fwd_f32(*o.args(mask, bias, dropout_p, seed), out.data_ptr(), p.data_ptr() if need_p else None,
                                     lse.data_ptr(), torch.cuda.current_stream(o.device).cuda_stream), "spacap_mha_fwd_f32")
    return out, p, lse


def mha_backward(o, mask, bias, dropout_p, seed, lse, d_out, d_p):
    """One call of spacap_mha_bwd_f32 for d_out (B,Lq,h,d_k) (any strides) and the optional gradient d_p of the attention map:
    the tensors of ``o.grads()``."""
    with torch.cuda.device(o.device):
        d_out_c = d_out.contiguous()
        d_p_c = d_p.contiguous() if d_p is not None else None
        g, gptrs, ld = o.grads()
        ws = torch.empty(max(int(lib.spacap_mha_bwd_workspace_bytes(o.B, o.h, o.Lq)), 16), dtype=torch.uint8, device=o.device)
        check(lib.spacap_mha_bwd_f32(*o.args(mask, bias, dropout_p, seed), lse.data_ptr(), d_out_c.data_ptr(),
                                     d_p_c.data_ptr() if d_p_c is not None else None, ws.data_ptr(), *gptrs, ld,
                                     torch.cuda.current_stream(o.device).cuda_stream), "spacap_mha_bwd_f32")
    return g


def mha_backward_delta(o, mask, dropout_p, seed, lse, d_out, delta):
    """One launch of spacap_mha_bwd_delta_f32 (dQ and dK / dV halves side by side) for a dense d_out whose row term
    delta[b, head, q] = sum_d out d_out the caller already has (tf_layer.AttnFfn1): the tensors of ``o.grads()``."""
    with torch.cuda.device(o.device):
        g, gptrs, ld = o.grads()
        check(lib.spacap_mha_bwd_delta_f32(*o.args(mask, None, dropout_p, seed), lse.data_ptr(), d_out.data_ptr(), delta.data_ptr(),
                                           *gptrs, ld, torch.cuda.current_stream(o.device).cuda_stream), "spacap_mha_bwd_delta_f32")
    return g


class FusedAttention(Function):
    @staticmethod
    def forward(ctx, q, k, v, mask_u8, mask_sb, mask_sq, bias, dropout_p, seed, need_p):
        if not q.is_cuda:
            raise RuntimeError("CPU not supported")
        q, k, v = (t if t.stride(3) == 1 else t.contiguous() for t in (q, k, v))
        out, p, lse = mha_forward(Operands.separate(q, k, v), (mask_u8, mask_sb, mask_sq), bias, dropout_p, seed, need_p)
        ctx.save_for_backward(q, k, v, mask_u8, bias, lse)
        ctx.set_materialize_grads(False)   # no zero tensor for the unused second output's gradient
        ctx.meta = (mask_sb, mask_sq, dropout_p, seed, need_p)
        out_v = out.transpose(1, 2)
        if need_p:
            return out_v, p
        ctx.mark_non_differentiable(lse)
        return out_v, lse  # second output unused by callers when need_p is False

    @staticmethod
    def backward(ctx, d_out, d_p):
        q, k, v, mask_u8, bias, lse = ctx.saved_tensors
        mask_sb, mask_sq, dropout_p, seed, need_p = ctx.meta
        if d_out is None:   # only the attention map was used downstream
            d_out = torch.zeros(q.shape, dtype=torch.float32, device=q.device)
        dq, dk, dv = mha_backward(Operands.separate(q, k, v), (mask_u8, mask_sb, mask_sq), bias, dropout_p, seed, lse,
                                  d_out.transpose(1, 2), d_p if need_p else None)
        return (dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2), None, None, None, None, None, None, None)


class FusedSelfAttentionPacked(Function):
    """Self-attention on a packed projection qkv (B, L, 3*h*d_k) = [q | k | v] (one GEMM instead of three): the
    kernels read q, k, v through strides and the backward writes dq, dk, dv straight into one (B, L, 3*h*d_k)
    buffer, so the projection's backward is one dX GEMM, one dW GEMM and one bias sum instead of three each plus
    two accumulations.  Returns (out (B,L,h*d_k), p_attn (B,h,L,L) or the row statistics)."""

    @staticmethod
    def forward(ctx, qkv, h, mask_u8, mask_sb, mask_sq, dropout_p, seed, need_p):
        if not qkv.is_cuda:
            raise RuntimeError("CPU not supported")
        qkv = qkv.contiguous()
        out, p, lse = mha_forward(Operands.packed(qkv, h), (mask_u8, mask_sb, mask_sq), None, dropout_p, seed, need_p)
        ctx.save_for_backward(qkv, mask_u8, lse)
        ctx.set_materialize_grads(False)   # no zero tensor for the unused second output's gradient
        ctx.meta = (h, mask_sb, mask_sq, dropout_p, seed, need_p)
        out = out.view(qkv.shape[0], qkv.shape[1], -1)
        if need_p:
            return out, p
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, d_out, d_p):
        qkv, mask_u8, lse = ctx.saved_tensors
        h, mask_sb, mask_sq, dropout_p, seed, need_p = ctx.meta
        if d_out is None:   # only the attention map was used downstream
            d_out = torch.zeros(qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3, dtype=torch.float32, device=qkv.device)
        (dqkv,) = mha_backward(Operands.packed(qkv, h), (mask_u8, mask_sb, mask_sq), None, dropout_p, seed, lse, d_out,
                               d_p if need_p else None)
        return dqkv, None, None, None, None, None, None, None


def self_attention_packed(qkv, h, mask=None, dropout_p=0.0, training=False, need_p=True):
    """qkv (B,L,3*h*d_k) packed [q | k | v] -> (out (B,L,h*d_k), p_attn (B,h,L,L) or None)."""
    B, L, _ = qkv.shape
    m, msb, msq = _prep_mask(mask, B, L, L)
    p = float(dropout_p) if training else 0.0
    seed = _next_seed() if p > 0.0 else 0
    out, second = FusedSelfAttentionPacked.apply(qkv, h, m, msb, msq, p, seed, need_p)
    return out, (second if need_p else None)


def attention(query, key, value, mask=None, dropout_p=0.0, training=False, need_p=True, bias=None):
    """(out (B,h,Lq,d_k), p_attn (B,h,Lq,Lk) or None); see the module docstring."""
    B, h, Lq, dk = query.shape
    Lk = key.shape[2]
    if bias is not None and bias.requires_grad:
        raise RuntimeError("attention: no gradient is formed for the bias (it is a constant of the logits); pass bias.detach()")
    m, msb, msq = _prep_mask(mask, B, Lq, Lk)
    p = float(dropout_p) if training else 0.0
    seed = _next_seed() if p > 0.0 else 0
    out, second = FusedAttention.apply(query, key, value, m, msb, msq, bias, p, seed, need_p)
    return out, (second if need_p else None)


def _ln_backward(xc, a, stats, dyc, add, eps):
    """dx, da, db of the LayerNorm; the (da, db) column sums over the workgroup partials go through ``sum_slabs``
    (same 4-group order as the library's own reduction kernel) so that a training step can batch them with the
    weight-gradient sums (deferred_slab_sums)."""
    D = xc.shape[-1]
    rows = xc.numel() // D
    with torch.cuda.device(xc.device):
        dx = torch.empty_like(xc)
        nbytes = int(lib.spacap_layernorm_bwd_workspace_bytes(rows, D))
        if D <= 512 and D % 2 == 0 and nbytes >= 8 * D:
            part = torch.empty(nbytes // (8 * D), 2 * D, dtype=torch.float32, device=xc.device)
            check(lib.spacap_layernorm_bwd_add_f32(xc.data_ptr(), a.data_ptr(), stats.data_ptr(), dyc.data_ptr(),
                                                   add.data_ptr() if add is not None else None, rows, D, eps,
                                                   dx.data_ptr(), None, None, part.data_ptr(),
                                                   torch.cuda.current_stream(xc.device).cuda_stream),
                  "spacap_layernorm_bwd_add_f32")
            s = sum_slabs(part, deferrable=True)
            return dx, s[:D], s[D:]
        da = torch.empty(D, dtype=torch.float32, device=xc.device)
        db = torch.empty(D, dtype=torch.float32, device=xc.device)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=xc.device)
        check(lib.spacap_layernorm_bwd_add_f32(xc.data_ptr(), a.data_ptr(), stats.data_ptr(), dyc.data_ptr(),
                                               add.data_ptr() if add is not None else None, rows, D, eps,
                                               dx.data_ptr(), da.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                               torch.cuda.current_stream(xc.device).cuda_stream),
              "spacap_layernorm_bwd_add_f32")
    return dx, da, db


class FusedLayerNorm(Function):
    """a * (x - mean) / (std_unbiased + eps) + b  (models/transformer_captioner.py:102-113) in one launch
    forward and two backward (spacap_layernorm_*_f32).  With ``residual``: (norm(x), x) for the pre-norm residual block
    ``x + dropout(sublayer(norm(x)))`` (:115-123) -- the second output is x itself, to be used as the residual operand, so
    that BOTH gradient paths into x arrive at this node and the backward kernel adds them while it writes dx
    (spacap_layernorm_bwd_add_f32); otherwise autograd sums them with one more pass per sub-layer."""

    @staticmethod
    def forward(ctx, x, a, b, eps, residual):
        if not x.is_cuda:
            raise RuntimeError("CPU not supported")
        xc = x.contiguous()
        D = xc.shape[-1]
        rows = xc.numel() // D
        with torch.cuda.device(x.device):
            y = torch.empty_like(xc)
            stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
            check(lib.spacap_layernorm_fwd_f32(xc.data_ptr(), a.data_ptr(), b.data_ptr(), rows, D, float(eps),
                                               y.data_ptr(), stats.data_ptr(),
                                               torch.cuda.current_stream(x.device).cuda_stream), "spacap_layernorm_fwd_f32")
        ctx.save_for_backward(xc, a, stats)
        ctx.eps = float(eps)
        if not residual:
            return y
        ctx.set_materialize_grads(False)
        return y, xc.view_as(xc)

    @staticmethod
    def backward(ctx, dy, dres=None):
        xc, a, stats = ctx.saved_tensors
        if dy is None:      # (residual form only: the norm was not used downstream)
            return dres, None, None, None, None
        dx, da, db = _ln_backward(xc, a, stats, dy.contiguous(), dres.contiguous() if dres is not None else None, ctx.eps)
        return dx, da, db, None, None


def layer_norm(x, a, b, eps=1e-6):
    return FusedLayerNorm.apply(x, a, b, eps, False)


def layer_norm_residual(x, a, b, eps=1e-6):
    """(norm(x), residual operand) -- see FusedLayerNorm."""
    return FusedLayerNorm.apply(x, a, b, eps, True)


def __getattr__(name):
    """The relation feature and first-layer nodes moved to relation.py; their names stay importable from here."""
    if name in ("RelationFeature", "RelationLayer1", "relation_feature", "relation_layer1"):
        from . import relation
        return getattr(relation, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
