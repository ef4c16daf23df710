"""Spatiality-guided Transformer captioner -- counterpart of ``models/transformer_captioner.py``.

Same module tree / parameter names as the reference (so its state dicts load), same ``data_dict``
contract.  The hot spots run on the HIP library:
  * ``attention()`` (reference :27-37) -> one fused kernel (``spacap3d_amd.attention``); the L x L matrix
    ``p_attn`` is materialised only for layers whose ``self.attn`` is consumed (``store_attn``), i.e. the
    last encoder layer (relation head, :392-394) -- or for every layer when ``store_attn_all`` is set,
    which reproduces the reference's always-on ``self.attn`` (used by its eval-time attention dumps);
  * the relation feature  R[b,i,j,(h,d)] = P[b,h,i,j] * V[b,h,j,d]  (:393-396) is formed by one broadcast
    product (the reference materialises an extra ``repeat`` copy of P first).
"""
import copy
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .backend import ops
from .loss_helper import nn_distance

MAX_DES_LEN = 30  # lib/config.py:55
PROPOSAL_FEATURE_DIM = 128  # models/proposal_module.py:39 (vote aggregation mlp [..., 128])


def subsequent_mask(size, device=None):
    """(1, size, size) bool, True on and below the diagonal (:16-20)."""
    return torch.ones(1, size, size, dtype=torch.bool, device=device).tril()


def clones(module, N):
    return nn.ModuleList([copy.deepcopy(module) for _ in range(N)])


def attention(query, key, value, mask=None, dropout=None, need_p=True):
    """Reference signature (:27) plus ``need_p``; returns (P V, p_attn)."""
    p = dropout.p if dropout is not None else 0.0
    training = dropout.training if dropout is not None else False
    return ops().attention(query, key, value, mask=mask, dropout_p=p, training=training, need_p=need_p)


def _linear(x, lin):
    """``lin(x)`` through the backend's Linear op (one-launch weight + bias gradient) when it has one."""
    f = getattr(ops(), "linear", None)
    if f is None or lin.bias is None or not x.is_cuda:
        return lin(x)
    return f(x, lin.weight, lin.bias)


def _linear_wb(x, w, b):
    f = getattr(ops(), "linear", None)
    return f(x, w, b) if (f is not None and x.is_cuda) else F.linear(x, w, b)


class MultiHeadedAttention(nn.Module):
    def __init__(self, h, d_model, dropout=0.1, keep_value=False, store_attn=None):
        super().__init__()
        assert d_model % h == 0
        self.d_k = d_model // h
        self.h = h
        self.linears = clones(nn.Linear(d_model, d_model), 4)
        self.attn = None
        self.value = None
        self.dropout = nn.Dropout(p=dropout)
        self.keep_value = keep_value
        # None: follow the module-wide default (see TransformerDecoderModel.store_attn_all)
        self.store_attn = store_attn

    def forward(self, query, key, value, mask=None):
        nb = query.size(0)
        packed = getattr(ops(), "self_attention_packed", None) if (query is key and key is value) else None
        if packed is not None and query.is_cuda:
            # self-attention: q, k, v from ONE GEMM over the concatenated weights; the kernels read the packed result
            # through strides and write one packed gradient (see attention.FusedSelfAttentionPacked)
            hd = self.h * self.d_k
            pk = getattr(self, "_packed_qkv", None)
            if pk is not None and pk[0].data_ptr() == self.linears[0].weight.data_ptr():
                # the three weights are adjacent in the optimizer's flat buffer (engine.py): no concatenation
                from .linear import PackedLinear
                qkv = PackedLinear.apply(query, pk[0], pk[1], *[l.weight for l in self.linears[:3]],
                                         *[l.bias for l in self.linears[:3]])
            else:
                w = torch.cat([l.weight for l in self.linears[:3]], dim=0)
                b = torch.cat([l.bias for l in self.linears[:3]], dim=0)
                qkv = _linear_wb(query, w, b)
            need_p = self.keep_value if self.store_attn is None else (self.store_attn or self.keep_value)
            p = self.dropout.p
            x, self.attn = packed(qkv, self.h, mask=mask, dropout_p=p, training=self.dropout.training, need_p=need_p)
            if self.keep_value:
                self.value = qkv[..., 2 * hd:].view(nb, -1, self.h, self.d_k).transpose(1, 2)
            return _linear(x, self.linears[-1])
        if mask is not None:
            mask = mask.unsqueeze(1)
        query, key, value = [l(x).view(nb, -1, self.h, self.d_k).transpose(1, 2)
                             for l, x in zip(self.linears, (query, key, value))]
        need_p = self.keep_value if self.store_attn is None else (self.store_attn or self.keep_value)
        x, self.attn = attention(query, key, value, mask=mask, dropout=self.dropout, need_p=need_p)
        if self.keep_value:
            self.value = value
        x = x.transpose(1, 2).contiguous().view(nb, -1, self.h * self.d_k)
        return _linear(x, self.linears[-1])


    def forward_incremental(self, x_new, cache, mask=None):
        """Self-attention for the newest token(s) only: project q/k/v of ``x_new`` (B, t_new, d), append k/v to
        ``cache`` (a dict holding 'k' and 'v' of the previous positions), attend over everything cached.  ``mask``
        (B, t_new, t_total) is only needed when several new tokens are fed at once (the first step)."""
        nb = x_new.size(0)
        q, k, v = [l(x_new).view(nb, -1, self.h, self.d_k).transpose(1, 2) for l in self.linears[:3]]
        if cache.get("k") is not None:
            k = torch.cat([cache["k"], k], dim=2)
            v = torch.cat([cache["v"], v], dim=2)
        cache["k"], cache["v"] = k, v
        m = mask.unsqueeze(1) if mask is not None else None
        x, _ = attention(q, k.contiguous(), v.contiguous(), mask=m, dropout=self.dropout, need_p=False)
        x = x.transpose(1, 2).contiguous().view(nb, -1, self.h * self.d_k)
        return self.linears[-1](x)


class PositionwiseFeedForward(nn.Module):
    def __init__(self, d_model, d_ff, dropout=0.1):
        super().__init__()
        self.w_1 = nn.Linear(d_model, d_ff)
        self.w_2 = nn.Linear(d_ff, d_model)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x):
        h = _linear(x, self.w_1)
        tail = getattr(ops(), "ffn_tail", None)
        if tail is not None and h.is_cuda:
            out = tail(h, self.w_2.weight, self.w_2.bias, self.dropout.p, self.dropout.training)
            if out is not None:
                return out
        f = getattr(ops(), "relu_dropout", None)
        h = f(h, self.dropout.p, self.dropout.training) if (f is not None and h.is_cuda) else self.dropout(F.relu(h))
        return _linear(h, self.w_2)


class Embeddings(nn.Module):
    def __init__(self, d_model, vocab):
        super().__init__()
        self.lut = nn.Embedding(vocab, d_model)
        self.d_model = d_model

    def forward(self, x):
        return self.lut(x) * math.sqrt(self.d_model)


class Generator(nn.Module):
    def __init__(self, d_model, vocab):
        super().__init__()
        self.proj = nn.Linear(d_model, vocab)

    def forward(self, x):
        return F.log_softmax(self.proj(x), dim=-1)


class LayerNorm(nn.Module):
    """a * (x - mean) / (std_unbiased + eps) + b   (:102-113) -- NOT nn.LayerNorm."""

    def __init__(self, features, eps=1e-6):
        super().__init__()
        self.a_2 = nn.Parameter(torch.ones(features))
        self.b_2 = nn.Parameter(torch.zeros(features))
        self.eps = eps

    def forward(self, x):
        return ops().layer_norm(x, self.a_2, self.b_2, self.eps)


class SublayerConnection(nn.Module):
    def __init__(self, size, dropout):
        super().__init__()
        self.norm = LayerNorm(size)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x, sublayer):
        nr = getattr(ops(), "layer_norm_residual", None)
        if nr is not None and x.is_cuda and torch.is_grad_enabled() and x.requires_grad:
            # norm and residual operand from one node: its backward adds the two gradient paths into x itself
            normed, x = nr(x, self.norm.a_2, self.norm.b_2, self.norm.eps)
            y = sublayer(normed)
        else:
            y = sublayer(self.norm(x))
        f = getattr(ops(), "dropout_add", None)
        if f is not None and y.is_cuda:
            return f(x, y, self.dropout.p, self.dropout.training)
        return x + self.dropout(y)


class PositionalEncoding(nn.Module):
    def __init__(self, d_model, dropout, max_len=5000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len).unsqueeze(1).float()
        div_term = torch.exp(torch.arange(0, d_model, 2).float() * -(math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe", pe.unsqueeze(0))

    def forward(self, x, src_pos=None):
        return self.dropout(x + self.pe[:, :x.size(1)])


class PositionalEncodingLearned(nn.Module):
    def __init__(self, input_channel, d_model=128):
        super().__init__()
        self.position_embedding_head = nn.Sequential(
            nn.Conv1d(input_channel, d_model, kernel_size=1), nn.BatchNorm1d(d_model), nn.ReLU(inplace=True),
            nn.Conv1d(d_model, d_model, kernel_size=1))

    def forward(self, x, xyz):
        h = self.position_embedding_head
        t = xyz.transpose(1, 2).contiguous()
        if self.training and t.is_cuda and getattr(ops(), "bn_relu_train", None) is not None:
            conv = getattr(ops(), "conv1x1", None)

            def c(m, v):   # 1x1 convolution whose weight gradient joins the step's deferred batch (linear.Conv1x1)
                y = conv(v, m) if conv is not None else None
                return m(v) if y is None else y
            t = c(h[3], ops().bn_relu_train(c(h[0], t), h[1]))   # Conv1d -> [BatchNorm1d -> ReLU as one fused op] -> Conv1d
        elif t.is_cuda and not torch.is_grad_enabled() and getattr(ops(), "conv1x1", None) is not None:
            conv = ops().conv1x1     # inference forward: the two 1x1 convolutions on the library's kernel, BatchNorm on running statistics

            def c(m, v):
                y = conv(v, m)
                return m(v) if y is None else y
            g = getattr(ops(), "bn_relu_eval", None)
            u = c(h[0], t)
            v = g(u, h[1]) if g is not None else None
            t = c(h[3], h[2](h[1](u)) if v is None else v)
        else:
            t = h(t)
        return x + t.transpose(1, 2).contiguous()


class Encoder(nn.Module):
    def __init__(self, layer, N):
        super().__init__()
        self.layers = clones(layer, N)
        self.norm = LayerNorm(layer.size)

    def forward(self, x, mask):
        st = getattr(ops(), "tf_stack", None)
        if st is not None and st.stack_supported(self.layers, x):
            return st.run_stack(self.layers, self.norm, x, mask)   # 4 launches per layer (spacap3d_amd/tf_layer.py)
        for layer in self.layers:
            x = layer(x, mask)
        return self.norm(x)


class EncoderLayer(nn.Module):
    def __init__(self, size, self_attn, feed_forward, dropout):
        super().__init__()
        self.self_attn = self_attn
        self.feed_forward = feed_forward
        self.sublayer = clones(SublayerConnection(size, dropout), 2)
        self.size = size

    def forward(self, x, mask):
        x = self.sublayer[0](x, lambda y: self.self_attn(y, y, y, mask))
        return self.sublayer[1](x, self.feed_forward)


class Decoder(nn.Module):
    def __init__(self, layer, N):
        super().__init__()
        self.layers = clones(layer, N)
        self.norm = LayerNorm(layer.size)

    def forward(self, x, memory, src_mask, tgt_mask, obj_indicator=None):
        if obj_indicator is not None:
            x = torch.cat((obj_indicator, x), dim=1)
        st = getattr(ops(), "tf_stack", None)
        if st is not None and st.stack_supported(self.layers, x):   # early guide: self-attention + feed-forward only
            return st.run_stack(self.layers, self.norm, x, tgt_mask)
        for layer in self.layers:
            x = layer(x, memory, src_mask, tgt_mask)
        return self.norm(x)


class DecoderLayer(nn.Module):
    def __init__(self, size, self_attn, src_attn, feed_forward, dropout, early_guide=True):
        super().__init__()
        self.size = size
        self.self_attn = self_attn
        self.src_attn = src_attn
        self.feed_forward = feed_forward
        self.early_guide = early_guide
        self.sublayer = clones(SublayerConnection(size, dropout), 3)

    def forward(self, x, memory, src_mask, tgt_mask):
        m = memory
        x = self.sublayer[0](x, lambda y: self.self_attn(y, y, y, tgt_mask))
        if not self.early_guide:
            x = self.sublayer[1](x, lambda y: self.src_attn(y, m, m, src_mask))
        return self.sublayer[2](x, self.feed_forward)


def decode_incremental(decoder, x_new, caches, memory=None, src_mask=None, mask=None):
    """Run ``x_new`` (B, t_new, d) -- the positions not seen yet -- through the decoder stack, reusing the cached
    keys / values of earlier positions (one dict per layer).  Pre-LN layers with a causal mask make this exactly
    the last rows of the full recomputation the reference performs at every step (:435-438)."""
    x = x_new
    for layer, cache in zip(decoder.layers, caches):
        x = x + layer.sublayer[0].dropout(layer.self_attn.forward_incremental(layer.sublayer[0].norm(x), cache, mask))
        if not layer.early_guide:
            x = layer.sublayer[1](x, lambda y: layer.src_attn(y, memory, memory, src_mask))
        x = layer.sublayer[2](x, layer.feed_forward)
    return decoder.norm(x)


class _Identity(nn.Module):
    def forward(self, x, *a):
        return x


class EncoderDecoder(nn.Module):
    def __init__(self, encoder, decoder, src_embed, tgt_embed, generator, early_guide=True):
        super().__init__()
        self.encoder = encoder
        self.decoder = decoder
        self.src_embed = src_embed
        self.tgt_embed = tgt_embed
        self.generator = generator
        self.early_guide = early_guide

    def forward(self, src, tgt, src_mask, tgt_mask, obj_indicator=None, src_pos=None, obj_idx=None, memory=None):
        if memory is None:
            if self.encoder is None:
                memory = self.src_embed(src, src_pos) if src_pos is not None else src
            else:
                memory = self.encode(src, src_pos, src_mask)
        return self.decode(memory, src_mask, tgt, tgt_mask, obj_indicator=obj_indicator, obj_idx=obj_idx)

    def encode(self, src, src_pos, src_mask):
        return self.encoder(self.src_embed(src, src_pos), src_mask)

    def decode(self, memory, src_mask, tgt, tgt_mask, obj_indicator=None, obj_idx=None):
        if memory.shape[0] != tgt.shape[0]:  # inference: B*K sequences over B scenes (:252-257)
            assert memory.shape[0] * memory.shape[1] == tgt.shape[0]
            B, K, _ = memory.shape
            obj_indicator = obj_indicator + memory.reshape(B * K, -1).unsqueeze(1)
            if self.early_guide:
                # the reference materialises repeat_interleave(memory, K) = (B*K, K, d); in early-guide mode
                # the decoder never reads it (no cross-attention, :223-224), so it is not built here
                memory = None
        if obj_idx is not None:  # training (:260-261)
            obj_indicator = obj_indicator + torch.gather(
                memory, 1, obj_idx.repeat(1, memory.size(-1)).unsqueeze(1))
        if self.early_guide:
            return self.decoder(self.tgt_embed(tgt), memory, src_mask, tgt_mask, obj_indicator=obj_indicator)
        return self.decoder(self.tgt_embed(tgt), obj_indicator, None, tgt_mask, None)


class TransformerDecoderModel(nn.Module):
    def __init__(self, vocabulary, N, h, d_model, d_ff, transformer_dropout, bn_momentum=0.1, src_pos_type=None,
                 use_transformer_encoder=False, early_guide=True, check_relation=False, store_attn_all=False):
        super().__init__()
        self.word_to_idx = vocabulary["word2idx"]
        self.src_pos_type = src_pos_type
        self.vocabulary = vocabulary
        self.use_transformer_encoder = use_transformer_encoder
        self.check_relation = check_relation
        self.early_guide = early_guide
        self.store_attn_all = store_attn_all
        self.model = self.make_model(len(vocabulary["word2idx"]), N=N, h=h, d_model=d_model, d_ff=d_ff,
                                     dropout=transformer_dropout, bn_momentum=bn_momentum,
                                     src_pos_type=src_pos_type, use_transformer_encoder=use_transformer_encoder,
                                     early_guide=early_guide)
        # DEVIATION (BASELINE configs[4] "d_model=512"): the reference has no input projection, so
        # its encoder only runs with d_model == 128 (the proposal feature width, :163-164).  For other widths the 128-d
        # proposal tokens go through one Linear(128, d_model) first; with d_model == 128 (every reference configuration)
        # the module does not exist and the state-dict layout is the reference's.
        self.token_proj = nn.Linear(PROPOSAL_FEATURE_DIM, d_model) if d_model != PROPOSAL_FEATURE_DIM else None
        if check_relation:
            self.relation_proposal = nn.Sequential(nn.Linear(d_model, d_model), nn.ReLU(),
                                                   nn.Linear(d_model, d_model), nn.ReLU(), nn.Linear(d_model, 9))
        if store_attn_all:
            for mod in self.modules():
                if isinstance(mod, MultiHeadedAttention):
                    mod.store_attn = True

    def make_model(self, tgt_vocab, N=6, h=8, d_model=512, d_ff=2048, dropout=0.1, bn_momentum=0.1,
                   src_pos_type=None, use_transformer_encoder=False, early_guide=True):
        c = copy.deepcopy
        attn = MultiHeadedAttention(h, d_model)
        ff = PositionwiseFeedForward(d_model, d_ff, dropout)
        position = PositionalEncoding(d_model, dropout)
        if src_pos_type is not None:
            src_position = PositionalEncodingLearned(3 if src_pos_type in ("xyz", "center") else 6, d_model)
        else:
            src_position = c(position)
        encoder = None
        if use_transformer_encoder:
            # only the LAST encoder layer's P and V are read (relation head), the reference keeps all six
            layer = EncoderLayer(d_model, MultiHeadedAttention(h, d_model, keep_value=False), c(ff), dropout)
            encoder = Encoder(layer, N)
            encoder.layers[-1].self_attn.keep_value = self.check_relation
        model = EncoderDecoder(
            encoder,
            Decoder(DecoderLayer(d_model, c(attn), c(attn), c(ff), dropout, early_guide), N),
            src_position if use_transformer_encoder else _Identity(),
            nn.Sequential(Embeddings(d_model, tgt_vocab), c(position)),
            Generator(d_model, tgt_vocab), early_guide=early_guide)
        for p in model.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        for m in model.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.momentum = bn_momentum
        return model

    def _prepare_feature(self, seq):
        seq = seq[:, :-1] if self.early_guide else seq[:, 1:-1]
        seq_mask = (seq > 0).unsqueeze(-2)
        seq_mask = seq_mask & subsequent_mask(seq.size(-1), device=seq.device)
        return (seq[:, 1:] if self.early_guide else seq), seq_mask

    def forward(self, data_dict, is_eval=False):
        return self.forward_eval(data_dict) if is_eval else self.forward_train(data_dict)

    def _src_pos(self, ep):
        if self.src_pos_type == "xyz":
            return ep["aggregated_vote_xyz"]
        if self.src_pos_type == "center":
            return ep["center"]
        if self.src_pos_type == "loc":
            return torch.cat([ep["center"], ep["pred_size"]], -1)
        return None

    def relation_feature(self):
        """R[b,i,j,h*16+d] = P[b,h,i,j] * V[b,h,j,d] of the last encoder layer (:393-396)."""
        sa = self.model.encoder.layers[-1].self_attn
        return ops().relation_feature(sa.attn, sa.value)   # (B,h,K,K), (B,h,K,d_k) -> (B,K,K,h*d_k)

    def forward_train(self, ep):
        src = ep["aggregated_vote_features"]
        if self.token_proj is not None:
            src = _linear(src, self.token_proj)
        src_pos = self._src_pos(ep)
        prep = getattr(ops(), "caption_prep", None) if (src.is_cuda and self.early_guide and self.model.encoder is not None) else None
        src_mask = ep["bbox_mask"].unsqueeze(1)
        x0 = out_full = None
        scst = self.self_critical if self.training else None
        dxe = self.dense_xe if self.training else None
        if dxe is not None and scst is not None:
            raise ValueError("dense_xe and self_critical are both set: one training mode at a time")
        if scst is not None and prep is None:
            raise RuntimeError("self_critical: CPU tensors, a backend without caption_prep, the late guide and a captioner without "
                               "the Transformer encoder are not supported")
        if dxe is not None and prep is None:
            raise RuntimeError("dense_xe: CPU tensors, a backend without caption_prep, the late guide and a captioner without "
                               "the Transformer encoder are not supported")
        if prep is not None:
            # encoder first, then nearest proposal + object indicator + token embedding + positional encoding + dropout + mask
            # as one launch (csrc/caption_prep.hip) and the decoder stack on its output
            memory = self.model.encode(src, src_pos, src_mask)
            if self.check_relation:
                self._relation_head_forked(ep)
            if scst is not None:
                return self._self_critical_train(ep, scst, prep, src, memory)
            if dxe is not None:
                return self._dense_xe_train(ep, dxe, prep, src, memory)
            te = self.model.tgt_embed
            got = prep(ep["aggregated_vote_xyz"], ep["ref_center_label"], src, memory, ep["lang_label"], te[0], te[1])
            if got is not None:
                x0, m8, idx1, dist, good, pred_ious = got
                ep["match_idx"] = idx1
                out_full = self.model.decoder(x0, None, None, m8)
                out = out_full[:, 1:, :]
        if x0 is None:
            _, _, target_ious, idx = nn_distance(ep["aggregated_vote_xyz"], ep["ref_center_label"].unsqueeze(1))
            ep["match_idx"] = idx.squeeze(1)
            ref_obj_feature = torch.gather(src, 1, idx.repeat(1, src.size(-1)).unsqueeze(1))
            seq, seq_mask = self._prepare_feature(ep["lang_label"])
            if prep is None:
                memory = None
                if self.model.encoder is not None:
                    memory = self.model.encode(src, src_pos, src_mask)
                    if self.check_relation:
                        self._relation_head(ep)  # reads the last encoder layer only
            out = self.model(src=src, tgt=seq, src_mask=src_mask, tgt_mask=seq_mask,
                             obj_indicator=ref_obj_feature, src_pos=src_pos,
                             obj_idx=idx if self.use_transformer_encoder else None, memory=memory)
            out = out[:, 1:, :] if self.early_guide else out
            good = (target_ious > -1).squeeze(1)
            # mean over the good boxes without a host sync (the reference branches on .sum() > 0, :385)
            pred_ious = (target_ious.squeeze(1) * good).sum() / good.sum().clamp(min=1)
        fused = getattr(ops(), "caption_head_loss", None) if (out.is_cuda and self.training and "lang_ids" in ep) else None
        if fused is not None and ep["lang_ids"].shape[1] >= out.shape[1] + 1:
            # vocabulary projection, then log-softmax + the caption loss / accuracy in one op (fused_losses.CaptionHeadLoss);
            # loss_helper.get_scene_cap_loss picks the pair up instead of recomputing it from the log-probabilities
            # (the projection reads positions 1.. of the decoder output in place and writes its data gradient into the full
            # layout: no slice copy, no padding of the gradient -- linear.VocabProjection)
            vp = getattr(ops(), "vocab_projection", None) if out_full is not None else None
            logits = vp(out_full, self.model.generator.proj, 1) if vp is not None else None
            if logits is None:
                logits = self.model.generator.proj(out)
            ep["lang_cap"], cl, ca, ep["_cap_vec"] = fused(logits, ep["lang_ids"], good)
            ep["_cap_loss"] = (cl, ca)
        else:
            ep["lang_cap"] = self.model.generator(out)
        ep["pred_ious"] = pred_ious
        ep["good_bbox_masks"] = good
        if self.check_relation and "relation_pred" not in ep:
            self._relation_head(ep)
        return ep

    # Self-critical training: None = off, else a self_critical.SelfCritical.  A plain attribute, not in the
    # state dict; read in training mode only.
    self_critical = None

    def _self_critical_train(self, ep, sc, prep, src, memory):
        """The captioner's part of a self-critical training step, after the encoder and the relation head: S captions drawn for
        the referred object's proposal (and, with the greedy baseline, its greedy caption), their CIDEr-D rewards, the
        teacher-forced pass over the samples and the reward-weighted loss in place of the cross-entropy.  Drawing and scoring run
        under ``no_grad`` through the cached decode kernels (no dropout); only the teacher-forced pass is differentiated.  No
        value is read back on the host.

        With ``sc.reward`` other than CIDEr-D alone the rewards are the weighted sums of the mixed launch
        and their terms are left as ``scst_reward_terms`` / ``scst_baseline_terms``.  With ``sc.xe_weight`` > 0 the teacher-forced
        pass runs once over the B ground-truth captions (``lang_label``, at the same proposals) AND the B S samples, and
        ``mixed_caption_loss`` leaves L_rl + xe_weight L_xe with ``scst_xe_loss`` / ``scst_xe_acc``: one embedding, one vocabulary
        projection, one loss node -- every parameter keeps one autograd use."""
        if sc.proposals == "matched":
            return self._self_critical_matched(ep, sc, prep, src, memory)
        for k in ("object_id", "dataset_idx"):
            if k not in ep:
                raise KeyError(f"self_critical: the batch has no {k!r}")
        xe = sc.xe_weight > 0.0
        self._scst_xe_keys(ep, xe)
        cd = getattr(ops(), "caption_decode", None)
        loss_op = getattr(ops(), "mixed_caption_loss" if xe else "self_critical_loss", None)
        te, dec, gen = self.model.tgt_embed, self.model.decoder, self.model.generator
        B, _, D = src.shape
        S, n_words = sc.num_samples, MAX_DES_LEN + 1
        with torch.no_grad():
            # the nearest proposal and whether it is good, as the cross-entropy path finds them: a B-row caption_prep over two
            # token columns (no word row is embedded), outside autograd -- the embedding table keeps ONE use in the graph
            got = prep(ep["aggregated_vote_xyz"], ep["ref_center_label"], src, memory,
                       torch.ones(B, 2, dtype=torch.int64, device=src.device), te[0], te[1])
            if got is None or cd is None or loss_op is None:
                raise RuntimeError("self_critical: these tensors are not supported by the fused caption path")
            _, _, idx, _, good, pred_ious = got
            sel = idx.view(B, 1, 1).expand(B, 1, D)
            indicator = (src.gather(1, sel) + memory.gather(1, sel)).squeeze(1)
            if not cd.decode_supported(dec.layers, indicator, n_words):
                raise RuntimeError("self_critical: this decoder stack is not supported by the fused decode")
            ys, score, _ = self._scst_draw(cd, sc, dec, gen, te, indicator, n_words)
            didx, oid = ep["dataset_idx"].reshape(-1), ep["object_id"].reshape(-1)
            words = ys.view(B * S, n_words)
            # (with the settings of section 7l the reward and the baseline's reward come from the mixed launch, with their terms)
            reward, key, length, tf_tok, *terms = sc.rewards(words, didx, oid, S, terms=sc.mixed)
            base = base_terms = None
            if sc.baseline == "greedy":
                base, _, _, _, *base_terms = sc.rewards(cd.greedy_decode(dec, gen, te[0], te[1].pe, indicator, sc.sos, n_words), didx,
                                                        oid, 1, terms=sc.mixed)
            count = good & (key.view(B, S)[:, 0] >= 0)
            # the token row caption_prep reads is lang_label's layout: one leading column, then sos and the words (tf_tok is
            # lang_ids' layout); its T = n_words + 2 columns give one logit row per decoded word
            tok = torch.cat([torch.ones(B * S, 1, dtype=torch.int64, device=src.device), tf_tok[:, :-1]], 1)
            if xe:
                gt_tok, tok, loss_words, xe_positions = self._scst_xe_rows(ep, tok, words)
        if xe:
            # ONE teacher-forced pass over B ground-truth rows and B S sample rows: every parameter keeps one autograd use
            rep = lambda t: torch.cat([t, t.repeat_interleave(S, 0)], 0)
            tok = torch.cat([gt_tok, tok], 0)
        else:
            rep = lambda t: t.repeat_interleave(S, 0)      # autograd sums the S gradients of every scene row
        got = prep(rep(ep["aggregated_vote_xyz"]), rep(ep["ref_center_label"]), rep(src), rep(memory), tok, te[0], te[1])
        if got is None:
            raise RuntimeError("self_critical: these tensors are not supported by the fused caption path")
        x0, m8 = got[0], got[1]
        out_full = dec(x0, None, None, m8)
        vp = getattr(ops(), "vocab_projection", None)
        logits = vp(out_full, gen.proj, 1) if vp is not None else None
        if logits is None:
            logits = gen.proj(out_full[:, 1:, :])
        if xe:
            out, adv, rowlogp = loss_op(logits, ep["lang_ids"], good, loss_words, length, reward, base, count, S, sc.xe_weight,
                                        xe_positions)
            ep["_cap_loss"] = (out[0], out[3])
            ep["scst_xe_loss"], ep["scst_xe_acc"] = out[2].detach(), out[4].detach()
        else:
            out, adv, rowlogp = loss_op(logits, words, length, reward, base, count, S)
            ep["_cap_loss"] = (out[0], out[1])
        ep["match_idx"], ep["pred_ious"], ep["good_bbox_masks"] = idx, pred_ious, good
        ep["scst_samples"], ep["scst_reward"] = ys, reward.view(B, S)
        ep["scst_baseline"] = base if base is not None else reward.view(B, S).mean(1)
        ep["scst_advantage"], ep["scst_logp"] = adv.view(B, S), rowlogp.view(B, S)
        ep["scst_sample_scores"], ep["scst_count"] = score, count
        ep["scst_stats"] = out.detach()
        if sc.mixed:
            ep["scst_reward_terms"] = terms[0].view(B, S, 3)
            ep["scst_baseline_terms"] = base_terms[0] if base_terms is not None else terms[0].view(B, S, 3).mean(1)
        return ep

    @staticmethod
    def _scst_xe_keys(ep, xe):
        """With a cross-entropy term the batch carries the referred object's ground-truth caption."""
        if xe:
            for k in ("lang_label", "lang_ids", "ref_center_label"):
                if k not in ep:
                    raise KeyError(f"self_critical: the batch has no {k!r}")

    @staticmethod
    def _scst_xe_rows(ep, tok, words):
        """The rows of the one teacher-forced pass of section 7l at one width: ``lang_label`` (B, Tg) and the samples' token rows
        ``tok`` (R, Ts) padded with the pad id 0 to T = max(Tg, Ts) columns, and the drawn ``words`` (R, n_words) padded to the
        W = T - 2 word positions of the pass (behind every row's length: never counted).  The ground-truth rows keep their own
        Tg - 2 word positions for the loss: what is padded behind them counts for nothing, the denominator included, so the
        cross-entropy is the plain training forward's.  Returns (ground-truth token rows, sample token rows, words, Tg - 2)."""
        pad = torch.nn.functional.pad
        gt, ids = ep["lang_label"], ep["lang_ids"]
        if gt.dtype != torch.int64 or ids.dtype != torch.int64 or gt.dim() != 2 or ids.dim() != 2 or gt.shape[0] != ids.shape[0]:
            raise RuntimeError(f"self_critical: lang_label / lang_ids must be int64 (B, T), got {tuple(gt.shape)} {gt.dtype}, "
                               f"{tuple(ids.shape)} {ids.dtype}")
        Tg = gt.shape[1]
        if Tg < 3 or ids.shape[1] < Tg - 1:
            raise RuntimeError(f"self_critical: lang_label {tuple(gt.shape)} gives {Tg - 2} word positions and needs lang_ids of "
                               f"{Tg - 1} columns or more, got {tuple(ids.shape)}")
        T = max(Tg, tok.shape[1])
        W = T - 2
        gt = pad(gt, (0, T - Tg)) if Tg < T else gt
        tok = pad(tok, (0, T - tok.shape[1])) if tok.shape[1] < T else tok
        words = pad(words, (0, W - words.shape[1])) if words.shape[1] < W else words
        return gt, tok, words, Tg - 2

    @staticmethod
    def _scst_draw(cd, sc, dec, gen, te, indicator, n_words):
        """The S samples of every row of ``indicator`` for a self-critical step: ``caption_decode.sample_decode`` with the
        sampler's settings."""
        got = cd.sample_decode(dec, gen, te[0], te[1].pe, indicator, sc.sos, sc.eos, n_words, sc.num_samples, sc.temperature, sc.top_k,
                               sc.seed, sc.top_p)
        if got is None:
            raise ValueError(f"self_critical: top_p needs a vocabulary of at most {cd.NUCLEUS_MAX_V} words")
        return got

    def _self_critical_matched(self, ep, sc, prep, src, memory):
        """The same step over every matched object of a scene: ``sc.select`` pairs up to M annotated
        objects per scene with their nearest proposals, the B M groups play the part the B scenes play above -- S samples, a
        baseline, S rewards against the object's own references per group; an empty slot draws from a zero indicator and counts
        for nothing -- and ``caption_prep_rows`` reads the encoder rows by index, so that autograd gets the sum of a proposal's
        gradients from one launch instead of from M S copies of ``src`` and ``memory``.  No value is read back on the host.
        ``sc.reward`` and ``sc.xe_weight`` as in ``_self_critical_train``."""
        for k in ("center_label", "box_label_mask", "scene_object_ids", "dataset_idx"):
            if k not in ep:
                raise KeyError(f"self_critical: the batch has no {k!r}")
        xe = sc.xe_weight > 0.0
        self._scst_xe_keys(ep, xe)
        cd = getattr(ops(), "caption_decode", None)
        loss_op = getattr(ops(), "mixed_caption_loss" if xe else "self_critical_loss", None)
        prep_rows = getattr(ops(), "caption_prep_rows", None)
        te, dec, gen = self.model.tgt_embed, self.model.decoder, self.model.generator
        B, _, D = src.shape
        S, M, n_words = sc.num_samples, sc.max_proposals, MAX_DES_LEN + 1
        dev = src.device
        with torch.no_grad():
            # match_idx / pred_ious / good_bbox_masks keep their meaning: the referred object's nearest proposal
            got = prep(ep["aggregated_vote_xyz"], ep["ref_center_label"], src, memory,
                       torch.ones(B, 2, dtype=torch.int64, device=dev), te[0], te[1])
            if got is None or cd is None or loss_op is None or prep_rows is None:
                raise RuntimeError("self_critical: these tensors are not supported by the fused caption path")
            _, _, idx, _, good, pred_ious = got
            prop, obj, _, key, _, _ = sc.select(ep["aggregated_vote_xyz"], ep["center_label"], ep["box_label_mask"],
                                                ep["scene_object_ids"], ep["dataset_idx"])
            count = prop >= 0
            sel = prop.clamp(min=0).unsqueeze(-1).expand(B, M, D)
            indicator = (src.gather(1, sel) + memory.gather(1, sel)).masked_fill(~count.unsqueeze(-1), 0.0).reshape(B * M, D)
            if not cd.decode_supported(dec.layers, indicator, n_words):
                raise RuntimeError("self_critical: this decoder stack is not supported by the fused decode")
            ys, score, _ = self._scst_draw(cd, sc, dec, gen, te, indicator, n_words)
            didx, oid = ep["dataset_idx"].reshape(B, 1).expand(B, M).reshape(-1), obj.reshape(-1)
            words = ys.view(B * M * S, n_words)
            reward, _, length, tf_tok, *terms = sc.rewards(words, didx, oid, S, terms=sc.mixed)
            base = base_terms = None
            if sc.baseline == "greedy":
                base, _, _, _, *base_terms = sc.rewards(cd.greedy_decode(dec, gen, te[0], te[1].pe, indicator, sc.sos, n_words), didx,
                                                        oid, 1, terms=sc.mixed)
            tok = torch.cat([torch.ones(B * M * S, 1, dtype=torch.int64, device=dev), tf_tok[:, :-1]], 1)
            if xe:
                # ONE teacher-forced pass over B ground-truth rows and B M S sample rows (every parameter keeps one autograd
                # use).  caption_prep_rows addresses (scene, proposal) per row and takes its rows scene by scene: with one row per
                # group, scene b holds its ground-truth row at the referred object's proposal, then its M S sample rows; `first`
                # then brings the B ground-truth rows to the front, where the loss expects them.
                gt_tok, tok, loss_words, xe_positions = self._scst_xe_rows(ep, tok, words)
                T, MS = tok.shape[1], M * S
                row_prop = torch.cat([idx.view(B, 1), prop.view(B, M, 1).expand(B, M, S).reshape(B, MS)], 1)
                row_tok = torch.cat([gt_tok.view(B, 1, T), tok.view(B, MS, T)], 1).reshape(B * (1 + MS), T)
                at = torch.arange(B, device=dev) * (1 + MS)
                first = torch.cat([at, (at.view(B, 1) + 1 + torch.arange(MS, device=dev).view(1, MS)).reshape(-1)])
        if xe:
            got = prep_rows(src, memory, row_prop, row_tok, te[0], te[1], 1)
        else:
            got = prep_rows(src, memory, prop, tok, te[0], te[1], S)
        if got is None:
            raise RuntimeError("self_critical: these tensors are not supported by the fused caption path")
        x0, m8 = got
        if xe:
            x0, m8 = x0.index_select(0, first), m8.index_select(0, first)
        out_full = dec(x0, None, None, m8)
        vp = getattr(ops(), "vocab_projection", None)
        logits = vp(out_full, gen.proj, 1) if vp is not None else None
        if logits is None:
            logits = gen.proj(out_full[:, 1:, :])
        if xe:
            out, adv, rowlogp = loss_op(logits, ep["lang_ids"], good, loss_words, length, reward, base, count.reshape(-1), S,
                                        sc.xe_weight, xe_positions)
            ep["_cap_loss"] = (out[0], out[3])
            ep["scst_xe_loss"], ep["scst_xe_acc"] = out[2].detach(), out[4].detach()
        else:
            out, adv, rowlogp = loss_op(logits, words, length, reward, base, count.reshape(-1), S)
            ep["_cap_loss"] = (out[0], out[1])
        if sc.mixed:
            ep["scst_reward_terms"] = terms[0].view(B, M, S, 3)
            ep["scst_baseline_terms"] = base_terms[0].view(B, M, 3) if base_terms is not None else terms[0].view(B, M, S, 3).mean(2)
        ep["match_idx"], ep["pred_ious"], ep["good_bbox_masks"] = idx, pred_ious, good
        ep["scst_proposal"], ep["scst_object_id"], ep["scst_count"], ep["scst_key"] = prop, obj, count, key
        ep["scst_samples"], ep["scst_reward"] = ys.view(B, M, S, n_words), reward.view(B, M, S)
        ep["scst_baseline"] = base.view(B, M) if base is not None else reward.view(B, M, S).mean(2)
        ep["scst_advantage"], ep["scst_logp"] = adv.view(B, M, S), rowlogp.view(B, M, S)
        ep["scst_sample_scores"] = score.view(B, M, S)
        ep["scst_stats"] = out.detach()
        return ep

    # Cross-entropy training over every matched object of a scene: None = off, else a
    # dense_xe.DenseCaptionXE.  A plain attribute, not in the state dict; read in training mode only.
    dense_xe = None

    def _dense_xe_train(self, ep, dx, prep, src, memory):
        """The captioner's part of a cross-entropy step over every matched object of a scene, after the encoder and the relation
        head: ``dx.select`` pairs up to M annotated objects per scene with their nearest proposals, ``dx.targets`` draws r of each
        object's reference sentences as teacher-forcing rows, ``caption_prep_rows`` reads the encoder rows by index (a proposal
        matched by two objects gets the sum of both gradients from one launch), and the decoder, the vocabulary projection and
        the plain caption loss run over the B M r rows in the place of the B scenes; a row without a sentence is the empty
        caption and counts for nothing.  No value is read back on the host."""
        for k in ("center_label", "box_label_mask", "scene_object_ids", "dataset_idx", "ref_center_label"):
            if k not in ep:
                raise KeyError(f"dense_xe: the batch has no {k!r}")
        prep_rows = getattr(ops(), "caption_prep_rows", None)
        loss_op = getattr(ops(), "caption_head_loss", None)
        vp = getattr(ops(), "vocab_projection", None)
        te, dec, gen = self.model.tgt_embed, self.model.decoder, self.model.generator
        B = src.shape[0]
        M, r = dx.max_proposals, dx.refs_per_object
        with torch.no_grad():
            # match_idx / pred_ious / good_bbox_masks keep their meaning: the referred object's nearest proposal
            got = prep(ep["aggregated_vote_xyz"], ep["ref_center_label"], src, memory,
                       torch.ones(B, 2, dtype=torch.int64, device=src.device), te[0], te[1])
            if got is None or prep_rows is None or loss_op is None or vp is None:
                raise RuntimeError("dense_xe: these tensors are not supported by the fused caption path")
            _, _, idx, _, good, pred_ious = got
            prop, obj, _, key, _, _ = dx.select(ep["aggregated_vote_xyz"], ep["center_label"], ep["box_label_mask"],
                                                ep["scene_object_ids"], ep["dataset_idx"])
            tok, ids, ref, row_good, length = dx.targets(key)
        got = prep_rows(src, memory, prop, tok, te[0], te[1], r)
        if got is None:
            raise RuntimeError("dense_xe: these tensors are not supported by the fused caption path")
        x0, m8 = got
        out_full = dec(x0, None, None, m8)
        logits = vp(out_full, gen.proj, 1)
        if logits is None:
            raise RuntimeError("dense_xe: this decoder output is not supported by the fused vocabulary projection")
        _, cl, ca, _ = loss_op(logits, ids, row_good)
        ep["_cap_loss"] = (cl, ca)
        ep["match_idx"], ep["pred_ious"], ep["good_bbox_masks"] = idx, pred_ious, good
        ep["dense_proposal"], ep["dense_object_id"], ep["dense_key"] = prop, obj, key
        ep["dense_ref"], ep["dense_count"], ep["dense_length"] = ref.view(B, M, r), row_good.view(B, M, r).bool(), length.view(B, M, r)
        ep["dense_lang_ids"] = ids.view(B, M, r, ids.shape[1])
        return ep

    # The relation head reads the last encoder layer only and the decoder reads the encoder's output only: the two are independent
    # until the losses are added.  `fork_relation` (set by engine.Trainer for its captured step) runs the head on a stream of its own;
    # autograd then runs its backward on that stream as well, beside the decoder's backward (the engine orders the streams where
    # gradients cross).  Values are those of the serial order: no kernel changes, only placement.  The head's persistent grids
    # leave the decoder's launches room (spacap_relation_fused_leave_cus).
    fork_relation = False

    def _relation_head_forked(self, ep):
        src = ep["aggregated_vote_features"]
        if not (self.fork_relation and src.is_cuda and torch.is_grad_enabled()):
            return self._relation_head(ep)
        dev = src.device
        from .engine import _role_stream
        rs = _role_stream(dev, "relation")
        cur = torch.cuda.current_stream(dev)
        rs.wait_stream(cur)
        sa = self.model.encoder.layers[-1].self_attn
        with torch.cuda.stream(rs):
            self._relation_head(ep)
        # The caching allocator must know that both streams touch these -- INSIDE a capture as well: a block freed on the stream it
        # was allocated on is handed to the next allocation of that stream at once (the graph's private pool included), while the
        # other stream's kernel may still be reading it (seen: NaN losses at 2 scenes per GPU, the relation head's backward reading
        # an attention map whose memory the encoder's backward had already been given).  A recorded block is held back instead.
        for t in (sa.attn, sa.value):
            if torch.is_tensor(t):
                t.record_stream(rs)
        ep["relation_pred"].record_stream(cur)
        ep["_rel_stream"] = rs    # loss_helper.get_scene_cap_loss joins the streams before it reads relation_pred

    def _relation_head(self, ep):
        """relation_pred (B,K,K,9) from the last encoder layer's attention map and values (:392-397)."""
        rp = self.relation_proposal  # Linear-ReLU-Linear-ReLU-Linear (:319-326)
        sa = self.model.encoder.layers[-1].self_attn
        pred = getattr(ops(), "relation_pred", None)
        if pred is not None:      # the form that takes the shape (spacap3d_amd/relation.py: tier)
            ep["relation_pred"] = pred(sa.attn, sa.value, rp[0], rp[2], rp[4])
        else:                     # a backend with the first layer only (the CPU oracle)
            from .relation import tall_linear
            hid = ops().relation_layer1(sa.attn, sa.value, rp[0].weight, rp[0].bias)
            ep["relation_pred"] = tall_linear(F.relu(tall_linear(hid, rp[2])), rp[4])

    # Decoding attributes (not parameters, not in the state-dict): the beam width and the exponent of the length in the final
    # ranking, read by forward_eval when its arguments are None (engine.Evaluator sets them).  beam_return_all adds every final
    # hypothesis to the outputs; beam_generic sends every width -- 1 included -- through beam_search.beam_search (parity tests).
    beam_size = 1
    length_penalty = 0.0
    beam_return_all = False
    beam_generic = False
    last_beam_trace = None
    # Sampled decoding, set the same way: num_samples = S >= 1 draws S captions per proposal from
    # softmax(logits / temperature), over the whole vocabulary (top_k = 0), the top_k <= 8 most probable words or -- top_p in
    # (0, 1), with top_k = 0 -- the row's nucleus; num_samples = 0 = off.
    # sample_generic sends it through sampling.sample (parity tests); last_sample_trace then holds its per-step gaps.
    num_samples = 0
    temperature = 1.0
    top_k = 0
    top_p = None
    sample_generic = False
    sample_seed = None          # an integer: the same draws at every call (forward_eval's sample_seed, when that is None)
    last_sample_trace = None

    # Constrained decoding, set the same way; every one is off at its default.
    min_length = 0
    no_repeat_ngram = 0
    repetition_penalty = 1.0
    bad_words = ()

    last_decode_slot = None     # forward_eval with a decode_mask: int32 (B K,), the packed row of every proposal (-1: not decoded)

    def forward_eval(self, ep, use_cache=True, beam_size=None, length_penalty=None, num_samples=None, temperature=None, top_k=None,
                     sample_seed=None, top_p=None, decode_mask=None, decode_capacity=None, min_length=None, no_repeat_ngram=None,
                     repetition_penalty=None, bad_words=None):
        """Greedy decoding of B*K captions (:402-453).  The reference re-runs the 6-layer encoder AND the whole
        decoder prefix at each of the 31 steps; the encoder output does not depend on the words (computed once),
        and with ``use_cache`` the decoder keeps the keys / values of earlier positions so that each step only
        processes the newest token (16x fewer token-layer evaluations).  ``use_cache=False`` recomputes the prefix
        as the reference does (kept for parity tests).

        ``beam_size`` > 1 (default: the module attribute, 1): beam search instead (the reference has none)
        -- ``lang_cap`` (B, K, n_words) holds the winners' words (eos repeats after the first eos), ``lang_cap_score`` (B, K)
        their summed log-probabilities, and with ``beam_return_all`` ``lang_cap_beams`` (B, K, W, n_words),
        ``lang_cap_beam_scores`` and ``lang_cap_beam_lengths`` (B, K, W) every final hypothesis.  The winner maximises
        score / length ** ``length_penalty``.

        ``num_samples`` = S >= 1 (default: the module attribute, 0 = off): sampled decoding instead (the reference has none;
        DESIGN.md section 7i) -- S captions per proposal drawn from softmax(logits / ``temperature``), over the whole vocabulary
        (``top_k`` = 0), the ``top_k`` <= 8 most probable words, or -- ``top_p`` in (0, 1), not together with ``top_k`` >= 1 --
        the row's nucleus: the words whose strictly more probable words hold less than ``top_p`` of that distribution
        (``sampling.py``).  ``lang_cap`` (B, K, n_words) is sample 0 (eos repeats after
        the first eos) and ``lang_cap_score`` (B, K) its summed log-probability under the model's own distribution;
        ``lang_cap_samples`` (B, K, S, n_words), ``lang_cap_sample_scores`` and ``lang_cap_sample_lengths`` (B, K, S) hold every
        sample.  ``sample_seed``: an integer draws the same captions at every call; None draws new ones per call and, in a
        captured graph, after every ``attention.advance_rng``.

        ``decode_mask`` (B, K) bool or uint8 (default: ``ep["decode_mask"]``; none: everything above, unchanged): decode only
        the flagged proposals.  The encoder still sees all K tokens; the flagged (scene, proposal) pairs
        are packed in flat order into a dense row list (``decode_select``), the unchanged decoders run on those rows, and every
        output above comes back in its usual shape.  A proposal that was not decoded holds the empty caption (eos, then zeros --
        once per hypothesis / sample), score 0.0 and length 1: the length ``sample_next_kernel`` and ``beam_step_kernel`` /
        ``beam_finish_kernel`` report for a caption whose first word is eos.  Two more outputs: ``lang_cap_decoded`` bool
        (B, K), True where the proposal was decoded, and ``lang_cap_rows`` int32 (2,) = the number of flags and the number of
        them decoded.  ``decode_capacity`` (default: ``ep["decode_capacity"]``):

        * an int in 1..B K -- the row list has that length whatever the mask holds: no value is read back on the host and the
          call can be captured in a graph.  Flags beyond the capacity, in flat order, are not decoded
          (``lang_cap_decoded`` is False there, ``lang_cap_rows[0]`` > ``lang_cap_rows[1]``); rows behind the last flag are
          zero indicator rows, decoded to finite values and dropped;
        * None -- the exact mode: the row list has the length of the number of flags, read back from the device.  That
          4-byte device-to-host copy is the one host synchronisation of the feature (the call cannot be captured); no flag set
          skips the decoder.

        With a mask ``use_cache=False`` raises ``ValueError``.  ``last_beam_trace`` / ``last_sample_trace`` keep the packed-row
        layout; ``last_decode_slot`` (and the traces' ``"slot"``) maps proposals to rows.  The sampler's noise is keyed by
        ROW: a fixed ``sample_seed`` repeats the draws for a fixed mask, another mask gives other draws.

        ``min_length``, ``no_repeat_ngram``, ``repetition_penalty``, ``bad_words`` (defaults: the module attributes, all off):
        constrained decoding in every mode above (``decode_constraints.py``) -- no eos before
        ``min_length`` words, no n-gram twice in a caption, the logits of used words divided (positive) or multiplied (else)
        by the penalty, and a fixed set of words that are never chosen.  Log-probabilities and scores are those of the
        constrained distribution.  With everything off the decoders run exactly the launches they run without the arguments;
        with ``use_cache=False`` an active constraint raises ``ValueError``."""
        from .decode_constraints import DecodeConstraints
        cons = DecodeConstraints(self.min_length if min_length is None else min_length,
                                 self.no_repeat_ngram if no_repeat_ngram is None else no_repeat_ngram,
                                 self.repetition_penalty if repetition_penalty is None else repetition_penalty,
                                 self.bad_words if bad_words is None else bad_words)
        cons = cons if cons.active() else None
        if cons is not None:
            if not use_cache:
                raise ValueError("forward_eval: constrained decoding keeps key / value caches (use_cache=False is the greedy parity path)")
            cons.check("forward_eval", self.model.generator.proj.out_features, MAX_DES_LEN + 1, self.word_to_idx["eos"])
        W = int(self.beam_size if beam_size is None else beam_size)
        alpha = float(self.length_penalty if length_penalty is None else length_penalty)
        if W < 1:
            raise ValueError(f"forward_eval: beam_size {W} < 1")
        beam = W > 1 or self.beam_generic
        if beam and not use_cache:
            raise ValueError("forward_eval: beam search keeps key / value caches (use_cache=False is the greedy parity path)")
        S = int(self.num_samples if num_samples is None else num_samples)
        tau = float(self.temperature if temperature is None else temperature)
        topk = int(self.top_k if top_k is None else top_k)
        sample_seed = self.sample_seed if sample_seed is None else sample_seed
        top_p = self.top_p if top_p is None else top_p
        if S < 0 or (S < 1 and num_samples is not None):      # (the attribute's 0 means off; an argument asks for samples)
            raise ValueError(f"forward_eval: num_samples {S} < 1")
        if S >= 1:
            from .sampling import check_arguments
            if W > 1:
                raise ValueError("forward_eval: sampling and beam search (beam_size > 1) exclude each other")
            check_arguments("forward_eval", S, tau, topk, self.model.generator.proj.out_features, top_p)
            if not use_cache:
                raise ValueError("forward_eval: sampling keeps key / value caches (use_cache=False is the greedy parity path)")
        decode_mask = ep.get("decode_mask") if decode_mask is None else decode_mask
        if decode_mask is not None:
            decode_capacity = ep.get("decode_capacity") if decode_capacity is None else decode_capacity
            decode_mask, decode_capacity = self._check_decode_mask(ep, decode_mask, decode_capacity, use_cache)
        obj_features = ep["aggregated_vote_features"]
        if self.token_proj is not None:
            obj_features = self.token_proj(obj_features)
        B, K, _ = obj_features.shape
        src_pos = self._src_pos(ep)
        if not self.use_transformer_encoder:
            src = torch.repeat_interleave(obj_features, K, dim=0)
            if src_pos is not None:
                src_pos = torch.repeat_interleave(src_pos, K, dim=0)
        else:
            src = obj_features
        src_mask = ep["bbox_mask"].unsqueeze(1)
        if self.model.encoder is None:
            memory = self.model.src_embed(src, src_pos) if src_pos is not None else src
        else:
            memory = self.model.encode(src, src_pos, src_mask)
        obj_flat = obj_features.reshape(B * K, -1)
        if not use_cache:
            ys = torch.full((B * K, 1), self.word_to_idx["sos"], dtype=torch.long, device=obj_features.device)
            for _ in range(MAX_DES_LEN + 1):
                L = ys.size(1) + 1 if self.early_guide else ys.size(1)
                out = self.model(src, ys, src_mask, subsequent_mask(L, device=ys.device),
                                 obj_flat.unsqueeze(1), src_pos=src_pos, memory=memory)
                next_word = self.model.generator(out[:, -1, :]).argmax(dim=-1)
                ys = torch.cat([ys, next_word.unsqueeze(1)], dim=1)
            ep["lang_cap"] = ys[:, 1:].view(B, K, -1)
            return ep
        # -- cached path -----------------------------------------------------------------------------------
        dec = self.model.decoder
        if decode_mask is not None:
            return self._decode_kept(ep, B, K, dec, obj_flat, memory.reshape(B * K, -1) if memory.shape[0] != B * K else None,
                                     decode_mask, decode_capacity, W, alpha, beam, S, tau, topk, sample_seed, top_p, cons)
        if memory.shape[0] != B * K:  # encoder ran once per scene: the indicator adds that proposal's memory row
            indicator = obj_flat.unsqueeze(1) + memory.reshape(B * K, -1).unsqueeze(1)
        else:
            indicator = obj_flat.unsqueeze(1)
        return self._decode_rows(ep, B, K, dec, indicator, W, alpha, beam, S, tau, topk, sample_seed, top_p, cons)

    def _decode_rows(self, ep, B, K, dec, indicator, W, alpha, beam, S, tau, topk, sample_seed, top_p, cons=None):
        """The cached decoding of ``forward_eval`` over the B K rows of ``indicator`` (B K, 1, d): sampled, beam or greedy, fused
        or through the cached per-operator decoder; the outputs go to ``ep`` as (B, K, ...).  ``cons``: an active
        ``DecodeConstraints`` or None."""
        caches = [dict() for _ in dec.layers]
        ys = torch.full((B * K, 1), self.word_to_idx["sos"], dtype=torch.long, device=indicator.device)
        embed, pos = self.model.tgt_embed[0], self.model.tgt_embed[1]
        cd = getattr(ops(), "caption_decode", None)
        fused = self.early_guide and not self.training and cd is not None \
            and cd.decode_supported(dec.layers, indicator.squeeze(1), MAX_DES_LEN + 1)
        if S >= 1:
            sos, eos = self.word_to_idx["sos"], self.word_to_idx["eos"]
            if fused and not self.sample_generic:
                # the greedy loop below at B K S rows with a drawn word in place of the arg-max (caption_decode.sample_decode)
                got = cd.sample_decode(dec, self.model.generator, embed, pos.pe, indicator.squeeze(1), sos, eos, MAX_DES_LEN + 1,
                                       S, tau, topk, sample_seed, top_p, constraints=cons)
                if got is not None:       # (None: a nucleus over more words than the fused entry takes)
                    self.last_sample_trace = None
                    return self._sample_outputs(ep, B, K, *got)
            return self._sample_generic(ep, B, K, S, tau, topk, sample_seed, dec, indicator, top_p, cons)
        if beam and fused and not self.beam_generic:
            # the greedy loop below at B K W rows: top-W log-probabilities, one selection per sequence, attention through an
            # ancestor table (caption_decode.beam_decode, csrc/caption_decode.hip)
            self.last_beam_trace = {}       # parent int8 / word int32 (n_words, R, W): the selections, for parity tests
            got = cd.beam_decode(dec, self.model.generator, embed, pos.pe, indicator.squeeze(1), self.word_to_idx["sos"],
                                 self.word_to_idx["eos"], MAX_DES_LEN + 1, W, alpha, return_all=self.beam_return_all,
                                 trace=self.last_beam_trace, constraints=cons)
            return self._beam_outputs(ep, B, K, *got)
        if beam:
            return self._beam_generic(ep, B, K, W, alpha, dec, indicator, cons)
        if fused:
            # pre-allocated key / value caches, one token per sequence and step, four launches per layer (caption_decode.greedy_decode)
            more = {} if cons is None else dict(eos=self.word_to_idx["eos"], constraints=cons)    # (off: today's call, as it stands)
            words = cd.greedy_decode(dec, self.model.generator, embed, pos.pe, indicator.squeeze(1), self.word_to_idx["sos"],
                                     MAX_DES_LEN + 1, **more)
            ep["lang_cap"] = words.view(B, K, -1)
            return ep
        words = ys[:, 0]
        for step in range(MAX_DES_LEN + 1):
            out = self._cached_step(dec, caches, indicator, step, words)
            if cons is None:
                words = self.model.generator(out).argmax(dim=-1)
            else:       # the arg-max of the constrained logits over the row's own words so far (ys without sos)
                from .decode_constraints import apply
                words = apply(cons, self.model.generator.proj(out), ys[:, 1:], step, self.word_to_idx["eos"]).argmax(dim=-1)
            ys = torch.cat([ys, words.unsqueeze(1)], dim=1)
        ep["lang_cap"] = ys[:, 1:].view(B, K, -1)
        return ep

    @staticmethod
    def _check_decode_mask(ep, mask, capacity, use_cache):
        """The arguments of decoding under a mask (``forward_eval``), checked before anything runs."""
        B, K = ep["aggregated_vote_features"].shape[:2]
        if not use_cache:
            raise ValueError("forward_eval: decode_mask packs the rows of the cached decoders (use_cache=False is the greedy parity path)")
        if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (B, K):
            raise ValueError(f"forward_eval: decode_mask must be a (B, K) = ({B}, {K}) tensor, got "
                             f"{tuple(mask.shape) if isinstance(mask, torch.Tensor) else type(mask).__name__}")
        if mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"forward_eval: decode_mask must be bool or uint8, got {mask.dtype}")
        if capacity is not None:
            if isinstance(capacity, bool) or not isinstance(capacity, int) or not 1 <= capacity <= B * K:
                raise ValueError(f"forward_eval: decode_capacity {capacity!r} must be None or an int in 1..B K = {B * K}")
        if not mask.is_cuda:
            raise RuntimeError("forward_eval: decode_mask: CPU not supported")
        return mask, capacity

    def _decode_kept(self, ep, B, K, dec, obj_flat, memory_flat, mask, capacity, W, alpha, beam, S, tau, topk, sample_seed, top_p,
                     cons=None):
        """``forward_eval`` under a ``decode_mask``: pack the flagged proposals (``decode_select.select``),
        form the indicator of the packed rows only (``gather``: obj + memory without the B K-row sum), run ``_decode_rows`` on
        them as one scene of that many proposals, and scatter what it returned back to (B, K, ...)."""
        from . import decode_select as ds
        n, eos, L = B * K, self.word_to_idx["eos"], MAX_DES_LEN + 1
        dev = obj_flat.device
        rows, slot, count = ds.select(mask, n if capacity is None else capacity)
        if capacity is None:
            kept = int(count[:1].cpu()[0])    # the exact mode's host read: 4 bytes, the feature's one synchronisation
            rows = rows[:kept]
        else:
            kept = capacity
        got = {}
        if kept > 0:
            self._decode_rows(got, 1, kept, dec, ds.gather(obj_flat, memory_flat, rows).unsqueeze(1), W, alpha, beam, S, tau, topk,
                              sample_seed, top_p, cons)
        else:   # nothing to decode: one row of the right shapes that no slot points at
            z = lambda *shape, dtype=torch.float32: torch.zeros(1, 1, *shape, dtype=dtype, device=dev)  # noqa: E731
            got["lang_cap"] = z(L, dtype=torch.long)
            if S >= 1:
                got["lang_cap_score"], got["lang_cap_samples"] = z(), z(S, L, dtype=torch.long)
                got["lang_cap_sample_scores"], got["lang_cap_sample_lengths"] = z(S), z(S, dtype=torch.int32)
            elif beam:
                got["lang_cap_score"] = z()
                if self.beam_return_all:
                    got["lang_cap_beams"] = z(W, L, dtype=torch.long)
                    got["lang_cap_beam_scores"], got["lang_cap_beam_lengths"] = z(W), z(W, dtype=torch.int32)
        for k, t in got.items():
            t = t[0]                          # (kept, ...)
            if t.dtype == torch.int64:
                out = ds.scatter_words(t, slot, eos)
            else:                             # scores: 0.0; lengths: the empty caption's, 1
                out = ds.scatter_values(t, slot, 0.0 if t.dtype == torch.float32 else 1)
            ep[k] = out.view(B, K, *t.shape[1:])
        ep["lang_cap_decoded"] = (slot >= 0).view(B, K)
        ep["lang_cap_rows"] = count
        self.last_decode_slot = slot
        trace = self.last_sample_trace if S >= 1 else self.last_beam_trace if beam else None
        if isinstance(trace, dict) and kept > 0:
            trace["slot"] = slot
        return ep

    def _cached_step(self, dec, caches, ind, i, words, parents=None):
        """The decoder's output row (rows, d_model) for the words (rows,) of step ``i`` through the cached per-operator decoder
        (``decode_incremental``); ``parents`` (rows,) first reorders the key / value caches of the earlier steps (beam search).
        Early guide: positions 0 = object indicator ``ind`` (rows, 1, d), 1.. = words (sinusoid added to the words only, as
        tgt_embed does), so step 0 feeds two positions under a causal mask; late guide: cross-attention over the 1-token
        indicator (:266)."""
        embed, pos = self.model.tgt_embed[0], self.model.tgt_embed[1]
        if parents is not None and i > 0:
            for c in caches:
                c["k"], c["v"] = c["k"].index_select(0, parents), c["v"].index_select(0, parents)
        x_new = pos.dropout(embed(words.unsqueeze(1)) + pos.pe[:, i:i + 1])
        mask = None
        if i == 0 and self.early_guide:
            x_new = torch.cat((ind, x_new), dim=1)
            mask = subsequent_mask(2, device=words.device).expand(ind.shape[0], -1, -1)
        out = decode_incremental(dec, x_new, caches, memory=None if self.early_guide else ind, src_mask=None, mask=mask)
        return out[:, -1, :]

    def _beam_outputs(self, ep, B, K, ys, score, beams=None, scores=None, lengths=None):
        ep["lang_cap"] = ys.view(B, K, -1)
        ep["lang_cap_score"] = score.view(B, K)
        if beams is not None:
            ep["lang_cap_beams"] = beams.view(B, K, beams.shape[1], -1)
            ep["lang_cap_beam_scores"] = scores.view(B, K, -1)
            ep["lang_cap_beam_lengths"] = lengths.view(B, K, -1)
        return ep

    def _sample_outputs(self, ep, B, K, ys, score, length):
        ep["lang_cap"] = ys[:, 0].reshape(B, K, -1)
        ep["lang_cap_score"] = score[:, 0].reshape(B, K)
        ep["lang_cap_samples"] = ys.view(B, K, ys.shape[1], -1)
        ep["lang_cap_sample_scores"] = score.view(B, K, -1)
        ep["lang_cap_sample_lengths"] = length.view(B, K, -1)
        return ep

    def _sample_generic(self, ep, B, K, S, tau, topk, seed, dec, indicator, top_p=None, cons=None):
        """Sampled decoding through the cached per-operator decoder (``decode_incremental``): everything the fused path does not
        take -- late guide, other head counts, the CPU oracle backend.  Row r S + s is sample s of sequence r."""
        from .sampling import sample
        R = B * K
        ind = indicator.repeat_interleave(S, 0)
        caches = [dict() for _ in dec.layers]
        seed_dev = None
        if seed is None:   # as the fused path: a host word per call and the device's step counter
            from .attention import _next_seed, rng_state
            seed = _next_seed()
            seed_dev = rng_state(ind.device) if ind.is_cuda else None

        def step_fn(i, words):
            return self.model.generator.proj(self._cached_step(dec, caches, ind, i, words))

        got = sample(step_fn, R, S, MAX_DES_LEN + 1, self.word_to_idx["sos"], self.word_to_idx["eos"], tau, topk, seed, seed_dev,
                     device=indicator.device, top_p=top_p, constraints=cons)
        self.last_sample_trace = {"gap": got["gap"]}     # (n_words, R S): for parity tests
        return self._sample_outputs(ep, B, K, got["ys"], got["score"], got["length"])

    def _beam_generic(self, ep, B, K, W, alpha, dec, indicator, cons=None):
        """Beam search through the cached per-operator decoder (``decode_incremental``): everything the fused path does not
        take -- late guide, other head counts, the CPU oracle backend.  Row r W + w is hypothesis w of sequence r; a selection
        reorders the key / value caches with ``index_select``."""
        from .beam_search import beam_search
        R = B * K
        ind = indicator.repeat_interleave(W, 0)
        caches = [dict() for _ in dec.layers]

        gen = self.model.generator if cons is None else self.model.generator.proj    # (constraints are a rule on the logits)

        def step_fn(s, words, parents):
            return gen(self._cached_step(dec, caches, ind, s, words, parents))

        got = beam_search(step_fn, R, W, MAX_DES_LEN + 1, self.word_to_idx["sos"], self.word_to_idx["eos"], alpha,
                          device=indicator.device, constraints=cons)
        self.last_beam_trace = {k: got[k] for k in ("parent", "word", "gap")}   # (n_words, R, W) twice, (n_words, R): for parity tests
        if self.beam_return_all:
            return self._beam_outputs(ep, B, K, got["ys"], got["score"], got["beams"], got["scores"], got["lengths"].to(torch.int32))
        return self._beam_outputs(ep, B, K, got["ys"], got["score"])
