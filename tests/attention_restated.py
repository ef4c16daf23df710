"""Scaled-dot-product attention of csrc/mha.hip restated in float64 on the host, the dispatch of its host code restated as
``tier()``, and the case tables that walk every instantiation the dispatch can pick.  Not a test module;
tests/test_attention_restated_cpu.py checks the restatement and the tables, tests/test_attention_tiers_gpu.py runs the tables
through the kernels.  Imports nothing from the package under test.

    logits = Q K^T / sqrt(d_k) (+ bias);  logits.masked_fill(mask == 0, -1e9);  P = softmax(logits) (* keep / (1 - p));  O = P V

The restatement draws no random numbers: a dropout case hands in the keep mask (already divided by 1 - p)."""
import collections
import math

import torch

B, H = 2, 3                      # every case: an odd head count, so that a head-stride slip lands on another head's data
D_KS = (16, 32, 64)
KEY_EDGES = (32, 64, 128, 256, 512)   # launch_fwd / launch_bwd / launch_bwd_both: last key count of tiers 1..5
QUERY_EDGE = 64                       # launch_bwd: Lq <= 64 one wave per 16 keys, above it four
MASKS = ("none", "key", "query")

# the bars of tests/test_attention_gpu.py, here against float64
P_RTOL, P_ATOL = 1e-4, 1e-6
O_RTOL, O_ATOL = 1e-4, 1e-5
GRAD_BAR = 2e-4


# ---- the float64 statement ----------------------------------------------------------------------------------------------
def attention64(q, k, v, mask=None, bias=None, keep_scale=None):
    """(O, P) in float64 on the host.  q (B,h,Lq,d_k), k / v (B,h,Lk,d_k); mask broadcastable to (B,1,Lq,Lk), 0 = masked;
    bias broadcastable to (B,h,Lq,Lk); keep_scale (B,h,Lq,Lk) = keep / (1 - p) or None."""
    q, k, v = (t.double() for t in (q, k, v))
    logits = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(q.size(-1))
    if bias is not None:
        logits = logits + bias.double()
    if mask is not None:
        logits = logits.masked_fill(mask == 0, -1e9)
    p = torch.softmax(logits, dim=-1)
    if keep_scale is not None:
        p = p * keep_scale.double()
    return torch.matmul(p, v), p


Ref = collections.namedtuple("Ref", "o p dq dk dv")


def reference(q, k, v, w_o, w_p, mask=None, bias=None, keep_scale=None):
    """O, P and the gradients of  sum O w_o + sum P w_p  with respect to q, k, v, by float64 autograd (w_p may be None)."""
    q, k, v = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    o, p = attention64(q, k, v, mask, bias, keep_scale)
    loss = (o * w_o.double()).sum()
    if w_p is not None:
        loss = loss + (p * w_p.double()).sum()
    loss.backward()
    return Ref(o.detach(), p.detach(), q.grad, k.grad, v.grad)


def excess(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): at most 1 inside the bar of assert_allclose(rtol, atol)."""
    got, want = got.double(), want.double()
    if got.numel() == 0:
        return 0.0
    return float(((got - want).abs() / (atol + rtol * want.abs())).max())


def grad_error(got, want):
    """max |got - want| / max |want|; a gradient that is identically zero (one key: P = 1 whatever q and k are) must be
    reproduced exactly."""
    err, ref = float((got.double() - want.double()).abs().max()), float(want.double().abs().max())
    if ref == 0.0:
        return 0.0 if err == 0.0 else math.inf
    return err / ref


# ---- the dispatch ---------------------------------------------------------------------------------------------------------
Tier = collections.namedtuple("Tier", "tier fwd dq dkv both")


def tier(Lq, Lk, d_k):
    """Which forward, dQ, dK/dV and single-launch instantiation the host code picks for (Lq, Lk, d_k): kernel name and template
    arguments.  ``both`` is None where spacap_mha_bwd_delta_f32 refuses the pair."""
    if d_k not in D_KS or not 1 <= Lk <= KEY_EDGES[-1] or Lq < 1:
        raise ValueError(f"unsupported (Lq={Lq}, Lk={Lk}, d_k={d_k})")
    t = 1 + sum(Lk > e for e in KEY_EDGES[:-1])
    split = Lk > KEY_EDGES[1]                     # four waves share 16 queries and split the keys
    tiles = {1: 2, 2: 4, 3: 2, 4: 4, 5: 8}[t]     # 16-key tiles per wave
    four = Lq > QUERY_EDGE                        # four waves share 16 keys and split the queries
    w = 4 if split else 1                         # template argument W: waves per 16-row tile
    both = ("mha_bwd_both_kernel", tiles, d_k, w) if split == four else None
    return Tier(t, ("mha_fwd_kernel", tiles, d_k, w), ("mha_bwd_dq_kernel", tiles, d_k, w),
                ("mha_bwd_dkv_kernel", d_k, 4 if four else 1), both)


# ---- the case tables ------------------------------------------------------------------------------------------------------
# per tier the smallest shapes that reach each branch: both dK/dV families, a key count that is a multiple of 4 and one that is
# not (both P stores, both mask4 loads), Lq in {65, 66, 67, 130} (row statistics by scalar loads), ragged last tiles
TIER_SHAPES = {
    1: ((17, 1), (64, 32), (65, 31)),
    2: ((15, 33), (64, 64), (67, 64)),
    3: ((16, 65), (65, 128), (130, 127)),
    4: ((33, 129), (65, 256), (132, 255)),
    5: ((1, 257), (66, 512), (80, 509)),
}
Case = collections.namedtuple("Case", "tier Lq Lk d_k mask")
TIER_CASES = [Case(t, Lq, Lk, d, m) for t, shapes in TIER_SHAPES.items() for (Lq, Lk) in shapes for d in D_KS for m in MASKS]


def _pick(t, four):
    """the first shape of tier t in the asked dK/dV family"""
    return next(s for s in TIER_SHAPES[t] if (s[0] > QUERY_EDGE) == four)


# a per-query mask whose base is 1 byte past an allocation (mask4 by byte loads although Lk % 4 == 0): split tiers
OFFSET_MASK_CASES = [Case(3, 65, 128, 32, "query"), Case(4, 65, 256, 16, "query"), Case(5, 66, 512, 64, "query")]

# bias, backward included: every (tier, family) at d_k = 16, tiers 3 and 5 at d_k = 64; each with a full and an expanded bias
BIAS_KINDS = ("full", "expanded")
BIAS_CASES = [Case(t, *_pick(t, four), 16, "key") for t in TIER_SHAPES for four in (False, True)] + \
             [Case(t, *_pick(t, four), 64, "key") for t in (3, 5) for four in (False, True)]

# dropout: one case per (tier, d_k), the dK/dV family and the mask kind alternating
DROPOUT_P = 0.25
DROPOUT_CASES = [Case(t, *_pick(t, (t + i) % 2 == 1), d, MASKS[(t + i) % 3]) for t in TIER_SHAPES for i, d in enumerate(D_KS)]

# q / k / v bases 4 bytes past a 16-byte boundary (operands by scalar loads): the split tiers, both families
SCALAR_CASES = [Case(t, *_pick(t, four), d, "key") for t in (3, 4, 5) for d in D_KS for four in (False, True)]

# self_attention_packed: (L, d_k)
PACKED_CASES = [(L, d) for L in (33, 65, 130, 260) for d in (32, 64)]

# spacap_mha_bwd_delta_f32 through the C ABI: (Lq, Lk) -- every (tier, d_k) of the single-launch form with Lq == Lk and with
# Lq != Lk
SINGLE_SHAPES = ((20, 50), (64, 33), (100, 300), (65, 512), (96, 96),
                 (17, 17), (40, 31), (64, 64), (67, 128), (130, 130), (65, 255), (260, 260))
SINGLE_CASES = [(Lq, Lk, d) for (Lq, Lk) in SINGLE_SHAPES for d in D_KS]
SINGLE_BIAS_CASES = [(64, 33, 16), (100, 300, 64)]
SINGLE_REFUSED = ((40, 130), (130, 40))


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def make_mask(kind, Lq, Lk, seed):
    """key:   (B,1,1,Lk) int64, the last scene fully masked (uniform rows), key 0 kept in the others.
    query: (B,1,Lq,Lk) bool, random; query row 0 fully masked; in scene 0 the last key is masked for every query."""
    g = torch.Generator().manual_seed(1000 + seed)
    if kind == "none":
        return None
    if kind == "key":
        m = (torch.rand(B, 1, 1, Lk, generator=g) > 0.3).long()
        m[..., 0] = 1
        m[B - 1] = 0
        return m
    assert kind == "query"
    m = torch.rand(B, 1, Lq, Lk, generator=g) > 0.3
    m[:, :, 0] = False
    if Lk > 1:
        m[0, :, :, Lk - 1] = False
    return m


Inputs = collections.namedtuple("Inputs", "q k v w_o w_p mask")


def make_inputs(Lq, Lk, d_k, mask_kind, seed=0):
    """randn q, k, v as the (B,h,L,d_k) transposed views of dense (B,L,h,d_k) projections, the weights of the two outputs
    in the test loss, and the mask; all float32 on the host, fixed by (shape, seed)."""
    g = torch.Generator().manual_seed(((Lq * 521 + Lk) * 67 + d_k) * 7 + seed)
    q = torch.randn(B, Lq, H, d_k, generator=g).transpose(1, 2)
    k = torch.randn(B, Lk, H, d_k, generator=g).transpose(1, 2)
    v = torch.randn(B, Lk, H, d_k, generator=g).transpose(1, 2)
    w_o = torch.randn(B, H, Lq, d_k, generator=g)
    w_p = torch.randn(B, H, Lq, Lk, generator=g)
    return Inputs(q, k, v, w_o, w_p, make_mask(mask_kind, Lq, Lk, seed + Lq + Lk))


def make_bias(kind, Lq, Lk, seed=0):
    g = torch.Generator().manual_seed(77 + seed + Lq * 3 + Lk)
    if kind == "full":
        return torch.randn(B, H, Lq, Lk, generator=g)
    assert kind == "expanded"
    return torch.randn(1, 1, Lq, Lk, generator=g).expand(B, H, Lq, Lk)    # strides (0, 0, Lk, 1)


def unmasked(mask, Lq, Lk):
    """bool (B,1,Lq,Lk): the entries that are not masked"""
    if mask is None:
        return torch.ones(B, 1, Lq, Lk, dtype=torch.bool)
    return (mask != 0).expand(B, 1, Lq, Lk)
