"""Every instantiation the host code of csrc/mha.hip can pick (five key-count tiers x d_k in {16, 32, 64} x both dK/dV kernels,
the single-launch backward, the scalar operand path, both mask4 loads, both row-statistics loads) against the float64
statement of tests/attention_restated.py, at the smallest shapes that reach each branch (B = 2, h = 3).

Bars, against float64: P rtol 1e-4 / atol 1e-6, O rtol 1e-4 / atol 1e-5, each gradient max |error| / max |reference| < 2e-4
(tests/test_attention_gpu.py's own; the fp32 restatement uses under a tenth of them, tests/test_attention_restated_cpu.py).
Each comparison prints its figures before it asserts (pytest -s): P and O as the largest |error| / (atol + rtol |reference|), at
most 1 inside the bar, the gradients as max |error| / max |reference|."""
import math

import pytest
import torch

import attention_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H = R.B, R.H
_ids = lambda c: "-".join(map(str, c))


@pytest.fixture(scope="module")
def att():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spacap3d_amd import attention
    return attention


def _dev(t):
    return t.to(DEV) if t is not None else None


Got = R.Ref


def _run(att, q, k, v, w_o, w_p, mask, bias=None, need_p=True, dropout_p=0.0):
    """forward + backward of sum O w_o (+ sum P w_p) through attention(); q, k, v are used as given when they already live on
    the device (views with a chosen alignment), else moved there with their strides."""
    qg, kg, vg = (t if t.is_cuda else t.to(DEV).requires_grad_(True) for t in (q, k, v))
    for t in (qg, kg, vg):
        t.grad = None
    o, p = att.attention(qg, kg, vg, mask=mask, dropout_p=dropout_p, training=dropout_p > 0.0, need_p=need_p, bias=bias)
    loss = (o * _dev(w_o)).sum()
    if w_p is not None:
        loss = loss + (p * _dev(w_p)).sum()
    loss.backward()
    return Got(o.detach(), p.detach() if p is not None else None, qg.grad.clone(), kg.grad.clone(), vg.grad.clone())


def _hold(kind, c, got, want):
    """print the five figures, then hold them to the bars"""
    fig = {"P": R.excess(got.p.cpu(), want.p, R.P_RTOL, R.P_ATOL), "O": R.excess(got.o.cpu(), want.o, R.O_RTOL, R.O_ATOL)}
    for n in ("dq", "dk", "dv"):
        fig[n] = R.grad_error(getattr(got, n).cpu(), getattr(want, n))
    print(f"ATTN-TIERS {kind} tier={c.tier} d_k={c.d_k} Lq={c.Lq} Lk={c.Lk} mask={c.mask} "
          + " ".join(f"{n}={e:.3e}" for n, e in fig.items()))
    assert fig["P"] <= 1.0, fig
    assert fig["O"] <= 1.0, fig
    for n in ("dq", "dk", "dv"):
        assert fig[n] < R.GRAD_BAR, fig


def _same(a, b):
    for n, x, y in zip(Got._fields, a, b):
        if x is None or y is None:
            assert x is None and y is None, n
        else:
            assert x.shape == y.shape and torch.equal(x, y), n


def _exact_mask_properties(c, mask, got):
    if mask is None:
        return
    un = R.unmasked(mask, c.Lq, c.Lk)                              # (B,1,Lq,Lk)
    row_has = un.any(-1, keepdim=True)
    p, dk, dv = got.p.cpu(), got.dk.cpu(), got.dv.cpu()
    zero_p = (~un & row_has).expand(B, H, c.Lq, c.Lk)
    assert bool((p[zero_p] == 0).all())                            # exp(-1e9 - max) is 0, not small
    dead = ~un.any(2)                                              # (B,1,Lk): masked for every query of the scene
    dead_rows = dead.view(B, 1, c.Lk, 1).expand(B, H, c.Lk, c.d_k)
    assert bool((dk[dead_rows] == 0).all())
    whole_scene = row_has.all(2).view(B, 1, 1, 1)                  # no uniform row in the scene: P is 0 down the dead columns
    assert bool((dv[dead_rows & whole_scene] == 0).all())
    assert bool((dead_rows & whole_scene).any()) or c.mask == "query" or c.Lk == 1


# ---- every tier, both dK/dV kernels, three mask kinds ------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.TIER_CASES, ids=_ids)
def test_tier_against_float64(att, c):
    x = R.make_inputs(c.Lq, c.Lk, c.d_k, c.mask)
    want = R.reference(x.q, x.k, x.v, x.w_o, x.w_p, x.mask)
    got = _run(att, x.q, x.k, x.v, x.w_o, x.w_p, _dev(x.mask))
    _hold("tier", c, got, want)
    _exact_mask_properties(c, x.mask, got)
    _same(got, _run(att, x.q, x.k, x.v, x.w_o, x.w_p, _dev(x.mask)))   # no atomics: bit for bit


@pytest.mark.parametrize("c", R.OFFSET_MASK_CASES, ids=_ids)
def test_mask_one_byte_past_an_allocation(att, c):
    """A contiguous uint8 (B,Lq,Lk) mask passes through _prep_mask untouched; based 1 byte past an allocation, no row of it is
    4-byte aligned although Lk % 4 == 0, so mask4 reads bytes: same values as the aligned mask, bit for bit."""
    x = R.make_inputs(c.Lq, c.Lk, c.d_k, c.mask)
    m8 = (x.mask[:, 0] != 0).to(torch.uint8)
    buf = torch.zeros(m8.numel() + 1, dtype=torch.uint8, device=DEV)
    off = buf[1:].view(B, c.Lq, c.Lk)
    off.copy_(m8)
    assert off.is_contiguous() and off.data_ptr() % 4 == 1
    assert att._prep_mask_uncached(off, B, c.Lq, c.Lk)[0].data_ptr() == off.data_ptr()
    want = R.reference(x.q, x.k, x.v, x.w_o, x.w_p, x.mask)
    got = _run(att, x.q, x.k, x.v, x.w_o, x.w_p, off)
    _hold("offset-mask", c, got, want)
    _same(got, _run(att, x.q, x.k, x.v, x.w_o, x.w_p, _dev(x.mask)))


# ---- bias ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.BIAS_KINDS)
@pytest.mark.parametrize("c", R.BIAS_CASES, ids=_ids)
def test_bias_forward_and_backward(att, c, kind):
    x = R.make_inputs(c.Lq, c.Lk, c.d_k, c.mask)
    bias = R.make_bias(kind, c.Lq, c.Lk)
    bd = bias.to(DEV) if kind == "full" else bias[:1, :1].to(DEV).expand(B, H, c.Lq, c.Lk)
    assert bd.stride()[:2] == ((H * c.Lq * c.Lk, c.Lq * c.Lk) if kind == "full" else (0, 0))
    want = R.reference(x.q, x.k, x.v, x.w_o, x.w_p, x.mask, bias)
    got = _run(att, x.q, x.k, x.v, x.w_o, x.w_p, _dev(x.mask), bias=bd)
    _hold("bias-" + kind, c, got, want)


def test_bias_that_asks_for_a_gradient_is_refused(att):
    x = R.make_inputs(17, 33, 16, "none")
    bias = R.make_bias("full", 17, 33).to(DEV).requires_grad_(True)
    with pytest.raises(RuntimeError, match="bias"):
        att.attention(_dev(x.q), _dev(x.k), _dev(x.v), bias=bias)
    o, _ = att.attention(_dev(x.q), _dev(x.k), _dev(x.v), bias=bias.detach())
    assert o.shape == (B, H, 17, 16)


# ---- dropout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.DROPOUT_CASES, ids=_ids)
def test_dropout_mask_is_the_same_in_forward_and_backward(att, c):
    """The keep mask is read off the forward's P and handed to the float64 statement: a backward kernel that rebuilds another
    flat index regenerates another mask and misses the gradients by O(1)."""
    p = R.DROPOUT_P
    x = R.make_inputs(c.Lq, c.Lk, c.d_k, c.mask)
    md = _dev(x.mask)
    att._next_seed()
    saved, word = att._CALL_COUNTER[0], att.rng_state(DEV).clone()
    c0 = (20261019 + c.tier * 8 + c.d_k) << 20
    try:
        att.rng_state(DEV).zero_()
        att._CALL_COUNTER[0] = c0
        got = _run(att, x.q, x.k, x.v, x.w_o, x.w_p, md, dropout_p=p)
        att._CALL_COUNTER[0] = c0
        with_p = _run(att, x.q, x.k, x.v, x.w_o, None, md, dropout_p=p)
        att._CALL_COUNTER[0] = c0
        without_p = _run(att, x.q, x.k, x.v, x.w_o, None, md, dropout_p=p, need_p=False)
    finally:
        att._CALL_COUNTER[0] = saved
        att.rng_state(DEV).copy_(word)
    keep = got.p.cpu() != 0
    want = R.reference(x.q, x.k, x.v, x.w_o, x.w_p, x.mask, keep_scale=keep.double() / (1.0 - p))
    _hold("dropout", c, got, want)
    un = R.unmasked(x.mask, c.Lq, c.Lk).expand(B, H, c.Lq, c.Lk)
    n = int(un.sum())
    assert n > 0
    rate = float(keep[un].double().mean())
    print(f"ATTN-TIERS keep-rate tier={c.tier} d_k={c.d_k} n={n} rate={rate:.4f}")
    assert abs(rate - (1.0 - p)) <= 5.0 * math.sqrt(p * (1.0 - p) / n), (rate, n)
    assert torch.equal(with_p.p, got.p) and without_p.p is None
    _same(with_p._replace(p=None), without_p)


# ---- operands by scalar loads --------------------------------------------------------------------------------------------------
def _four_bytes_off(t):
    """the same values in a (B,h,L,d_k) view of a dense (B,L,h,d_k) buffer whose base is 4 bytes past a 16-byte boundary"""
    Bn, h, L, d = t.shape
    flat = torch.zeros(t.numel() + 1, device=DEV)
    view = flat[1:].view(Bn, L, h, d).transpose(1, 2)
    view.copy_(t.detach())
    assert view.data_ptr() % 16 == 4 and view.stride() == (L * h * d, d, h * d, 1)
    return view.requires_grad_(True)


@pytest.mark.parametrize("c", R.SCALAR_CASES, ids=_ids)
def test_unaligned_operands_give_the_same_bits(att, c):
    """q, k, v based 4 bytes past a 16-byte boundary: fill_args clears A.vec and the split kernels load their operands float by
    float -- the same values into the same registers, so everything is bitwise equal to the aligned run."""
    x = R.make_inputs(c.Lq, c.Lk, c.d_k, c.mask)
    md = _dev(x.mask)
    aligned = _run(att, x.q, x.k, x.v, x.w_o, x.w_p, md)
    off = _run(att, _four_bytes_off(x.q), _four_bytes_off(x.k), _four_bytes_off(x.v), x.w_o, x.w_p, md)
    _same(aligned, off)
    _hold("scalar", c, off, R.reference(x.q, x.k, x.v, x.w_o, x.w_p, x.mask))


# ---- packed projection ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,d_k", R.PACKED_CASES)
def test_packed_projection_equals_attention_on_its_slices(att, L, d_k):
    hd = H * d_k
    x = R.make_inputs(L, L, d_k, "key")
    qkv = torch.cat([t.transpose(1, 2).reshape(B, L, hd) for t in (x.q, x.k, x.v)], -1).to(DEV)
    md = _dev(x.mask)
    w_o, w_p = x.w_o.to(DEV), x.w_p.to(DEV)
    a = qkv.clone().requires_grad_(True)
    out, p = att.self_attention_packed(a, H, mask=md, need_p=True)
    ((out * w_o.transpose(1, 2).reshape(B, L, hd)).sum() + (p * w_p).sum()).backward()
    b = qkv.clone().requires_grad_(True)
    q, k, v = (b[..., i * hd:(i + 1) * hd].view(B, L, H, d_k).transpose(1, 2) for i in range(3))
    o2, p2 = att.attention(q, k, v, mask=md, need_p=True)
    ((o2 * w_o).sum() + (p2 * w_p).sum()).backward()
    assert torch.equal(out.detach(), o2.detach().transpose(1, 2).reshape(B, L, hd)) and torch.equal(p.detach(), p2.detach())
    assert torch.equal(a.grad, b.grad)
    c = R.Case(R.tier(L, L, d_k).tier, L, L, d_k, "key")
    grads = [a.grad[..., i * hd:(i + 1) * hd].view(B, L, H, d_k).transpose(1, 2) for i in range(3)]
    _hold("packed", c, Got(out.detach().view(B, L, H, d_k).transpose(1, 2), p.detach(), *grads),
          R.reference(x.q, x.k, x.v, x.w_o, x.w_p, x.mask))


# ---- the C ABI: single-launch backward, d_out alignment, zero-length queries ------------------------------------------------------
class _Capi:
    """q (B,Lq,h*d_k), k / v (B,Lk,h*d_k) dense, a key mask, optionally a bias; forward run, gradient buffers at hand"""

    def __init__(self, Lq, Lk, d_k, with_bias=False):
        from spacap3d_amd._native import check, lib
        self.check, self.lib = check, lib
        self.Lq, self.Lk, self.d_k, hd = Lq, Lk, d_k, H * d_k
        g = torch.Generator().manual_seed(Lq * 1000 + Lk + d_k)
        self.q = torch.randn(B, max(Lq, 1), hd, generator=g).to(DEV)
        self.k, self.v = torch.randn(B, Lk, hd, generator=g).to(DEV), torch.randn(B, Lk, hd, generator=g).to(DEV)
        self.dout = torch.randn(B * max(Lq, 1) * hd + 4, generator=g).to(DEV)      # (room for a view 4 bytes on)
        self.mask = (R.make_mask("key", Lq, Lk, Lq + Lk)[:, 0] != 0).to(torch.uint8).to(DEV).contiguous()   # (B,1,Lk)
        self.bias = torch.randn(B, H, Lq, Lk, generator=g).to(DEV) if with_bias else None
        bs = (H * Lq * Lk, Lq * Lk, Lk) if with_bias else (0, 0, 0)
        self.st = torch.cuda.current_stream().cuda_stream
        self.args = (self.q.data_ptr(), self.k.data_ptr(), self.v.data_ptr(), Lq * hd, d_k, hd, Lk * hd, d_k, hd, Lk * hd, d_k, hd,
                     self.mask.data_ptr(), Lk, 0, self.bias.data_ptr() if with_bias else None, *bs, B, H, Lq, Lk, d_k,
                     1.0 / math.sqrt(d_k), 0.0, 0, None)
        self.out = torch.empty(B, max(Lq, 1), hd, device=DEV)
        self.lse = torch.empty(B, H, max(Lq, 1), 2, device=DEV)
        self.ws = torch.empty(B * H * max(Lq, 1), device=DEV)
        if Lq:
            check(lib.spacap_mha_fwd_f32(*self.args, self.out.data_ptr(), None, self.lse.data_ptr(), self.st), "fwd")

    def grads(self, fill=float("nan")):
        hd = H * self.d_k
        return (torch.full((B, max(self.Lq, 1), hd), fill, device=DEV), torch.full((B, self.Lk, hd), fill, device=DEV),
                torch.full((B, self.Lk, hd), fill, device=DEV))

    def two_launch(self, dout_off=0, fill=float("nan")):
        g = self.grads(fill)
        rc = self.lib.spacap_mha_bwd_f32(*self.args, self.lse.data_ptr(), self.dout.data_ptr() + 4 * dout_off, None, self.ws.data_ptr(),
                                         *(t.data_ptr() for t in g), 0, self.st)
        return rc, g

    def one_launch(self, dout_off=0, fill=float("nan")):
        g = self.grads(fill)
        rc = self.lib.spacap_mha_bwd_delta_f32(*self.args, self.lse.data_ptr(), self.dout.data_ptr() + 4 * dout_off, self.ws.data_ptr(),
                                               *(t.data_ptr() for t in g), 0, self.st)
        return rc, g


def _single_launch_equals_two(Lq, Lk, d_k, with_bias):
    assert R.tier(Lq, Lk, d_k).both is not None
    s = _Capi(Lq, Lk, d_k, with_bias)
    rc, g1 = s.two_launch()        # leaves delta in the workspace
    s.check(rc, "bwd")
    rc, g2 = s.one_launch()
    s.check(rc, "bwd delta")
    for a, b in zip(g1, g2):
        assert not bool(torch.isnan(a).any()) and torch.equal(a, b)


@pytest.mark.parametrize("Lq,Lk,d_k", R.SINGLE_CASES)
def test_single_launch_backward_equals_the_two_launch_form(att, Lq, Lk, d_k):
    """spacap_mha_bwd_delta_f32 fed the delta that spacap_mha_bwd_f32 left in its workspace: the same bodies, so the same bits --
    at every (tier, d_k) of the single-launch form, with Lq == Lk and with Lq != Lk."""
    _single_launch_equals_two(Lq, Lk, d_k, False)


@pytest.mark.parametrize("Lq,Lk,d_k", R.SINGLE_BIAS_CASES)
def test_single_launch_backward_with_a_bias(att, Lq, Lk, d_k):
    _single_launch_equals_two(Lq, Lk, d_k, True)


@pytest.mark.parametrize("Lq,Lk", R.SINGLE_REFUSED)
def test_single_launch_backward_refuses_mixed_shapes(att, Lq, Lk):
    s = _Capi(Lq, Lk, 16)
    s.check(s.two_launch()[0], "bwd")
    rc, g = s.one_launch(fill=7.0)
    assert rc != 0 and b"no single-launch form" in s.lib.spacap_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in g)


@pytest.mark.parametrize("Lq,Lk,d_k", [(65, 128, 32), (130, 130, 64), (67, 64, 16)])
def test_d_out_needs_no_alignment(att, Lq, Lk, d_k):
    """The four-wave kernels read d_out by 16-byte loads only where its base allows them: a d_out 4 bytes past a 16-byte
    boundary gives the gradients of the aligned one, bit for bit, through both entry points."""
    s = _Capi(Lq, Lk, d_k)
    n = B * Lq * H * d_k
    rc, g1 = s.two_launch()
    s.check(rc, "bwd")
    s.dout[1:n + 1].copy_(s.dout[:n].clone())
    assert (s.dout.data_ptr() + 4) % 16 == 4
    rc, g2 = s.two_launch(dout_off=1)
    s.check(rc, "bwd, d_out off by 4 bytes")
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    if R.tier(Lq, Lk, d_k).both is not None:
        rc, g3 = s.one_launch(dout_off=1)
        s.check(rc, "bwd delta, d_out off by 4 bytes")
        for a, b in zip(g1, g3):
            assert torch.equal(a, b)


@pytest.mark.parametrize("d_k", R.D_KS)
def test_zero_length_queries_leave_zero_key_gradients(att, d_k):
    """Lq == 0 through both backward entry points: dk and dv (dense, pre-filled with 7) come back all zero, nothing else is
    needed but a valid q pointer."""
    s = _Capi(0, 33, d_k)
    for entry in ("spacap_mha_bwd_f32", "spacap_mha_bwd_delta_f32"):
        dq, dk, dv = s.grads(7.0)
        tail = (None, None, None, None) if entry == "spacap_mha_bwd_f32" else (None, None, None)
        s.check(getattr(s.lib, entry)(*s.args, *tail, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), 0, s.st), entry)
        torch.cuda.synchronize()
        assert bool((dk == 0).all()) and bool((dv == 0).all()) and bool((dq == 7.0).all())
