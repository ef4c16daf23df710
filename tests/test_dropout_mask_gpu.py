"""The dropout keep mask (csrc/dropout.hpp) against a numpy restatement of its contract, bit for bit.

Contract: seed = host word + device-resident counter * 0x9E3779B97F4A7C15 (mod 2^64; the counter is optional);
hash = murmur3 fmix32 over the flat element index mixed with both halves of the seed; keep iff hash >= floor(p * 2^32)
(p as the float the C ABI receives); p = 0 keeps everything.  Every backward regenerates this mask and the fused Transformer
layer must draw the masks of the composed operators, so the kernels are compared EXACTLY with the restatement wherever an
output exposes the mask and the element index is the flat output index: the two elementwise operators and the attention
forward's returned probabilities."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = (0xA5A51234 << 32) | 0x0F0F7777   # both 32-bit words non-zero
PS = [0.0, 0.1, 0.5]
COUNTERS = [None, 3]                     # seed_dev null / a one-word device tensor (the 64-bit multiply wraps)


@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spacap3d_amd import _native
    return _native


def expected_keep(n, p, seed, counter):
    """keep[i] of flat element index i = 0 .. n-1, in uint32 / uint64 array arithmetic (which wraps as the device's does)"""
    s = np.array([seed], dtype=np.uint64)
    if counter is not None:
        s = s + np.array([counter], dtype=np.uint64) * np.array([0x9E3779B97F4A7C15], dtype=np.uint64)
    s_lo, s_hi = (s & np.uint64(0xFFFFFFFF)).astype(np.uint32), (s >> np.uint64(32)).astype(np.uint32)
    idx = np.arange(n, dtype=np.uint64)
    h = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32) ^ s_lo
    h = h + ((idx >> np.uint64(32)).astype(np.uint32) ^ s_hi) * np.uint32(0x9E3779B1)
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    h = h ^ (h >> np.uint32(16))
    assert h.dtype == np.uint32
    thresh = int(float(np.float32(p)) * 4294967296.0) if p > 0 else 0
    return np.ones(n, dtype=bool) if thresh == 0 else h >= np.uint32(thresh)


def _counter_tensor(counter):
    return None if counter is None else torch.tensor([counter], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("counter", COUNTERS)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n", [3, 4, 1031])   # tail only / one vector / two workgroups and a tail
@pytest.mark.parametrize("op", ["relu_dropout", "dropout_add"])
def test_elementwise_dropout_draws_the_restated_mask(native, op, n, p, counter):
    x = torch.ones(n, device=DEV)
    out = torch.full((n,), -1.0, device=DEV)
    cnt = _counter_tensor(counter)
    cp = cnt.data_ptr() if cnt is not None else None
    st = torch.cuda.current_stream().cuda_stream
    if op == "relu_dropout":
        native.check(native.lib.spacap_relu_dropout_fwd_f32(x.data_ptr(), n, p, SEED, cp, out.data_ptr(), st), op)
    else:
        res = torch.zeros(n, device=DEV)
        native.check(native.lib.spacap_dropout_add_fwd_f32(res.data_ptr(), x.data_ptr(), n, p, SEED, cp, out.data_ptr(), st), op)
    y = out.cpu().numpy()
    keep = expected_keep(n, p, SEED, counter)
    assert np.array_equal(y > 0, keep)
    assert np.all(y[~keep] == 0) and np.all(y[keep] == np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


@pytest.mark.parametrize("counter", COUNTERS)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("B,h,Lq,Lk,dk", [(2, 2, 17, 33, 16), (1, 2, 20, 80, 16)])   # the second: key-split kernels
def test_attention_dropout_draws_the_restated_mask(native, B, h, Lq, Lk, dk, p, counter):
    g = torch.Generator().manual_seed(5)
    q = (torch.randn(B, h, Lq, dk, generator=g) * 0.1).to(DEV)   # small logits: every probability is > 0
    k = (torch.randn(B, h, Lk, dk, generator=g) * 0.1).to(DEV)
    v = torch.randn(B, h, Lk, dk, generator=g).to(DEV)
    out = torch.empty(B, Lq, h, dk, device=DEV)
    probs = torch.full((B, h, Lq, Lk), -1.0, device=DEV)
    stats = torch.empty(B, h, Lq, 2, device=DEV)
    cnt = _counter_tensor(counter)
    sq, sk = (h * Lq * dk, Lq * dk, dk), (h * Lk * dk, Lk * dk, dk)
    native.check(native.lib.spacap_mha_fwd_f32(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), *sq, *sk, *sk, None, 0, 0, None, 0, 0, 0, B, h, Lq, Lk, dk,
        1.0 / math.sqrt(dk), p, SEED, cnt.data_ptr() if cnt is not None else None, out.data_ptr(), probs.data_ptr(),
        stats.data_ptr(), torch.cuda.current_stream().cuda_stream), "spacap_mha_fwd_f32")
    pn = probs.cpu().numpy().reshape(-1)    # flat index ((b h + head) Lq + q) Lk + key
    assert np.all(pn >= 0)
    assert np.array_equal(pn != 0, expected_keep(pn.size, p, SEED, counter))
