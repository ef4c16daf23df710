"""Every attention kernel at B 8, h 8: packed self-attention forward + backward at L in 32 .. 512 x d_k in 16, 32, 64, the
single-launch backward at the same shapes through the C ABI, and one cross shape (Lq 32, Lk 256, d_k 16); 3 warm-up + 20
iterations per shape.  Run under rocprofv3 --kernel-trace --stats for the per-kernel averages (a kernel that serves two
shapes is told apart by its grid in the trace); profiles/r08_mha_fold.md was taken with it in two trees."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from spacap3d_amd import attention as att
dev = torch.device("cuda:0")
torch.manual_seed(0)
B, h = 8, 8
for L in (32, 64, 128, 256, 512):
    for dk in (16, 32, 64):
        qkv = torch.randn(B, L, 3 * h * dk, device=dev, requires_grad=True)
        mask = (torch.rand(B, 1, L, device=dev) > 0.2)
        w = torch.randn(B, L, h * dk, device=dev)
        for it in range(23):
            out, p = att.self_attention_packed(qkv, h, mask=mask, dropout_p=0.1, training=True, need_p=False)
            (out * w).sum().backward()
            qkv.grad = None
# the single-launch backward (what the fused Transformer layers call) at the same self-attention shapes, through the C ABI
import math
from spacap3d_amd._native import check, lib
st = torch.cuda.current_stream().cuda_stream
for L in (32, 64, 128, 256, 512):
    for dk in (16, 32, 64):
        hd = h * dk
        qkv = torch.randn(B, L, 3 * hd, device=dev)
        m8 = (torch.rand(B, 1, L, device=dev) > 0.2).to(torch.uint8).contiguous()
        o, lse, dout = torch.empty(B, L, hd, device=dev), torch.empty(B, h, L, 2, device=dev), torch.randn(B, L, hd, device=dev)
        delta, dqkv = torch.zeros(B, h, L, device=dev), torch.empty_like(qkv)
        base, gb, sr = qkv.data_ptr(), dqkv.data_ptr(), (L * 3 * hd, dk, 3 * hd)
        args = (base, base + 4 * hd, base + 8 * hd, *sr, *sr, *sr, m8.data_ptr(), L, 0, None, 0, 0, 0, B, h, L, L, dk,
                1.0 / math.sqrt(dk), 0.1, 12345, att.rng_state(dev).data_ptr())
        check(lib.spacap_mha_fwd_f32(*args, o.data_ptr(), None, lse.data_ptr(), st), "fwd")
        for it in range(23):
            check(lib.spacap_mha_bwd_delta_f32(*args, lse.data_ptr(), dout.data_ptr(), delta.data_ptr(), gb, gb + 4 * hd, gb + 8 * hd,
                                               3 * hd, st), "delta")
Lq, Lk, dk = 32, 256, 16
q = torch.randn(B, h, Lq, dk, device=dev, requires_grad=True)
k = torch.randn(B, h, Lk, dk, device=dev, requires_grad=True)
v = torch.randn(B, h, Lk, dk, device=dev, requires_grad=True)
w = torch.randn(B, h, Lq, dk, device=dev)
mask = (torch.rand(B, 1, 1, Lk, device=dev) > 0.2).long()
for it in range(23):
    out, p = att.attention(q, k, v, mask=mask, dropout_p=0.1, training=True, need_p=False)
    (out * w).sum().backward()
torch.cuda.synchronize()
print("done")
