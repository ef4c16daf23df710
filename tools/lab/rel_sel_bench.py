"""Relation head backward at the benchmark shape (B = 8, K = 256) for 0, 4, 96 and 256 selected proposals per scene:
the dense entry (spacap_relation_fused_bwd_f32), the selected entry (spacap_relation_fused_bwd_sel_f32: scan + zero fill,
compaction, backward) and its first two launches alone (spacap_relation_fused_sel_lists_f32); the backward kernel alone is
the difference of the last two.  HIP events around ITERS launches after a warm-up.
    python tools/lab/rel_sel_bench.py [ITERS]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from spacap3d_amd._native import check, lib  # noqa: E402

DEV = torch.device("cuda:0")
ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 20


def t(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / ITERS


def main():
    B, K, H = 8, 256, 8
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    P, U = torch.softmax(r(B, H, K, K), -1), r(B, K, H, 128) * 0.3
    b1, W2, b2, W3, b3 = r(128) * 0.1, r(128, 128) * 0.1, r(128) * 0.1, r(9, 128) * 0.1, r(9)
    hid2, pred = torch.empty(B, K, K, 128, device=DEV), torch.empty(B, K, K, 9, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    check(lib.spacap_relation_fused_fwd_f32(P.data_ptr(), U.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr(), W3.data_ptr(),
                                            b3.data_ptr(), B, K, hid2.data_ptr(), pred.data_ptr(), st), "fwd")
    nparts = int(lib.spacap_relation_fused_nparts(B, K))
    zs = int(lib.spacap_relation_fused_sel_zsplit(B, K, nparts))
    dP, dU = torch.empty_like(P), torch.empty(zs, B, K, H, 128, device=DEV)
    part = torch.empty(nparts, int(lib.spacap_relation_fused_part_floats()), device=DEV)
    ws = torch.empty(int(lib.spacap_relation_fused_sel_workspace_bytes(B, K)), dtype=torch.uint8, device=DEV)
    print(f"B={B} K={K} nparts={nparts} zslots={zs} (dense rule: {int(lib.spacap_relation_fused_zsplit(B, K, nparts))})")
    print(f"{'selected':>8s} {'dense us':>10s} {'selected us':>12s} {'lists us':>10s} {'kernel us':>10s}")
    for n in (0, 4, 96, 256):
        m = torch.zeros(B, K)
        for b in range(B):
            m[b, torch.randperm(K, generator=g)[:n]] = 1
        dpred = (torch.randn(B, K, K, 9, generator=g) * m[:, :, None, None] * m[:, None, :, None]).to(DEV)
        dense = t(lambda: check(lib.spacap_relation_fused_bwd_f32(
            dpred.data_ptr(), hid2.data_ptr(), P.data_ptr(), U.data_ptr(), b1.data_ptr(), W2.data_ptr(), W3.data_ptr(), B, K, nparts, zs,
            dP.data_ptr(), dU.data_ptr(), part.data_ptr(), st), "dense"))
        sel = t(lambda: check(lib.spacap_relation_fused_bwd_sel_f32(
            dpred.data_ptr(), hid2.data_ptr(), P.data_ptr(), U.data_ptr(), b1.data_ptr(), W2.data_ptr(), W3.data_ptr(), B, K, nparts, zs,
            dP.data_ptr(), dU.data_ptr(), part.data_ptr(), ws.data_ptr(), st), "sel"))
        lists = t(lambda: check(lib.spacap_relation_fused_sel_lists_f32(dpred.data_ptr(), B, K, zs, dP.data_ptr(), dU.data_ptr(),
                                                                        ws.data_ptr(), st), "lists"))
        print(f"{n:8d} {dense:10.1f} {sel:12.1f} {lists:10.1f} {sel - lists:10.1f}", flush=True)


if __name__ == "__main__":
    main()
