"""The relation head (models/transformer_captioner.py:319-326, 392-397): pred = lin3(relu(lin2(relu(lin1(R))))) on the B*K*K
proposal pairs, with the pair feature R[b,i,j,h*D+d] = P[b,h,i,j] * V[b,h,j,d] of the last encoder layer's attention map
P (B,H,K,K) and values V (B,H,K,D).  lin1 is (C, H*D), lin2 (C, C), lin3 (NO, C).

``relation_pred`` runs the first form of this ladder that takes the shape; ``tier`` names it:

  "fused"         one kernel each way (``RelationHead``, csrc/relation_fused.hip):       H = 8, C = 128, NO = 9, K a multiple of 8
  "wide"          ``RelationWide`` (csrc/gemm_bf3.hip, csrc/dense_rows.hip):             H in 8 / 16 / 32, C in 128 / 256 / 512, NO = 9,
                                                                                         any K -- so also the 128-wide head at K % 8 != 0
  "l1+tail"       first-layer kernel (``RelationLayer1``) + ``RelationTail``:            H in 4 / 8 / 16 / 32, C = 128, NO = 9, gradients on
  "l1+tall"       first-layer kernel + two ``tall_linear``:                              the same H at other C / NO, or gradients off
  "feature+tail"  pair feature (``RelationFeature``) + BLAS Linear + ``RelationTail``:   other H, C = 128, NO = 9, gradients on
  "feature+tall"  pair feature + BLAS Linear + two ``tall_linear``:                      everything else

``relation_head``, ``relation_head_wide`` and ``relation_tail`` are the entries of the first two forms and of the tail node: each
returns ``None`` for operands it does not take.
"""
import torch
import torch.nn.functional as F
from torch.autograd import Function

from ._native import check, lib, sum_slabs
from .linear import _dense, bf3_pieces, bf3_product, dense_product


class RelationFeature(Function):
    """R[b,i,j,h*D+d] = P[b,h,i,j] * V[b,h,j,d]  (models/transformer_captioner.py:393-396) in one launch each way."""

    @staticmethod
    def forward(ctx, P, V):
        if not P.is_cuda:
            raise RuntimeError("CPU not supported")
        P = P.contiguous()
        if V.stride(3) != 1 or any(s % 4 for s in V.stride()[:3]) or V.data_ptr() % 16:
            V = V.contiguous()
        B, H, K, D = V.shape
        with torch.cuda.device(P.device):
            R = torch.empty(B, K, K, H * D, dtype=torch.float32, device=P.device)
            check(lib.spacap_relation_feature_fwd_f32(P.data_ptr(), V.data_ptr(), V.stride(0), V.stride(1), V.stride(2),
                                                      B, H, K, D, R.data_ptr(),
                                                      torch.cuda.current_stream(P.device).cuda_stream),
                  "spacap_relation_feature_fwd_f32")
        ctx.save_for_backward(P, V)
        return R

    @staticmethod
    def backward(ctx, dR):
        P, V = ctx.saved_tensors
        B, H, K, D = V.shape
        dR = dR.contiguous()
        with torch.cuda.device(P.device):
            dP = torch.empty_like(P)
            dV = torch.empty(B, K, H, D, dtype=torch.float32, device=P.device)
            check(lib.spacap_relation_feature_bwd_f32(dR.data_ptr(), P.data_ptr(), V.data_ptr(), V.stride(0), V.stride(1),
                                                      V.stride(2), B, H, K, D, dP.data_ptr(), dV.data_ptr(),
                                                      torch.cuda.current_stream(P.device).cuda_stream),
                  "spacap_relation_feature_bwd_f32")
        return dP, dV.transpose(1, 2)


def relation_feature(P, V):
    return RelationFeature.apply(P, V)


class RelationLayer1(Function):
    """relu(b1 + sum_h P[b,h,i,j] * U[b,j,h,:])  -- see csrc/relation.hip."""

    @staticmethod
    def forward(ctx, P, U, b1):
        P, U = P.contiguous(), U.contiguous()
        B, H, K, _ = P.shape
        C = U.shape[-1]
        with torch.cuda.device(P.device):
            H1 = torch.empty(B, K, K, C, dtype=torch.float32, device=P.device)
            check(lib.spacap_relation_l1_fwd_f32(P.data_ptr(), U.data_ptr(), b1.data_ptr(), B, H, K, C, H1.data_ptr(),
                                                 torch.cuda.current_stream(P.device).cuda_stream), "spacap_relation_l1_fwd_f32")
        ctx.save_for_backward(P, U, H1)
        return H1

    @staticmethod
    def backward(ctx, dH1):
        P, U, H1 = ctx.saved_tensors
        B, H, K, _ = P.shape
        C = U.shape[-1]
        dH1 = dH1.contiguous()
        with torch.cuda.device(P.device):
            dP = torch.empty_like(P)
            dU = torch.empty(int(lib.spacap_relation_l1_isplit()), *U.shape, dtype=torch.float32, device=P.device)
            part = torch.empty(int(lib.spacap_relation_l1_blocks(B, K, C)), C, dtype=torch.float32, device=P.device)
            check(lib.spacap_relation_l1_bwd_f32(dH1.data_ptr(), H1.data_ptr(), P.data_ptr(), U.data_ptr(), B, H, K, C,
                                                 dP.data_ptr(), dU.data_ptr(), part.data_ptr(),
                                                 torch.cuda.current_stream(P.device).cuda_stream), "spacap_relation_l1_bwd_f32")
        return dP, sum_slabs(dU), sum_slabs(part)


def relation_layer1(P, V, weight, bias):
    """First Linear + ReLU of the relation MLP applied to the relation feature of (P, V), without forming the feature:
    P (B,h,K,K), V (B,h,K,d) (any strides), weight (C, h*d), bias (C) -> (B,K,K,C)."""
    if not P.is_cuda:
        raise RuntimeError("CPU not supported")
    B, H, K, D = V.shape
    C = weight.shape[0]
    if not lib.spacap_relation_l1_supported(H, K, C):
        # shapes without a first-layer kernel: the feature is formed (one launch) and multiplied by BLAS
        return torch.relu(torch.nn.functional.linear(RelationFeature.apply(P, V), weight, bias))
    U = torch.einsum("bhjd,ohd->bjho", V, weight.view(C, H, D))  # (B,K,H,C): tiny, autograd gives dV and dW1
    return RelationLayer1.apply(P, U, bias)


def _sum_slabs(t):
    if not t.is_cuda:
        return t.sum(0)
    return sum_slabs(t.contiguous())


class _TallLinear(torch.autograd.Function):
    """y = x W^T + b for inputs with very many rows (the relation head runs its MLP on B*K*K = 524 288 pair
    features).  Forward and dX are ordinary GEMMs; the weight gradient dW = G^T X reduces over all rows into a
    128 x 128 output, which the BLAS heuristics run as a handful of tiles with no split over K (1.08 ms per
    layer on MI355X); here the rows are cut into 64 slabs, multiplied as one batched GEMM and summed
    (0.15 ms, fixed summation order)."""

    SLABS = 64

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g2 = g.reshape(-1, g.shape[-1])
        x2 = x.reshape(-1, x.shape[-1])
        rows, S = g2.shape[0], _TallLinear.SLABS
        dx = (g2 @ weight).view_as(x) if ctx.needs_input_grad[0] else None
        if rows % S == 0 and rows >= 64 * S:
            dw = _sum_slabs(torch.bmm(g2.view(S, rows // S, -1).transpose(1, 2), x2.view(S, rows // S, -1)))
        else:
            dw = g2.t() @ x2
        # column sums of a very tall, narrow matrix: torch's reduction takes 0.66 ms for 524 288 x 9; two stages 17 us
        db = g2.view(1024, rows // 1024, -1).sum(1).sum(0) if rows % 1024 == 0 and rows >= 65536 else g2.sum(0)
        return dx, dw, db


def tall_linear(x, lin):
    return _TallLinear.apply(x, lin.weight, lin.bias)


class RelationTail(Function):
    """pred = W3 relu(W2 hid1 + b2) + b3 on the B*K*K pair rows of the relation head
    (models/transformer_captioner.py:319-326, 392-397; hid1 = the first layer's ReLU output, 524 288 x 128 at the
    benchmark shape).  Forward: ONE kernel reads hid1 and writes hid2 and pred (csrc/sa_fwd.hip: sa_mid_fwd_kernel, TAIL).
    Backward: one streaming kernel gives dz2 = (dpred W3) * (hid2 > 0) and the partial sums of dW3, db2, db3
    (csrc/rel_tail.hip: rel_tail_bwd_kernel); dhid1 = dz2 W2 and dW2 = dz2^T hid1 are MFMA-bound BLAS GEMMs (the latter cut into 64 row
    slabs: the BLAS heuristics do not split that reduction)."""

    SLABS = 64

    @staticmethod
    def forward(ctx, hid1, W2, b2, W3, b3):
        shape = hid1.shape
        h1 = hid1.reshape(-1, 128).contiguous()
        R = h1.shape[0]
        dev = h1.device
        W2c, W3c = W2.contiguous(), W3.contiguous()
        with torch.cuda.device(dev):
            hid2 = torch.empty_like(h1)
            pred = torch.empty(R, W3.shape[0], dtype=torch.float32, device=dev)
            check(lib.spacap_rel_tail_fwd_f32(h1.data_ptr(), W2c.data_ptr(), b2.data_ptr(), W3c.data_ptr(), b3.data_ptr(), R,
                                              hid2.data_ptr(), pred.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                  "spacap_rel_tail_fwd_f32")
        ctx.save_for_backward(h1, hid2, W2c, W3c)
        ctx.shape = shape
        return pred.view(*shape[:-1], W3.shape[0])

    @staticmethod
    def backward(ctx, g):
        h1, hid2, W2, W3 = ctx.saved_tensors
        NO = W3.shape[0]
        g2 = g.reshape(-1, NO).contiguous()
        R = g2.shape[0]
        dev = g2.device
        with torch.cuda.device(dev):
            nparts = int(lib.spacap_rel_tail_bwd_nparts(R))
            PW = NO * 128 + 128 + 16
            part = torch.empty(nparts, PW, dtype=torch.float32, device=dev)
            dz2 = torch.empty_like(hid2)
            check(lib.spacap_rel_tail_bwd_f32(g2.data_ptr(), W3.data_ptr(), hid2.data_ptr(), R, dz2.data_ptr(), part.data_ptr(),
                                              torch.cuda.current_stream(dev).cuda_stream), "spacap_rel_tail_bwd_f32")
            s = sum_slabs(part, deferrable=True)
            dW3, db2, db3 = s[:NO * 128].view(NO, 128), s[NO * 128:NO * 128 + 128], s[NO * 128 + 128:NO * 128 + 128 + NO]
            dh1 = None
            if ctx.needs_input_grad[0]:
                if R >= 49152 and lib.spacap_gemm_rows_supported(128, 128):
                    # dz2 W2 on the streaming split-bf16 kernel (fp32-equivalent; 170 us in BLAS -> ~125 us at 524 288 rows)
                    dh1 = torch.empty_like(hid2)
                    W2t = W2.t().contiguous()
                    check(lib.spacap_gemm_rows_f32(dz2.data_ptr(), W2t.data_ptr(), R, 128, 128, dh1.data_ptr(),
                                                   torch.cuda.current_stream(dev).cuda_stream), "spacap_gemm_rows_f32")
                    dh1 = dh1.view(ctx.shape)
                else:
                    dh1 = (dz2 @ W2).view(ctx.shape)
            S = RelationTail.SLABS
            if R % S == 0 and R >= 64 * S:
                dW2 = sum_slabs(torch.bmm(dz2.view(S, R // S, 128).transpose(1, 2), h1.view(S, R // S, 128)).view(S, -1),
                                deferrable=True).view(128, 128)
            else:
                dW2 = dz2.t() @ h1
        return dh1, dW2, db2, dW3, db3


def relation_tail(hid1, lin2, lin3):
    """``lin3(relu(lin2(hid1)))`` for the relation head's 128 -> 128 -> 9 tail; ``None`` for other shapes."""
    if not hid1.is_cuda or hid1.dtype != torch.float32 or tuple(lin2.weight.shape) != (128, 128) or \
            tuple(lin3.weight.shape) != (9, 128) or lin2.bias is None or lin3.bias is None or hid1.shape[-1] != 128:
        return None
    return RelationTail.apply(hid1, lin2.weight, lin2.bias, lin3.weight, lin3.bias)


class RelationU(Function):
    """U[b, j, h, :] = W1[:, d h : d h + d] V[b, h, j, :]: the relation head's first Linear applied per head to the value vectors
    (models/transformer_captioner.py:319-326 with the pair feature of :393-397 factored, see relation_head).  V is the (B, h, K, d)
    VIEW of the packed q | k | v projection (row stride 3 h d): read in place.  h independent products of one launch each way;
    the weight gradient is h diagonal blocks of dU^T V (per-slab partials in dW1's own layout + one deferrable sum)."""

    @staticmethod
    def forward(ctx, V, W1):
        B, H, K, D = V.shape
        C = W1.shape[0]
        Vr = V.transpose(1, 2)                      # (B, K, H, D)
        if not (Vr.stride(3) == 1 and Vr.stride(2) == D and Vr.stride(0) == K * Vr.stride(1)):
            Vr = Vr.contiguous()
        W1c = W1.contiguous()
        lda = Vr.stride(1)
        dev = V.device
        with torch.cuda.device(dev):
            U = torch.empty(B, K, H, C, dtype=torch.float32, device=dev)
            _dense(dev, Vr.data_ptr(), lda, W1c.data_ptr(), H * D, True, None, B * K, D, C, U.data_ptr(), H * C, slices=H,
                   slice_stride=C, batch=1, a_z=D, w_z=D)
        ctx.save_for_backward(Vr, W1c)
        return U

    @staticmethod
    def backward(ctx, dU):
        Vr, W1 = ctx.saved_tensors
        B, K, H, D = Vr.shape
        C = W1.shape[0]
        R = B * K
        dev = dU.device
        dU = dU.contiguous()
        lda = Vr.stride(1)
        st = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            dV = None
            if ctx.needs_input_grad[0]:
                dVr = torch.empty(B, K, H, D, dtype=torch.float32, device=dev)
                _dense(dev, dU.data_ptr(), H * C, W1.data_ptr(), H * D, False, None, R, C, D, dVr.data_ptr(), H * D, slices=H,
                       slice_stride=D, batch=1, a_z=C, w_z=D)
                dV = dVr.transpose(1, 2)
            nslab = int(lib.spacap_dense_wgrad_blocks_slabs(R))
            part = torch.empty(nslab, C * H * D, dtype=torch.float32, device=dev)
            check(lib.spacap_dense_wgrad_blocks_f32(dU.data_ptr(), H * C, Vr.data_ptr(), lda, R, H, C, D, nslab, part.data_ptr(), st),
                  "spacap_dense_wgrad_blocks_f32")
            dW1 = sum_slabs(part, deferrable=True).view(C, H * D)
        return dV, dW1


class RelationHead(Function):
    """The whole relation head (models/transformer_captioner.py:319-326, 392-397) as one kernel each way
    (csrc/relation_fused.hip): pred = W3 relu(W2 relu(b1 + sum_h P U) + b2) + b3 on the B*K*K pairs, with
    U[b,j,h,:] = V[b,h,j,:] W1[:, 16h:16h+16]^T formed by the caller.  Neither the pair feature nor the first hidden layer
    nor any gradient of pair size exists in HBM: the forward stores hid2 (the backward's one large input) and pred; the
    backward returns dP, the dU partials and per-workgroup partial sums of dW2, dW3, db1, db2, db3.  It visits only the
    (query row) x (key column) sub-grid on which the incoming gradient is not zero (found on the device from the gradient
    itself: the relation loss weights pair (i, j) by "both proposals selected")."""

    @staticmethod
    def forward(ctx, P, U, b1, W2, b2, W3, b3):
        P, U, W2c, W3c = P.contiguous(), U.contiguous(), W2.contiguous(), W3.contiguous()
        B, H, K, _ = P.shape
        dev = P.device
        with torch.cuda.device(dev):
            hid2 = torch.empty(B, K, K, 128, dtype=torch.float32, device=dev)
            pred = torch.empty(B, K, K, 9, dtype=torch.float32, device=dev)
            check(lib.spacap_relation_fused_fwd_f32(P.data_ptr(), U.data_ptr(), b1.data_ptr(), W2c.data_ptr(), b2.data_ptr(),
                                                    W3c.data_ptr(), b3.data_ptr(), B, K, hid2.data_ptr(), pred.data_ptr(),
                                                    torch.cuda.current_stream(dev).cuda_stream), "spacap_relation_fused_fwd_f32")
        ctx.save_for_backward(P, U, b1, W2c, W3c, hid2)
        return pred

    @staticmethod
    def backward(ctx, g):
        P, U, b1, W2, W3, hid2 = ctx.saved_tensors
        B, H, K, _ = P.shape
        dev = P.device
        g = g.contiguous()
        with torch.cuda.device(dev):
            PW = int(lib.spacap_relation_fused_part_floats())
            nparts = int(lib.spacap_relation_fused_nparts(B, K))
            zslots = int(lib.spacap_relation_fused_sel_zsplit(B, K, nparts))
            part = torch.empty(nparts, PW, dtype=torch.float32, device=dev)
            dP = torch.empty_like(P)
            dU = torch.empty(zslots, *U.shape, dtype=torch.float32, device=dev)
            ws = torch.empty(int(lib.spacap_relation_fused_sel_workspace_bytes(B, K)), dtype=torch.uint8, device=dev)
            check(lib.spacap_relation_fused_bwd_sel_f32(g.data_ptr(), hid2.data_ptr(), P.data_ptr(), U.data_ptr(), b1.data_ptr(),
                                                        W2.data_ptr(), W3.data_ptr(), B, K, nparts, zslots, dP.data_ptr(),
                                                        dU.data_ptr(), part.data_ptr(), ws.data_ptr(),
                                                        torch.cuda.current_stream(dev).cuda_stream),
                  "spacap_relation_fused_bwd_sel_f32")
            s = sum_slabs(part, deferrable=True)
        o = 128 * 128
        dW2, dW3 = s[:o].view(128, 128), s[o:o + 9 * 128].view(9, 128)
        o += 9 * 128
        return dP, sum_slabs(dU), s[o:o + 128], dW2, s[o + 128:o + 256], dW3, s[o + 256:o + 265]


class RelationWide(Function):
    """The relation head at shapes the one-kernel form has no kernel for (the 512-wide / 32-head stress configuration, and the
    128-wide head when K is not a multiple of 8; models/transformer_captioner.py:319-326, 392-397), composed of this library's
    kernels:
        hid1 = relu(b1 + sum_h P U)            csrc/gemm_bf3.hip: rel_wide_l1_* (the pair feature is never formed: U = per-head first
                                               Linear of V; one workgroup per key column on the matrix cores, P read transposed)
        hid2 = relu(hid1 W2^T + b2)            csrc/gemm_bf3.hip (tiled split-bf16 product, bias + ReLU in its epilogue)
        pred = hid2 W3^T + b3                  csrc/dense_rows.hip
    backward: dz2 / dW3 / db2 / db3 in one pass over hid2 (rel_wide_tail_bwd_kernel), dW2 = dz2^T hid1 and dhid1 = dz2 W2 as
    split-bf16 products, then the first layer's backward (masks by hid1 > 0 itself).  Three tensors of pair size live between
    forward and backward (hid1, hid2; dz2 in the backward; dhid1 reuses hid2's memory)."""

    @staticmethod
    def forward(ctx, P, U, b1, W2, b2, W3, b3):
        P, U, W2c, W3c = P.contiguous(), U.contiguous(), W2.contiguous(), W3.contiguous()
        B, H, K, _ = P.shape
        C = U.shape[-1]
        dev = P.device
        st = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            Pt = torch.empty(B, K, H, K, dtype=torch.float32, device=dev)      # Pt[b,j,h,i] = P[b,h,i,j]: a key column's block contiguous
            check(lib.spacap_rel_wide_transpose_f32(P.data_ptr(), Pt.data_ptr(), B, H, K, 1, st), "spacap_rel_wide_transpose_f32")
            hid1 = torch.empty(B * K * K, C, dtype=torch.float32, device=dev)
            check(lib.spacap_rel_wide_l1_fwd_f32(Pt.data_ptr(), U.data_ptr(), b1.data_ptr(), B, H, K, C, hid1.data_ptr(), st),
                  "spacap_rel_wide_l1_fwd_f32")
            hid2 = bf3_product(hid1, bf3_pieces(W2c), b2, relu=True)
            pred = dense_product(hid2, W3c, True, bias=b3)
        ctx.save_for_backward(Pt, U, W2c, W3c, hid1, hid2)
        ctx.spent = False
        return pred.view(B, K, K, W3c.shape[0])

    @staticmethod
    def backward(ctx, g):
        if ctx.spent:    # (dhid1 is written into hid2's memory: a second backward over a retained graph would read garbage)
            raise RuntimeError("RelationWide: its backward can run once per forward (retain_graph is not supported)")
        ctx.spent = True
        Pt, U, W2, W3, hid1, hid2 = ctx.saved_tensors
        B, K, H, _ = Pt.shape
        C = U.shape[-1]
        NO = W3.shape[0]
        R = B * K * K
        dev = Pt.device
        st = torch.cuda.current_stream(dev).cuda_stream
        g2 = g.reshape(R, NO).contiguous()
        with torch.cuda.device(dev):
            nparts = int(lib.spacap_rel_wide_tail_nparts(R))
            part = torch.empty(nparts, NO * C + C + 16, dtype=torch.float32, device=dev)
            dz2 = torch.empty_like(hid2)
            check(lib.spacap_rel_wide_tail_bwd_f32(g2.data_ptr(), W3.data_ptr(), hid2.data_ptr(), R, C, nparts, dz2.data_ptr(),
                                                   part.data_ptr(), st), "spacap_rel_wide_tail_bwd_f32")
            s = sum_slabs(part, deferrable=True)
            dW3, db2, db3 = s[:NO * C].view(NO, C), s[NO * C:NO * C + C], s[NO * C + C:NO * C + C + NO]
            nslab = int(lib.spacap_gemm_bf3_wgrad_slabs(R, C, C))
            pw = torch.empty(nslab, C * C, dtype=torch.float32, device=dev)
            # the Linear layers' split-bf16 weight-gradient kernel (row-major images read by transposing LDS reads:
            # csrc/linear_grad.hip)
            check(lib.spacap_linear_wgrad_nslab_f32(dz2.data_ptr(), hid1.data_ptr(), R, C, C, 0, nslab, pw.data_ptr(), st),
                  "spacap_linear_wgrad_nslab_f32")
            dW2 = sum_slabs(pw, deferrable=True).view(C, C)
            dh1 = bf3_product(dz2, bf3_pieces(W2, trans=True), out=hid2)      # hid2 is dead: its memory takes dhid1
            del dz2
            dPt, dU = torch.empty_like(Pt), torch.empty_like(U)
            pb = torch.empty(B * K, C, dtype=torch.float32, device=dev)
            check(lib.spacap_rel_wide_l1_bwd_f32(dh1.data_ptr(), hid1.data_ptr(), Pt.data_ptr(), U.data_ptr(), B, H, K, C, dPt.data_ptr(),
                                                 dU.data_ptr(), pb.data_ptr(), st), "spacap_rel_wide_l1_bwd_f32")
            dP = torch.empty(B, H, K, K, dtype=torch.float32, device=dev)
            check(lib.spacap_rel_wide_transpose_f32(dPt.data_ptr(), dP.data_ptr(), B, H, K, 0, st), "spacap_rel_wide_transpose_f32")
        return dP, dU, sum_slabs(pb), dW2, db2, dW3, db3


# ---- the ladder ----------------------------------------------------------------------------------------------------------------

def _fused_shape(H, K, C, NO):
    return C == 128 and bool(lib.spacap_relation_fused_supported(H, K, 128, NO))


def _wide_shape(H, K, C, NO):
    return NO == 9 and bool(lib.spacap_rel_wide_l1_supported(H, K, C)) and bool(lib.spacap_gemm_bf3_supported(C, C)) and \
        bool(lib.spacap_rel_wide_tail_supported(C))


def tier(H, K, D, C, NO, cuda, grad):
    """The name of the form (module docstring) that ``relation_pred`` runs for P (B,H,K,K), V (B,H,K,D), a C-wide MLP with NO
    outputs, float32 operands on the device (``cuda``) and gradient recording on or off (``grad``); ``None`` without a device:
    no form runs on the CPU.  (No form is chosen by D today: every first layer takes the head width it is given.)"""
    if not cuda:
        return None
    if _fused_shape(H, K, C, NO):
        return "fused"
    if _wide_shape(H, K, C, NO):
        return "wide"
    first = "l1" if lib.spacap_relation_l1_supported(H, K, C) else "feature"
    return first + ("+tail" if grad and C == 128 and NO == 9 else "+tall")


def _mlp_of(P, V, lin1, lin2, lin3):
    """(H, K, C, NO) when the operands are what the first two forms read -- float32 on the device, three Linear layers with a
    bias of shapes (C, H*D), (C, C), (NO, C) -- else None."""
    B, H, K, D = V.shape
    C, NO = lin1.weight.shape[0], lin3.weight.shape[0]
    if not P.is_cuda or P.dtype != torch.float32 or lin1.bias is None or lin2.bias is None or lin3.bias is None or \
            tuple(lin1.weight.shape) != (C, H * D) or tuple(lin2.weight.shape) != (C, C) or lin3.weight.shape[1] != C:
        return None
    return H, K, C, NO


def relation_head_wide(P, V, lin1, lin2, lin3):
    """The "wide" form (``RelationWide``) -> (B,K,K,9); ``None`` when its kernels do not cover the operands."""
    s = _mlp_of(P, V, lin1, lin2, lin3)
    if s is None or not _wide_shape(*s):
        return None
    U = RelationU.apply(V, lin1.weight)
    return RelationWide.apply(P, U, lin1.bias, lin2.weight, lin2.bias, lin3.weight, lin3.bias)


def relation_head(P, V, lin1, lin2, lin3):
    """``lin3(relu(lin2(relu(lin1(feature(P, V))))))`` -> (B,K,K,9) by the "fused" form (``RelationHead``) or, for shapes
    that one has no kernel for, the "wide" form; ``None`` when neither takes the operands (the caller then composes
    relation_layer1 with relation_tail or tall_linear: ``relation_pred``).  P (B,h,K,K), V (B,h,K,d)."""
    s = _mlp_of(P, V, lin1, lin2, lin3)
    if s is None or not _fused_shape(*s):
        return relation_head_wide(P, V, lin1, lin2, lin3)
    U = RelationU.apply(V, lin1.weight)   # (B,K,H,C): the first Linear applied per head to the value vectors
    return RelationHead.apply(P, U, lin1.bias, lin2.weight, lin2.bias, lin3.weight, lin3.bias)


def relation_pred(P, V, lin1, lin2, lin3):
    """relation_pred (B,K,K,NO) of the three Linear layers on the pair feature of (P, V), by the form ``tier`` names."""
    if not P.is_cuda:
        raise RuntimeError("CPU not supported")
    B, H, K, D = V.shape
    t = tier(H, K, D, lin1.weight.shape[0], lin3.weight.shape[0], True, torch.is_grad_enabled())
    pred = None
    if t == "fused":
        pred = relation_head(P, V, lin1, lin2, lin3)
    elif t == "wide":
        pred = relation_head_wide(P, V, lin1, lin2, lin3)
    if pred is None:
        # (also what is left for operands the entries above decline: a layer without bias, another dtype)
        hid = relation_layer1(P, V, lin1.weight, lin1.bias)       # "l1": one kernel; "feature": the pair feature + BLAS
        if t.endswith("+tail"):
            pred = relation_tail(hid, lin2, lin3)
        if pred is None:
            pred = tall_linear(F.relu(tall_linear(hid, lin2)), lin3)
    return pred
