"""Training-mode shared MLP of a set-abstraction module on libspacap_hip.so, point-major layout.

One autograd op for what the reference runs per SA module as QueryAndGroup -> SharedMLP -> max_pool2d
(lib/pointnet2/pointnet2_modules.py:241-259; SharedMLP = [Conv2d 1x1 -> BatchNorm2d -> ReLU] x 3,
lib/pointnet2/pytorch_utils.py:11-36).  See ``csrc/sa_common.hpp`` for the data flow, ``csrc/sa_fwd.hip`` / ``sa_bwd.hip`` / ``sa_rows.hip`` for the kernels.
The grouping indices come from ``ball_query`` as before; MLP shapes without kernels keep using the per-operator path
(``QueryAndGroup`` + ``SharedMLP``), which is also HIP.

``plan(C1, C2, C3, S, R, has_pm, need_xyz)`` decides ONCE per node, from the switches below and the library's predicates, which
launches the module makes; ``_SAMLP.forward`` keeps the record on ``ctx`` and the backward follows it:

    first    "moments"     l1_moments -> l1_moments_finalize -> mid_fwd_l1in      (SA1-shaped: z1 is rebuilt, never stored)
             "stats"       l1_stats -> bn_finalize -> mid_fwd_l1in                (the same with L1_MOMENTS off)
             "stored"      l1_fwd -> bn_finalize -> mid_fwd
    tail     "candidates"  mid_fwd_pool -> bn_finalize -> pool_finalize
             "plain"       mid_fwd -> bn_finalize -> pool_fwd
    l3_wgrad "z2"          wgrad_pool -> l3bwd_dw
             "dense"       wgrad + slab sum
    l2_l1    "one_pass"    dgrad_wgrad_l1in                                       } SA1-shaped; each ends with
             "l1in"        wgrad_l1in + dgrad_l1in    (FUSE_L2_WGRAD off)         } bwd_finalize -> l1_dw
             "l1_sums"     wgrad + dgrad_l1           (RECOMPUTE_Z1 off)          }
             "generic"     wgrad, dgrad, l1_bwd, then the feature and coordinate gradients

``sa_mlp_eval`` runs the "stored" / "plain" passes on the running statistics, without the finalisations.
"""
from typing import NamedTuple

import torch
from torch.autograd import Function

from .layout import ChannelMajorOf, point_major_of
from ._native import check, lib, sum_slabs


# SA1-shaped modules (no point features, 64 -> 64 -> ...): do not store the first layer's pre-activation (see _SAMLP.forward)
RECOMPUTE_Z1 = True
# ... and take that layer's BatchNorm statistics from the first and second moments of the rows' four inputs (z1 is linear in
# them): 14 sums per row, one thread per row, instead of 2 x 64 sums with 16 threads per row (csrc/sa_fwd.hip:
# sa_l1_moments_kernel; 87 -> ~20 us at SA1).  The statistics differ from the summed-z1 form by rounding only (~1e-7 relative).
L1_MOMENTS = True
# pooled last layer: its WEIGHT gradient from z2 alone (csrc/sa_l3bwd.inc: sa_wgrad_pool_kernel -- the sparse
# term (g d)^T a2 plus the Gram matrix a2^T a2) instead of the dense kernel that streams z3 and z2 and multiplies a [C3 x rows]
# operand with one non-zero per group and channel.  SA1: 92 + 12 us against 249 + 12 us (tools/lab/wgrad_pool_bench.py).  Used
# from POOL_WGRAD_MIN_ROWS rows on (below, the two extra launches of the reduction cost more than the pass saves).
POOL_WGRAD = True
POOL_WGRAD_MIN_ROWS = 131072
# SA1's second layer: weight gradient from the data-gradient kernel's pass (tests: False keeps the two kernels apart)
FUSE_L2_WGRAD = True


class Plan(NamedTuple):
    """Which launches a module makes: the table of the module docstring."""
    first: str
    tail: str
    l3_wgrad: str
    l2_l1: str


# What _SAMLP.forward saves for its backward, in save order (z1 is the rows' four inputs (R, 4) unless plan.first is "stored";
# feat / pm / zmax are None where the module has no inline feature / no point-major features / not the "candidates" tail)
Saved = NamedTuple("Saved", [(name, torch.Tensor) for name in
                             "xyz new_xyz idx feat pm W1 W2 W3 z1 z2 z3 st1 st2 st3 out arg zmax".split()])


def _sa1_shaped(C1, C2, has_pm, need_xyz):
    """No point-major features, 64 -> 64, no coordinate gradient: the first layer can be rebuilt from the rows' four inputs
    (csrc/sa_common.hpp: L1In) and its weight gradient comes out of the second layer's data-gradient pass as three sums."""
    return not has_pm and not need_xyz and C1 == 64 and C2 == 64


def plan(C1, C2, C3, S, R, has_pm, need_xyz):
    """The launches of one SA module (R = B * N * S grouped rows; has_pm: point-major features, i.e. a (B, Np, C1) product Y;
    need_xyz: a coordinate input requires a gradient).  The only reader of the switches above."""
    sa1 = _sa1_shaped(C1, C2, has_pm, need_xyz)
    rebuilt = sa1 and RECOMPUTE_Z1
    first = ("moments" if L1_MOMENTS else "stats") if rebuilt else "stored"
    tail = "candidates" if lib.spacap_sa_mid_fwd_pool_supported(C2, C3, S) else "plain"
    from_z2 = POOL_WGRAD and R >= POOL_WGRAD_MIN_ROWS and lib.spacap_sa_wgrad_pool_supported(C2, C3, S)
    if not sa1:
        l2_l1 = "generic"
    elif not rebuilt:
        l2_l1 = "l1_sums"
    else:   # (one read of dy2 / z2 instead of two, one launch fewer: csrc/sa_bwd.hip, sa_dgrad_kernel<.., WG>)
        l2_l1 = "one_pass" if FUSE_L2_WGRAD else "l1in"
    return Plan(first, tail, "z2" if from_z2 else "dense", l2_l1)


def _ptr(t):
    return t.data_ptr() if t is not None else None


_SELFTESTED = set()


def _selftest(dev):
    """Once per process and device, before the first fused SA op: the streaming split-bf16 kernels (csrc/sa_bf3.inc,
    sa_bf3_dgrad.inc) land their prefetched rows in AGPRs that are named inside inline asm and therefore invisible to the
    register allocator.  The build checks the generated assembly for compiler uses of those registers
    (tools/check_landing_regs.py); this is the matching check at RUN time, on the library that was actually loaded: a few
    tiles through the forward layer kernel and the data-gradient kernel against float64 -- a clobbered landing register gives
    errors of order one, the bar is 1e-4 of the result's scale.  Raises instead of training on garbage."""
    key = (dev.type, dev.index)
    if key in _SELFTESTED:
        return
    _SELFTESTED.add(key)
    with torch.cuda.device(dev), torch.no_grad():
        st = torch.cuda.current_stream(dev).cuda_stream
        if torch.cuda.is_current_stream_capturing():
            _SELFTESTED.discard(key)   # (never inside a graph capture: it synchronises)
            return
        g = torch.Generator(device="cpu").manual_seed(1234)
        R, ci, co = 49152 + 96, 128, 128
        zin, W = torch.randn(R, ci, generator=g).to(dev), (0.1 * torch.randn(co, ci, generator=g)).to(dev)
        stats = torch.tensor([0.05, 1.0, 1.1, 0.02], device=dev).repeat(ci, 1).contiguous()
        zout = torch.empty(R, co, dtype=torch.float32, device=dev)
        part = torch.empty(int(lib.spacap_sa_nparts()) * 2 * max(ci, co), dtype=torch.float64, device=dev)
        check(lib.spacap_sa_mid_fwd_f32(zin.data_ptr(), stats.data_ptr(), W.data_ptr(), R, ci, co, zout.data_ptr(), part.data_ptr(), st),
              "spacap_sa_mid_fwd_f32 (self-test)")
        a = ((zin.double() - 0.05) * 1.1 + 0.02).clamp_min(0)
        ref = a @ W.double().t()
        e1 = float((zout.double() - ref).abs().max() / ref.abs().max())
        # data gradient: dy_prev = (dz W) * [relu(bn(z_prev)) > 0], dz = g dy + k0 - k1 z
        dy, zk = torch.randn(R, co, generator=g).to(dev), torch.randn(R, co, generator=g).to(dev)
        coef = torch.tensor([1.05, 0.01, 0.02, 0.0], device=dev).repeat(co, 1).contiguous()
        dyp = torch.empty(R, ci, dtype=torch.float32, device=dev)
        check(lib.spacap_sa_dgrad_f32(dy.data_ptr(), None, 0, zk.data_ptr(), coef.data_ptr(), W.data_ptr(), zin.data_ptr(), stats.data_ptr(),
                                      R, co, ci, dyp.data_ptr(), part.data_ptr(), st), "spacap_sa_dgrad_f32 (self-test)")
        dz = 1.05 * dy.double() + 0.01 - 0.02 * zk.double()
        pre = (zin.double() - 0.05) * 1.1 + 0.02
        ref2 = (dz @ W.double()) * (pre > 0)
        near = pre.abs() < 1e-6
        e2 = float(((dyp.double() - ref2).abs() * (~near)).max() / ref2.abs().max())
    if not (e1 < 1e-4 and e2 < 1e-4):
        raise RuntimeError(f"libspacap_hip.so self-test failed: streaming shared-MLP kernels differ from float64 by {e1:.2e} (forward) / "
                           f"{e2:.2e} (data gradient) of the result's scale -- the landing registers of csrc/sa_bf3*.inc are not safe "
                           f"in this build (tools/check_landing_regs.py); set SPACAP_SA_F32MFMA=1 to run the fp32-MFMA kernels")


# ---- the passes.  Shared conventions: src = the pointers (feat or None, xyz, new_xyz, idx) and dims = (B, Np, N, S), in the order
# every first-layer entry point takes them; W / stats / z / coef are indexable by layer; norm = (BatchNorm module, gamma, beta) of
# the layer whose statistics a pass finalises, or None in inference (the statistics rows are the running statistics already).

def _bn_args(bn, gamma, beta):
    """What both finalisation entry points take about their training-mode BatchNorm: eps, momentum, gamma, beta and the running
    statistics to update (if it tracks any; its batch counter is bumped then)."""
    track = bn.track_running_stats and bn.running_mean is not None
    if track:
        from .fused_bn import bump_counter
        bump_counter(bn)
    return (float(bn.eps), 0.0 if bn.momentum is None else float(bn.momentum), gamma.data_ptr(), beta.data_ptr(),
            _ptr(bn.running_mean if track else None), _ptr(bn.running_var if track else None))


def _bn_finalize(part, R, norm, stats, st):
    """stats (C, 4) = (mean, 1/std, gamma/std, beta) from the sums a layer kernel left in part."""
    if norm is not None:
        check(lib.spacap_sa_bn_finalize_f32(part.data_ptr(), stats.shape[0], R, *_bn_args(*norm), stats.data_ptr(), st),
              "spacap_sa_bn_finalize_f32")


def _layer1(first, Y, src, W1, has_feat, rdiv, dims, R, nparts, z1, part, norm, stats, st):
    """plan.first: the first BatchNorm's statistics and, "stored", z1 (R, C1) = W1 . (rel, feature) [+ the gathered rows of Y];
    "moments" / "stats" leave the rows' four inputs in z1 (R, 4) instead (16 bytes per row: z1 itself never exists in HBM, every
    later pass rebuilds it from them; csrc/sa_common.hpp: L1In)."""
    C1, ld = W1.shape
    if first == "moments":
        mom = torch.empty(nparts * 16, dtype=torch.float64, device=z1.device)
        check(lib.spacap_sa_l1_moments_f32(*src, rdiv, *dims, z1.data_ptr(), mom.data_ptr(), st), "spacap_sa_l1_moments_f32")
        check(lib.spacap_sa_l1_moments_finalize_f32(mom.data_ptr(), W1.data_ptr(), ld, has_feat, C1, R, *_bn_args(*norm),
                                                    stats.data_ptr(), st), "spacap_sa_l1_moments_finalize_f32")
        return
    if first == "stats":
        check(lib.spacap_sa_l1_stats_f32(*src, W1.data_ptr(), ld, rdiv, *dims, C1, z1.data_ptr(), part.data_ptr(), st),
              "spacap_sa_l1_stats_f32")
    else:
        check(lib.spacap_sa_l1_fwd_f32(_ptr(Y), *src, W1.data_ptr(), ld, rdiv, *dims, C1, z1.data_ptr(), part.data_ptr(), st),
              "spacap_sa_l1_fwd_f32")
    _bn_finalize(part, R, norm, stats, st)


def _layer(k, z, W, stats, R, part, norm, st, l1in=None):
    """z[k] = relu(bn(z[k-1])) W[k]^T with layer k's BatchNorm sums and statistics; l1in = (ld of W1, has_feat): z[0] holds the
    rows' four inputs and the first layer is rebuilt in registers (k = 1 only)."""
    if l1in is None:
        check(lib.spacap_sa_mid_fwd_f32(z[k - 1].data_ptr(), stats[k - 1].data_ptr(), W[k].data_ptr(), R, W[k].shape[1],
                                        W[k].shape[0], z[k].data_ptr(), part.data_ptr(), st), "spacap_sa_mid_fwd_f32")
    else:
        check(lib.spacap_sa_mid_fwd_l1in_f32(z[0].data_ptr(), W[0].data_ptr(), *l1in, stats[0].data_ptr(), W[1].data_ptr(), R,
                                             z[1].data_ptr(), part.data_ptr(), st), "spacap_sa_mid_fwd_l1in_f32")
    _bn_finalize(part, R, norm, stats[k], st)


def _pool(z3, st3, G, S, out, arg, st):
    """plan.tail "plain", after _layer(2): out = max over each group's S rows of relu(bn(z3)), arg = the first maximum's row."""
    check(lib.spacap_sa_pool_fwd_f32(z3.data_ptr(), st3.data_ptr(), G, S, st3.shape[0], out.data_ptr(), arg.data_ptr(), st),
          "spacap_sa_pool_fwd_f32")


def _layer3_candidates(z, W, stats, R, G, S, part, norm, out, arg, zmax, st):
    """plan.tail "candidates": the last layer's kernel leaves the two best pooling candidates per (sub-group, channel); once the
    layer's statistics are final a G x C3 pass picks the first maximum: z3 is not read again in the forward.  zmax = the arg-max
    rows' pre-activations (the pooled layer's BatchNorm sums in the backward read them instead of gathering out of z3)."""
    C3, C2 = W[2].shape
    f32 = dict(dtype=torch.float32, device=out.device)
    g3c = norm[1].contiguous()
    cand_v = torch.empty(R // min(S, 32), C3, 2, **f32)
    cand_i = torch.empty(R // min(S, 32), C3, 2, dtype=torch.uint8, device=out.device)
    check(lib.spacap_sa_mid_fwd_pool_f32(z[1].data_ptr(), stats[1].data_ptr(), W[2].data_ptr(), g3c.data_ptr(), R, C2, C3,
                                         S, _ptr(z[2]), part.data_ptr(), cand_v.data_ptr(), cand_i.data_ptr(), st),
          "spacap_sa_mid_fwd_pool_f32")
    _bn_finalize(part, R, norm, stats[2], st)
    check(lib.spacap_sa_pool_finalize_f32(cand_v.data_ptr(), cand_i.data_ptr(), stats[2].data_ptr(), g3c.data_ptr(),
                                          G, S, C3, out.data_ptr(), arg.data_ptr(), _ptr(zmax), st), "spacap_sa_pool_finalize_f32")


def _wgrad(dy, arg, S, z, coef, W, zin, stin, R, st):
    """The dense weight gradient dW = dz^T relu(bn(zin)) of a layer with weight W (dy per group and arg / S given: the pooled layer)."""
    Co, Ci = W.shape
    pw = torch.empty(int(lib.spacap_sa_wgrad_slabs(R, Co, Ci, int(arg is not None))), Co, Ci, dtype=torch.float32, device=z.device)
    check(lib.spacap_sa_wgrad_f32(dy.data_ptr(), _ptr(arg), S, z.data_ptr(), coef.data_ptr(), zin.data_ptr(), stin.data_ptr(),
                                  R, Co, Ci, pw.data_ptr(), st), "spacap_sa_wgrad_f32")
    return sum_slabs(pw, deferrable=True)


def _wgrad_z2(dym, s, S, coef3, R, st):
    """plan.l3_wgrad "z2": the pooled layer's weight gradient from z2 alone, dW3 = (g d)^T a2 + k0 (x) colsum a2 - diag(k1) W3 a2^T a2."""
    C3, C2 = s.W3.shape
    f32 = dict(dtype=torch.float32, device=dym.device)
    npw, nfl = int(lib.spacap_sa_wgrad_pool_parts(R, C2, C3, S)), int(lib.spacap_sa_l3bwd_part_floats(C2, C3))
    pw = torch.empty(npw, nfl, **f32)
    check(lib.spacap_sa_wgrad_pool_f32(dym.data_ptr(), s.arg.data_ptr(), S, coef3.data_ptr(), s.z2.data_ptr(),
                                       s.st2.data_ptr(), R, C3, C2, pw.data_ptr(), st), "spacap_sa_wgrad_pool_f32")
    sums = torch.empty(nfl, dtype=torch.float64, device=dym.device)
    dW3 = torch.empty(C3, C2, **f32)
    check(lib.spacap_sa_l3bwd_dw_f32(pw.data_ptr(), npw, coef3.data_ptr(), s.W3.data_ptr(), C3, C2, sums.data_ptr(),
                                     dW3.data_ptr(), st), "spacap_sa_l3bwd_dw_f32")
    return dW3


def _dgrad(dy, arg, S, z, coef, W, zin, stin, R, dyin, part, st):
    """dyin = (dz W) * [relu(bn(zin)) > 0], dz = g dy + k0 - k1 z; its epilogue leaves the BatchNorm sums of the layer below."""
    check(lib.spacap_sa_dgrad_f32(dy.data_ptr(), _ptr(arg), S, z.data_ptr(), coef.data_ptr(), W.data_ptr(), zin.data_ptr(),
                                  stin.data_ptr(), R, W.shape[0], W.shape[1], dyin.data_ptr(), part.data_ptr(), st),
          "spacap_sa_dgrad_f32")


def _l2_l1_sums(form, dy2, s, coef2, src, has_feat, rdiv, dims, R, nparts, part, st):
    """plan.l2_l1 "one_pass" / "l1in" / "l1_sums" (SA1-shaped): dW2, and the first layer's weight gradient as three sums per
    part (pl1: csrc/sa_bwd.hip, L1Args) out of the data-gradient kernel's epilogue; dy1 is never written."""
    (C2, C1), ld = s.W2.shape, s.W1.shape[1]
    f32 = dict(dtype=torch.float32, device=dy2.device)
    l1in = (s.z1.data_ptr(), s.W1.data_ptr(), ld, has_feat, s.st1.data_ptr())     # the rebuilt first layer, as the kernels take it
    B, _, N, S = dims
    if form == "one_pass":
        pw = torch.empty(int(lib.spacap_sa_dgrad_wgrad_l1in_slabs(R)), C2, C1, **f32)
        pl1 = torch.empty(nparts, C1 * 8 + 4, **f32)
        check(lib.spacap_sa_dgrad_wgrad_l1in_f32(dy2.data_ptr(), s.z2.data_ptr(), coef2.data_ptr(), s.W2.data_ptr(), *l1in, B, N, S,
                                                 part.data_ptr(), pl1.data_ptr(), pw.data_ptr(), st), "spacap_sa_dgrad_wgrad_l1in_f32")
        dW2 = sum_slabs(pw, deferrable=True)
    elif form == "l1in":
        pw = torch.empty(int(lib.spacap_sa_wgrad_slabs(R, C2, C1, 0)), C2, C1, **f32)
        check(lib.spacap_sa_wgrad_l1in_f32(dy2.data_ptr(), s.z2.data_ptr(), coef2.data_ptr(), *l1in, R, pw.data_ptr(), st),
              "spacap_sa_wgrad_l1in_f32")
        dW2 = sum_slabs(pw, deferrable=True)
        pl1 = torch.empty(nparts, C1 * 8 + 4, **f32)
        check(lib.spacap_sa_dgrad_l1in_f32(dy2.data_ptr(), s.z2.data_ptr(), coef2.data_ptr(), s.W2.data_ptr(), *l1in, B, N, S,
                                           part.data_ptr(), pl1.data_ptr(), st), "spacap_sa_dgrad_l1in_f32")
    else:   # "l1_sums": z1 is stored, the kernel forms the rows' inputs itself
        dW2 = _wgrad(dy2, None, 0, s.z2, coef2, s.W2, s.z1, s.st1, R, st)
        pl1 = torch.empty(nparts, C1 * 8 + 4, **f32)
        check(lib.spacap_sa_dgrad_l1_f32(dy2.data_ptr(), s.z2.data_ptr(), coef2.data_ptr(), s.W2.data_ptr(), s.z1.data_ptr(),
                                         s.st1.data_ptr(), *src, rdiv, *dims, C2, C1, part.data_ptr(), pl1.data_ptr(), st),
              "spacap_sa_dgrad_l1_f32")
    return dW2, pl1


def _l1_generic(dy1, s, coef1, src, rdiv, dims, nparts, ri, need_xyz, want, st):
    """plan.l2_l1 "generic", first layer: dz1 in place of dy1, then dW1 ([coordinate columns | feature columns]) and, as asked for
    (want = needs_input_grad of xyz, new_xyz, pm), the gradients of the point-major features and of the coordinates."""
    dev, (B, Np, N, S), (C1, ld) = dy1.device, dims, s.W1.shape
    f32 = dict(dtype=torch.float32, device=dev)
    has_Y = s.pm is not None
    pw1 = torch.empty(nparts, C1, 4, **f32)
    drel = torch.empty(B * N * S, 3, **f32) if need_xyz else None
    check(lib.spacap_sa_l1_bwd_f32(dy1.data_ptr(), s.z1.data_ptr(), coef1.data_ptr(), *src, s.W1.data_ptr(), ld, rdiv, *dims,
                                   C1, pw1.data_ptr(), _ptr(drel), int(has_Y), st), "spacap_sa_l1_bwd_f32")
    ws = dpm = dxyz = dnew = None
    nbytes = int(lib.spacap_sa_rows_scatter_workspace_bytes(B, Np, N * S))
    if ri is not None and not (ri.numel() == nbytes and ri.device == dev):
        ri = None
    if has_Y:
        dY = torch.empty(B, Np, C1, **f32)
        if ri is not None:
            # the inverted index came with the geometry pyramid: only the gather is left
            check(lib.spacap_sa_rows_gather_f32(dy1.data_ptr(), B, Np, N * S, C1, ri.data_ptr(), dY.data_ptr(), st),
                  "spacap_sa_rows_gather_f32")
        else:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            check(lib.spacap_sa_rows_scatter_f32(dy1.data_ptr(), s.idx.data_ptr(), B, Np, N * S, C1, dY.data_ptr(),
                                                 ws.data_ptr(), st), "spacap_sa_rows_scatter_f32")
        # gradient of Y = pm W1[:, 3:]^T: d pm = dY W1[:, 3:]; the weight part reduces over all B*Np source points
        Cf = ld - 3
        g2, x2 = dY.view(-1, C1), _rows2d(s.pm)
        if want[2]:
            from .linear import dense_product
            dpm = dense_product(g2, s.W1, False, col0=3).view_as(s.pm)    # dY W1[:, 3:]
        # [rel columns | feature columns] from the two sets of partial results in one launch (the values of the two
        # slab sums + the concatenation).  Feature partials: the Linear layers' slab kernel for multiples of 128
        # channels (SA2 - SA4), else the tall-and-narrow kernel (SA1 with 7 / 132 feature channels: cfg3, cfg4)
        nslab = int(lib.spacap_linear_wgrad_slabs(B * Np, C1, Cf))
        if nslab:
            x2c = x2.contiguous()
            pf = torch.empty(nslab, C1 * Cf, **f32)
            check(lib.spacap_linear_wgrad_f32(g2.data_ptr(), x2c.data_ptr(), B * Np, C1, Cf, 0, pf.data_ptr(), st),
                  "spacap_linear_wgrad_f32")
        else:   # (reads the rows at their own stride)
            nslab = int(lib.spacap_dense_wgrad_tall_slabs(B * Np, C1, Cf))
            pf = torch.empty(nslab, C1 * Cf, **f32)
            check(lib.spacap_dense_wgrad_tall_f32(g2.data_ptr(), C1, x2.data_ptr(), x2.stride(0), B * Np, C1, Cf, nslab,
                                                  pf.data_ptr(), st), "spacap_dense_wgrad_tall_f32")
        dW1 = torch.empty(C1, 3 + Cf, **f32)
        check(lib.spacap_sa_dw1_assemble_f32(pw1.data_ptr(), nparts, pf.data_ptr(), nslab, C1, Cf, dW1.data_ptr(), st),
              "spacap_sa_dw1_assemble_f32")
    else:
        dW1 = sum_slabs(pw1)[:, :ld].contiguous()    # (C1, 4): rel x, y, z, inline feature
    if drel is not None:
        # gradient of rel = (xyz[idx] - new_xyz) / r to both sources, one launch, fixed summation orders
        want_x, want_n = want[0], want[1]
        if want_x and ri is None and ws is None:
            ws = rows_index(s.idx, Np)
        index = ri if ri is not None else ws
        dxyz = torch.empty(B, Np, 3, **f32) if want_x else None
        dnew = torch.empty(B, N, 3, **f32) if want_n else None
        if want_x or want_n:
            check(lib.spacap_sa_drel_sums_f32(drel.data_ptr(), B, Np, N, S, _ptr(index) if want_x else None, _ptr(dxyz), _ptr(dnew),
                                              st), "spacap_sa_drel_sums_f32")
    return dW1, dpm, dxyz, dnew


class _SAMLP(Function):
    """inputs: xyz (B,Np,3), new_xyz (B,N,3), idx (B,N,S) int32, feat (B,Np) or None [inline 1-channel feature],
    pm (B,Np,Cf) or None [point-major features of the source points: the first layer commutes with the gather, so
    Y = pm W1[:, 3:]^T is formed once per SOURCE point], W1 (C1, 3 + Cf) the FULL first-layer weight (the kernels read
    its first 3 / 4 columns through the row stride), W2 (C2,C1), W3 (C3,C2), gamma/beta x3, then the three BatchNorm
    modules (running statistics are updated in place) and rdiv.  output: (B,N,C3) pooled features.
    One node for the whole module: W1's gradient is assembled once ([xyz columns | feature columns])."""

    @staticmethod
    def forward(ctx, xyz, new_xyz, idx, feat, pm, W1, W2, W3, g1, b1, g2, b2, g3, b3, bns, rdiv, rows_index=None):
        dev = xyz.device
        _selftest(dev)
        B, Np, _ = xyz.shape
        N, S = idx.shape[1], idx.shape[2]
        R, G, dims, rdiv = B * N * S, B * N, (B, Np, N, S), float(rdiv)
        st = torch.cuda.current_stream(dev).cuda_stream
        f32 = dict(dtype=torch.float32, device=dev)
        xyz, new_xyz, idx = xyz.contiguous(), new_xyz.contiguous(), idx.contiguous()
        W = [W1.contiguous(), W2.contiguous(), W3.contiguous()]
        C = [w.shape[0] for w in W]
        norm = [(bns[0], g1, b1), (bns[1], g2, b2), (bns[2], g3, b3)]
        feat = feat.contiguous() if feat is not None else None
        src, has_feat = (_ptr(feat), xyz.data_ptr(), new_xyz.data_ptr(), idx.data_ptr()), int(feat is not None)
        # first layer commuted with the gather: Y = F W1[:, 3:]^T over the SOURCE points (csrc/dense_rows.hip reads the column
        # slice of W1 in place)
        # (rows of Cf contiguous floats at a uniform stride are read in place: the input features of a (B, N, 3 + C) cloud are a
        # column window of its rows -- no transposed / gathered copy of the 170 MB feature block of BASELINE config 4)
        pmc = pm if (pm is None or _uniform_rows(pm)) else pm.contiguous()
        Y = _feature_product(pmc, W[0]) if pm is not None else None
        need_xyz = xyz.requires_grad or new_xyz.requires_grad
        p = plan(*C, S, R, pm is not None, need_xyz)
        nparts = int(lib.spacap_sa_nparts())
        with torch.cuda.device(dev):
            part = torch.empty(nparts * 2 * max(C), dtype=torch.float64, device=dev)
            stats = [torch.empty(c, 4, **f32) for c in C]
            z = [torch.empty(R, C[0] if p.first == "stored" else 4, **f32), torch.empty(R, C[1], **f32), torch.empty(R, C[2], **f32)]
            zmax = torch.empty(B, N, C[2], **f32) if p.tail == "candidates" else None
            _layer1(p.first, Y, src, W[0], has_feat, rdiv, dims, R, nparts, z[0], part, norm[0], stats[0], st)
            _layer(1, z, W, stats, R, part, norm[1], st, l1in=None if p.first == "stored" else (W[0].shape[1], has_feat))
            out = torch.empty(B, N, C[2], **f32)
            arg = torch.empty(B, N, C[2], dtype=torch.uint8, device=dev)
            if p.tail == "candidates":
                _layer3_candidates(z, W, stats, R, G, S, part, norm[2], out, arg, zmax, st)
            else:
                _layer(2, z, W, stats, R, part, norm[2], st)
                _pool(z[2], stats[2], G, S, out, arg, st)
        from . import selections
        if selections.HOOK is not None:    # tests only: see selections.py
            selections.visit("sa", gammas=[g1, g2, g3], zs=[z[0] if p.first == "stored" else None, z[1], z[2]], stats=stats, arg=arg,
                             out=out, zmax=zmax, dims=(B, N, S))
        ctx.save_for_backward(*Saved(xyz, new_xyz, idx, feat, pmc, *W, *z, *stats, out, arg, zmax))
        ctx.plan, ctx.rdiv, ctx.need_xyz = p, rdiv, need_xyz
        ctx.rows_index = rows_index   # prebuilt inverted index of idx (rows_index(idx, Np)), or None
        return out

    @staticmethod
    def backward(ctx, dout):
        s, p = Saved(*ctx.saved_tensors), ctx.plan
        dev = s.xyz.device
        B, Np, _ = s.xyz.shape
        N, S = s.idx.shape[1], s.idx.shape[2]
        C = [s.W1.shape[0], s.W2.shape[0], s.W3.shape[0]]
        R, G, dims = B * N * S, B * N, (B, Np, N, S)
        st = torch.cuda.current_stream(dev).cuda_stream
        f32 = dict(dtype=torch.float32, device=dev)
        dout = dout.contiguous()
        src, has_feat = (_ptr(s.feat), s.xyz.data_ptr(), s.new_xyz.data_ptr(), s.idx.data_ptr()), int(s.feat is not None)
        nparts = int(lib.spacap_sa_nparts())
        with torch.cuda.device(dev):
            part = torch.empty(nparts * 2 * max(C), dtype=torch.float64, device=dev)
            coef = [torch.empty(c, 4, **f32) for c in C]
            dg = [torch.empty(c, **f32) for c in C]
            db = [torch.empty(c, **f32) for c in C]

            def finalize(k, stats):   # coef[k] (the rows of dz = g dy + k0 - k1 z), dgamma, dbeta from the sums a kernel left in part
                check(lib.spacap_sa_bwd_finalize_f32(part.data_ptr(), C[k], R, stats.data_ptr(), coef[k].data_ptr(),
                                                     dg[k].data_ptr(), db[k].data_ptr(), st), "spacap_sa_bwd_finalize_f32")

            # pooled layer: masked gradient + BN sums over the arg-max rows
            dym = torch.empty(G, C[2], **f32)
            check(lib.spacap_sa_pool_bwd_f32(dout.data_ptr(), s.out.data_ptr(), s.arg.data_ptr(), s.z3.data_ptr(), _ptr(s.zmax),
                                             s.st3.data_ptr(), G, S, C[2], dym.data_ptr(), part.data_ptr(), st), "spacap_sa_pool_bwd_f32")
            finalize(2, s.st3)
            dy2 = torch.empty(R, C[1], **f32)
            # layer 3: weight gradient, then data gradient (its epilogue produces layer 2's BN sums)
            if p.l3_wgrad == "z2":
                dW3 = _wgrad_z2(dym, s, S, coef[2], R, st)
            else:
                dW3 = _wgrad(dym, s.arg, S, s.z3, coef[2], s.W3, s.z2, s.st2, R, st)
            _dgrad(dym, s.arg, S, s.z3, coef[2], s.W3, s.z2, s.st2, R, dy2, part, st)
            finalize(1, s.st2)
            dpm = dxyz = dnew = None
            if p.l2_l1 == "generic":
                dW2 = _wgrad(dy2, None, 0, s.z2, coef[1], s.W2, s.z1, s.st1, R, st)
                dy1 = torch.empty(R, C[0], **f32)
                _dgrad(dy2, None, 0, s.z2, coef[1], s.W2, s.z1, s.st1, R, dy1, part, st)
                del dy2
                finalize(0, s.st1)
                dW1, dpm, dxyz, dnew = _l1_generic(dy1, s, coef[0], src, ctx.rdiv, dims, nparts, ctx.rows_index, ctx.need_xyz,
                                                   (ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[4]), st)
            else:
                dW2, pl1 = _l2_l1_sums(p.l2_l1, dy2, s, coef[1], src, has_feat, ctx.rdiv, dims, R, nparts, part, st)
                del dy2
                finalize(0, s.st1)
                dW1 = torch.empty(s.W1.shape, **f32)     # = g S1 + k0 S2 - k1 S3 from the kernel's three sums, one launch
                check(lib.spacap_sa_l1_dw_f32(pl1.data_ptr(), nparts, coef[0].data_ptr(), C[0], s.W1.shape[1], dW1.data_ptr(), st),
                      "spacap_sa_l1_dw_f32")
        return (dxyz, dnew, None, None, dpm, dW1, dW2, dW3, dg[0], db[0], dg[1], db[1], dg[2], db[2], None, None, None)


def _uniform_rows(pm):
    """(B, Np, Cf) whose B * Np rows of Cf contiguous floats lie at ONE uniform stride (dense, or a column window of wider rows)."""
    return pm.stride(2) == 1 and pm.stride(0) == pm.shape[1] * pm.stride(1) and pm.data_ptr() % 4 == 0


def _rows2d(pm):
    """The (B * Np, Cf) view of a ``_uniform_rows`` tensor (row stride pm.stride(1))."""
    B, Np, Cf = pm.shape
    return pm.as_strided((B * Np, Cf), (pm.stride(1), 1), pm.storage_offset())


def _feature_product(pm, W1c):
    """Y (B, Np, C1) = pm (B, Np, Cf) W1[:, 3:]^T."""
    from .linear import dense_product
    B, Np, Cf = pm.shape
    return dense_product(_rows2d(pm), W1c, True, col0=3).view(B, Np, W1c.shape[0])


def supported(mlp_module, nsample):
    layers = list(mlp_module.children())
    if len(layers) != 3 or not all(getattr(l, "has_bn", False) for l in layers):
        return False
    if any(l.bn.bn.momentum is None for l in layers):
        return False   # cumulative-average running statistics need the batch count on the host: per-operator path
    c = [l.conv.out_channels for l in layers]
    return bool(lib.spacap_sa_mlp_supported(*c)) and 1 <= nsample <= 255


def rows_index(idx, Np):
    """Inverted index of a grouping idx (B,N,S) over Np source points (which grouped rows reference each point, in
    ascending row order) as an opaque uint8 tensor: what the feature-gradient gather of the fused SA op needs.  It
    depends on idx only, so a trainer can build it ahead of the step (detector.geometry_pyramid)."""
    B, N, S = idx.shape
    with torch.cuda.device(idx.device):
        ws = torch.empty(int(lib.spacap_sa_rows_scatter_workspace_bytes(B, Np, N * S)), dtype=torch.uint8, device=idx.device)
        check(lib.spacap_sa_rows_index_f32(idx.data_ptr(), B, Np, N * S, ws.data_ptr(),
                                           torch.cuda.current_stream(idx.device).cuda_stream), "spacap_sa_rows_index_f32")
    return ws


def _operands(mlp_module, features, inline):
    """([W1, W2, W3] as matrices, the three BatchNorm modules, feat, pm) of a module call on features (B,Cf,Np) or None: one
    feature channel is read by the kernels themselves where ``inline`` allows (feat (B,Np): no (B,Np,C1) product needed),
    anything else goes in point-major (pm (B,Np,Cf)): the first layer commutes with the gather, multiply once per source point."""
    layers = list(mlp_module.children())
    W = [l.conv.weight.view(l.conv.out_channels, -1) for l in layers]
    assert (features.shape[1] if features is not None else 0) == W[0].shape[1] - 3
    feat = pm = None
    if features is not None and features.shape[1] == 1 and inline:
        feat = features.reshape(features.shape[0], -1)
    elif features is not None:
        pm = point_major_of(features)   # (B,Np,Cf) form of a previous module's output, if any
        pm = pm if pm is not None else features.transpose(1, 2)
    return W, [l.bn.bn for l in layers], feat, pm


def sa_mlp_train(xyz, new_xyz, features, idx, mlp_module, rdiv, use_xyz=True, rows_idx=None):
    """xyz (B,Np,3), new_xyz (B,N,3), features (B,Cf,Np) or None, idx (B,N,S) -> (B,C3,N) [a ``layout.ChannelMajorOf``: the transposed view of the point-major (B,N,C3) result].  ``mlp_module``: the SharedMLP whose parameters / BatchNorm statistics are used and
    updated.  Returns None when this MLP has no fused kernels (the caller then uses the per-operator path)."""
    if not use_xyz or not xyz.is_cuda or not supported(mlp_module, idx.shape[2]):
        return None
    W, bns, feat, pm = _operands(mlp_module, features, inline=features is None or not features.requires_grad)
    out = _SAMLP.apply(xyz, new_xyz, idx, feat, pm, *W, bns[0].weight, bns[0].bias, bns[1].weight, bns[1].bias, bns[2].weight,
                       bns[2].bias, bns, rdiv, rows_idx)
    # (B,C3,N) as a transposed VIEW of the point-major result, typed (layout.ChannelMajorOf): the next SA module and the
    # proposal head ask for the point-major tensor itself, so no transposed copy is made unless a consumer needs one
    return ChannelMajorOf.wrap(out)


def _running_stats_rows(bn):
    """stats rows (mean, 1/std, gamma/std, beta) of a BatchNorm layer in inference mode: running statistics."""
    istd = torch.rsqrt(bn.running_var + bn.eps)
    return torch.stack([bn.running_mean, istd, bn.weight * istd, bn.bias], 1).contiguous()


@torch.no_grad()
def sa_mlp_eval(xyz, new_xyz, features, idx, mlp_module, rdiv, use_xyz=True):
    """Inference-mode counterpart of ``sa_mlp_train``: the same fused point-major kernels with the BatchNorm layers
    folded to their running statistics (what ``model.eval()`` computes per operator: QueryAndGroup -> [Conv2d 1x1 ->
    BatchNorm2d(running stats) -> ReLU] x 3 -> max_pool2d, lib/pointnet2/pointnet2_modules.py:241-259) -- no grouped
    (B, C+3, P, S) tensor, no statistics passes.  Returns (B, C3, N) or None when the shape has no fused kernels."""
    if not use_xyz or not xyz.is_cuda or not supported(mlp_module, idx.shape[2]):
        return None
    W, bns, feat, pm = _operands(mlp_module, features, inline=True)
    if any(not b.track_running_stats or b.running_mean is None for b in bns):
        return None
    dev = xyz.device
    B, Np, _ = xyz.shape
    N, S = idx.shape[1], idx.shape[2]
    W = [w.contiguous() for w in W]
    C1, C2, C3 = (w.shape[0] for w in W)
    feat, Y = feat.contiguous() if feat is not None else None, None
    if pm is not None:   # (the product over the source points holds the feature columns: the kernel gets the coordinate columns alone)
        Y = _feature_product(pm if _uniform_rows(pm) else pm.contiguous(), W[0])
        W[0] = W[0][:, :3].contiguous()
    R, G, dims = B * N * S, B * N, (B, Np, N, S)
    st = torch.cuda.current_stream(dev).cuda_stream
    f32 = dict(dtype=torch.float32, device=dev)
    xyz, new_xyz, idx = xyz.contiguous(), new_xyz.contiguous(), idx.contiguous()
    src = (_ptr(feat), xyz.data_ptr(), new_xyz.data_ptr(), idx.data_ptr())
    with torch.cuda.device(dev):
        # the "stored" / "plain" passes of the training forward, norm = None: the statistics rows are final, the sums in part ignored
        part = torch.empty(int(lib.spacap_sa_nparts()) * 2 * max(C1, C2, C3), dtype=torch.float64, device=dev)
        stats = [_running_stats_rows(b) for b in bns]
        z = [torch.empty(R, C1, **f32), None, None]
        _layer1("stored", Y, src, W[0], None, float(rdiv), dims, R, None, z[0], part, None, stats[0], st)
        z[1] = torch.empty(R, C2, **f32)
        _layer(1, z, W, stats, R, part, None, st)
        z[0] = None                   # (each pre-activation is freed as soon as the next layer has read it)
        z[2] = torch.empty(R, C3, **f32)
        _layer(2, z, W, stats, R, part, None, st)
        z[1] = None
        out = torch.empty(B, N, C3, **f32)
        arg = torch.empty(B, N, C3, dtype=torch.uint8, device=dev)
        _pool(z[2], stats[2], G, S, out, arg, st)
    return ChannelMajorOf.wrap(out)
