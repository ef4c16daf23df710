"""Small fused operators of the step's glue against their PyTorch compositions (the specification):
the caption head's log-softmax + masked cross entropy + accuracy (models/transformer_captioner.py:93-99,
lib/loss_helper.py:199-238) and the row-wise L2 normalisation of the vote features (models/SpaCapNet.py:66-67)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _reference_cap(logits, lang_ids, good):
    lang_cap = F.log_softmax(logits, dim=-1)
    from spacap3d_amd.loss_helper import compute_cap_loss
    loss, acc = compute_cap_loss({"lang_cap": lang_cap, "lang_ids": lang_ids, "good_bbox_masks": good})
    return lang_cap, loss, acc


@pytest.mark.parametrize("B,W,V", [(8, 31, 3001), (2, 31, 40), (3, 7, 513)])
@pytest.mark.parametrize("good_pattern", ["all", "some", "none"])
def test_caption_head_loss_matches_the_composition(B, W, V, good_pattern):
    from spacap3d_amd.fused_losses import caption_head_loss
    g = torch.Generator().manual_seed(B * W + V)
    logits = (torch.randn(B, W, V, generator=g) * 3).to(DEV)
    ids = torch.zeros(B, W + 2, dtype=torch.long)
    for b in range(B):
        n = int(torch.randint(3, W + 1, (1,), generator=g))
        ids[b, 0] = 2
        ids[b, 1:1 + n] = torch.randint(1, V, (n,), generator=g)     # word ids, 0 = pad beyond the caption
    ids = ids.to(DEV)
    good = {"all": torch.ones(B, dtype=torch.bool), "some": torch.arange(B) % 2 == 0, "none": torch.zeros(B, dtype=torch.bool)}[good_pattern].to(DEV)
    # make one row's arg-max the target and plant an exact tie to pin the first-maximum rule
    logits[0, 0, int(ids[0, 1])] = 50.0
    logits[0, 1, 5] = logits[0, 1, 9] = 60.0
    la = logits.clone().requires_grad_(True)
    lb = logits.clone().requires_grad_(True)
    cap_a, loss_a, acc_a, vec_a = caption_head_loss(la, ids, good)
    assert vec_a.shape == (4,) and float(vec_a[0]) == float(loss_a)
    cap_b, loss_b, acc_b = _reference_cap(lb, ids, good)
    assert float((cap_a - cap_b).abs().max()) < 2e-5
    assert abs(float(loss_a) - float(loss_b)) <= 1e-5 * max(1.0, abs(float(loss_b)))
    assert abs(float(acc_a) - float(acc_b)) < 1e-6
    (loss_a * 1.7).backward()
    (loss_b * 1.7).backward()
    scale = float(lb.grad.abs().max()) + 1e-12
    assert float((la.grad - lb.grad).abs().max()) <= 2e-6 * max(scale, 1e-6) + 1e-9
    assert not cap_a.requires_grad


@pytest.mark.parametrize("shape", [(8, 1024, 256), (2, 64, 128), (1, 5, 4)])
def test_l2norm_rows_matches_div_by_norm(shape):
    from spacap3d_amd.fused_losses import l2norm_rows
    x = torch.randn(*shape, device=DEV) * 3
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    ya = l2norm_rows(a)
    yb = b.div(torch.norm(b, p=2, dim=-1).unsqueeze(-1))
    assert float((ya - yb).abs().max()) < 2e-7
    w = torch.randn_like(x)
    (ya * w).sum().backward()
    (yb * w).sum().backward()
    assert float((a.grad - b.grad).abs().max()) <= 2e-6 * float(b.grad.abs().max())


def test_loss_tail_matches_the_composition():
    """fused_losses.LossTail (one launch each way) against lib/loss_helper.py:340-383 composed from scalar ops."""
    from spacap3d_amd.fused_losses import loss_tail
    g = torch.Generator().manual_seed(3)
    det = torch.rand(8, generator=g).to(DEV).requires_grad_()
    cap = torch.rand(4, generator=g).to(DEV).requires_grad_()
    rel = torch.rand(7, generator=g).to(DEV).requires_grad_()
    n = 8 * 256
    label = (torch.rand(n, generator=g) > 0.7).long().to(DEV)
    mask = (torch.rand(n, generator=g) > 0.4).float().to(DEV)
    bbox = (torch.rand(n, generator=g) > 0.5).long().to(DEV)
    loss, out = loss_tail(det, cap, rel, label.view(8, 256), mask.view(8, 256), bbox.view(8, 256))
    (loss * 1.3).backward()
    d6, c6, r6 = (t.detach().double().requires_grad_() for t in (det, cap, rel))
    box = d6[2] + 0.1 * d6[3] + d6[4] + 0.1 * d6[5] + d6[6]
    dl = d6[0] + 0.5 * d6[1] + box + 0.1 * d6[7]
    rl = r6[0] + r6[1] + r6[2]
    want = 10 * dl + c6[0] + 0.1 * rl
    (want * 1.3).backward()
    pos = label.double().sum() / n
    ref = [box, dl, rl, want, pos, mask.double().sum() / n - pos, ((bbox == label).double() * mask.double()).sum() / (mask.double().sum() + 1e-6)]
    for i, w in enumerate(ref):
        assert abs(float(out[i]) - float(w)) < 1e-5 * max(1.0, abs(float(w))), i
    assert float(loss) == float(out[3]) and not out.requires_grad
    for a, b in ((det, d6), (cap, c6), (rel, r6)):
        assert float((a.grad.double() - b.grad).abs().max()) < 1e-6


@pytest.mark.parametrize("B,K,NH", [(8, 256, 1), (2, 70, 1), (1, 64, 12)])
def test_proposal_decode_matches_the_composition(B, K, NH):
    """fused_losses.ProposalDecode against ProposalModule.decode_scores / decode_pred_box composed from torch ops (the
    specification: models/proposal_module.py:81-158), values exact and every gradient."""
    import math
    from spacap3d_amd import synthetic as S
    from spacap3d_amd.fused_losses import proposal_decode
    NS, NC = 18, 18
    CH = 5 + 2 * NH + 4 * NS + NC
    g = torch.Generator().manual_seed(B * K)
    net0 = torch.randn(B, CH, K, generator=g).to(DEV)
    net0[0, 5 + 2 * NH + 3, 0] = net0[0, 5 + 2 * NH + 7, 0] = 9.0      # an exact tie among the size scores: first maximum
    agg0 = torch.randn(B, K, 3, generator=g).to(DEV)
    msa64 = S.mean_size_arr().double().to(DEV)
    msa = msa64.float()
    na, aa = net0.clone().requires_grad_(), agg0.clone().requires_grad_()
    nt, center, hres, sres, corners, bmask, sem, scls = proposal_decode(na, aa, msa, msa64, NH, NS)
    nb, ab = net0.clone().requires_grad_(), agg0.clone().requires_grad_()
    ntb = nb.transpose(2, 1).contiguous()
    cb = ab + ntb[:, :, 2:5]
    hb = ntb[:, :, 5 + NH:5 + 2 * NH] * (math.pi / NH)
    sb = ntb[:, :, 5 + 2 * NH + NS:5 + 2 * NH + 4 * NS].view(B, K, NS, 3) * msa
    clsb = torch.argmax(ntb[:, :, 5 + 2 * NH:5 + 2 * NH + NS], -1)
    signs = torch.tensor([[1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1], [1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1]],
                         dtype=torch.float64, device=DEV)
    size_res = torch.gather(sb.detach(), 2, clsb.unsqueeze(-1).unsqueeze(-1).expand(-1, -1, 1, 3)).squeeze(2)
    cornb = cb.detach().double().unsqueeze(2) + signs * ((msa64[clsb] + size_res.double()) / 2).unsqueeze(2)
    assert torch.equal(nt, ntb) and torch.equal(center, cb) and torch.equal(hres, hb) and torch.equal(sres, sb)
    assert torch.equal(scls, clsb) and torch.equal(bmask, ntb[:, :, 0:2].argmax(-1)) and torch.equal(sem, ntb[:, :, 5 + 2 * NH + 4 * NS:].argmax(-1))
    assert torch.equal(corners, cornb)
    w = [torch.randn_like(t) for t in (nt, center, hres, sres)]
    (nt * w[0]).sum().add((center * w[1]).sum()).add((hres * w[2]).sum()).add((sres * w[3]).sum()).backward()
    (ntb * w[0]).sum().add((cb * w[1]).sum()).add((hb * w[2]).sum()).add((sb * w[3]).sum()).backward()
    assert float((na.grad - nb.grad).abs().max()) <= 1e-6 * float(nb.grad.abs().max())
    assert torch.equal(aa.grad, ab.grad)


@pytest.mark.parametrize("B,C,N", [(8, 256, 1024), (2, 100, 77), (1, 256, 33)])
def test_vote_assemble_matches_the_tensor_operations(B, C, N):
    """fused_losses.vote_assemble (csrc/proposal_decode.hip) against the voting module's own lines (models/voting_module.py:49-60):
    vote_xyz and the point-major vote features bit for bit, and the gradients of the convolution output and of the seed
    features (exact: every element has one contribution)."""
    from spacap3d_amd.fused_losses import vote_assemble
    g = torch.Generator().manual_seed(B + C + N)
    net = torch.randn(B, 3 + C, N, generator=g).to(DEV)
    sx = torch.randn(B, N, 3, generator=g).to(DEV)
    sf = torch.randn(B, C, N, generator=g).to(DEV)
    wx, wf = torch.randn(B, N, 3, generator=g).to(DEV), torch.randn(B, N, C, generator=g).to(DEV)
    na, fa = net.clone().requires_grad_(True), sf.clone().requires_grad_(True)
    t = na.transpose(2, 1).view(B, N, 1, 3 + C)
    want_x = (sx.unsqueeze(2) + t[:, :, :, 0:3]).contiguous().view(B, N, 3)
    want_f = (fa.transpose(2, 1).unsqueeze(2) + t[:, :, :, 3:]).contiguous().view(B, N, C)
    ((want_x * wx).sum() + (want_f * wf).sum()).backward()
    nb, fb = net.clone().requires_grad_(True), sf.clone().requires_grad_(True)
    got_x, got_f = vote_assemble(nb, sx, fb)
    assert torch.equal(got_x, want_x) and torch.equal(got_f, want_f)
    ((got_x * wx).sum() + (got_f * wf).sum()).backward()
    assert torch.equal(nb.grad, na.grad) and torch.equal(fb.grad, fa.grad)
    # only one of the two outputs used
    nc = net.clone().requires_grad_(True)
    (vote_assemble(nc, sx, sf)[1] * wf).sum().backward()
    assert torch.equal(nc.grad[:, 3:], na.grad[:, 3:]) and float(nc.grad[:, :3].abs().max()) == 0.0


def test_copy_batched_moves_every_tensor_in_one_launch():
    """_native.copy_batched (csrc/elementwise.hip): ~200 tensors of four dtypes, sizes from 0 to a few MB incl. byte counts
    that are not multiples of 16 and unaligned views -- every destination equals its source, nothing around it is touched."""
    from spacap3d_amd._native import copy_batched
    g = torch.Generator().manual_seed(0)
    srcs, dsts, guards = [], [], []
    for i in range(200):
        n = int(torch.randint(0, 3000, (1,), generator=g)) if i % 7 else int(torch.randint(100000, 700000, (1,), generator=g))
        dt = (torch.float32, torch.int64, torch.int32, torch.uint8)[i % 4]
        src = (torch.rand(n + 3, generator=g) * 100).to(dt).to(DEV)[1:n + 1] if i % 5 == 0 else (torch.rand(n, generator=g) * 100).to(dt).to(DEV)
        buf = torch.full((n + 8,), 7, dtype=dt, device=DEV)
        srcs.append(src.contiguous() if i % 5 else src)
        dsts.append(buf[4:4 + n])
        guards.append(buf)
    copy_batched(dsts, srcs)
    for d, s_, b in zip(dsts, srcs, guards):
        assert torch.equal(d, s_)
        assert bool((b[:4] == 7).all()) and bool((b[-4:] == 7).all())
    # shapes that do not match fall back to the library copy (broadcast)
    a, bsrc = torch.zeros(4, 3, device=DEV), torch.ones(3, device=DEV)
    copy_batched([a], [bsrc.expand(4, 3)])
    assert bool((a == 1).all())



@pytest.mark.parametrize("B,m,n,K1,K2,known_pm", [(8, 256, 512, 256, 256, True), (8, 512, 1024, 256, 256, False), (2, 37, 61, 64, 7, True),
                                                  (3, 5, 33, 32, 40, False)])
def test_feature_propagation_input_in_one_launch_each_way(B, m, n, K1, K2, known_pm):
    """FPConcat (csrc/interpolate.hip: fp_concat_*) = torch.cat([three_interpolate(known, idx, weight), skip], 1) of
    PointnetFPModule.forward (lib/pointnet2/pointnet2_modules.py:406-412): identical values (the three products are added in the
    operator's order), gradients of both inputs against the composition of the separate operators."""
    from spacap3d_amd import pointnet2_utils as pu
    from spacap3d_amd.layout import ChannelMajorOf
    g = torch.Generator().manual_seed(B * n + K2)
    known_pm_t = torch.randn(B, m, K1, generator=g).to(DEV)
    skip_pm_t = torch.randn(B, n, K2, generator=g).to(DEV)
    idx = torch.randint(0, m, (B, n, 3), generator=g, dtype=torch.int32).to(DEV)
    w = torch.rand(B, n, 3, generator=g).to(DEV)
    w = (w / w.sum(-1, keepdim=True)).contiguous()
    go = torch.randn(B, K1 + K2, n, generator=g).to(DEV)
    # fused
    a1, s1 = known_pm_t.clone().requires_grad_(True), skip_pm_t.clone().requires_grad_(True)
    known_arg = a1 if known_pm else a1.transpose(1, 2).contiguous()      # channel-major (B, K1, m) input in the second mode
    if not known_pm:
        known_arg = known_arg.detach().requires_grad_(True)
    out = pu.FPConcat.apply(known_arg, idx, w, s1, known_pm)
    out.backward(go)
    # composition of the separate operators
    kc = known_pm_t.transpose(1, 2).contiguous().requires_grad_(True)    # (B, K1, m)
    sc = skip_pm_t.transpose(1, 2).contiguous().requires_grad_(True)     # (B, K2, n)
    ref = torch.cat([pu.three_interpolate(kc, idx, w), sc], dim=1)
    ref.backward(go)
    assert torch.equal(out, ref)
    dk = known_arg.grad if not known_pm else a1.grad.transpose(1, 2)
    assert float((dk - kc.grad).abs().max()) <= 1e-5 * float(kc.grad.abs().max())
    assert torch.equal(s1.grad.transpose(1, 2), sc.grad)


@pytest.mark.parametrize("shape", [(8, 256, 1024), (8, 128, 256, 1), (3, 128, 96)])
def test_inference_batchnorm_relu_on_the_running_statistics(shape):
    """fused_bn.bn_relu_eval: relu(bn(z)) of a BatchNorm module in eval mode as one launch of the library's apply kernel
    (lib/pointnet2/pytorch_utils.py:11-36 and models/voting_module.py:28-61 under model.eval()), against the stock modules; the
    folded statistics follow the module's buffers (a training-mode update or load_state_dict invalidates the fold); with gradient
    recording on, or in training mode, the function declines."""
    from spacap3d_amd.fused_bn import bn_relu_eval
    g = torch.Generator().manual_seed(5)
    C = shape[1]
    bn = (torch.nn.BatchNorm2d(C) if len(shape) == 4 else torch.nn.BatchNorm1d(C)).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g)), bn.bias.copy_(torch.randn(C, generator=g))
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.3), bn.running_var.copy_(torch.rand(C, generator=g) + 0.2)
    z = torch.randn(*shape, generator=g).to(DEV)
    bn.eval()
    assert bn_relu_eval(z, bn) is None      # gradient recording on
    with torch.no_grad():
        want = torch.relu(bn(z))
        got = bn_relu_eval(z, bn)
        assert got is not None and float((got - want).abs().max()) < 2e-6 * max(1.0, float(want.abs().max()))
        assert bn_relu_eval(z, bn).equal(got)                 # from the cached fold
        bn.running_mean.add_(0.5)                             # the buffers move: a new fold
        want2 = torch.relu(bn(z))
        got2 = bn_relu_eval(z, bn)
        assert float((got2 - want2).abs().max()) < 2e-6 * max(1.0, float(want2.abs().max())) and not got2.equal(got)
        bn.train()
        assert bn_relu_eval(z, bn) is None


def test_inference_batchnorm_fold_is_not_shared_between_modules_that_reuse_memory():
    """Modules created and dropped one after the other reuse ids, buffer addresses and version numbers: every one must get the
    fold of ITS running statistics."""
    import gc
    from spacap3d_amd.fused_bn import bn_relu_eval
    g = torch.Generator().manual_seed(9)
    z = torch.randn(4, 64, 128, generator=g).to(DEV)
    for i in range(6):
        bn = torch.nn.BatchNorm1d(64).to(DEV)
        with torch.no_grad():
            bn.running_mean.copy_(torch.full((64,), 0.1 * i))      # same history (one in-place copy each), different values
            bn.running_var.copy_(torch.full((64,), 0.5 + 0.2 * i))
        bn.eval()
        with torch.no_grad():
            got, want = bn_relu_eval(z, bn), torch.relu(bn(z))
        assert float((got - want).abs().max()) < 2e-6 * max(1.0, float(want.abs().max())), i
        del bn
        gc.collect()
