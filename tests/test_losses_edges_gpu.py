"""The loss kernels of csrc/losses.hip at every edge of their dispatch, against the numpy restatement of
tests/losses_restated.py: ``fused_losses.DetectionLosses``, ``RelationLoss`` and ``CaptionHeadLoss`` called directly on the
synthetic tensors of its tables (no model, no backbone), and the C ABI itself for what the autograd ops hide (every output
element written, the refusals).

Integer outputs are compared with ``torch.equal`` on every element; values and gradients are held to the project's own bars
(tests/test_engine_gpu.py, tests/test_fused_small_gpu.py), here against float64 -- tests/test_losses_restated_cpu.py shows
that float32 done right uses a small share of each at these inputs, and that no input sits where one ulp of a device square
root could turn a comparison.  Where an element of a reference gradient is exactly zero the kernel's must be exactly zero.
Each comparison prints its figures before it asserts (``LOSSES-EDGES ...``, pytest -s)."""
import numpy as np
import pytest
import torch

import losses_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_name = lambda c: c.name if hasattr(c, "name") else "-".join(map(str, c))
_NAN = float("nan")


@pytest.fixture(scope="module")
def fl():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spacap3d_amd import fused_losses
    return fused_losses


def _dev(a):
    return torch.tensor(a).to(DEV)


def _cpu(t):
    return t.detach().cpu().numpy()


# ---- detection -------------------------------------------------------------------------------------------------------------
def _det_apply(fl, x):
    net, cen, vote = (_dev(a).requires_grad_(True) for a in (x.net, x.center, x.vote_xyz))
    losses, label, mask, oa = fl.DetectionLosses.apply(
        net, cen, vote, _dev(x.agg_xyz), _dev(x.gt_center), _dev(x.box_mask), _dev(x.heading_cls_label), _dev(x.heading_res_label),
        _dev(x.size_cls_label), _dev(x.size_res_label), _dev(x.sem_cls_label), _dev(x.mean_size), _dev(x.seed_xyz), _dev(x.seed_inds),
        _dev(x.vote_label), _dev(x.vote_mask), x.NH, x.NS, x.near, x.far, x.w0, x.w1)
    (losses * torch.tensor(R.DET_UPSTREAM, device=DEV)).sum().backward()
    return losses.detach(), label, mask, oa, net.grad, cen.grad, vote.grad


@pytest.mark.parametrize("case", R.DET_CASES, ids=_name)
def test_detection_losses_against_the_restatement(fl, case):
    x, want = R.detection_inputs(case), R.detection_reference(case)
    if case.name == "K-last-staged":
        # the largest K with 4 (12 M + 6 K + 3 NS + 4) + 4 K CH <= 150 * 1024 at M = 128, NS = 18, CH = 97 (the host code's
        # lds_staged): staged in LDS here, read from global memory one proposal further
        M, NS, CH = case.M, case.NS, x.net.shape[2]
        assert 4 * (12 * M + 6 * case.K + 3 * NS + 4) + 4 * case.K * CH <= 150 * 1024 < 4 * (12 * M + 6 * (case.K + 1) + 3 * NS + 4) + 4 * (case.K + 1) * CH
        assert R.DET_BY_NAME["K-first-unstaged"].K == case.K + 1 == 358
    losses, label, mask, oa, gnet, gcen, gvote = _det_apply(fl, x)
    ints = (torch.equal(label.cpu(), torch.tensor(want.obj_label)), torch.equal(mask.cpu(), torch.tensor(want.obj_mask)),
            torch.equal(oa.cpu(), torch.tensor(want.assignment)))
    got = {"losses": _cpu(losses), "dnet": _cpu(gnet), "dcenter": _cpu(gcen), "dvote": _cpu(gvote)}
    fig = {"losses": R.excess(got["losses"], want.losses, R.DET_LOSS_RTOL, R.DET_LOSS_ATOL)}
    fig.update({k: R.figure(got[k], getattr(want, k)) for k in ("dnet", "dcenter", "dvote")})
    print(f"LOSSES-EDGES det {case.name} label/mask/assignment equal={ints} losses (of the bar)={fig['losses']:.3f} "
          + " ".join(f"{k}={fig[k]:.2e}" for k in ("dnet", "dcenter", "dvote")))
    assert label.dtype == oa.dtype == torch.int64 and mask.dtype == torch.float32
    assert all(ints), ints
    assert fig["losses"] <= 1.0, (got["losses"], want.losses)
    for k in ("dnet", "dcenter", "dvote"):
        assert fig[k] < R.DET_GRAD_BAR, (k, fig)
        assert R.zero_where_reference_is(got[k], getattr(want, k)), k
    assert np.isfinite(got["losses"]).all()
    if case.kind == "none-near":      # n_obj = 0: the five losses over the positives are 0.0, not merely small
        assert (got["losses"][3:8] == 0.0).all() and (got["dnet"][..., 5:] == 0.0).all()
        assert (want.losses[3:8] == 0.0).all() and want.losses[2] > 0.0     # (the centre loss keeps its box -> proposal term)
    if case.kind == "all-grey":
        assert got["losses"][1] == 0.0 and (got["dnet"][..., 0:2] == 0.0).all() and float(mask.sum()) == 0.0
    if case.kind == "dup-proposals":  # the box -> proposal gradient of box 1 lands on proposal 4 alone
        assert not np.array_equal(got["dcenter"][:, 4], got["dcenter"][:, 9])
    if case.kind == "exact-thresholds":
        assert label[0, :2].tolist() == [0, 0] and mask[0, :2].tolist() == [0.0, 0.0]


def _det_capi(case, fill_f, fill_i, K=None, M=None):
    """spacap_det_losses_fwd_f32 on a row of the table, the output buffers pre-filled (K or M overridden for the refusals:
    buffers of that size with random contents, of which nothing is read)"""
    from spacap3d_amd._native import lib
    if K is None and M is None:
        x = R.detection_inputs(case)
        B, K, M = case.B, case.K, case.M
        t = [_dev(a) for a in (x.net, x.center, x.agg_xyz, x.gt_center, x.box_mask, x.heading_cls_label, x.heading_res_label,
                               x.size_cls_label, x.size_res_label, x.sem_cls_label, x.mean_size, x.seed_xyz, x.vote_xyz)]
        t += [_dev(x.seed_inds).to(torch.int32), _dev(x.vote_label), _dev(x.vote_mask)]
    else:
        B, K, M = case.B, K or case.K, M or case.M
        CH = 5 + 2 * case.NH + 4 * case.NS + case.NC
        f, i = lambda *s: torch.rand(*s, device=DEV), lambda *s: torch.zeros(*s, dtype=torch.int64, device=DEV)
        t = [f(B, K, CH), f(B, K, 3), f(B, K, 3), f(B, M, 3), f(B, M), i(B, M), f(B, M), i(B, M), f(B, M, 3), i(B, M),
             f(case.NS, 3) + 0.3, f(B, case.NSEED, 3), f(B, case.NSEED, 3), torch.zeros(B, case.NSEED, dtype=torch.int32, device=DEV),
             f(B, case.N, 9), i(B, case.N)]
    CH = t[0].shape[2]
    npart = int(lib.spacap_det_npart())
    ff = lambda *s: torch.full(s, fill_f, dtype=torch.float32, device=DEV)
    fi = lambda *s: torch.full(s, fill_i, dtype=torch.int64, device=DEV)
    out = {"obj_label": fi(B, K), "obj_mask": ff(B, K), "assignment": fi(B, K), "dnet_num": ff(B, K, CH), "dcenter_num": ff(B, K, 6),
           "dvote_num": ff(B, case.NSEED, 3), "part": ff(B * (npart + 2)), "losses": ff(8), "inv_den": ff(4)}
    rc = lib.spacap_det_losses_fwd_f32(*(a.data_ptr() for a in t), B, K, M, case.NSEED, case.N, case.NH, case.NS, case.NC,
                                       R.NEAR, R.FAR, R.OBJ_W[0], R.OBJ_W[1], *(o.data_ptr() for o in out.values()),
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out, t, npart


@pytest.mark.parametrize("name", ["K41", "K41-NC1000"])
def test_every_output_element_is_written(fl, name):
    """K CH odd: the scalar staging copy out of LDS (K41), and the rows written straight to global memory by the four lanes of a
    proposal (K41-NC1000).  Every float output starts as NaN.  Defined afterwards (csrc/losses.hip): all of dnet_num (B,K,CH),
    dcenter_num (B,K,6), dvote_num, obj_mask, losses (8) and inv_den (4); of part, slots 1..11 of each scene's 12 and the two
    vote sums per scene behind them -- slot 0 of a scene is never written nor read."""
    from spacap3d_amd._native import check
    case = R.DET_BY_NAME[name]
    assert R.staged(case.K, case.M, case.NH, case.NS, case.NC) == (name == "K41")
    rc, out, _, npart = _det_capi(case, _NAN, -7)
    check(rc, "spacap_det_losses_fwd_f32")
    part = out["part"].cpu()
    unused = torch.zeros(part.numel(), dtype=torch.bool)
    unused[torch.arange(case.B) * npart] = True
    left = {k: int(torch.isnan(v).sum()) for k, v in out.items() if v.dtype == torch.float32 and k != "part"}
    left["part (slots in use)"] = int(torch.isnan(part[~unused]).sum())
    print(f"LOSSES-EDGES written {name} NaN left: {left} part slot 0 still NaN: {int(torch.isnan(part[unused]).sum())}/{case.B}")
    assert npart == 12 and all(v == 0 for v in left.values()), left
    assert bool(torch.isnan(part[unused]).all())
    want = R.detection_reference(case)
    assert torch.equal(out["obj_label"].cpu(), torch.tensor(want.obj_label)) and torch.equal(out["assignment"].cpu(), torch.tensor(want.assignment))


@pytest.mark.parametrize("K,M,message", [(None, 257, "bad sizes"), (2400, 128, "too large")])
def test_sizes_without_a_kernel_are_refused_before_any_launch(fl, K, M, message):
    """M above MAXM = 256, and a K whose centres and vote positions alone exceed the 60 000 bytes of LDS the unstaged kernel may
    ask for: the library's error through check(), and every output buffer as it was filled."""
    from spacap3d_amd._native import check, lib
    assert M > 256 or R.lds_bytes(K, M, 18) > 60000
    rc, out, _, _ = _det_capi(R.DET_BY_NAME["K256"], 7.0, -7, K=K, M=M)
    print(f"LOSSES-EDGES refused K={K} M={M} rc={rc} error={lib.spacap_last_error()!r}")
    assert rc != 0
    with pytest.raises(RuntimeError, match=message):
        check(rc, "spacap_det_losses_fwd_f32")
    for k, v in out.items():
        assert bool((v == (7.0 if v.dtype == torch.float32 else -7)).all()), k


# ---- relation loss -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.REL_CASES, ids=_name)
def test_relation_loss_against_the_restatement(fl, case):
    x, want = R.relation_inputs(case), R.relation_reference(case)
    pred = _dev(x.pred).requires_grad_(True)
    out = fl.RelationLoss.apply(pred, _dev(x.assignment), _dev(x.box_mask_int), _dev(x.obj_label), _dev(x.x_label), _dev(x.y_label),
                                _dev(x.z_label))
    (out[0:3] * torch.tensor(R.REL_UPSTREAM, device=DEV)).sum().backward()
    got, grad = _cpu(out), _cpu(pred.grad)
    fig = (R.excess(got[:6], want.out[:6], R.REL_LOSS_RTOL, R.REL_LOSS_ATOL), R.excess(grad, want.dpred, R.REL_GRAD_RTOL, R.REL_GRAD_ATOL))
    print(f"LOSSES-EDGES rel {case.name} pairs={want.n_pairs} out (of the bar)={fig[0]:.3f} dpred (of the bar)={fig[1]:.3f} "
          f"1/n={got[6]!r}")
    assert fig[0] <= 1.0, (got, want.out)
    assert fig[1] <= 1.0
    assert got[6] == np.float32(1.0) / np.float32(max(want.n_pairs, 1))
    assert R.zero_where_reference_is(grad, want.dpred)
    if case.select == "none":
        assert (got[:6] == 0.0).all() and got[6] == 1.0 and (grad == 0.0).all()


# ---- caption head --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CAP_CASES, ids=_name)
def test_caption_head_against_the_restatement(fl, case):
    x, want = R.caption_inputs(case), R.caption_reference(case)
    logits = _dev(x.logits).requires_grad_(True)
    logp, out = fl.CaptionHeadLoss.apply(logits, _dev(x.lang_ids), _dev(x.good))
    (out[0] * R.CAP_UPSTREAM).backward()
    got_logp, got, grad = _cpu(logp), _cpu(out), _cpu(logits.grad)
    scale = max(float(np.abs(want.dlogits).max()), 1e-6)
    fig = {"logp": float(np.abs(got_logp - want.logp).max()) / R.CAP_LOGP_ABS,
           "loss": abs(float(got[0]) - want.loss) / (R.CAP_LOSS_REL * max(1.0, abs(want.loss))),
           "acc": abs(float(got[1]) - want.acc) / R.CAP_ACC_ABS,
           "dlogits": float(np.abs(grad - want.dlogits).max()) / (R.CAP_GRAD_REL * scale + R.CAP_GRAD_ABS)}
    print(f"LOSSES-EDGES cap {_name(case)} valid={want.n_valid} acc={float(got[1]):.6f} (of the bar) "
          + " ".join(f"{k}={v:.3f}" for k, v in fig.items()))
    assert not logp.requires_grad and np.isfinite(got_logp).all() and np.isfinite(grad).all()
    assert fig["logp"] < 1.0 and fig["loss"] <= 1.0 and fig["acc"] < 1.0 and fig["dlogits"] <= 1.0, fig
    assert R.zero_where_reference_is(grad, want.dlogits)
    assert float(got[3]) == float(x.good.sum() * case.W)
    if case.good == "none":
        assert float(got[0]) == 0.0 and float(got[1]) == 0.0 and (grad == 0.0).all()
