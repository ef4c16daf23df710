"""FlatAdam's grouped mode on the GPU (csrc/optim.hip): per-group lr / weight_decay, the float64
squared-norm pass, clipping by the global norm, the skipped (non-finite) update and torch-format state, against
``torch.optim.Adam`` with the same groups, ``clip_grad_norm_`` and the numpy restatement (tests/optim_restated.py)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import optim_restated as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(128, 128), (7,), (3, 5, 2), (2048, 128), (1,), (259, 128, 1, 1)]
GROUP_OF = [0, 1, 0, 1, 1, 0]
LRS, WDS = [1e-3, 5e-4], [1e-5, 1e-4]
RTOL, ATOL = 2e-6, 2e-7      # the project's Adam tolerance (tests/test_engine_gpu.py: FlatAdam against torch)
# Clipped runs use Adam's eps = 1e-3 (as this project's trajectory tests do).  torch forms the norm in float32, the kernel and
# the restatement in float64: the coefficients differ by an ulp, g*coef by ~1e-10, and where g*coef + wd*p cancels to ~1e-8 the
# first update lr * g' / (|g'| + eps) amplifies that by lr / eps = 1e5 at the default eps -- a property of eps, not of the code.
EPS_CLIP = 1e-3


def _make(seed=0, eps=1e-8, max_grad_norm=None, groups=True, one_group=False):
    """(pa, bucket, FlatAdam) and (pb, torch Adam) over the same values and the same two groups."""
    from spacap3d_amd.distributed import FlatGradBucket
    from spacap3d_amd.optim import FlatAdam
    g = torch.Generator().manual_seed(seed)
    pa = [torch.nn.Parameter(torch.randn(*s, generator=g).to(DEV)) for s in SHAPES]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]

    def dicts(ps):
        if one_group:
            return [{"params": list(ps)}]
        return [{"params": [p for p, k in zip(ps, GROUP_OF) if k == j], "lr": LRS[j], "weight_decay": WDS[j]} for j in range(2)]
    bucket = FlatGradBucket(pa, views=False)
    opt = FlatAdam(bucket, lr=LRS[0], weight_decay=WDS[0], eps=eps, groups=dicts(pa) if groups else None, max_grad_norm=max_grad_norm)
    ref = torch.optim.Adam(dicts(pb), lr=LRS[0], weight_decay=WDS[0], eps=eps)
    return pa, bucket, opt, pb, ref, g


def _grads(g, scale=1.0):
    return [torch.randn(*s, generator=g).to(DEV) * scale for s in SHAPES]


def _feed(ps, bucket, grads):
    for p, gr in zip(ps, grads):
        p.grad = gr.clone()
    if bucket is not None:
        bucket.pack()


def _scrub(*tensors):
    """Two tests below put NaN and 1e18 into device memory on purpose.  They zero it before it goes back to the caching
    allocator, which hands the same blocks to the next test's ``torch.empty``: what this module leaves behind is finite."""
    for t in tensors:
        t.detach().zero_()


def _opt_buffers(opt):
    return [opt.bucket.flat, opt.flat_p, opt.m, opt.v, opt._partials, opt.grad_sqnorm, opt._ctrl]


def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(float(a) - float(b)) / float(np.spacing(np.float32(max(abs(a), abs(b)))))


def test_grouped_rates_match_torch_adam_with_the_same_groups():
    pa, bucket, opt, pb, ref, g = _make()
    assert all(torch.equal(p, q) for p, q in zip(pa, pb))
    for step in range(5):
        grads = _grads(g, 10.0 ** (step - 2))
        _feed(pa, bucket, grads)
        _feed(pb, None, grads)
        opt.step()
        ref.step()
        for p, q in zip(pa, pb):
            assert torch.allclose(p, q, rtol=RTOL, atol=ATOL), (step, float((p - q).abs().max()))
        sq = R.sqnorms([x.cpu().numpy() for x in grads], GROUP_OF, 2)
        got = [float(x) for x in opt.group_grad_norm] + [float(opt.grad_norm)]
        assert all(_ulps(a, np.float32(np.sqrt(b))) <= 2 for a, b in zip(got, sq)), (got, np.sqrt(sq))
    assert float(opt.step_t) == 5 and int(opt.skipped_updates) == 0 and float(opt.clip_coef) == 1.0


@pytest.mark.parametrize("mode", ["one-group", "huge-max-norm"])
def test_one_group_without_clipping_is_the_old_kernel_bit_for_bit(mode):
    from spacap3d_amd.optim import FlatAdam
    pa, ba, old, _, _, g = _make(groups=False)
    assert not old.grouped
    if mode == "one-group":
        pc, bc, new, _, _, _ = _make(one_group=True)
    else:
        pc, bc, new, _, _, _ = _make(groups=False, max_grad_norm=1e30)
    assert new.grouped and len(new.param_groups) == 1
    for step in range(5):
        grads = _grads(g, 10.0 ** (step - 2))
        _feed(pa, ba, grads)
        _feed(pc, bc, grads)
        old.step(grad_scale=0.5)
        new.step(grad_scale=0.5)
        assert float(new.clip_coef) == 1.0
        for name in ("flat_p", "m", "v"):
            assert torch.equal(getattr(old, name), getattr(new, name)), (mode, step, name)
    assert float(old.step_t) == float(new.step_t) == 5


# ---- the squared-norm pass ---------------------------------------------------------------------------------------------------
def _norm_case(n, seed):
    """A flat buffer of n elements cut into two groups at a multiple of 4 (one group when n is too short to cut)."""
    g = torch.Generator().manual_seed(seed)
    flat = torch.randn(n, generator=g)
    cut = (n // 2) // 4 * 4
    seg_off, seg_group = ([0, cut, n], [0, 1]) if cut else ([0, n], [1])
    return flat, seg_off, seg_group


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 4096 * 256 * 4 + 5])
def test_squared_norm_against_float64(n):
    from spacap3d_amd.optim import grad_sqnorm
    flat, seg_off, seg_group = _norm_case(n, seed=n % 97)
    dflat = flat.to(DEV)
    sq, norms, _ = grad_sqnorm(dflat, seg_off, seg_group, 2, grad_scale=0.25)
    sq2, norms2, _ = grad_sqnorm(dflat, seg_off, seg_group, 2, grad_scale=0.25)
    assert torch.equal(sq, sq2) and torch.equal(norms, norms2)             # same input, same bits
    x = flat.numpy().astype(np.float64)
    x2 = x * x
    want = [0.0, 0.0]
    for s, k in enumerate(seg_group):
        want[k] = math.fsum(x2[seg_off[s]:seg_off[s + 1]])                # correctly rounded: the reference's own error is 2^-53
    want.append(math.fsum(x2))
    got = sq.cpu().numpy()
    for k in range(3):
        # n exact, non-negative terms summed in any order: relative error <= n * 2^-53
        assert abs(got[k] - want[k]) <= n * 2.0 ** -53 * want[k], (n, k, got[k], want[k])
        assert _ulps(norms[k].item(), np.float32(0.25 * np.sqrt(want[k]))) <= 2, (n, k)


def test_squared_norm_of_a_one_element_group_and_of_extreme_entries():
    from spacap3d_amd.distributed import FlatGradBucket
    from spacap3d_amd.optim import FlatAdam
    g = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g).to(DEV)) for n in (1023, 1, 5)]
    bucket = FlatGradBucket(ps, views=False)
    opt = FlatAdam(bucket, lr=0.0, groups=[{"params": [ps[0], ps[2]]}, {"params": [ps[1]]}])
    grads = [torch.randn(n, generator=g) for n in (1023, 1, 5)]
    grads[0][17] = 1e18                                                    # its square fits in a double
    held = [gr.to(DEV) for gr in grads]
    for p, gr in zip(ps, held):
        p.grad = gr
    bucket.pack()
    opt.step()
    x = [gr.numpy().astype(np.float64) for gr in grads]
    want = [math.fsum(np.concatenate([x[0], x[2]]) ** 2), float(x[1][0] ** 2)]
    got = opt.grad_sqnorm.cpu().numpy()
    assert got[1] == want[1]                                               # one exact product
    assert abs(got[0] - want[0]) <= 1028 * 2.0 ** -53 * want[0] and abs(got[2] - (want[0] + want[1])) <= 1029 * 2.0 ** -53 * got[2]
    assert math.isfinite(float(opt.grad_norm)) and _ulps(float(opt.grad_norm), np.float32(np.sqrt(want[0] + want[1]))) <= 2
    assert float(opt.step_t) == 1 and int(opt.skipped_updates) == 0
    grads[2][3] = float("nan")
    held += [gr.to(DEV) for gr in grads]
    for p, gr in zip(ps, held[3:]):
        p.grad = gr
    bucket.pack()
    opt.step()
    try:
        assert not math.isfinite(float(opt.grad_sqnorm[2])) and not math.isfinite(float(opt.grad_norm))
        assert math.isfinite(float(opt.group_grad_norm[1]))                # the NaN stays in its own group
        assert float(opt.step_t) == 1 and int(opt.skipped_updates) == 1
    finally:
        _scrub(*held, *_opt_buffers(opt))


def test_entry_points_check_their_tables():
    from spacap3d_amd.optim import grad_sqnorm
    flat = torch.zeros(16, device=DEV)
    with pytest.raises(RuntimeError, match="16-byte boundary"):
        grad_sqnorm(flat, [0, 6, 16], [0, 1], 2)
    with pytest.raises(RuntimeError, match="outside"):
        grad_sqnorm(flat, [0, 8, 16], [0, 1], 9)
    with pytest.raises(RuntimeError, match="group is outside"):
        grad_sqnorm(flat, [0, 8, 16], [0, 2], 2)
    with pytest.raises(RuntimeError, match="span"):
        grad_sqnorm(flat, [0, 8, 12], [0, 1], 2)


# ---- clipping ---------------------------------------------------------------------------------------------------------------
def test_clipping_matches_the_restatement_and_torch():
    from spacap3d_amd.optim import grad_sqnorm
    pa, bucket, opt, pb, ref, g = _make(eps=EPS_CLIP, max_grad_norm=1.0)
    mine = R.RestatedAdam([p.detach().cpu().numpy() for p in pa], GROUP_OF, LRS, WDS, eps=EPS_CLIP, max_norm=1.0)
    seg_off, seg_group = bucket.offsets + [bucket.flat.numel()], GROUP_OF
    for step in range(5):
        grads = _grads(g, 10.0 ** (step - 2))
        _feed(pa, bucket, grads)
        _feed(pb, None, grads)
        measured = float(grad_sqnorm(bucket.flat, seg_off, seg_group, 2)[1][2])
        max_norm = 0.5 * measured                                          # half the measured norm: every step clips
        opt.set_max_grad_norm(max_norm)
        mine.max_norm = max_norm
        opt.step()
        torch.nn.utils.clip_grad_norm_(pb, max_norm)
        ref.step()
        assert mine.step([x.cpu().numpy() for x in grads])
        coef = float(opt.clip_coef)
        assert 0.49 < coef < 0.51 and _ulps(coef, mine.coef) <= 2, (step, coef, mine.coef)
        assert _ulps(float(opt.grad_norm), mine.norm) <= 2
        for p, q, r in zip(pa, pb, mine.p):
            assert np.allclose(p.detach().cpu().numpy(), r, rtol=RTOL, atol=ATOL), (step, "restatement")
            assert torch.allclose(p, q, rtol=RTOL, atol=ATOL), (step, "torch", float((p - q).abs().max()))


# ---- a non-finite gradient skips the update -------------------------------------------------------------------------------------
def test_nan_gradient_skips_one_update_and_nothing_else():
    pa, ba, a, _, _, g = _make(max_grad_norm=5.0)
    pb, bb, b, _, _, _ = _make(max_grad_norm=5.0)        # the twin: only ever sees the four finite steps
    for step in range(5):
        grads = _grads(g)
        if step == 2:
            grads[3][5, 7] = float("nan")
            before = [t.clone() for t in (a.flat_p, a.m, a.v)]
            held = [gr.clone() for gr in grads]
            for p, gr in zip(pa, held):
                p.grad = gr
            ba.pack()
            a.step()
            torch.cuda.synchronize()
            try:
                assert all(torch.equal(x, y) for x, y in zip(before, (a.flat_p, a.m, a.v)))
                assert float(a.step_t) == 2 and int(a.skipped_updates) == 1 and not math.isfinite(float(a.grad_norm))
            finally:
                _scrub(grads[3], *held, ba.flat, a._partials, a.grad_sqnorm, a._ctrl[4:])   # (the next step rewrites the last four)
            continue
        _feed(pa, ba, grads)
        _feed(pb, bb, grads)
        a.step()
        b.step()
    assert float(a.step_t) == float(b.step_t) == 4 and int(a.skipped_updates) == 1 and int(b.skipped_updates) == 0
    for name in ("flat_p", "m", "v"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    # the sticky skip word of the overlapped gradient exchange still blocks the update
    word = torch.ones(1, dtype=torch.int64, device=DEV)
    before = a.flat_p.clone()
    _feed(pa, ba, _grads(g))
    a.step(skip_word=word)
    assert torch.equal(before, a.flat_p) and float(a.step_t) == 4 and int(a.skipped_updates) == 2


# ---- torch-format state -----------------------------------------------------------------------------------------------------
def _continue(pa, bucket, opt, pb, ref, g, steps=3):
    for step in range(steps):
        grads = _grads(g)
        _feed(pa, bucket, grads)
        _feed(pb, None, grads)
        opt.step()
        ref.step()
        for p, q in zip(pa, pb):
            assert torch.allclose(p, q, rtol=RTOL, atol=ATOL), (step, float((p - q).abs().max()))


@pytest.mark.parametrize("grouped", [True, False])
def test_state_dict_goes_to_torch_and_back(grouped):
    pa, bucket, opt, pb, ref, g = _make(groups=grouped, one_group=not grouped)
    for _ in range(3):
        _feed(pa, bucket, _grads(g))
        opt.step()
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(6)) and all(float(e["step"]) == 3 for e in sd["state"].values())
    assert [set(a) for a in sd["param_groups"]] == [set(a) for a in ref.state_dict()["param_groups"]]
    ref.load_state_dict(sd)                               # a fresh torch.optim.Adam over the same groups accepts it
    with torch.no_grad():
        for p, q in zip(pa, pb):
            q.copy_(p)
    _continue(pa, bucket, opt, pb, ref, g)
    # the reverse: torch's state into a fresh FlatAdam
    pc, bc, fresh, _, _, _ = _make(seed=9, groups=grouped, one_group=not grouped)
    with torch.no_grad():
        for p, q in zip(pc, pb):
            p.copy_(q)
    fresh.load_state_dict(ref.state_dict())
    assert float(fresh.step_t) == 6
    _continue(pc, bc, fresh, pb, ref, g)
    if grouped:
        # set_lr: the next update follows the new rates, as the twin's param_groups[i]["lr"] does
        fresh.set_lr(group_lrs=[2e-3, None])
        ref.param_groups[0]["lr"] = 2e-3
        _continue(pc, bc, fresh, pb, ref, g, steps=1)
        fresh.set_lr(lr=3e-4)
        for grp in ref.param_groups:
            grp["lr"] = 3e-4
        _continue(pc, bc, fresh, pb, ref, g, steps=1)
        assert [a["lr"] for a in fresh.state_dict()["param_groups"]] == [3e-4, 3e-4]
    else:
        with pytest.raises(RuntimeError, match="grouped mode"):
            fresh.set_lr(lr=1e-4)


def test_parameters_outside_the_bucket_only_count_in_the_numbering():
    from spacap3d_amd.distributed import FlatGradBucket
    from spacap3d_amd.optim import FlatAdam
    g = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g).to(DEV)) for s in [(5, 3), (7,), (2, 2)]]
    outside = torch.nn.Parameter(torch.zeros(4, device=DEV))
    bucket = FlatGradBucket(ps, views=False)
    groups = [{"params": [ps[0], outside, ps[2]]}, {"params": [ps[1]], "lr": 5e-4}]
    opt = FlatAdam(bucket, lr=1e-3, groups=groups)
    assert opt.state_dict()["state"] == {}                # no update yet: no state, as in torch
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    bucket.pack()
    opt.step()
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 2, 3] and sd["param_groups"][0]["params"] == [0, 1, 2] and sd["param_groups"][1]["params"] == [3]
    twin = torch.optim.Adam([dict(x) for x in groups], lr=1e-3)
    twin.load_state_dict(sd)
    with pytest.raises(ValueError, match="in no group"):
        FlatAdam(FlatGradBucket(ps, views=False), groups=[{"params": ps[:2]}])
    with pytest.raises(ValueError, match="appears in groups"):
        FlatAdam(FlatGradBucket(ps, views=False), groups=[{"params": ps}, {"params": ps[:1]}])
    with pytest.raises(ValueError, match="parameter groups"):
        FlatAdam(FlatGradBucket(ps, views=False), groups=[{"params": ps}] + [{"params": []}] * 8)
