"""tests/bn_relu_restated.py is right, and its inputs and bars are fit for the device test, checked without a device.  For every
row of its tables:
  * the float64 restatement against PyTorch's float64 composition on the CPU (``BatchNorm1d/2d(train).double()`` -> ``relu`` ->
    ``max_pool2d([1, S])`` under autograd): values, the three gradients, the running buffers and the arg-max, to 1e-12 of the
    largest reference entry (two float64 computations of one formula); the eval form against ``bn.eval()``; what a NaN or a
    +Inf in one channel does, against the same composition;
  * the conditioning: no float64 pre-activation within the margin of the ReLU's kink, no runner-up of a group within the margin
    of its maximum -- of every element and every group, with nothing left out but what is exempt by rule (the planted exact
    ties, which count as one value, and groups without a positive sample, whose answer is index 0);
  * the bars: the float32 variant (the kernels' expressions, float64 sums) against float64, the largest figure per quantity
    printed (``BN-EDGES cpu ...``, pytest -s) and held to the constants recorded in bn_relu_restated.py; each bar is 16 times
    its figure, capped at what tests/test_ops_gpu.py allows today;
  * the teeth: seven wrong expressions planted in the float32 variant, one at a time, each of which must break a bar or an
    integer equality on at least one case;
  * the dispatch: the branch each case is in the table for, worked out from its sizes with the host code's own formulas."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_relu_restated as R

_name = lambda c: c.name
_POISONED = ("nan", "inf")


def _torch_run(case, x):
    """the composition in float64: (y, pooled, arg, dz, dgamma, dbeta, running_mean, running_var, eval y on those buffers)"""
    C = case.shape[1]
    bn = (torch.nn.BatchNorm2d if len(case.shape) == 4 else torch.nn.BatchNorm1d)(
        C, eps=R.EPS, momentum=case.momentum or 0.0, track_running_stats=True).double()
    # (momentum None means a cumulative average to torch and "leave the buffers" to fused_bn.bn_relu_train: 0.0 states the latter)
    with torch.no_grad():
        bn.weight.copy_(torch.tensor(x.gamma)), bn.bias.copy_(torch.tensor(x.beta))
        bn.running_mean.copy_(torch.tensor(x.running_mean)), bn.running_var.copy_(torch.tensor(x.running_var))
    z = torch.tensor(x.z).double().requires_grad_(True)
    y = F.relu(bn(z))
    out, arg = y, None
    if case.S:
        out, idx = F.max_pool2d(y, kernel_size=[1, case.S], return_indices=True)
        out = out.squeeze(-1)
        arg = (idx.squeeze(-1) - torch.arange(case.shape[2]) * case.S).numpy()
    (out * torch.tensor(x.up).double()).sum().backward()
    bn.eval()
    with torch.no_grad():
        ye = F.relu(bn(z.detach()))
    n = lambda t: t.detach().numpy()
    return n(y), (n(out) if case.S else None), arg, n(z.grad), n(bn.weight.grad), n(bn.bias.grad), n(bn.running_mean), n(bn.running_var), n(ye)


@pytest.mark.parametrize("case", R.ALL_CASES, ids=_name)
def test_restatement_against_the_float64_composition(case):
    x, want = R.inputs(case), R.reference(case)
    y, pooled, arg, dz, dgamma, dbeta, rm, rv, ye = _torch_run(case, x)
    got = {"y": (want.fwd.y, y), "dz": (want.bwd.dz, dz), "dgamma": (want.bwd.dgamma, dgamma), "dbeta": (want.bwd.dbeta, dbeta),
           "running_mean": (want.running_mean, rm), "running_var": (want.running_var, rv),
           "eval": (R.eval_forward(x.z, x.gamma, x.beta, rm, rv), ye)}
    if case.S:
        got["pooled"] = (want.fwd.pooled, pooled)
    fig = {k: R.figure(a, b) for k, (a, b) in got.items()}
    print(f"BN-EDGES cpu float64 {case.name} " + " ".join(f"{k}={v:.1e}" for k, v in fig.items()))
    for k, (a, b) in got.items():
        assert a.dtype == np.float64 and a.shape == b.shape, k
        assert fig[k] < R.F64_BAR, (k, fig[k])
        assert R.same_nonfinite(a, b), k            # NaN where the composition has NaN, +Inf where it has +Inf
        if k in ("y", "pooled", "dz", "eval"):
            assert R.same_zeros(a, b), k
    if case.S:
        keep = np.ones(case.shape[:3], bool)
        if case.kind in _POISONED:                  # among several NaNs the restatement (and the kernels) take the first,
            keep[:, R.POISON_CHANNEL] = False       # torch's pooling the last: the value is NaN either way
        assert want.fwd.arg.dtype == np.uint8 and np.array_equal(want.fwd.arg[keep], arg[keep])
    if case.kind in _POISONED:
        c = R.POISON_CHANNEL
        assert np.isnan(want.fwd.y[:, c]).all() and np.isnan(want.bwd.dz[:, c]).all() and np.isnan(want.bwd.dgamma[c])
        assert np.isnan(want.fwd.istd[c]) and np.isnan(want.running_var[c]) and not np.isfinite(want.running_mean[c])
        assert np.isfinite(np.delete(want.fwd.y, c, 1)).all() and np.isfinite(np.delete(want.bwd.dz, c, 1)).all()
        if case.S:
            assert np.isnan(want.fwd.pooled[:, c]).all() and (want.fwd.arg[:, c] == 0).all()
    if case.momentum is None:
        assert np.array_equal(want.running_mean, x.running_mean.astype(np.float64))
    if case.kind == "tie":
        for b, c, p, i, j in R.TIE_SLOTS:
            assert x.z[b, c, p, i] == x.z[b, c, p, j] and want.fwd.arg[b, c, p] == i and want.fwd.pooled[b, c, p] > 0.0
    if case.kind == "top-index":
        assert want.fwd.arg[0, 1, 0] == 255
    if case.kind == "clamped":
        assert (want.fwd.y[0, 2, 0] == 0.0).all() and want.fwd.arg[0, 2, 0] == 0 and want.fwd.pooled[0, 2, 0] == 0.0
        assert (want.fwd.y[1, 3, 6] == 0.0).all() and want.fwd.arg[1, 3, 6] == 0
    if case.kind in ("gamma0+", "gamma0-"):
        assert (want.fwd.y[:, 1] == max(float(x.beta[1]), 0.0)).all() and (want.bwd.dz[:, 1] == 0.0).all()
        if case.S:
            assert (want.fwd.arg[:, 1] == 0).all()
    if case.kind == "const":
        assert (want.fwd.var[1] == 0.0) and (want.fwd.y[:, 1] == float(x.beta[1])).all()
    if case.kind == "offset":
        assert 500.0 < want.fwd.mean[1] * want.fwd.istd[1] < 2000.0


@pytest.mark.parametrize("case", R.ALL_CASES, ids=_name)
def test_inputs_are_clear_of_the_kink_and_of_near_ties(case):
    x = R.inputs(case)
    z = R.unpoisoned(case)           # the poison goes in after the conditioning: the other channels are what is compared
    kink, gap, f = R.conditions(z, x.gamma, x.beta, case.S)
    groups = "" if gap is None else f" smallest gap / margin={gap.min():.3g} groups without two positive values={int(np.isinf(gap).sum())}/{gap.size}"
    print(f"BN-EDGES cpu conditioning {case.name} nudging rounds={x.rounds} smallest |pre| / margin={kink.min():.3g}" + groups)
    assert kink.shape == z.shape and np.isfinite(kink).all() and kink.min() >= 1.0
    if case.S:
        assert gap.shape == z.shape[:3] and gap.min() >= 1.0
        # a group has no finite gap only if it has fewer than two distinct positive values: clamped, all tied, or one survivor
        pos = np.where(f.pre > 0.0, f.pre, -np.inf)
        distinct = np.asarray([len(np.unique(g[np.isfinite(g)])) for g in pos.reshape(-1, case.S)]).reshape(gap.shape)
        assert np.array_equal(np.isinf(gap), distinct < 2)
    else:
        # the eval form on the batch's own statistics rounded to float32: the same pre-activations to within that rounding, so
        # still clear of the kink, and the float32 variant within the bar of y
        rm, rv = R.eval_buffers(case)
        bc = lambda a: a.astype(np.float64)[None, :, None]
        pre = (z.astype(np.float64) - bc(rm)) / np.sqrt(bc(rv) + R.EPS) * bc(x.gamma) + bc(x.beta)
        margin = R.MARGIN * (np.abs(pre - bc(x.beta)) + np.abs(bc(x.beta)))
        fig = R.figure(R.eval_forward(x.z, x.gamma, x.beta, rm, rv, dtype=R.F32), R.eval_forward(x.z, x.gamma, x.beta, rm, rv))
        print(f"BN-EDGES cpu conditioning {case.name} eval form: smallest |pre| / margin={(np.abs(pre) / margin).min():.3g} float32 y={fig:.2e}")
        assert (np.abs(pre) / margin).min() >= 0.5 and fig < R.bars(case)["y"]


@functools.lru_cache(maxsize=None)
def _float32_figures(case):
    want, got = R.reference(case), R.run(case, R.F32)
    fig = R.figures(got, want, case)
    exact = (case.S is None or np.array_equal(got.fwd.arg, want.fwd.arg)) and R.same_zeros(got.fwd.y, want.fwd.y) \
        and R.same_zeros(got.bwd.dz, want.bwd.dz) and R.same_nonfinite(got.fwd.y, want.fwd.y) and R.same_nonfinite(got.bwd.dz, want.bwd.dz)
    return fig, exact


def test_float32_figures_are_the_recorded_constants():
    """the largest figure per quantity over the tables (the offset-channel cases on their own), and the bars made of them"""
    for kinds, recorded, bar in ((False, R.FIGURE_32, R.BAR), (True, R.FIGURE_32_OFFSET, R.BAR_OFFSET)):
        worst = dict.fromkeys(R.QUANTITIES, (0.0, "-"))
        for case in R.ALL_CASES:
            if (case.kind == "offset") == kinds:
                fig, exact = _float32_figures(case)
                assert exact, case.name
                for q, v in fig.items():
                    worst[q] = max(worst[q], (v, case.name))
        for q in R.QUANTITIES:
            print(f"BN-EDGES cpu float32 {'offset-channel cases' if kinds else 'all other cases'} {q}: figure={worst[q][0]:.4e} "
                  f"({worst[q][1]}) recorded={recorded[q]:.4e} bar={bar[q]:.4e} cap={R.CAP[q]:.0e}")
        for q in R.QUANTITIES:
            assert math.isclose(worst[q][0], recorded[q], rel_tol=1e-3), (q, worst[q], recorded[q])
            assert bar[q] == min(16.0 * recorded[q], R.CAP[q]) and 0.0 < bar[q] <= R.CAP[q]
    # float32 does lose digits in the offset channel, and nowhere else
    assert R.FIGURE_32_OFFSET["y"] > 4.0 * R.FIGURE_32["y"]


def _caught(case, mutant):
    want, got = R.reference(case), R.run(case, R.F32, mutant)
    bar = R.bars(case)
    broken = [f"{q}={v:.1e}" for q, v in R.figures(got, want, case).items() if not v < bar[q]]
    if case.S and not np.array_equal(got.fwd.arg, want.fwd.arg):
        broken.append("arg-max")
    if not (R.same_zeros(got.fwd.y, want.fwd.y) and R.same_zeros(got.bwd.dz, want.bwd.dz)):
        broken.append("exact zeros")
    return broken


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_bars_have_teeth(mutant):
    """each wrong expression breaks a bar or an integer equality somewhere; without it, nothing breaks anywhere"""
    small = [c for c in R.ALL_CASES if np.prod(c.shape) <= 300000 and c.kind not in _POISONED]
    hits = {c.name: b for c in small for b in [_caught(c, mutant)] if b}
    first = next(iter(hits.items()), None)
    print(f"BN-EDGES cpu mutant {mutant}: caught on {len(hits)}/{len(small)} cases, first {first}")
    assert hits
    assert not any(_caught(c, "") for c in small)


def test_each_case_reaches_the_edge_it_is_in_the_table_for():
    """the host code's branch conditions (csrc/bn_relu.hip: bn_small, pick_split, grid_x), evaluated at the cases' sizes"""
    sh = lambda n: R.BY_NAME[n].shape
    M = lambda n: sh(n)[0] * int(np.prod(sh(n)[2:]))
    small = {n: R.bn_small(*sh(n)) for n in ("small-last", "small-one-group-over", "small-C63", "small-L-odd", "small-tiny", "d-nan", "d-inf")}
    assert small == {"small-last": True, "small-one-group-over": False, "small-C63": False, "small-L-odd": False, "small-tiny": True,
                     "d-nan": True, "d-inf": True}
    assert M("small-last") == 32768 and M("small-one-group-over") == 32768 + 4 * 4 and sh("small-one-group-over")[2] % 4 == 0
    assert M("small-L-odd") <= 32768 and sh("small-L-odd")[1] >= 64 and sh("small-L-odd")[2] % 4 == 2
    split = lambda n: R.pick_split(sh(n)[1], M(n))
    assert 4096 // 16 == 256 and M("split-256") // 2048 + 1 == 256 and split("split-256") == 256
    assert 4096 // 5000 == 0 and split("split-C5000") == 1
    assert split("split-scalar-ragged") == 5 and sh("split-scalar-ragged")[2] % 4 == 3 and M("split-scalar-ragged") % (5 * 256) != 0
    assert split("small-L-odd") == 5 and split("rows-65535") == 1
    assert [R.grid_x(sh(n)[2]) for n in ("grid-L4096", "grid-L4100", "grid-64-full", "grid-64-one-group-over")] == [1, 2, 64, 64]
    # a workgroup covers 1024 elements a trip, a quarter of the 4096 grid_x counts: four trips wherever L is a multiple of 4096,
    # and a fifth, of one thread, for the float4 group past 64 x 4096
    assert [R.apply_trips(sh(n)[2]) for n in ("grid-L4096", "grid-L4100", "grid-64-full", "grid-64-one-group-over")] == [4, 3, 4, 5]
    assert sh("grid-scalar-trips")[2] % 4 == 3 and R.grid_x(16387) == 5 and R.apply_trips(16387) == 13 and R.apply_trips(522240) == 8
    assert sh("rows-65535")[0] * sh("rows-65535")[1] == 65535 and M("M2") == 2
    for S in (16, 32, 64, 128):
        rpw = 64 // (S // 4)                                  # rows a wave takes per step
        blocks = lambda rows: max(min((rows * (S // 4) + 1023) // 1024 // 4, 65535 * 8), 1)
        rows = [int(np.prod(R.BY_NAME[f"p{S}-{n}"].shape[:3])) for n in ("one-row", "odd-rows", "blocks")]
        assert rows == [1, 15, 2096] and rows[1] % rpw != 0 and rows[2] % rpw == 0 and blocks(rows[2]) >= 2 and blocks(rows[1]) == 1
        assert rows[0] < rpw and rows[1] % 2 == 1              # one row is less than a wave's step at every S, 15 at S = 16
        assert R.pick_split(8, 2 * 131) == 1 and R.BY_NAME[f"p{S}-blocks"].shape[0] >= 2
    # the pooled backward of the C ABI: scalar for S % 4 != 0 whatever L is, vector at an S no forward serves, uint8's top
    assert [(c.shape[2] * c.S % 4, c.S % 4) for c in R.CABI_CASES] == [(0, 3), (3, 3), (0, 0), (0, 0)]
    assert [c.S for c in R.CABI_CASES] == [7, 7, 20, 256] and all(c.S not in (16, 32, 64, 128) for c in R.CABI_CASES)


@pytest.mark.parametrize("case", R.GM_CASES, ids=_name)
def test_group_max_restatement_against_max_pool2d(case):
    x = R.gm_inputs(case)
    S = case.shape[3]
    val, arg = R.group_max(x.x)
    xt = torch.tensor(x.x).requires_grad_(True)
    out, idx = F.max_pool2d(xt, kernel_size=[1, S], return_indices=True)
    (out.squeeze(-1) * torch.tensor(x.go)).sum().backward()
    assert arg.dtype == np.uint8 and val.dtype == np.float32
    assert np.array_equal(val, out.detach().squeeze(-1).numpy(), equal_nan=True)
    assert np.array_equal(arg, (idx.squeeze(-1) - torch.arange(case.shape[2]) * S).numpy())
    assert np.array_equal(R.group_max_grad(x.go, arg, S), xt.grad.numpy())
    rows = x.x.reshape(-1, S)
    if S >= 7:
        assert (arg.reshape(-1)[:-1:3] == 2).all()          # the first of five equal maxima
    if rows.shape[0] > 1 and S > 1:
        assert np.isnan(val.reshape(-1)[-1]) and arg.reshape(-1)[-1] == S // 2
    if S == 256:
        assert arg.reshape(-1)[1] == 255
    # the first of several NaNs, and the last maximum for the mutant
    two = np.asarray([[1.0, np.nan, 3.0, np.nan], [2.0, 5.0, 5.0, 1.0]], np.float32)
    assert R.group_max(two)[1].tolist() == [1, 1] and R.group_max(two, last=True)[1].tolist() == [3, 2]
