"""tests/attention_restated.py is right and its tables are whole, checked without a device:
  * the float64 statement reproduces the reference's own outputs (tests/golden/attention_ref.npz) inside that file's bars;
  * ``tier()`` and the case tables walk every instantiation the host code of csrc/mha.hip can pick -- a moved threshold or a
    dropped row fails here, not silently on the device;
  * the float32 restatement (oracle/attention_ref.py) sits far inside the bars of tests/test_attention_tiers_gpu.py against
    float64 at every case of the tables, so a correct fp32 kernel has room and a miss on the device is the kernel's."""
import os

import numpy as np
import pytest
import torch

import attention_restated as R
from oracle import attention_ref as ref32

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_ref.npz")


@pytest.mark.parametrize("tag", ["enc", "dec", "cross1", "odd"])
def test_float64_statement_reproduces_the_reference_outputs(tag):
    fx = np.load(G)
    q, k, v, mask = (torch.from_numpy(fx[f"{tag}_{n}"]) for n in ("q", "k", "v", "mask"))
    o, p = R.attention64(q, k, v, mask)
    np.testing.assert_allclose(p.numpy(), fx[f"{tag}_p"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(o.numpy(), fx[f"{tag}_out"], rtol=1e-4, atol=1e-5)
    want = torch.from_numpy(fx[f"{tag}_logits"])
    keep = want > -1e8
    err = ((torch.log(p.clamp_min(1e-37)) - torch.log(torch.from_numpy(fx[f"{tag}_p"]).double().clamp_min(1e-37))) * keep).abs().max()
    assert float(err) < 1e-3


def test_tier_restates_the_dispatch_at_every_threshold():
    """Both sides of each key-count edge and of the query-count edge, against the instantiations written out by hand from
    launch_fwd, launch_bwd and launch_bwd_both."""
    want = {1: (1, 2), 2: (1, 4), 3: (4, 2), 4: (4, 4), 5: (4, 8)}   # tier: (W waves per 16-row tile, NT key tiles per wave)
    edges = [(1, 1), (32, 1), (33, 2), (64, 2), (65, 3), (128, 3), (129, 4), (256, 4), (257, 5), (512, 5)]
    for d in R.D_KS:
        for Lk, t in edges:
            for Lq in (1, 64, 65, 512):
                got = R.tier(Lq, Lk, d)
                w, n = want[t]
                four = Lq >= 65
                assert got.tier == t
                assert got.fwd == ("mha_fwd_kernel", n, d, w) and got.dq == ("mha_bwd_dq_kernel", n, d, w)
                assert got.dkv == ("mha_bwd_dkv_kernel", d, 4 if four else 1)
                assert got.both == (("mha_bwd_both_kernel", n, d, w) if (t >= 3) == four else None)
    for bad in ((4, 513, 16), (4, 0, 16), (0, 4, 16), (4, 4, 24)):
        with pytest.raises(ValueError):
            R.tier(*bad)
    # 15 forward, 15 dQ, 6 dK/dV and 15 single-launch instantiations, and the tables reach every one of them
    every = [R.tier(Lq, Lk, d) for Lq in (64, 65) for Lk in range(1, 513) for d in R.D_KS]
    for field, n in (("fwd", 15), ("dq", 15), ("dkv", 6), ("both", 15)):
        assert len({getattr(t, field) for t in every} - {None}) == n
    two_launch = [R.tier(c.Lq, c.Lk, c.d_k) for c in R.TIER_CASES]
    assert {t.fwd for t in two_launch} == {t.fwd for t in every} and {t.dq for t in two_launch} == {t.dq for t in every}
    assert {t.dkv for t in two_launch} == {t.dkv for t in every}
    assert {R.tier(*c).both for c in R.SINGLE_CASES} == {t.both for t in every} - {None}


def _coverage_gaps(tier_cases, single_cases):
    """The cells of the grid that no row reaches (empty when the tables are whole)."""
    gaps = []
    seen, signatures, single, ragged = set(), {}, set(), set()
    for c in tier_cases:
        t = R.tier(c.Lq, c.Lk, c.d_k)
        if t.tier != c.tier:
            gaps.append(("row files under another tier", c, t.tier))
        four = t.dkv[2] == 4
        seen.add((t.tier, c.d_k, four, c.mask))
        signatures.setdefault((t.tier, c.d_k, c.mask), set()).add((four, c.Lk % 4 == 0))
        if c.Lq % 4:
            ragged.add(t.dkv)
    for Lq, Lk, d in single_cases:
        t = R.tier(Lq, Lk, d)
        if t.both is None:
            gaps.append(("no single-launch form", (Lq, Lk, d)))
        single.add((t.tier, d, Lq == Lk))
    for t in range(1, 6):
        for d in R.D_KS:
            for m in R.MASKS:
                gaps += [("tier cell", t, d, four, m) for four in (False, True) if (t, d, four, m) not in seen]
                # both families and both key-count parities, and not tied to each other: three of the four combinations
                sig = signatures.get((t, d, m), set())
                if len(sig) < 3:
                    gaps.append(("family x (Lk % 4 == 0)", t, d, m, sorted(sig)))
            gaps += [("single launch", t, d, same) for same in (False, True) if (t, d, same) not in single]
    for d in R.D_KS:
        gaps += [("Lq % 4 != 0", "mha_bwd_dkv_kernel", d, w) for w in (1, 4) if ("mha_bwd_dkv_kernel", d, w) not in ragged]
    return gaps


def test_case_tables_cover_the_whole_grid(monkeypatch):
    """{tier 1..5} x {d_k} x {Lq <= 64, Lq > 64} x {no, key, per-query mask}; every (tier, d_k) of the single-launch form with
    Lq == Lk and with Lq != Lk; both dK/dV kernels at each d_k with Lq % 4 != 0.  The check has teeth: it reports a gap for
    each single row taken out and for each threshold moved by one."""
    assert _coverage_gaps(R.TIER_CASES, R.SINGLE_CASES) == []
    assert len(set(R.TIER_CASES)) == len(R.TIER_CASES) == 135 and len(set(R.SINGLE_CASES)) == len(R.SINGLE_CASES)
    for i in range(len(R.TIER_CASES)):
        assert _coverage_gaps(R.TIER_CASES[:i] + R.TIER_CASES[i + 1:], R.SINGLE_CASES), R.TIER_CASES[i]
    for i in range(len(R.SINGLE_CASES)):
        if R.SINGLE_CASES[i][:2] in ((20, 50), (64, 33), (100, 300), (65, 512)):
            continue   # (two pairs each in tier 2 and tier 5 with Lq != Lk; test_the_other_tables_sit_where_they_claim names them)
        assert _coverage_gaps(R.TIER_CASES, R.SINGLE_CASES[:i] + R.SINGLE_CASES[i + 1:]), R.SINGLE_CASES[i]
    for i in range(len(R.KEY_EDGES) - 1):
        for step in (-1, 1):
            edges = list(R.KEY_EDGES)
            edges[i] += step
            monkeypatch.setattr(R, "KEY_EDGES", tuple(edges))
            assert _coverage_gaps(R.TIER_CASES, R.SINGLE_CASES), edges
            monkeypatch.undo()
    for step in (-1, 1):
        monkeypatch.setattr(R, "QUERY_EDGE", 64 + step)
        assert _coverage_gaps(R.TIER_CASES, R.SINGLE_CASES), step
        monkeypatch.undo()
    assert _coverage_gaps(R.TIER_CASES, R.SINGLE_CASES) == []


def test_the_other_tables_sit_where_they_claim():
    fam = lambda c: R.tier(c.Lq, c.Lk, c.d_k).dkv[2] == 4
    for c in R.BIAS_CASES + R.DROPOUT_CASES + R.SCALAR_CASES + R.OFFSET_MASK_CASES:
        assert R.tier(c.Lq, c.Lk, c.d_k).tier == c.tier
    assert {(c.tier, fam(c)) for c in R.BIAS_CASES if c.d_k == 16} == {(t, f) for t in range(1, 6) for f in (False, True)}
    assert {c.tier for c in R.BIAS_CASES if c.d_k == 64} == {3, 5}
    assert sorted((c.tier, c.d_k) for c in R.DROPOUT_CASES) == [(t, d) for t in range(1, 6) for d in R.D_KS]
    for d in R.D_KS:   # the family alternates along the tiers
        fams = [fam(c) for c in R.DROPOUT_CASES if c.d_k == d]
        assert all(a != b for a, b in zip(fams, fams[1:]))
    assert {(c.tier, c.d_k, fam(c)) for c in R.SCALAR_CASES} == {(t, d, f) for t in (3, 4, 5) for d in R.D_KS for f in (False, True)}
    assert all(c.tier >= 3 and c.mask == "query" and c.Lk % 4 == 0 for c in R.OFFSET_MASK_CASES)
    assert set(R.PACKED_CASES) == {(L, d) for L in (33, 65, 130, 260) for d in (32, 64)}
    assert {(Lq, Lk) for Lq, Lk, _ in R.SINGLE_CASES} >= {(20, 50), (64, 33), (100, 300), (65, 512), (96, 96)}
    assert all(R.tier(Lq, Lk, 16).both is None for Lq, Lk in R.SINGLE_REFUSED)
    # the masks: a fully masked scene / row, key 0 kept elsewhere, and keys masked for every query of a scene
    for c in R.TIER_CASES:
        m = R.make_mask(c.mask, c.Lq, c.Lk, 0)
        if c.mask == "key":
            assert m.shape == (R.B, 1, 1, c.Lk) and not m[-1].any() and m[:-1, ..., 0].all()
        elif c.mask == "query":
            assert m.shape == (R.B, 1, c.Lq, c.Lk) and not m[:, :, 0].any() and (c.Lq == 1 or m.any())
            assert c.Lk == 1 or not m[0, :, :, -1].any()


def _fp32_against_float64(c, bias_kind=None, p=0.0):
    x = R.make_inputs(c.Lq, c.Lk, c.d_k, c.mask)
    bias = R.make_bias(bias_kind, c.Lq, c.Lk) if bias_kind else None
    keep_scale = None
    if p > 0.0:
        g = torch.Generator().manual_seed(c.Lq + c.Lk)
        keep_scale = (torch.rand(R.B, R.H, c.Lq, c.Lk, generator=g) >= p).float() / (1.0 - p)
    want = R.reference(x.q, x.k, x.v, x.w_o, x.w_p, x.mask, bias, keep_scale)
    q, k, v = (t.clone().requires_grad_(True) for t in (x.q, x.k, x.v))
    p32 = torch.softmax(ref32.attention_logits(q, k, x.mask, bias), dim=-1)
    if keep_scale is not None:
        p32 = p32 * keep_scale
    o32 = torch.matmul(p32, v)
    ((o32 * x.w_o).sum() + (p32 * x.w_p).sum()).backward()
    assert o32.dtype == p32.dtype == torch.float32
    # a tenth of each bar for the fp32 formulation itself: nine tenths stay for a kernel that orders its sums another way
    assert R.excess(p32.detach(), want.p, R.P_RTOL, R.P_ATOL) < 0.1
    assert R.excess(o32.detach(), want.o, R.O_RTOL, R.O_ATOL) < 0.1
    for got, ref in ((q.grad, want.dq), (k.grad, want.dk), (v.grad, want.dv)):
        assert R.grad_error(got, ref) < R.GRAD_BAR / 10


@pytest.mark.parametrize("c", R.TIER_CASES + R.OFFSET_MASK_CASES + R.SCALAR_CASES, ids=lambda c: "-".join(map(str, c)))
def test_float32_restatement_has_margin_at_every_tier_case(c):
    _fp32_against_float64(c)


@pytest.mark.parametrize("kind", R.BIAS_KINDS)
@pytest.mark.parametrize("c", R.BIAS_CASES, ids=lambda c: "-".join(map(str, c)))
def test_float32_restatement_has_margin_with_a_bias(c, kind):
    _fp32_against_float64(c, bias_kind=kind)


@pytest.mark.parametrize("c", R.DROPOUT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_float32_restatement_has_margin_with_dropout(c):
    _fp32_against_float64(c, p=R.DROPOUT_P)


def test_measures_treat_an_identically_zero_gradient_exactly():
    z = torch.zeros(3)
    assert R.grad_error(z, z) == 0.0 and R.grad_error(z + 1e-30, z) == float("inf")
    assert R.excess(torch.tensor([1.0 + 2e-4]), torch.tensor([1.0]), 1e-4, 0.0) > 1.0
    x = R.make_inputs(17, 1, 16, "none")
    want = R.reference(x.q, x.k, x.v, x.w_o, x.w_p)
    assert float(want.dq.abs().max()) == 0.0 and float(want.dk.abs().max()) == 0.0 and float(want.dv.abs().max()) > 0.0
