"""tests/tf_layer_restated.py held to things that do not share its code (no GPU): float64 autograd of the reference formulas
(models/transformer_captioner.py: LayerNorm :102-113, SublayerConnection :115-127, PositionwiseFeedForward :72-81) on three
shapes, one with constant rows; the library's own host helpers over a grid of shapes and at their refusals; the argument checks
of every C entry point that fail before a launch; the workgroup map of the split-bf16 kernel; the float32 evaluation behind the
LayerNorm bars; and mutants: one wrong rule at a time, run through the comparisons the device test uses, each of which at least
one case of the tables must reject.  Also the lookup of the split-bf16 weight images (spacap3d_amd/tf_layer.py: ffn_pieces)."""
import ctypes
import gc
import weakref

import numpy as np
import pytest
import torch

import tf_layer_restated as T
from sampling_restated import GOLDEN

F64 = np.float64


def _ln64(x, a, b, eps):
    return a * (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + eps) + b


def _close(got, want, what):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    err = float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-300)
    assert got.shape == want.shape and np.isfinite(got).all() and err <= 1e-12, (what, err)


@pytest.mark.parametrize("R,Lq,constant", [(1, 1, False), (51, 17, False), (17, 1, True)], ids=["R1", "R51-Lq17", "R17-constant-rows"])
def test_row_kernel_restated_against_float64_autograd(R, Lq, constant):
    """x1 = res + dropout(a Wo^T + bo), n = LayerNorm(x1), out = n W^T + b: values, then every gradient the backward kernel returns
    (dx1 with the residual path as addend, dy, da = dy Wo, delta, the LayerNorm parameter sums)."""
    rng = np.random.default_rng(R)
    eps, p, seed, counter = float(np.float32(1e-6)), 0.5, 77, 3      # (eps crosses the C ABI as a float)
    t = lambda *s: torch.tensor(rng.standard_normal(s), dtype=torch.float64)
    att, res, Wo, bo, la, lb, W2, b2, G, Gx = t(R, 128), t(R, 128), t(128, 128), t(128), t(128) * 0.3 + 1, t(128), t(256, 128), t(256), t(R, 256), t(R, 128)
    keep = T.keep_mask(R, 128, 128, p, seed, counter)
    scale = T.drop_scale(p)
    if constant:      # an all-zero row and a row of 0.75: the first part is dropped there and the residual is constant
        keep[[3, 9]] = False
        res[3], res[9] = 0.0, 0.75
    att.requires_grad_(), la.requires_grad_(), lb.requires_grad_()
    pre = att @ Wo.t() + bo
    pre.retain_grad()
    x1 = res + torch.tensor(keep) * scale * pre
    x1.retain_grad()
    n = _ln64(x1, la, lb, eps)
    out = n @ W2.t() + b2
    ((out * G).sum() + (x1 * Gx).sum()).backward()
    # forward
    xo = res.numpy() + np.where(keep, scale * (att.detach().numpy() @ Wo.numpy().T + bo.numpy()), 0.0)
    f = T.ln_fwd(xo, la.detach().numpy(), lb.detach().numpy(), eps)
    _close(xo, x1.detach(), "x1"), _close(f["n"], n.detach(), "n"), _close(f["n"] @ W2.numpy().T + b2.numpy(), out.detach(), "out2")
    _close(f["mu"], x1.detach().mean(-1), "mu"), _close(f["r"], 1.0 / (x1.detach().std(-1) + eps), "r")
    if constant:
        assert (x1.detach().std(-1)[[3, 9]] == 0).all() and np.array_equal(f["n"][3], lb.detach().numpy())
    # backward: dn = G W2, addend = the residual path's gradient
    b = T.ln_bwd(G.numpy() @ W2.numpy(), xo, la.detach().numpy(), Gx.numpy(), eps, scale, keep)
    _close(b["dx"], x1.grad, "dx"), _close(b["dy"], pre.grad, "dy")
    _close(T.tile_sums(b["pa"]).sum(0), la.grad, "d ln_a"), _close(T.tile_sums(b["pb"]).sum(0), lb.grad, "d ln_b")
    da = b["dy"] @ Wo.numpy()
    _close(da, att.grad, "out2 = dy Wo")
    d, _ = T.delta_of(da, att.detach().numpy(), Lq)
    want = (att.grad * att.detach()).view(R // Lq, Lq, 8, 16).sum(-1).permute(0, 2, 1)
    _close(d, want, "delta")
    assert T.tile_sums(b["pa"]).shape == (T.rows_tiles(R), 128)


def test_feed_forward_restated_against_float64_autograd():
    """mode 0 on one table case, then mode 1 on its saved hidden layer: hid and the sum of the slices' partial results"""
    c0 = next(c for c in T.FFN_CASES if c.kind == "real" and not c.bf3 and c.mode == 0 and c.p and c.hid and c.bias and c.dff > 128)
    x0 = T.ffn_inputs(c0)
    hid, _, keep, _ = T.ffn_hid(c0, x0)
    part, _ = T.ffn_part(c0, x0, hid)
    t = lambda w: torch.tensor(T.inside(w).astype(F64))
    x, W1, W2, b = t(x0["x"]).requires_grad_(), t(x0["W1"]), t(x0["W2"]), t(x0["bias"])[0]
    pre = x @ W1.t() + b
    pre.retain_grad()
    h = torch.tensor(keep) * T.drop_scale(c0.p) * torch.relu(pre)
    o = h @ W2.t()
    dy = torch.tensor(np.random.default_rng(5).standard_normal(o.shape))
    (o * dy).sum().backward()
    _close(hid, h.detach(), "hid"), _close(part.sum(0), o.detach(), "sum of part[c]")
    assert part.shape == (c0.dff // 128, c0.R, 128) and (hid == 0).any()
    c1 = c0._replace(mode=1, bias=0)
    x1 = dict(x0, x=T.window(dy.numpy()), y=T.window(hid), bias=None)
    dyf = T.inside(x1["x"]).astype(F64)       # (the window holds float32)
    h1, _, _, _ = T.ffn_hid(c1, x1)
    want = (torch.tensor(dyf) @ W2) * (h.detach() > 0) * T.drop_scale(c0.p)
    _close(h1, want, "dhid")
    _close(T.ffn_part(c1, x1, h1)[0].sum(0), want @ W1, "sum of the backward's part[c]")


def test_split_product_restated_against_the_whole_product():
    for c in T.GEMM_CASES:
        if c.kind != "real" or c.entry != "gemm":
            continue
        x = T.gemm_inputs(c)
        want, bar, _, _ = T.gemm_reference(c, x)
        A, W = T.inside(x["x"]).astype(F64), T.inside(x["W"]).astype(F64)
        _close(want.sum(0), A @ (W.T if c.trans else W), c.name)
        assert want.shape == (c.nsplit, c.R, c.N) and (bar > 0).all()


def test_piece_images_hold_every_weight_once_per_image_and_add_up():
    rng = np.random.default_rng(3)
    W1, W2 = rng.standard_normal((256, 128)).astype(np.float32), rng.standard_normal((128, 256)).astype(np.float32)
    img = T.split_images(W1, W2)
    assert img.shape == (4, 3, 256 * 128)
    whole = img.sum(1)
    for i, W in enumerate((W1, W2, W2, W1)):
        assert np.array_equal(np.sort(whole[i]), np.sort(W.astype(F64).ravel())), i       # three pieces carry all 24 bits
    # the documented order: index 0 of slice c is unit 128 c (hidden) / 0 (model), contraction index 0; e runs fastest
    assert whole[0][0] == W1[0, 0] and whole[0][1] == W1[0, 1] and whole[0][8] == W1[1, 0] and whole[0][1 << 14] == W1[128, 0]
    assert whole[1][1] == W2[0, 1] and whole[1][1 << 14] == W2[0, 128] and whole[2][1] == W2[1, 0] and whole[3][1] == W1[1, 0] and whole[3][8] == W1[0, 1]


def test_dropout_mask_restated():
    """the threshold rule, the seed word with and without the device counter, the two index conventions"""
    assert T.drop_thresh(0.0) == 0 and T.drop_thresh(0.5) == 1 << 31 and T.drop_thresh(0.1) == int(np.floor(float(np.float32(0.1)) * 2.0 ** 32))
    assert T.drop_scale(0.5) == 2.0 and T.drop_scale(0.1) == float(np.float32(1) / (np.float32(1) - np.float32(0.1)))
    a, b, c = T.keep_mask(40, 128, 128, 0.25, 9), T.keep_mask(40, 128, 128, 0.25, 9, 0), T.keep_mask(40, 128, 128, 0.25, 9, 1)
    assert np.array_equal(a, b) and not np.array_equal(a, c) and abs(a.mean() - 0.75) < 0.02 and abs(c.mean() - 0.75) < 0.02
    wide = T.keep_mask(20, 256, 256, 0.25, 9)
    assert np.array_equal(wide.reshape(40, 128), a)          # one flat element index: row * stride + column
    assert not np.array_equal(T.keep_mask(40, 128, 256, 0.25, 9), a)
    golden = (9 + 5 * GOLDEN) & (2 ** 64 - 1)
    assert np.array_equal(T.keep_mask(8, 128, 128, 0.25, 9, 5), T.keep_mask(8, 128, 128, 0.25, golden))
    for idx in (0, 16 * 128 + 5, 2 ** 32 - 1):
        s = T.seed_hitting(idx, 1 << 31)
        assert int(T.hash32(np.array([idx], np.uint64), s)[0]) == 1 << 31
    for c in T.ROWS_CASES:
        if c.special == "drop-edge":
            x = T.rows_inputs(c)
            r, col = T.EDGE_ELEMENT
            assert T.rows_keep(c, x)[r, col] and not T.rows_keep(c, x, "keep>")[r, col] and (T.rows_keep(c, x) != T.rows_keep(c, x, "keep>")).sum() == 1


def test_host_rules_agree_with_the_library():
    from spacap3d_amd._native import lib
    for R in range(0, 4101):
        assert lib.spacap_tf_rows_parts(R) == T.rows_tiles(R), R
    Rs = sorted(set(range(1, 4101, 13)) | {1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1024, 1025, 2048, 4096, 4100})
    n = 0
    for R in Rs:
        for K in range(128, 2049, 128):
            for N in (128, 256, 384, 512):
                got = lib.spacap_tf_gemm_splits(R, K, N)
                assert got == T.gemm_splits(R, K, N) and got >= 1 and (K // 128) % got == 0, (R, K, N)
                n += 1
    for args in ((0, 128, 128), (-1, 128, 128), (5, 0, 128), (5, 192, 128), (5, 128, 0), (5, 128, 192), (5, 64, 128)):
        assert lib.spacap_tf_gemm_splits(*args) == T.gemm_splits(*args) == 0, args
    for dff in range(-128, 4097, 64):
        assert lib.spacap_tf_ffn_pieces_elems(dff) == T.pieces_elems(dff), dff
    assert T.pieces_elems(0) == T.pieces_elems(192) == 0 and T.pieces_elems(2048) == 12 * 2048 * 128
    assert [T.ny(R, N2, m) for R, N2, m in ((1024, 384, 0), (1025, 384, 0), (1024, 256, 0), (1025, 256, 0), (16, 128, 0), (16, 384, 1), (16, 512, 0))] == [3, 1, 2, 1, 1, 1, 4]
    assert T.ffn_small(512) and not T.ffn_small(513)
    print(f"TF-EDGES cpu host rules: rows_parts at 4101 R, gemm_splits at {n} shapes and 7 refusals, pieces_elems at {len(range(-128, 4097, 64))} widths")


@pytest.mark.parametrize("nslice", [1, 2, 3, 8, 9, 16, 24])
def test_bf3_workgroup_map_covers_every_tile_and_slice_once(nslice):
    for R in (1, 64, 65, 577):
        m = T.bf3_map(R, 128 * nslice)
        ntiles = -(-R // 64)
        assert sorted(m) == [(t, s) for t in range(ntiles) for s in range(nslice)], (R, nslice)
        if nslice % 8 == 0:       # workgroups are dealt to the XCDs round robin: XCD x sees nslice / 8 slices only
            for xcd in range(8):
                assert {s for (t, s) in m[xcd::8]} == set(range(xcd * nslice // 8, (xcd + 1) * nslice // 8))


def test_every_case_sits_on_the_edge_its_name_claims():
    names = [c.name for c in T.ROWS_CASES + T.GEMM_CASES + T.FFN_CASES + T.SPLIT_CASES]
    assert len(set(names)) == len(names)
    for c in T.ROWS_CASES:
        assert (f"-R{c.R}-" in c.name) and (("fwd" in c.name) == (c.mode == 0))
        if "ny" in c.name:
            assert f"ny{T.ny(c.R, c.N2, 0)}-" in c.name
    rows = lambda mode: [c for c in T.ROWS_CASES if c.mode == mode]
    for mode in (0, 1):
        for kind in ("int", "real"):
            cs = [c for c in rows(mode) if c.kind == kind]
            assert {c.R for c in cs} >= {1, 15, 16, 17, 33} and {c.K1 for c in cs} >= {0, 128, 256, 384, 512, 640}
            assert {c.nparts for c in cs} >= {0, 1, 2, 4, 5, 8, 9, 13, 16, 17, 24}
    fw = rows(0)
    assert {c.N2 for c in fw} == {0, 128, 256, 384, 512} and {(c.N2 > 0, c.bias2) for c in fw} >= {(True, 0), (True, 1)}
    assert {(c.p, c.counter is None) for c in fw if c.kind == "real" and c.p} >= {(0.1, True), (0.1, False), (0.5, True), (0.5, False)}
    assert {(c.K1 + c.nparts > 0, c.bias1) for c in fw} >= {(True, 0), (True, 1)}
    bw = rows(1)
    assert {(c.res, c.n_out, c.N2) for c in bw} >= {(a, b, n) for a in (0, 1) for b in (0, 1) for n in (0, 128)}
    assert {(c.R, c.lq) for c in bw if c.lq} == {(16, 1), (48, 3), (51, 17), (32, 16)}
    g = [c for c in T.GEMM_CASES if c.entry == "gemm"]
    assert {(c.K, c.nsplit) for c in g} == {(128, 1), (256, 1), (256, 2), (1024, 1), (1024, 2), (1024, 4), (1024, 8)}
    assert {c.R for c in g} == {1, 63, 64, 65, 129} and {c.N for c in g} == {128, 256, 384} and {c.trans for c in g} == {0, 1}
    f = [c for c in T.FFN_CASES if not c.bf3]
    assert {c.R for c in f} == {1, 15, 16, 17, 511, 512, 513, 575, 576, 577} and {c.dff for c in f} == {128, 256, 384}
    assert any(c.mode == 0 and not c.hid for c in f) and any(c.mode == 0 and not c.bias for c in f)
    for c in f:
        assert ("MT1" in c.name) == T.ffn_small(c.R)
    b3 = [c for c in T.FFN_CASES if c.bf3]
    assert {c.R for c in b3} == {1, 63, 64, 65, 513, 577} and {c.dff for c in b3} == {128, 384, 1024, 1152, 2048}
    for c in b3:
        assert ("xcd" in c.name) == ((c.dff // 128) % 8 == 0)
    assert {(("xcd" in c.name), c.R % 64 != 0) for c in b3} >= {(True, True), (True, False), (False, True)}
    assert {c.nlayers for c in T.SPLIT_CASES} >= {1, 16, 17}


def test_float32_evaluation_behind_the_layernorm_bars():
    """the figures recorded in the restated module are what its float32 evaluation (sums in index order) errs by on the real tables"""
    fig = T.measure_ln()
    for k, v in fig.items():
        print(f"TF-EDGES cpu LayerNorm stage {k}: float32 evaluation's largest error={v:.3f} recorded={T.LN_FIGURE[k]:.3f} bar={T.LN_BAR[k]:.3f} (units of 2^-24 x magnitude)")
    for k, v in fig.items():
        assert 0.0 < v <= T.LN_FIGURE[k] and T.LN_BAR[k] == 4.0 * T.LN_FIGURE[k], k


def _emulated(family, case, mutant):
    if family == "rows":
        x = T.rows_inputs(case)
        return T.rows_check(case, x, T.rows_emulate(case, x, mutant), tag="TF-EDGES cpu")
    if family == "gemm":
        x = T.gemm_inputs(case)
        return T.gemm_check(case, x, T.gemm_emulate(case, x, mutant), tag="TF-EDGES cpu")
    if family == "ffn":
        x = T.ffn_inputs(case)
        return T.ffn_check(case, x, T.ffn_emulate(case, x, mutant), tag="TF-EDGES cpu")
    x = T.split_inputs(case)
    return T.split_check(case, x, T.split_emulate(case, x, mutant), tag="TF-EDGES cpu")


_TABLES = {"rows": T.ROWS_CASES, "gemm": T.GEMM_CASES, "ffn": tuple(c for c in T.FFN_CASES if c.R * c.dff <= 600 * 1152), "split": T.SPLIT_CASES}
_FAMILIES = {"tail-rows": ("rows", "gemm", "ffn"), "ffn-drop-stride": ("gemm", "ffn"), "relu>=": ("gemm", "ffn"), "pieces-swapped": ("split",), "layer16": ("split",)}


@pytest.mark.parametrize("family", list(_TABLES))
def test_the_contract_itself_passes_every_comparison(family):
    """``*_emulate`` without a mutant is the float64 chain rounded once per output: it must pass what the kernels are held to"""
    n = 0
    for c in _TABLES[family]:
        for r in _emulated(family, c, ""):
            assert r.ok, r.line
            n += 1
    print(f"TF-EDGES cpu {family}: {len(_TABLES[family])} cases, {n} comparisons pass on the restated contract")


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_the_tables_have_teeth(mutant):
    rejected = []
    for family in _FAMILIES.get(mutant, ("rows",)):
        for c in _TABLES[family]:
            bad = [r for r in _emulated(family, c, mutant) if not r.ok]
            if bad:
                rejected.append((c.name, bad[0].line))
                break       # (one per family is enough; the first that rejects)
    print(f"TF-EDGES cpu mutant {mutant}: rejected by {[n for n, _ in rejected]}" + (f" -- {rejected[0][1]}" if rejected else ""))
    assert len(rejected) == len(_FAMILIES.get(mutant, ("rows",))), mutant


def test_argument_refusals_before_any_launch():
    from spacap3d_amd._native import TfRowsArgs, lib
    p = 1 << 12                       # non-null, 16-byte aligned and never dereferenced: every call returns from its checks

    def rows(**kw):
        a = TfRowsArgs()
        base = dict(mode=0, R=16, a1=None, w1=None, bias1=None, k1=0, drop_p=0.0, eps=1e-6, seed=0, seed_dev=None, res=p, x_out=p, ln_a=p, ln_b=p, n_out=p, stats=p,
                    x_ln=None, g=None, part=None, w2=None, bias2=None, out2=None, n2=0, nparts=0, attn_out=None, delta_out=None, lq=0)
        base.update(kw)
        for k, v in base.items():
            setattr(a, k, v)
        return lib.spacap_tf_rows_f32(ctypes.byref(a), None), lib.spacap_last_error().decode()

    bwd = dict(mode=1, g=p, x_ln=p, stats=p, x_out=p, part=p, res=None)
    refused = {
        "null block": (lib.spacap_tf_rows_f32(None, None), lib.spacap_last_error().decode()),
        "mode 2": rows(mode=2), "R < 0": rows(R=-1), "K1 = 192": rows(a1=p, w1=p, k1=192), "K1 = 0": rows(a1=p, w1=p, k1=0), "a1 without w1": rows(a1=p, k1=128),
        "N2 = 192": rows(n2=192, w2=p, out2=p), "N2 without w2": rows(n2=128, out2=p), "N2 without out2": rows(n2=128, w2=p),
        "backward N2 = 256": rows(**bwd, n2=256, w2=p, out2=p), "backward without a1 or g": rows(**dict(bwd, g=None)),
        "backward without part": rows(**dict(bwd, part=None)), "backward without stats": rows(**dict(bwd, stats=None)),
        "delta_out, lq not dividing R": rows(**bwd, n2=128, w2=p, out2=p, attn_out=p, delta_out=p, lq=3),
        "delta_out without attn_out": rows(**bwd, n2=128, w2=p, out2=p, delta_out=p, lq=4), "delta_out in the forward": rows(n2=128, w2=p, out2=p, attn_out=p, delta_out=p, lq=4),
        "delta_out with N2 = 0": rows(**bwd, attn_out=p, delta_out=p, lq=4), "misaligned res": rows(res=p + 4), "misaligned out2": rows(n2=128, w2=p, out2=p + 8),
        "misaligned ln_a": rows(ln_a=p + 4), "p = 1.0": rows(drop_p=1.0), "p < 0": rows(drop_p=-0.5), "nparts without a1": rows(nparts=2), "nparts < 0": rows(a1=p, nparts=-1),
        "forward without res": rows(res=None), "forward without ln_b": rows(ln_b=None),
    }
    gemm = lambda a=p, W=p, R=8, K=256, N=128, trans=1, ns=1, out=p: (lib.spacap_tf_gemm_f32(a, W, R, K, N, trans, ns, out, None), lib.spacap_last_error().decode())
    refused.update({"gemm nsplit not dividing K / 128": gemm(K=384, ns=2), "gemm nsplit = 0": gemm(ns=0), "gemm K = 192": gemm(K=192), "gemm N = 64": gemm(N=64),
                    "gemm null a": gemm(a=None), "gemm misaligned out": gemm(out=p + 4), "gemm R < 0": gemm(R=-1)})
    ffn1 = lambda x=p, W=p, b=None, R=8, N=128, dp=0.0, h=p: (lib.spacap_tf_ffn1_f32(x, W, b, R, N, dp, 0, None, h, None), lib.spacap_last_error().decode())
    refused.update({"ffn1 N = 192": ffn1(N=192), "ffn1 p = 1.0": ffn1(dp=1.0), "ffn1 null h": ffn1(h=None), "ffn1 misaligned bias": ffn1(b=p + 4)})
    dg = lambda g=p, W=p, y=p, R=8, K=128, N=128, out=p: (lib.spacap_tf_dgrad_mask_f32(g, W, y, 2.0, R, K, N, out, None), lib.spacap_last_error().decode())
    refused.update({"dgrad K = 256": dg(K=256), "dgrad N = 192": dg(N=192), "dgrad null y": dg(y=None), "dgrad misaligned g": dg(g=p + 4)})
    ffn = lambda mode=0, x=p, Wa=p, Wb=p, y=None, R=8, dff=128, dp=0.0, hid=p, part=p: (
        lib.spacap_tf_ffn_f32(mode, x, Wa, Wb, None, y, R, dff, dp, 0, None, hid, part, None), lib.spacap_last_error().decode())
    refused.update({"ffn mode 2": ffn(mode=2), "ffn dff = 192": ffn(dff=192), "ffn p = 1.0": ffn(dp=1.0), "ffn mode 1 without y": ffn(mode=1), "ffn mode 1 without hid": ffn(mode=1, y=p, hid=None),
                    "ffn null part": ffn(part=None), "ffn misaligned x": ffn(x=p + 4)})
    bf3 = lambda mode=0, x=p, pc=p, y=None, R=8, dff=128, dp=0.0, hid=p, part=p: (
        lib.spacap_tf_ffn_bf3_f32(mode, x, pc, None, y, R, dff, dp, 0, None, hid, part, None), lib.spacap_last_error().decode())
    refused.update({"bf3 mode 2": bf3(mode=2), "bf3 dff = 0": bf3(dff=0), "bf3 p = 1.0": bf3(dp=1.0), "bf3 null pieces": bf3(pc=None), "bf3 mode 1 without y": bf3(mode=1),
                    "bf3 misaligned pieces": bf3(pc=p + 2)})
    arr = (ctypes.c_void_p * 1)(p)
    null1 = (ctypes.c_void_p * 1)(None)
    sp = lambda w1=arr, w2=arr, pc=arr, n=1, dff=128: (lib.spacap_tf_ffn_split_f32(w1, w2, pc, n, dff, None), lib.spacap_last_error().decode())
    refused.update({"split dff = 192": sp(dff=192), "split nlayers < 0": sp(n=-1), "split null arrays": sp(w1=None), "split null layer": sp(w2=null1)})
    for k, (rc, text) in refused.items():
        print(f"TF-EDGES cpu refusal {k}: {rc} {text!r}")
    for k, (rc, text) in refused.items():
        assert rc == -1 and text, k
    # nothing to do is no refusal, and looks at no pointer
    assert rows(R=0, res=None, ln_a=None)[0] == 0 and gemm(R=0, a=None)[0] == 0 and ffn(R=0, x=None)[0] == 0 and bf3(R=0, pc=None)[0] == 0
    print(f"TF-EDGES cpu refusals: {len(refused)} calls refused by their argument checks")


def test_piece_images_are_served_only_for_the_weight_and_width_they_were_split_from():
    """the table filled by hand with CPU tensors: an entry answers only while its parameter is alive, still lives at the address
    it is registered under, and was split at the caller's width (no kernel runs)"""
    from spacap3d_amd import tf_layer as tf
    saved = dict(tf._FFN_PIECES)
    tf._FFN_PIECES.clear()
    try:
        w = torch.nn.Parameter(torch.zeros(256, 128))
        images = torch.zeros(4, dtype=torch.bfloat16)
        tf._FFN_PIECES[w.data_ptr()] = (weakref.ref(w), 256, images)
        assert tf.ffn_pieces(w, 256) is images
        assert tf.ffn_pieces(w, 384) is None                                  # another width
        assert tf.ffn_pieces(torch.zeros(256, 128), 256) is None               # a weight that was never registered
        # an optimizer flattens its parameters: the parameter moves, the old storage is free for any other tensor
        old = w.data
        key = w.data_ptr()
        w.data = torch.zeros(256, 128)
        assert w.data_ptr() != key and old.data_ptr() == key
        assert tf.ffn_pieces(old, 256) is None and tf.ffn_pieces(w, 256) is None
        tf._FFN_PIECES[w.data_ptr()] = (weakref.ref(w), 256, images)           # the next refresh registers the new address
        assert tf.ffn_pieces(w, 256) is images and tf.ffn_pieces(old, 256) is None
        # the parameter dies: its entries answer nothing, whoever asks at that address
        ghost = torch.zeros(256, 128)
        g = torch.zeros(256, 128)
        tf._FFN_PIECES[ghost.data_ptr()] = (weakref.ref(g), 256, images)       # (a registration whose parameter lives elsewhere)
        assert tf.ffn_pieces(ghost, 256) is None
        tf._FFN_PIECES[g.data_ptr()] = (weakref.ref(g), 256, images)
        assert tf.ffn_pieces(g, 256) is images
        key = g.data_ptr()
        del g
        gc.collect()

        class At:      # whatever tensor the allocator puts there next
            def data_ptr(self):
                return key
        assert tf._FFN_PIECES[key][0]() is None and tf.ffn_pieces(At(), 256) is None
    finally:
        tf._FFN_PIECES.clear()
        tf._FFN_PIECES.update(saved)
