"""The kernels of csrc/tf_layer.hip at every edge of their dispatch, against the float64 restatement of tests/tf_layer_restated.py:
the C ABI called through ``_native.lib`` on the windows of its tables.

``int`` cases (operands from {+-1, +-2, +-3}, dropout p = 0.5): the split product's slices, ``hid`` and ``part`` of the feed-forward
kernels (fp32 and split-bf16), ``x_out`` of the forward row kernel and the ``sum dn`` half of ``part`` under exact equality.
``real`` cases: stage by stage, each stage referenced from the kernel's own stored input to it, within the bars of the restated
module (a-priori for the products; 4 x the measured error of a plain float32 evaluation for the LayerNorm stages).  Always:
every sentinel outside what the call may write is intact, and no NaN stands where the reference is finite (every float of
padding is NaN on the way in).  The dropout masks are held bit for bit.  The comparisons themselves live in the restated module
(``*_check``), where tests/test_tf_layer_restated_cpu.py shows that they reject every mutant.
Each comparison prints its figures before it asserts (``TF-EDGES gpu <entry> <case> ...``, pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

import tf_layer_restated as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_name = lambda c: c.name
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spacap3d_amd import _native
    return _native


def _dev(win, dtype=torch.float32):
    t = torch.tensor(win.buf).to(DEV, dtype)
    assert t.data_ptr() % 16 == 0 and (win.start * t.element_size()) % 16 == 0
    return t, t.data_ptr() + t.element_size() * win.start


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _counter(value):
    """(tensor, pointer) of the device-resident step counter, or (None, None)"""
    if value is None:
        return None, None
    t = torch.tensor([value], dtype=torch.int64, device=DEV)
    return t, t.data_ptr()


def _settle(results):
    for r in results:
        print(r.line)
    for r in results:
        assert r.ok, r.line


# ---- spacap_tf_rows_f32 ---------------------------------------------------------------------------------------------------------------
_ROWS_OUT = ("x_out", "n_out", "stats_out", "part", "out2", "delta_out")


def _run_rows(native, case, x, nulls=(), R=None):
    """one call on fresh uploads of the windows of ``x``; {output name: whole allocation after the call}"""
    c = case
    devs = {k: _dev(w) for k, w in x.items() if w is not None}
    ptr = lambda k: devs[k][1] if (k in devs and k not in nulls) else None
    cnt, pc = _counter(c.counter)
    a = native.TfRowsArgs()
    a.mode, a.R, a.k1, a.n2, a.nparts, a.lq = c.mode, c.R if R is None else R, c.K1, c.N2, c.nparts, c.lq
    a.drop_p, a.eps, a.seed, a.seed_dev = c.p, c.eps, T.rows_seed(c, x), pc
    for k in ("a1", "w1", "bias1", "res", "x_out", "ln_a", "ln_b", "n_out", "x_ln", "g", "part", "w2", "bias2", "out2", "attn_out", "delta_out"):
        setattr(a, k, ptr(k))
    a.stats = ptr("stats_out") if c.mode == 0 else ptr("stats")
    native.check(native.lib.spacap_tf_rows_f32(ctypes.byref(a), _stream()), "spacap_tf_rows_f32")
    torch.cuda.synchronize()
    return {k: devs[k][0].cpu().numpy() for k in _ROWS_OUT if k in devs and k not in nulls}


@pytest.mark.parametrize("case", T.ROWS_CASES, ids=_name)
def test_row_kernel_at_every_edge(native, case):
    x = T.rows_inputs(case)
    _settle(T.rows_check(case, x, _run_rows(native, case, x), tag="TF-EDGES gpu"))


def _same(tag, name, a, b):
    same = np.array_equal(a, b, equal_nan=True)
    print(f"TF-EDGES gpu {tag}: {name} bit-identical={same}")
    return same


@pytest.mark.parametrize("kind,K1,nparts", [("int", 384, 0), ("real", 0, 5), ("real", 0, 0)], ids=["product-int", "slices-real", "no-first-part-real"])
def test_forward_outputs_passed_as_null_leave_the_others_bit_identical(native, kind, K1, nparts):
    """the decoders pass no x_out / n_out / stats: the second product and the outputs that remain must not change"""
    c = next(k for k in T.ROWS_CASES if k.mode == 0 and k.kind == kind and k.K1 == K1 and k.nparts == nparts and k.N2 and not k.special)
    x = T.rows_inputs(c)
    full = _run_rows(native, c, x)
    ok = True
    for null in ("x_out", "n_out", "stats_out", ("x_out", "n_out", "stats_out")):
        nulls = (null,) if isinstance(null, str) else null
        got = _run_rows(native, c, x, nulls=nulls)
        assert set(got) == set(full) - set(nulls)
        for k in got:
            ok &= _same(f"spacap_tf_rows_f32 {c.name} without {'+'.join(nulls)}", k, got[k], full[k])
    assert ok


@pytest.mark.parametrize("N2", [384, 256])
@pytest.mark.parametrize("kind", ["int", "real"])
def test_column_split_of_the_second_product_changes_no_bit(native, kind, N2):
    """R = 1024 (64 row tiles: N2 / 128 workgroups per tile, the first of which stores the rows) against R = 1025 (one workgroup
    per tile) on the same operands: rows 0 .. 1023 of every output bit-identical"""
    c = next(k for k in T.ROWS_CASES if k.name.startswith(f"fwd-split-R1025-N2_{N2}-") and k.kind == kind)
    assert T.ny(1024, N2, 0) == N2 // 128 and T.ny(1025, N2, 0) == 1
    x = T.rows_inputs(c)
    one, split = _run_rows(native, c, x), _run_rows(native, c, x, R=1024)
    ok = True
    for k in ("x_out", "n_out", "stats_out", "out2"):
        a, b = T.inside(x[k], one[k])[:1024], T.inside(x[k], split[k])[:1024]
        ok &= _same(f"spacap_tf_rows_f32 {c.name} R=1024 (ny={N2 // 128}) against R=1025 (ny=1)", k, a, b)
        assert (T.inside(x[k], split[k])[1024:] == T.SENTINEL).all() and not np.isnan(b).any()
    assert ok


def _bwd_case(name, R, p=0.0, N2=128):
    return T.RowsCase(name, "real", 1, R, 0, 0, 0, 1, N2, 0, p, None, 5, 0, 1, "", 1e-6)


def test_backward_tail_rows_contribute_nothing_to_the_parameter_sums(native):
    """R = 17: the second tile holds row 16 alone, so its partials are that row's terms, the ``sum dn`` half bit for bit"""
    c = _bwd_case("bwd-g-R17-tail-real", 17)
    x = T.rows_inputs(c)
    got = _run_rows(native, c, x)
    _settle(T.rows_check(c, x, got, tag="TF-EDGES gpu"))
    part, g = T.inside(x["part"], got["part"]), T.inside(x["g"])
    assert part.shape == (2, 256)
    print(f"TF-EDGES gpu spacap_tf_rows_f32 {c.name}: tile 1 sum dn half equals row 16 of g={np.array_equal(part[1, 128:], g[16])}")
    assert np.array_equal(part[1, 128:], g[16])


def test_backward_keeps_a_nan_and_an_inf_inside_their_rows_and_columns(native):
    c = _bwd_case("bwd-g-R33-nonfinite-real", 33)
    x = T.rows_inputs(c)
    clean = _run_rows(native, c, x)
    g = T.inside(x["g"]).copy()
    g[3, 7], g[20, 100] = np.nan, np.inf
    xp = dict(x, g=T.window(g))
    dirty = _run_rows(native, c, xp)
    rows, other = [3, 20], [r for r in range(33) if r not in (3, 20)]
    ok = True
    for k in ("x_out", "n_out", "out2"):
        a, b = T.inside(x[k], clean[k]), T.inside(x[k], dirty[k])
        nonfin = int((~np.isfinite(b[rows])).sum())
        ok &= _same(f"spacap_tf_rows_f32 {c.name}", f"{k} outside rows 3 and 20", a[other], b[other])
        print(f"TF-EDGES gpu spacap_tf_rows_f32 {c.name}: {k} non-finite in rows 3 and 20: {nonfin}/{b[rows].size}")
        ok &= nonfin == b[rows].size and np.isfinite(b[other]).all()
        ok &= bool((dirty[k][:x[k].start] == T.SENTINEL).all() and (dirty[k][x[k].start + b.size:] == T.SENTINEL).all())
    a, b = T.inside(x["part"], clean["part"]), T.inside(x["part"], dirty["part"])
    hit = np.zeros(a.shape, bool)
    hit[0, [7, 128 + 7]] = hit[1, [100, 128 + 100]] = True
    ok &= _same(f"spacap_tf_rows_f32 {c.name}", "part outside (tile 0, column 7) and (tile 1, column 100)", a[~hit], b[~hit])
    print(f"TF-EDGES gpu spacap_tf_rows_f32 {c.name}: part non-finite at the four struck sums: {int((~np.isfinite(b[hit])).sum())}/4")
    assert ok and (~np.isfinite(b[hit])).all() and np.isfinite(b[~hit]).all()


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_backward_of_constant_rows_is_finite_as_autograd_gives_it(native, p):
    """An all-zero row and a row of 0.75 among ordinary ones, statistics from the forward kernel, eps = 1e-6: std == 0 there, the
    term through the std is 0 (torch masks std == 0 to a zero gradient) and dx = r (dxh - mean(dxh)) + addend with r = 1 / eps.
    The other rows are bit-identical to a run without the constant rows."""
    c = _bwd_case(f"bwd-g-R17-constant-rows-p{p}-real", 17, p)
    x = T.rows_inputs(c)
    xl = T.inside(x["x_ln"]).copy()
    xl[0], xl[5] = 0.0, 0.75
    runs = {}
    for name, rows in (("ordinary", T.inside(x["x_ln"])), ("constant", xl)):
        # the forward kernel's own statistics of these rows
        fc = T.RowsCase(f"fwd-stats-{name}", "real", 0, 17, 0, 0, 0, 1, 0, 0, 0.0, None, 0, 0, 1, "", 1e-6)
        fx = T.rows_inputs(fc)
        fx["res"] = T.window(rows)
        stats = T.inside(fx["stats_out"], _run_rows(native, fc, fx)["stats_out"])
        xb = dict(x, x_ln=T.window(rows), stats=T.window(stats))
        runs[name] = (xb, _run_rows(native, c, xb), stats)
    xb, got, stats = runs["constant"]
    print(f"TF-EDGES gpu spacap_tf_rows_f32 {c.name}: r of the constant rows={stats[[0, 5], 1]} 1 / r - eps={F32(1) / stats[[0, 5], 1] - F32(1e-6)}")
    assert (stats[[0, 5], 0] == [0.0, 0.75]).all() and (F32(1) / stats[[0, 5], 1] - F32(1e-6) == 0).all()
    for k in ("x_out", "n_out", "out2"):
        v = T.inside(x[k], got[k])
        print(f"TF-EDGES gpu spacap_tf_rows_f32 {c.name}: {k} non-finite in the constant rows: {int((~np.isfinite(v[[0, 5]])).sum())}/{v[[0, 5]].size}")
    _settle(T.rows_check(c, xb, got, tag="TF-EDGES gpu"))
    other = [r for r in range(17) if r not in (0, 5)]
    ok = True
    for k in ("x_out", "n_out", "out2"):
        v = T.inside(x[k], got[k])
        ok &= bool(np.isfinite(v).all())
        ok &= _same(f"spacap_tf_rows_f32 {c.name}", f"{k} of the other rows", v[other], T.inside(x[k], runs["ordinary"][1][k])[other])
    assert ok


# ---- spacap_tf_gemm_f32, spacap_tf_ffn1_f32, spacap_tf_dgrad_mask_f32 -----------------------------------------------------------------
@pytest.mark.parametrize("case", T.GEMM_CASES, ids=_name)
def test_split_product_and_its_epilogues_at_every_edge(native, case):
    lib, check = native.lib, native.check
    c, x = case, T.gemm_inputs(case)
    (xt, px), (wt, pw), (out, po) = _dev(x["x"]), _dev(x["W"]), _dev(x["out"])      # (named: the operands live until the call has run)
    if c.entry == "gemm":
        assert 1 <= lib.spacap_tf_gemm_splits(c.R, c.K, c.N) == T.gemm_splits(c.R, c.K, c.N)
        check(lib.spacap_tf_gemm_f32(px, pw, c.R, c.K, c.N, c.trans, c.nsplit, po, _stream()), "spacap_tf_gemm_f32")
    elif c.entry == "ffn1":
        bias = _dev(x["bias"]) if c.bias else (None, None)
        cnt, pc = _counter(c.counter)
        check(lib.spacap_tf_ffn1_f32(px, pw, bias[1], c.R, c.N, c.p, c.seed, pc, po, _stream()), "spacap_tf_ffn1_f32")
    else:
        y = _dev(x["y"])
        check(lib.spacap_tf_dgrad_mask_f32(px, pw, y[1], T.drop_scale(c.p), c.R, c.K, c.N, po, _stream()), "spacap_tf_dgrad_mask_f32")
    torch.cuda.synchronize()
    _settle(T.gemm_check(c, x, {"out": out.cpu().numpy()}, tag="TF-EDGES gpu"))


# ---- spacap_tf_ffn_f32, spacap_tf_ffn_bf3_f32, spacap_tf_ffn_split_f32 ------------------------------------------------------------------
def _run_ffn(native, case, x, R=None):
    lib, check = native.lib, native.check
    c = case
    devs = {k: _dev(w) for k, w in x.items() if w is not None}
    ptr = lambda k: devs[k][1] if k in devs else None
    cnt, pc = _counter(c.counter)
    R = c.R if R is None else R
    if c.bf3:
        img = torch.tensor(T.split_images(T.inside(x["W1"]), T.inside(x["W2"])).reshape(-1)).to(DEV, torch.bfloat16)
        assert img.numel() == lib.spacap_tf_ffn_pieces_elems(c.dff)
        check(lib.spacap_tf_ffn_bf3_f32(c.mode, ptr("x"), img.data_ptr(), ptr("bias"), ptr("y"), R, c.dff, c.p, c.seed, pc, ptr("hid"), ptr("part"), _stream()),
              "spacap_tf_ffn_bf3_f32")
    else:
        wa, wb = ("W1", "W2") if c.mode == 0 else ("W2", "W1")
        check(lib.spacap_tf_ffn_f32(c.mode, ptr("x"), ptr(wa), ptr(wb), ptr("bias"), ptr("y"), R, c.dff, c.p, c.seed, pc, ptr("hid"), ptr("part"), _stream()),
              "spacap_tf_ffn_f32")
    torch.cuda.synchronize()
    return {k: devs[k][0].cpu().numpy() for k in ("hid", "part") if k in devs}


@pytest.mark.parametrize("case", T.FFN_CASES, ids=_name)
def test_feed_forward_block_at_every_edge(native, case):
    x = T.ffn_inputs(case)
    _settle(T.ffn_check(case, x, _run_ffn(native, case, x), tag="TF-EDGES gpu"))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", ["int", "real"])
def test_feed_forward_tile_sizes_agree_bit_for_bit(native, kind, mode):
    """R = 513 runs the 64-row tiles, R = 512 the 16-row tiles, on the same operands: rows 0 .. 511 of hid and of every part[c]"""
    c = next(k for k in T.FFN_CASES if not k.bf3 and k.R == 513 and k.kind == kind and k.mode == mode)
    assert not T.ffn_small(513) and T.ffn_small(512)
    x = T.ffn_inputs(c._replace(hid=1))
    c = c._replace(hid=1)
    big, small = _run_ffn(native, c, x), _run_ffn(native, c, x, R=512)
    ok = _same(f"spacap_tf_ffn_f32 {c.name} R=512 against R=513", "hid rows 0..511", T.inside(x["hid"], big["hid"])[:512], T.inside(x["hid"], small["hid"])[:512])
    # (part of R = 512 is laid out [dff / 128][512][128] from the same pointer)
    pb = T.inside(x["part"], big["part"])[:, :512]
    ps = small["part"][x["part"].start:x["part"].start + pb.size].reshape(pb.shape)
    ok &= _same(f"spacap_tf_ffn_f32 {c.name} R=512 against R=513", "part rows 0..511 of every slice", pb, ps)
    assert ok and not np.isnan(ps).any()


@pytest.mark.parametrize("case", T.SPLIT_CASES, ids=_name)
def test_piece_images_in_operand_order(native, case):
    """1, 16 and 17 layers (a second launch) against the restated pieces, exactly"""
    lib, check = native.lib, native.check
    c, x = case, T.split_inputs(case)
    w1, w2 = [_dev(w) for w in x["W1"]], [_dev(w) for w in x["W2"]]
    outs = [_dev(w, torch.bfloat16) for w in x["out"]]
    arr = ctypes.c_void_p * c.nlayers
    check(lib.spacap_tf_ffn_split_f32(arr(*[p for _, p in w1]), arr(*[p for _, p in w2]), arr(*[p for _, p in outs]), c.nlayers, c.dff, _stream()),
          "spacap_tf_ffn_split_f32")
    torch.cuda.synchronize()
    _settle(T.split_check(c, x, [t.float().cpu().numpy() for t, _ in outs], tag="TF-EDGES gpu"))


# ---- the autograd nodes with dropout ON: float64 autograd of the reference formulas under the restated masks ------------------------------
# Bars: the max-norm relative bars tests/test_tf_layer_gpu.py holds the same nodes to at p = 0 (3e-6 on values, 2e-5 on gradients).
# With the masks bit for bit the reference's, dropout adds no arithmetic to any stage but one scaling by float32(1 / (1 - p)).
B_, L_, DFF, P_SUB, P_FFN, EPS = 2, 20, 256, 0.1, 0.25, float(np.float32(1e-6))
VALUE_BAR, GRAD_BAR = 3e-6, 2e-5
ATTN_GRAD_BAR = 5e-5      # the gradient that also passes the attention backward: that file's bar for gradients through attention


def _ln64(x, a, b):
    return a * (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + EPS) + b


def _leaves():
    g = torch.Generator().manual_seed(11)
    rn = lambda *s, scale=1.0, shift=0.0: (torch.randn(*s, generator=g) * scale + shift).to(DEV).requires_grad_()
    return dict(a=rn(B_, L_, 128), x=rn(B_, L_, 128), Wo=rn(128, 128, scale=0.1), bo=rn(128), l2a=rn(128, scale=0.3, shift=1.0), l2b=rn(128),
                W1=rn(DFF, 128, scale=0.1), b1=rn(DFF, scale=0.1), W2=rn(128, DFF, scale=0.05), b2=rn(128), l3a=rn(128, scale=0.3, shift=1.0), l3b=rn(128),
                pw=rn(384, 128, scale=0.1), pb=rn(384), qkv=rn(B_, L_, 384))


def _keep(ncols, p, seed, counter):
    return torch.tensor(T.keep_mask(B_ * L_, ncols, ncols, p, seed, counter).reshape(B_, L_, ncols)).double() * T.drop_scale(p)


def _attention64(qkv):
    q, k, v = (t.reshape(B_, L_, 8, 16).transpose(1, 2) for t in qkv.split(128, -1))
    p = torch.softmax(q @ k.transpose(-1, -2) / 4.0, -1)
    return (p @ v).transpose(1, 2).reshape(B_, L_, 128)


def _chain64(v, seeds, counter, inside):
    """(x1, h, x2, n, qkv_next) in float64 from the float64 leaves ``v``"""
    a = _attention64(v["qkv"]) if inside else v["a"]
    x1 = v["x"] + _keep(128, P_SUB, seeds[0], counter) * (a @ v["Wo"].t() + v["bo"])
    h = _keep(DFF, P_FFN, seeds[1], counter) * torch.relu(_ln64(x1, v["l2a"], v["l2b"]) @ v["W1"].t() + v["b1"])
    x2 = x1 + _keep(128, P_SUB, seeds[2], counter) * (h @ v["W2"].t() + v["b2"])
    n = _ln64(x2, v["l3a"], v["l3b"])
    return x1, h, x2, n, n @ v["pw"].t() + v["pb"]


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("last", [False, True], ids=["next-projection", "final-norm"])
@pytest.mark.parametrize("inside", [False, True], ids=["AttnOutFfn1", "AttnFfn1"])
def test_nodes_with_dropout_against_float64_autograd_under_the_restated_masks(native, inside, last):
    from spacap3d_amd import attention as att, tf_layer as tf
    lv = _leaves()
    seeds = (4242, 777001, (1 << 40) + 12345)
    counter = int(att.rng_state(DEV).item())
    tail = (lv["Wo"], lv["bo"], lv["l2a"], lv["l2b"], lv["W1"], lv["b1"], lv["W2"], 1e-6, P_SUB, P_FFN, seeds[0], seeds[1])
    if inside:
        x1, h, parts = tf.AttnFfn1.apply(lv["qkv"], lv["x"], None, 0, 0, 8, 0.0, 0, *tail)
    else:
        x1, h, parts = tf.AttnOutFfn1.apply(lv["a"], lv["x"], *tail)
    args = (h, parts, x1, lv["W1"], lv["W2"], lv["b2"], lv["l3a"], lv["l3b"], 1e-6, P_SUB, P_FFN, seeds[2])
    g = torch.Generator().manual_seed(12)
    g1, g2, g3 = (torch.randn(B_, L_, n, generator=g).to(DEV) for n in (128, 384, 128))
    if last:
        (n,) = tf.Ffn2Ln.apply(*args, None, None)
        (n * g3).sum().backward()
    else:
        x2, qkv2 = tf.Ffn2Ln.apply(*args, lv["pw"], lv["pb"])
        ((x2 * g1).sum() + (qkv2 * g2).sum()).backward()
    v = {k: t.detach().double().cpu().requires_grad_() for k, t in lv.items()}
    r1, rh, r2, rn_, rq = _chain64(v, seeds, counter, inside)
    if last:
        (rn_ * g3.double().cpu()).sum().backward()
        values = {"x1": (x1, r1), "h": (h, rh), "n": (n, rn_)}
    else:
        ((r2 * g1.double().cpu()).sum() + (rq * g2.double().cpu()).sum()).backward()
        values = {"x1": (x1, r1), "h": (h, rh), "x2": (x2, r2), "qkv": (qkv2, rq)}
    used = [k for k in lv if k != ("a" if inside else "qkv") and not (last and k in ("pw", "pb"))]
    zeros = {k: int((a.detach().cpu() == 0).sum()) - int((b.detach() == 0).sum()) for k, (a, b) in values.items() if k == "h"}
    fig_v = {k: _rel(a, b) for k, (a, b) in values.items()}
    fig_g = {k: _rel(lv[k].grad, v[k].grad) for k in used}
    name = f"{'AttnFfn1' if inside else 'AttnOutFfn1'} -> Ffn2Ln ({'final norm' if last else 'next projection'})"
    print(f"TF-EDGES gpu nodes {name} p_sub={P_SUB} p_ffn={P_FFN} counter={counter}: values {fig_v} (bar {VALUE_BAR}) gradients {fig_g} (bar {GRAD_BAR}) "
          f"zeros of h beyond the reference's={zeros} dropped of h={int((T.keep_mask(B_ * L_, DFF, DFF, P_FFN, seeds[1], counter) == 0).sum())}")
    assert all(f < VALUE_BAR for f in fig_v.values()) and all(f < (ATTN_GRAD_BAR if k == "qkv" else GRAD_BAR) for k, f in fig_g.items())
    assert float((rh == 0).double().mean()) > P_FFN and all(lv[k].grad is not None for k in used)


def test_first_norm_and_projection_node_against_float64_autograd(native):
    from spacap3d_amd import tf_layer as tf
    lv = _leaves()
    qkv, xres = tf.LnQkv.apply(lv["x"], lv["l2a"], lv["l2b"], 1e-6, lv["pw"], lv["pb"])
    g = torch.Generator().manual_seed(13)
    gq, gr = torch.randn(B_, L_, 384, generator=g).to(DEV), torch.randn(B_, L_, 128, generator=g).to(DEV)
    ((qkv * gq).sum() + (xres * gr).sum()).backward()
    v = {k: lv[k].detach().double().cpu().requires_grad_() for k in ("x", "l2a", "l2b", "pw", "pb")}
    ref = _ln64(v["x"], v["l2a"], v["l2b"]) @ v["pw"].t() + v["pb"]
    ((ref * gq.double().cpu()).sum() + (v["x"] * gr.double().cpu()).sum()).backward()
    fig_g = {k: _rel(lv[k].grad, v[k].grad) for k in v}
    print(f"TF-EDGES gpu nodes LnQkv R={B_ * L_}: qkv {_rel(qkv, ref)} (bar {VALUE_BAR}) gradients {fig_g} (bar {GRAD_BAR})")
    assert _rel(qkv, ref) < VALUE_BAR and torch.equal(xres, lv["x"]) and all(f < GRAD_BAR for f in fig_g.values())
