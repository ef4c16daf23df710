"""The kernels of csrc/dense_rows.hip (and their parent, csrc/linear_rows.hip) at every edge of their dispatch, against the float64
restatement of tests/dense_rows_restated.py: the C ABI called through ``_native.lib`` on the windows of its tables, and a short
table through the Python layer (``linear.dense_product``, ``linear.vocab_projection``, ``relation.RelationU``).

``int`` cases (operands from {+-1, +-2, +-3}): every product and partial sum is exact in float32, so the written elements are
compared with the float64 reference under exact equality -- no tolerance.  ``real`` cases: elementwise within the a-priori bar
(n + 2) 2^-24 (sum |a| |w| + |bias|).  Always: every element outside the mask of what the call may write still holds the
sentinel the allocation was filled with, and no NaN appears (every float of padding the contract does not name is NaN on the
way in).  Partial results are compared slice by slice and slab by slab (the elementwise comparison of the whole buffer, with
the count per slice printed) and once more added in order.  A +Inf and a NaN in A (or X) must come out as the float64
reference has them, NaN, +Inf and -Inf each in its place, and exact everywhere else.
Each comparison prints its figures before it asserts (``DENSE-EDGES gpu <entry> <case> ...``, pytest -s)."""
import numpy as np
import pytest
import torch

import dense_rows_restated as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_name = lambda c: c.name


@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spacap3d_amd import _native
    return _native


def _dev(win):
    t = torch.tensor(win.buf).to(DEV)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * win.start


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _hold(entry, case, what, got, want, mask, allowed=None, before=None):
    """got: the whole allocation after the call (float32); want, mask: the reference's; allowed: the bar (``real`` cases);
    before: the allocation before the call (default: all sentinel).  Prints, then asserts."""
    got, want = np.asarray(got), np.asarray(want, np.float64)
    assert got.dtype == np.float32 and got.shape == want.shape == mask.shape
    before = np.full(got.shape, D.SENTINEL, np.float32) if before is None else before
    broken = int((got[~mask] != before[~mask]).sum())
    finite = mask & np.isfinite(want)
    nonfinite = D.same_nonfinite(got[mask], want[mask])
    stray = int(np.isnan(got[finite]).sum())
    cls = lambda v: np.isnan(v) * 1 + np.isposinf(v) * 2 + np.isneginf(v) * 3
    head = f"DENSE-EDGES gpu {entry} {case.name} {what}:"
    tail = f"sentinels broken={broken}/{int((~mask).sum())} NaN where the reference is finite={stray} non-finite as the reference={nonfinite}" \
        + (f" (NaN / +Inf / -Inf misplaced at {int((cls(got[mask]) != cls(want[mask])).sum())} of {int((mask & ~finite).sum())})" if (mask & ~finite).any() else "")
    if allowed is None:
        bad = D.mismatches(got[finite], want[finite])
        print(f"{head} mismatches={bad}/{int(finite.sum())} {tail}")
        assert bad == 0
    else:
        ratio = D.figure(got[finite], want[finite], np.asarray(allowed)[finite]) if finite.any() else 0.0
        print(f"{head} largest error / bar={ratio:.3f} over {int(finite.sum())} {tail}")
        assert ratio <= 1.0
    assert broken == 0 and stray == 0 and nonfinite


def _sum_f32(buf, n, count, stride):
    acc = buf[:n].copy()
    with np.errstate(invalid="ignore"):
        for z in range(1, count):
            acc = (acc + buf[z * stride:z * stride + n]).astype(np.float32)
    return acc


# ---- spacap_dense_rows_f32 and spacap_linear_rows_f32 ------------------------------------------------------------------------------
def _run_rows(native, case, parent=False):
    lib, check = native.lib, native.check
    c, x = case, D.rows_inputs(case)
    want, mask = D.rows_reference(c, x)
    allowed = D.bar(c.K, D.rows_magnitude(c, x)) if c.kind == "real" else None
    (a, pa), (W, pw), (out, po) = _dev(x.a), _dev(x.W), _dev(x.out)
    bias = torch.tensor(x.bias).to(DEV) if c.bias else None
    pb = bias.data_ptr() if c.bias else None
    if parent:
        entry = "spacap_linear_rows_f32"
        assert c.lda == c.K and c.ldo == c.CO and c.slices == 1 and lib.spacap_linear_rows_supported(c.R, c.K, c.CO) == 1
        check(lib.spacap_linear_rows_f32(pa, pw, pb, c.R, c.K, c.CO, c.trans, po, _stream()), entry)
    else:
        entry = "spacap_dense_rows_f32"
        check(lib.spacap_dense_rows_f32(pa, c.lda, *c.a_rows, pw, c.ldw, c.trans, pb, c.R, c.K, c.CO, po, c.ldo, *c.o_rows, c.o_zero, c.slices,
                                        c.sstride, c.batch, c.a_z, c.w_z, _stream()), entry)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    s = x.out.start
    if c.slices > 1:
        ok = mask & np.isfinite(want)
        sl = lambda v, z: v[s + z * c.sstride:][:c.sstride]
        per = [D.mismatches(sl(got, z)[sl(ok, z)], sl(want, z)[sl(ok, z)]) for z in range(c.slices)] \
            if c.kind == "int" and c.sstride >= D._extent(c.R, c.CO, c.ldo, c.o_rows) else "-"      # (interleaved batch results: see the total)
        print(f"DENSE-EDGES gpu {entry} {c.name} {'batch' if c.batch else 'split'} of {c.slices}: mismatches per slice={per}"
              f" chunks per slice={'all' if c.batch else D.slice_chunks(c.K, c.slices)}")
    _hold(entry, c, "values", got, want, mask, allowed)
    if c.slices > 1 and not c.batch:
        # the slices added in order: on the host in float32, and by spacap_dense_sum_slices_f32 where its contract takes the layout
        n = D._extent(c.R, c.CO, c.ldo, c.o_rows)
        m0 = mask[s:s + n]
        ref = D.rows_summed(c, want[s:])[:n]
        host = _sum_f32(got[s:], n, c.slices, c.sstride)
        bar = D.bar(c.K + c.slices, D.sum_parts(D.rows_magnitude(c, x)[s:], c.sstride, c.slices)[:n]) if c.kind == "real" else None
        keep = np.where(m0, host, D.SENTINEL).astype(np.float32)
        _hold(entry, c, "slices added in order (host, float32)", keep, np.where(m0, ref, D.SENTINEL), m0, bar)
        if c.sstride % 4 == 0 and s % 4 == 0:
            o2 = torch.full((n + 8,), float(D.SENTINEL), device=DEV)
            check(lib.spacap_dense_sum_slices_f32(po, c.slices, n, c.sstride, o2.data_ptr(), _stream()), "spacap_dense_sum_slices_f32")
            torch.cuda.synchronize()
            dev = o2.cpu().numpy()
            same = np.array_equal(dev[:n], host, equal_nan=True)
            print(f"DENSE-EDGES gpu spacap_dense_sum_slices_f32 {c.name}: bit-identical to the float32 sum in order={same} tail intact={bool((dev[n:] == D.SENTINEL).all())}")
            assert same and (dev[n:] == D.SENTINEL).all()


@pytest.mark.parametrize("case", D.ROWS_CASES, ids=_name)
def test_row_product_at_every_dispatch_edge(native, case):
    _run_rows(native, case)


@pytest.mark.parametrize("case", D.LIN_CASES, ids=_name)
def test_parent_row_panel_kernel_on_the_same_restatement(native, case):
    _run_rows(native, case, parent=True)


def test_row_product_of_no_rows_leaves_the_output_untouched(native):
    lib, check = native.lib, native.check
    c = D.ROWS_CASES[0]._replace(name="R0", R=0)
    x = D.rows_inputs(c._replace(R=4))
    (a, pa), (W, pw), (out, po) = _dev(x.a), _dev(x.W), _dev(x.out)
    check(lib.spacap_dense_rows_f32(pa, c.lda, 0, 0, 0, pw, c.ldw, c.trans, None, 0, c.K, c.CO, po, c.ldo, 0, 0, 0, 0, 1, 0, 0, 0, 0, _stream()), "R = 0")
    check(lib.spacap_dense_rows_f32(None, c.lda, 0, 0, 0, None, c.ldw, c.trans, None, 0, c.K, c.CO, None, c.ldo, 0, 0, 0, 0, 1, 0, 0, 0, 0, _stream()), "R = 0")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    print(f"DENSE-EDGES gpu spacap_dense_rows_f32 R0: elements changed={int((got != D.SENTINEL).sum())}/{got.size}")
    assert (got == D.SENTINEL).all()


# ---- spacap_dense_sum_slices_f32 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.SUM_CASES, ids=_name)
def test_slice_sum_at_the_grid_edges(native, case):
    """n around the float4 and the 1024-element workgroup edges, stride >= n: bit-identical to the float32 sum in order on any
    data, equal to the float64 sum on integers"""
    lib, check = native.lib, native.check
    entry = "spacap_dense_sum_slices_f32"
    c, x = case, D.sum_inputs(case)
    (parts, pp), (out, po) = _dev(x.parts), _dev(x.out)
    check(lib.spacap_dense_sum_slices_f32(pp, c.S, c.n, c.stride, po, _stream()), entry)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    w32, mask = D.sum_reference(c, x, np.float32)
    w64 = D.sum_reference(c, x)[0]
    same = np.array_equal(got[mask], w32[mask], equal_nan=True)
    print(f"DENSE-EDGES gpu {entry} {c.name}: bit-identical to the float32 sum in order={same} blocks={(c.n // 4 + 256) // 256}")
    assert same
    if c.kind == "int":
        _hold(entry, c, "against float64", got, w64, mask)
    else:
        mag = D.sum_slices(np.abs(x.parts.buf[x.parts.start:]), c.S, c.n, c.stride, np.zeros(c.n))[0]
        _hold(entry, c, "against float64", got, w64, mask, np.concatenate([np.zeros(x.out.start), D.bar(c.S, mag), np.zeros(len(got) - x.out.start - c.n)]))


# ---- the weight gradients -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.GRAD_CASES, ids=_name)
def test_weight_gradients_at_every_dispatch_edge(native, case):
    lib, check = native.lib, native.check
    c, x = case, D.grad_inputs(case)
    ref = D.grad_reference(c, x)
    mag = D.grad_reference(c, x, magnitude=True) if c.kind == "real" else None
    (G, pg), (X, px), (out, po) = _dev(x.G), _dev(x.X), _dev(x.out)
    entry = f"spacap_dense_wgrad_{c.entry}_f32"
    if c.entry == "small":
        db, pd = _dev(x.db) if c.db else (None, None)
        check(lib.spacap_dense_wgrad_small_f32(pg, c.ldg, px, c.ldx, *c.x_rows, c.R, c.M, c.N, po, pd, _stream()), entry)
        torch.cuda.synchronize()
        _hold(entry, c, f"dW (m per thread={D.wgrad_small_tier(c.M, c.N)})", out.cpu().numpy(), *ref["dW"], None if mag is None else D.bar(c.R, mag["dW"][0]))
        if c.db:
            _hold(entry, c, "db", db.cpu().numpy(), *ref["db"], None if mag is None else D.bar(c.R, mag["db"][0]))
        return
    if c.entry == "blocks":
        check(lib.spacap_dense_wgrad_blocks_f32(pg, c.ldg, px, c.ldx, c.R, c.Z, c.M, c.N, c.nslab, po, _stream()), entry)
        slabs = D.slab_rows(c.R, c.nslab)
    else:
        check(lib.spacap_dense_wgrad_tall_f32(pg, c.ldg, px, c.ldx, c.R, c.M, c.N, c.nslab, po, _stream()), entry)
        slabs = D.slab_rows(c.R, c.nslab, D.TALL_TILE)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want, mask = ref["part"]
    s, n = x.out.start, c.M * c.Z * c.N
    fin = np.isfinite(want)
    per = [D.mismatches(got[s + i * n:s + (i + 1) * n][fin[s + i * n:s + (i + 1) * n]], want[s + i * n:s + (i + 1) * n][fin[s + i * n:s + (i + 1) * n]])
           for i in range(c.nslab)]
    empty = [i for i, (r0, r1) in enumerate(slabs) if r1 <= r0]
    print(f"DENSE-EDGES gpu {entry} {c.name}: rows per slab={slabs[:6]}{'...' if c.nslab > 6 else ''} empty slabs={len(empty)}"
          + (f" mismatches per slab={per[:6]}{'...' if c.nslab > 6 else ''} (sum {sum(per)})" if c.kind == "int" else ""))
    _hold(entry, c, "slabs", got, want, mask, None if mag is None else D.bar(c.R, mag["part"][0]))
    for i in empty:
        assert (got[s + i * n:s + (i + 1) * n] == 0.0).all(), i
    total = _sum_f32(got[s:], n, c.nslab, n)
    _hold(entry, c, "slabs added in order (host, float32)", total, D.sum_parts(want[s:], n, c.nslab), np.ones(n, bool),
          None if mag is None else D.bar(c.R + c.nslab, D.sum_parts(mag["part"][0][s:], n, c.nslab)))


# ---- through the Python layer: int operands, float64 autograd of the composition -----------------------------------------------------
def _ints(g, *shape):
    return (torch.randint(1, 4, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()


def _exact(entry, name, pairs):
    bad = {k: int((a.detach().double().cpu() != b.detach().cpu()).sum()) for k, (a, b) in pairs.items()}
    print(f"DENSE-EDGES gpu {entry} {name}: mismatches={bad} of {({k: b.numel() for k, (a, b) in pairs.items()})}")
    assert all(a.shape == b.shape for a, b in pairs.values()) and not any(bad.values())


@pytest.mark.parametrize("trans", [True, False], ids=["wT", "w"])
@pytest.mark.parametrize("col0", [0, 1, 3])
def test_dense_product_through_the_python_layer(native, col0, trans):
    """a column slice of W beginning at column 0, 1 and 3 (the set-abstraction modules' W1[:, 3:]), a2 a column window of wider rows"""
    from spacap3d_amd import linear
    R, K, CO = 33, 131, 17
    g = torch.Generator().manual_seed(7 + col0)
    wide = _ints(g, R, K + 6).to(DEV)
    a2 = wide[:, 2:2 + K]
    W = _ints(g, CO if trans else K, col0 + (K if trans else CO)).to(DEV)
    bias = _ints(g, CO).to(DEV) if trans else None
    assert a2.stride(0) == K + 6 and not a2.is_contiguous()
    out = linear.dense_product(a2, W, trans, bias=bias, col0=col0)
    Wv = W[:, col0:].double()
    ref = a2.double() @ (Wv.t() if trans else Wv) + (bias.double() if trans else 0.0)
    _exact("linear.dense_product", f"col0={col0} {'W^T' if trans else 'W'}", {"out": (out, ref)})


@pytest.mark.parametrize("B,L,Dm,V,skip", [(2, 5, 128, 65, 0), (3, 9, 128, 517, 1), (2, 6, 128, 300, 2)])
def test_vocabulary_projection_through_the_python_layer(native, B, L, Dm, V, skip):
    """values and all three gradients, exactly; the data gradient of the skipped positions exactly zero; the second shape splits
    its data gradient over K"""
    from spacap3d_amd import linear
    g = torch.Generator().manual_seed(V)
    n = _ints(g, B, L, Dm).to(DEV).requires_grad_(True)
    lin = torch.nn.Linear(Dm, V).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(_ints(g, V, Dm)), lin.bias.copy_(_ints(g, V))
    slices = int(native.lib.spacap_dense_rows_slices(B * (L - skip), V, Dm))
    assert slices == D.rows_slices(B * (L - skip), V, Dm) and (slices > 1) == (V == 517)
    out = linear.vocab_projection(n, lin, skip)
    n64 = n.detach().double().requires_grad_(True)
    w64, b64 = lin.weight.detach().double().requires_grad_(True), lin.bias.detach().double().requires_grad_(True)
    ref = torch.nn.functional.linear(n64[:, skip:, :], w64, b64)
    go = _ints(g, *ref.shape).to(DEV)
    out.backward(go)
    ref.backward(go.double())
    _exact("linear.vocab_projection", f"B={B} L={L} V={V} skip={skip} slices={slices}",
           {"logits": (out, ref), "dn": (n.grad, n64.grad), "dW": (lin.weight.grad, w64.grad), "db": (lin.bias.grad, b64.grad)})
    assert float(n.grad[:, :skip].abs().sum()) == 0.0


@pytest.mark.parametrize("B,K", [(1, 1), (2, 40)])
def test_relation_value_projection_through_the_python_layer(native, B, K):
    """RelationU on the strided view of a packed q | k | v buffer, against the einsum it replaces"""
    from spacap3d_amd import relation
    H, Dh, C = 8, 16, 128
    g = torch.Generator().manual_seed(K)
    qkv = _ints(g, B, K, 3 * H * Dh).to(DEV).requires_grad_(True)
    W1 = _ints(g, C, H * Dh).to(DEV).requires_grad_(True)
    U = relation.RelationU.apply(qkv[..., 2 * H * Dh:].view(B, K, H, Dh).transpose(1, 2), W1)
    q64, w64 = qkv.detach().double().requires_grad_(True), W1.detach().double().requires_grad_(True)
    ref = torch.einsum("bhjd,ohd->bjho", q64[..., 2 * H * Dh:].view(B, K, H, Dh).transpose(1, 2), w64.view(C, H, Dh))
    go = _ints(g, *ref.shape).to(DEV)
    U.backward(go)
    ref.backward(go.double())
    _exact("relation.RelationU", f"B={B} K={K}", {"U": (U, ref), "dqkv": (qkv.grad, q64.grad), "dW1": (W1.grad, w64.grad)})
