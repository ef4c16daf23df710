"""tests/dense_rows_restated.py is right, and its tables are fit for the device test, checked without a device.
  * the anchor: every restatement against an independent float64 composition -- the operands cut out of their allocations by
    reshaping and slicing (``n[:, skip:, :]``), multiplied with ``@`` or ``einsum`` (``bhjd,ohd->bjho`` of the relation head,
    ``G.T @ X``), the slabs by assigning every row to its slab -- to 1e-12 of the largest reference entry;
  * the conditions the device test depends on: every ``int`` case stays below 2^24 in sum |a| |w| + |b|, none of its operands is
    zero, every case reaches the tier and the 16-byte switches its name claims, and every tier and every setting of every switch
    is reached;
  * the teeth: each wrong rule of ``MUTANTS`` planted in the restatement changes at least one element of at least one ``int``
    case under exact comparison;
  * the host helpers of libspacap_hip.so against their Python restatements over a grid of shapes, and every refusal of the entry
    points: -1 with the message of the argument check, from host code that touches no device.
Each check prints its figures (``DENSE-EDGES cpu ...``, pytest -s)."""
import functools
import itertools

import numpy as np
import pytest
import torch

import dense_rows_restated as D

_name = lambda c: c.name
_ALL_ROWS = D.ROWS_CASES + D.LIN_CASES


# ---- the anchor -----------------------------------------------------------------------------------------------------------------
def _cut(buf, R, ncols, ld, grp=0, gstride=0, skip=0):
    """rows 0 .. R-1 of ``ncols`` floats, cut out of the flat ``buf`` by reshaping and slicing alone (torch, float64)"""
    t = torch.tensor(np.asarray(buf, np.float64))
    pad = lambda n: torch.cat([t, torch.full((max(n - len(t), 0),), float("nan"), dtype=torch.float64)])[:n]
    if grp == 0:
        return pad(R * ld).view(R, ld)[:, :ncols]
    G = -(-R // grp)
    assert gstride >= (grp + skip) * ld
    return pad(G * gstride).view(G, gstride)[:, :(grp + skip) * ld].reshape(G, grp + skip, ld)[:, skip:, :ncols].reshape(-1, ncols)[:R]


def _scale(t):
    return max(float(t[torch.isfinite(t)].abs().max()) if torch.isfinite(t).any() else 0.0, 1.0)


@pytest.mark.parametrize("case", [c for c in _ALL_ROWS if not c.poison], ids=_name)
def test_row_product_restated_against_the_sliced_composition(case):
    c, x = case, D.rows_inputs(case)
    call = D.rows_call(c, x)
    exp, mask = D.rows(*call)
    a, W, out = call[0], call[5], call[12]
    worst, written = 0.0, 0
    total = torch.zeros(c.R, c.CO, dtype=torch.float64)
    for z in range(c.slices):
        az, wz = (z * c.a_z, z * c.w_z) if c.batch else (0, 0)
        A = _cut(a[az:], c.R, c.K, c.lda, *c.a_rows)
        Wop = _cut(W[wz:], c.CO, c.K, c.ldw).t() if c.trans else _cut(W[wz:], c.K, c.CO, c.ldw)
        ref = A @ Wop + (torch.tensor(x.bias, dtype=torch.float64) if c.bias else 0.0)
        got = _cut(exp[z * c.sstride:], c.R, c.CO, c.ldo, *c.o_rows)
        written += c.R * c.CO
        if c.batch or c.slices == 1:
            worst = max(worst, float((got - ref).abs().max()) / _scale(ref))
        else:
            total += got
            if z == c.slices - 1:
                worst = float((total - ref).abs().max()) / _scale(ref)
        if c.o_zero and c.o_rows[0] and c.o_rows[2]:      # the skipped rows: what the rows of a group with skip = 0 would be
            grp, gstride, skip = c.o_rows
            G = -(-c.R // grp)
            head = _cut(exp[z * c.sstride:], G * (grp + skip), c.CO, c.ldo, grp + skip, gstride, 0).view(G, grp + skip, c.CO)[:, :skip]
            assert bool((head == 0.0).all())
            written += G * skip * c.CO
    print(f"DENSE-EDGES cpu float64 rows {c.name} error / scale={worst:.1e} written={int(mask.sum())}")
    assert worst < D.F64_BAR and int(mask.sum()) == written
    assert np.array_equal(exp[~mask], np.asarray(out, np.float64)[~mask]) and not np.isnan(exp).any()
    if c.slices > 1 and not c.batch:      # the bias in slice 0 alone; a slice past the last chunk is zeros
        nch = -(-c.K // 128)
        per = -(-nch // c.slices)
        Wop = _cut(W, c.CO, c.K, c.ldw).t() if c.trans else _cut(W, c.K, c.CO, c.ldw)
        A = _cut(a, c.R, c.K, c.lda, *c.a_rows)
        for z in range(c.slices):
            got = _cut(exp[z * c.sstride:], c.R, c.CO, c.ldo, *c.o_rows)
            k0, k1 = z * per * 128, min((z + 1) * per * 128, c.K)
            ref = A[:, k0:k1] @ Wop[k0:k1] if k0 < c.K else torch.zeros(c.R, c.CO, dtype=torch.float64)
            if z == 0 and c.bias:
                ref = ref + torch.tensor(x.bias, dtype=torch.float64)
            assert float((got - ref).abs().max()) / _scale(ref) < D.F64_BAR, z
            if k0 >= c.K:
                assert bool((got == 0.0).all())
        summed = _cut(D.rows_summed(c, exp), c.R, c.CO, c.ldo, *c.o_rows)      # the slices added in order: the whole product
        assert float((summed - (A @ Wop + (torch.tensor(x.bias, dtype=torch.float64) if c.bias else 0.0))).abs().max()) / _scale(summed) < D.F64_BAR


@pytest.mark.parametrize("kind", ["int", "real"])
def test_relation_cases_against_the_einsum(kind):
    """the two batch-mode calls of RelationU at H = 3, D = 5, C = 17: U = einsum('bhjd,ohd->bjho', V, W1.view(C, H, D)) on the
    strided view of a packed q | k | v buffer, and dV = einsum('bjho,ohd->bjhd', dU, W1.view(C, H, D))"""
    H, Dh, C, B, Kp = 3, 5, 17, 2, 9
    by = {c.name: c for c in D.ROWS_CASES}
    u, dv = by[f"relation-u-{kind}"], by[f"relation-dv-{kind}"]
    x = D.rows_inputs(u)
    assert x.a.start % 4 == 2 and u.lda == 3 * H * Dh and u.R == B * Kp
    qkv = torch.tensor(np.asarray(x.a.buf[x.a.start - 2 * H * Dh:], np.float64))[:B * Kp * 3 * H * Dh].view(B, Kp, 3 * H * Dh)
    V = qkv[..., 2 * H * Dh:].view(B, Kp, H, Dh).transpose(1, 2)
    W1 = torch.tensor(np.asarray(x.W.buf[x.W.start:x.W.start + C * H * Dh], np.float64)).view(C, H * Dh)
    ref = torch.einsum("bhjd,ohd->bjho", V, W1.view(C, H, Dh))
    exp, mask = D.rows(*D.rows_call(u, x))
    got = torch.tensor(exp[:B * Kp * H * C]).view(B, Kp, H, C)
    assert float((got - ref).abs().max()) / _scale(ref) < D.F64_BAR and int(mask.sum()) == ref.numel() and mask[:ref.numel()].all()
    x = D.rows_inputs(dv)
    dU = torch.tensor(np.asarray(x.a.buf[x.a.start:x.a.start + B * Kp * H * C], np.float64)).view(B, Kp, H, C)
    W1 = torch.tensor(np.asarray(x.W.buf[x.W.start:x.W.start + C * H * Dh], np.float64)).view(C, H * Dh)
    ref = torch.einsum("bjho,ohd->bjhd", dU, W1.view(C, H, Dh))
    exp, mask = D.rows(*D.rows_call(dv, x))
    got = torch.tensor(exp[:B * Kp * H * Dh]).view(B, Kp, H, Dh)
    assert float((got - ref).abs().max()) / _scale(ref) < D.F64_BAR and int(mask.sum()) == ref.numel()


@pytest.mark.parametrize("case", [c for c in D.GRAD_CASES if not c.poison], ids=_name)
def test_weight_gradients_restated_against_the_transposed_product(case):
    """G.T @ X on the cut-out operands; the slabs by the slab every row belongs to (row / per, or tile / per), not by ranges"""
    c, x = case, D.grad_inputs(case)
    ref = D.grad_reference(c, x)
    G = _cut(x.G.buf[x.G.start:], c.R, c.Z * c.M, c.ldg)
    X = _cut(x.X.buf[x.X.start:], c.R, c.Z * c.N, c.ldx, *c.x_rows)
    if c.entry == "small":
        exp, mask = ref["dW"]
        dW = G.t() @ X
        got = torch.tensor(exp[x.out.start:x.out.start + c.M * c.N]).view(c.M, c.N)
        worst = float((got - dW).abs().max()) / _scale(dW)
        assert int(mask.sum()) == c.M * c.N
        if c.db:
            eb, mb = ref["db"]
            assert float((torch.tensor(eb[x.db.start:x.db.start + c.M]) - G.sum(0)).abs().max()) / _scale(G.sum(0)) < D.F64_BAR and int(mb.sum()) == c.M
        if c.R == 0:
            assert bool((got == 0.0).all())
    else:
        exp, mask = ref["part"]
        unit = 1 if c.entry == "blocks" else D.TALL_TILE
        n = -(-c.R // unit)
        per = -(-n // c.nslab)
        slab_of = (torch.arange(c.R) // unit) // per
        onehot = (slab_of[None, :] == torch.arange(c.nslab)[:, None]).double()          # [nslab][R]
        want = torch.einsum("sr,rzm,rzn->smzn", onehot, G.view(c.R, c.Z, c.M), X.view(c.R, c.Z, c.N))
        got = torch.tensor(exp[x.out.start:x.out.start + want.numel()]).view(want.shape)
        worst = float((got - want).abs().max()) / _scale(want)
        assert int(mask.sum()) == want.numel()
        for s in range(c.nslab):
            if not bool((slab_of == s).any()):
                assert bool((got[s] == 0.0).all())
        total = torch.tensor(D.sum_parts(exp[x.out.start:], c.M * c.Z * c.N, c.nslab)).view(c.M, c.Z, c.N)
        full = torch.einsum("rzm,rzn->mzn", G.view(c.R, c.Z, c.M), X.view(c.R, c.Z, c.N))
        assert float((total - full).abs().max()) / _scale(full) < D.F64_BAR
    print(f"DENSE-EDGES cpu float64 {c.entry} {c.name} error / scale={worst:.1e}")
    assert worst < D.F64_BAR and not np.isnan(exp).any()


@pytest.mark.parametrize("case", D.SUM_CASES, ids=_name)
def test_slice_sum_restated_against_a_plain_sum(case):
    x = D.sum_inputs(case)
    exp, mask = D.sum_reference(case, x)
    parts = _cut(x.parts.buf[x.parts.start:], case.S, case.n, case.stride)
    got = torch.tensor(exp[x.out.start:x.out.start + case.n])
    assert int(mask.sum()) == case.n and case.stride >= case.n and case.stride % 4 == 0
    if case.poison:
        assert D.same_nonfinite(got.numpy(), parts.sum(0).numpy()) and int(torch.isnan(got).sum()) == 2 and int(torch.isposinf(got).sum()) == 1
    else:
        assert float((got - parts.sum(0)).abs().max()) / _scale(parts.sum(0)) < D.F64_BAR
        e32 = D.sum_reference(case, x, np.float32)[0]
        assert e32.dtype == np.float32 and D.figure(e32, exp, D.bar(case.S, np.abs(parts.numpy()).sum(0).max())) <= 1.0


# ---- the conditions the device test depends on ---------------------------------------------------------------------------------
def test_integer_cases_are_exact_in_float32_and_hold_no_zero():
    worst = 0.0
    for c in _ALL_ROWS:
        x = D.rows_inputs(c)
        if c.kind == "int":
            mag, mask = D.rows_magnitude(c, x), D.rows_reference(c, x)[1]
            m = mag[mask & np.isfinite(mag)]
            worst = max(worst, float(m.max()))
            assert (x.a.buf != 0).all() and (x.W.buf != 0).all() and (x.bias is None or (x.bias != 0).all()), c.name
            if not c.poison:
                assert np.array_equal(np.rint(m), m)
    for c in D.GRAD_CASES:
        x = D.grad_inputs(c)
        if c.kind == "int":
            for q, (mag, mask) in D.grad_reference(c, x, magnitude=True).items():
                m = mag[mask & np.isfinite(mag)]
                worst = max(worst, float(m.max()))
            assert (x.G.buf != 0).all() and (x.X.buf != 0).all(), c.name
    for c in D.SUM_CASES:
        if c.kind == "int":
            x = D.sum_inputs(c)
            assert (x.parts.buf != 0).all() and 3 * c.S < 2 ** 24
    print(f"DENSE-EDGES cpu largest sum |a| |w| + |b| of an int case: {worst:.0f} (2^24 = {2 ** 24})")
    assert worst < 2 ** 24
    # a float32 sum of such terms in a random order is the float64 sum, to the bit
    rng = np.random.default_rng(0)
    a, w = D._values(rng, 401, "int"), D._values(rng, 401, "int")
    acc = np.float32(0)
    for k in rng.permutation(401):
        acc = np.float32(acc + np.float32(a[k] * w[k]))
    assert float(acc) == float(a.astype(np.float64) @ w.astype(np.float64))


def test_real_tables_hold_cases_with_a_bar_below_2_to_minus_18():
    """16 terms or fewer: (n + 2) 2^-24 <= 18 * 2^-24 < 2^-18 of sum |a| |w|, tight enough to notice a lost low-order piece"""
    assert any(c.kind == "real" and c.K <= 16 for c in D.ROWS_CASES) and (16 + 2) * D.U < 2.0 ** -18
    for table in (D.SMALL_CASES, D.BLOCKS_CASES, D.TALL_CASES):
        assert any(c.kind == "real" and 1 <= c.R <= 16 for c in table)


def test_every_case_reaches_the_tier_and_the_switches_its_name_claims():
    reached = set()
    for c in _ALL_ROWS:
        x = D.rows_inputs(c)
        vec = D.rows_vec_of(c, x)
        assert vec == tuple(s in c.vec for s in "awo"), (c.name, vec, c.vec)
        if c.tier:
            assert c.tier == D.rows_tier(c.R), c.name
        assert ("off-base" not in c.name) or (x.a.start % 4, x.W.start % 4, x.out.start % 4).count(1) == 1
        reached |= {(("lin-" if c in D.LIN_CASES else "") + D.rows_tier(c.R), bool(c.trans))} | {(s, on) for s, on in zip("awo", vec)}
        # each switch-off case has exactly the one switch off that it names
        if c.name.startswith("vec-"):
            assert [s for s, on in zip("awo", vec) if not on] == [c.name[4]], c.name
    want = {(t, w) for t in ("MT2", "MT4", "lin-MT2", "lin-MT4") for w in (True, False)} | {(s, on) for s in "awo" for on in (True, False)}
    assert reached == want, want - reached
    # all three switches on with K % 4 != 0 (the K tail inside a vectorised quad) and with CO % 4 != 0
    assert any(c.vec == "awo" and c.K % 4 and c.K > 4 and c.trans for c in D.ROWS_CASES) and any(c.vec == "awo" and c.CO % 4 for c in D.ROWS_CASES)
    assert D.rows_tier(1024) == "MT2" and D.rows_tier(1025) == "MT4"
    tiers = set()
    for c in D.SMALL_CASES + D.TALL_CASES:
        tier = D.wgrad_small_tier(c.M, c.N) if c.entry == "small" else D.wgrad_tall_tier(c.N)
        if c.tier is not None:
            assert c.tier == tier, c.name
        tiers.add((c.entry, tier))
    assert tiers == {("small", 2), ("small", 8), ("tall", 1), ("tall", 9)}
    assert (-(-1411 // 64)) * (-(-1027 // 128)) == 207 and (-(-1347 // 64)) * (-(-1027 // 128)) == 198
    # the split cases: counts that do not divide, and slices without a chunk
    assert D.slice_chunks(300, 4)[3] == (384, 300) and D.slice_chunks(401, 3) == [(0, 256), (256, 401), (512, 401)]
    assert D.slab_rows(13, 2) == [(0, 7), (7, 13)] and D.slab_rows(70, 2, 32) == [(0, 64), (64, 70)] and D.slab_rows(9, 10)[9] == (9, 9)


# ---- the teeth --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(case):
    if isinstance(case, D.RowsCase):
        x = D.rows_inputs(case)
        return x, {"out": D.rows_reference(case, x)}
    x = D.grad_inputs(case)
    return x, D.grad_reference(case, x)


def _differs(case, mutant):
    x, ref = _reference(case)
    got = {"out": D.rows_reference(case, x, mutant)} if isinstance(case, D.RowsCase) else D.grad_reference(case, x, mutant)
    return sum(D.mismatches(got[q][0], ref[q][0]) for q in ref)


@pytest.mark.parametrize("mutant", D.MUTANTS)
def test_the_integer_tables_have_teeth(mutant):
    cases = [c for c in D.ROWS_CASES + D.GRAD_CASES if c.kind == "int" and not c.poison and getattr(c, "M", 0) < 1000]
    hits = {c.name: n for c in cases for n in [_differs(c, mutant)] if n}
    first = next(iter(hits.items()), None)
    print(f"DENSE-EDGES cpu mutant {mutant}: {len(hits)}/{len(cases)} int cases differ, first {first}")
    assert hits
    assert not any(_differs(c, "") for c in cases[::7])


# ---- the host helpers and the refusals: libspacap_hip.so on the CPU ---------------------------------------------------------------
def test_host_helpers_agree_with_their_restatements():
    from spacap3d_amd._native import lib
    Rs = (0, 1, 31, 32, 33, 248, 1024, 1025, 2048, 4096, 8192, 40000, 320000)
    n = 0
    for R, K, CO in itertools.product(Rs, (1, 127, 128, 384, 385, 512, 513, 3001, 100000), (1, 64, 65, 128, 3001, 8192)):
        assert lib.spacap_dense_rows_slices(R, K, CO) == D.rows_slices(R, K, CO), (R, K, CO)
        n += 1
    assert D.rows_slices(248, 3001, 128) == lib.spacap_dense_rows_slices(248, 3001, 128) > 1 and D.rows_slices(24, 517, 128) == 5
    for R in Rs + (127, 128, 129, 8191, 8193, 10 ** 7):
        assert lib.spacap_dense_wgrad_blocks_slabs(R) == D.wgrad_blocks_slabs(R), R
    for R, M, N in itertools.product(Rs, (1, 3, 63, 64, 65, 100, 3001, 4096), (1, 7, 15, 16, 17, 132, 144, 145, 2049, 4096)):
        assert lib.spacap_dense_wgrad_tall_slabs(R, M, N) == D.wgrad_tall_slabs(R, M, N), (R, M, N)
        n += 1
    assert 4096 * 4096 > 8 << 20 and D.wgrad_tall_slabs(320000, 4096, 4096) == 1 and D.wgrad_tall_slabs(320000, 64, 7) > 1
    print(f"DENSE-EDGES cpu host helpers: {n} shapes agree")


def test_every_refusal_returns_minus_one_before_any_launch():
    from spacap3d_amd._native import lib
    p = 1 << 12                       # non-null, 16-byte aligned and never dereferenced: every call returns from its checks

    def rows(a=p, lda=8, a_grp=0, a_gs=0, a_skip=0, W=p, ldw=8, trans=1, R=1, K=8, CO=8, out=p, ldo=8, o_grp=0, o_gs=0, o_skip=0, slices=1, ss=0):
        rc = lib.spacap_dense_rows_f32(a, lda, a_grp, a_gs, a_skip, W, ldw, trans, None, R, K, CO, out, ldo, o_grp, o_gs, o_skip, 0, slices, ss, 0, 0, 0, None)
        return rc, lib.spacap_last_error().decode()

    refused = {"K=0": rows(K=0, lda=8), "CO=0": rows(CO=0), "lda<K": rows(lda=7), "ldo<CO": rows(ldo=7), "ldw<K (W^T)": rows(ldw=7, CO=4, ldo=4),
               "ldw<CO (W)": rows(trans=0, K=4, lda=4, ldw=7), "slices=0": rows(slices=0), "slices=65": rows(slices=65, ss=64)}
    for k, (rc, text) in refused.items():
        print(f"DENSE-EDGES cpu refusal rows {k}: {rc} {text!r}")
        assert rc == -1 and "unsupported" in text, k
    assert rows(R=0, a=None, W=None, out=None)[0] == 0                       # R = 0 is a no-op before any pointer is looked at
    for k, (rc, text) in {"a": rows(a=None), "W": rows(W=None), "out": rows(out=None)}.items():
        assert rc == -1 and "null pointer" in text, k
    groups = {"slices>1, slice_stride=0": rows(slices=2, ss=0), "a_grp<0": rows(a_grp=-1), "o_grp<0": rows(o_grp=-1), "a_skip<0": rows(a_grp=1, a_skip=-1),
              "o_skip<0": rows(o_grp=1, o_skip=-1)}
    for k, (rc, text) in groups.items():
        print(f"DENSE-EDGES cpu refusal rows {k}: {rc} {text!r}")
        assert rc == -1 and "bad row groups" in text, k

    def sums(parts=p, S=2, n=8, stride=8, out=p):
        return lib.spacap_dense_sum_slices_f32(parts, S, n, stride, out, None), lib.spacap_last_error().decode()
    for k, (rc, text) in {"stride<n": sums(stride=4), "stride%4": sums(n=5, stride=6), "unaligned parts": sums(parts=p + 4), "unaligned out": sums(out=p + 8),
                          "S=0": sums(S=0), "null": sums(parts=None)}.items():
        print(f"DENSE-EDGES cpu refusal sum_slices {k}: {rc} {text!r}")
        assert rc == -1 and "bad arguments" in text, k
    assert sums(n=0)[0] == 0

    def small(G=p, ldg=8, X=p, ldx=8, x_grp=0, x_skip=0, R=1, M=8, N=8, dW=p):
        return lib.spacap_dense_wgrad_small_f32(G, ldg, X, ldx, x_grp, 0, x_skip, R, M, N, dW, None, None), lib.spacap_last_error().decode()

    def blocks(G=p, ldg=16, X=p, ldx=16, R=1, Z=2, M=8, N=8, nslab=1, part=p):
        return lib.spacap_dense_wgrad_blocks_f32(G, ldg, X, ldx, R, Z, M, N, nslab, part, None), lib.spacap_last_error().decode()

    def tall(G=p, ldg=8, X=p, ldx=8, R=1, M=8, N=8, nslab=1, part=p):
        return lib.spacap_dense_wgrad_tall_f32(G, ldg, X, ldx, R, M, N, nslab, part, None), lib.spacap_last_error().decode()
    sizes = {"small ldg<M": small(ldg=7), "small ldx<N": small(ldx=7), "small x_grp<0": small(x_grp=-1), "small x_skip<0": small(x_skip=-1),
             "small M=0": small(M=0), "blocks ldg<Z M": blocks(ldg=15), "blocks ldx<Z N": blocks(ldx=15), "blocks nslab=0": blocks(nslab=0),
             "blocks nslab=65536": blocks(nslab=65536), "blocks Z=65536": blocks(Z=65536, ldg=1 << 20, ldx=1 << 20), "blocks R=0": blocks(R=0),
             "tall ldg<M": tall(ldg=7), "tall ldx<N": tall(ldx=7), "tall nslab=0": tall(nslab=0), "tall nslab=65536": tall(nslab=65536), "tall R=0": tall(R=0)}
    for k, (rc, text) in sizes.items():
        print(f"DENSE-EDGES cpu refusal {k}: {rc} {text!r}")
        assert rc == -1 and "bad sizes" in text, k
    nulls = {"small G": small(G=None), "small X": small(X=None), "small dW": small(dW=None), "blocks G": blocks(G=None), "blocks X": blocks(X=None),
             "blocks part": blocks(part=None), "tall G": tall(G=None), "tall X": tall(X=None), "tall part": tall(part=None)}
    for k, (rc, text) in nulls.items():
        assert rc == -1 and "null pointer" in text, k
    print(f"DENSE-EDGES cpu refusals: {len(refused) + 3 + len(groups) + 6 + len(sizes) + len(nulls)} calls refused by their argument checks")
