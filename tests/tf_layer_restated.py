"""The contracts of csrc/tf_layer.hip restated in numpy on the host, in float64: the row kernel forward and backward (first part as
a product, as partial sums added in order, or none; dropout; LayerNorm with the unbiased std and eps on the std; the second
product; the attention backward's row term ``delta`` and the per-tile partials of the LayerNorm parameter gradients), the three
epilogues of the split product, both modes of the chained feed-forward block (``hid`` and ``part[c]`` per 128-wide slice), the
four split-bf16 piece images in operand order, the dropout keep mask bit for bit, and the host rules as predicates.  With the
case tables that reach every edge of the dispatch, the seeded inputs, the comparisons the device test runs (``*_check``), and
``*_emulate``: what a kernel that follows the contract -- or, with ``mutant=``, breaks ONE rule of it -- leaves in memory.  Not a
test module; tests/test_tf_layer_restated_cpu.py anchors the restatement to float64 autograd, holds the predicates to the library
and shows that every mutant is rejected; tests/test_tf_layer_edges_gpu.py runs the tables through the kernels.

Written from the header of csrc/tf_layer.hip and include/spacap_hip.h (spacap_tf_rows_args), not from the kernels' loops.

Memory.  Every operand is a window inside a larger allocation with 16 rows of margin on each side: NaN for inputs (a read of
padding shows as a NaN), one finite sentinel for outputs (which must survive wherever the call may not write).

Two kinds of case.
``int``: operands, bias, residual and addend from {+-1, +-2, +-3}, dropout p = 0.5 (scale 2).  Every product, partial sum and sum
of slices is then an integer below 2^24 (asserted per case: ``_int_bound``), also on the split-bf16 path (three bf16 pieces carry
24 bits), so the split product's slices, ``hid`` and ``part`` of the feed-forward kernels, ``x_out`` of the forward row kernel
and the ``sum dn`` half of ``part`` are compared with exact equality.
``real``: standard normal operands, held stage by stage.
  * A product stage is referenced from the kernel's OWN stored input to it (``out2`` from the stored ``n_out`` / ``dy``,
    ``part[c]`` from the stored ``hid``) under the bound of a float32 sum of K exact products in any order,
    (K + 2) 2^-24 (sum |a| |w| + |bias|); K + S for a sum of S slices.
  * A split-bf16 product: each operand is its three bf16 pieces (split_bf16_restated.split3), the kernel adds six of the nine
    piece products, 6 K terms in any order, and leaves three out: (6 K + 2) 2^-24 sum |a_p| |w_q| over the six + sum |a_p| |w_q|
    over the three, all from the pieces themselves (``bf3_bar``).
  * The LayerNorm stages (``n_out``, ``stats``, ``dx``, ``dy``, the ``(x - mu) r`` half of ``part``, ``delta``) have no bound that
    can be derived here.  ``ln_fwd`` / ``ln_bwd`` / ``delta_of`` evaluate the same contract in plain float32 with every sum in
    index order; ``measure_ln`` takes that evaluation's largest error against float64 over all ``real`` cases, in units of
    2^-24 x the natural magnitude of each output (n: |a| |x - mu| r + |b|;  mu: mean |x|;  r: r;  dx: r |dxh| + |c2| |x - mu| +
    |c1| + |addend|;  dy: that x scale;  part: sum over the tile's rows of |dn| (|x| + |mu|) r;  delta: sum |out2| |a|).  The bar is 4
    times the figure (a different order of summation).  Measured on the tables below (the CPU test prints them again and holds
    the measurement to these records):
        output     figure   bar (units of 2^-24 x magnitude)
        n           13.66    54.64
        mu           4.56    18.24
        r            6.37    25.48
        dx          35.67   142.68
        dy          35.67   142.68
        part         8.37    33.48
        delta        2.71    10.84
    Where the backward's first part is a product or a sum of slices, ``dn`` itself is never stored: its a-priori bound e is
    carried through the LayerNorm backward (r |a| e + r mean(|a| e) + |x - mu| r^2 sum(|a| e |x - mu|) / (std 127)) and added.
  ``real`` rows keep their std at or above 1e-3, so the ``1 / r - eps`` cancellation stays out of the bars.  The constant-row
  cases are separate and named: there the restatement is what autograd gives (the term through the std is 0 when std == 0).

numpy only (torch inside split3)."""
import collections
import math

import numpy as np

from sampling_restated import hash32
from split_bf16_restated import PA, PB, split3

F32, F64 = np.float32, np.float64
SENTINEL = F32(-777.25)
U = 2.0 ** -24
D, BM, FM, HEADS, DK = 128, 16, 64, 8, 16
MARGIN_ROWS = 16
# the float32 evaluation's largest error over the ``real`` tables, in units of 2^-24 x magnitude (see the docstring)
LN_FIGURE = {"n": 13.66, "mu": 4.56, "r": 6.37, "dx": 35.67, "dy": 35.67, "part": 8.37, "delta": 2.71}
LN_BAR = {k: 4.0 * v for k, v in LN_FIGURE.items()}
MUTANTS = ("tail-rows", "nparts-skip", "k-chunk", "no-bias1", "biased-std", "eps-under-root", "rows-drop-stride", "ffn-drop-stride",
           "keep>", "relu>=", "delta-head", "ny-overwrite", "pieces-swapped", "layer16")
_cdiv = lambda a, b: -(-a // b)


# ---- host rules ------------------------------------------------------------------------------------------------------------------
def rows_tiles(R):
    """spacap_tf_rows_parts: workgroups (and rows of ``part``) of the row kernel, one per 16 rows"""
    return _cdiv(R, BM)


def ny(R, N2, mode):
    """column blocks of the forward's second product on separate workgroups: N2 / 128 when N2 > 128 on at most 64 row tiles"""
    return N2 // 128 if (mode == 0 and N2 > 128 and rows_tiles(R) <= 64) else 1


def ffn_small(R):
    """tf_ffn_kernel: 16-row tiles up to 512 rows, 64-row tiles beyond"""
    return R <= 512


def gemm_splits(R, K, N):
    """spacap_tf_gemm_splits: the largest divisor of K / 128 that keeps tiles x slices within 512; 0 for a refused shape"""
    if R < 1 or K < 128 or K % 128 or N < 128 or N % 128:
        return 0
    want = max(512 // (_cdiv(R, FM) * (N // 128)), 1)
    return max(s for s in range(1, K // 128 + 1) if (K // 128) % s == 0 and s <= max(want, 1))


def pieces_elems(dff):
    return 4 * 3 * dff * D if dff >= 128 and dff % 128 == 0 else 0


def bf3_map(R, dff):
    """[(row tile, slice of d_ff)] by workgroup of tf_ffn_bf3_kernel: slices dealt to the 8 XCDs when their number is a multiple
    of 8 (XCD x takes slices x n/8 .. (x+1) n/8 - 1 for all tiles), else slice-major"""
    nslice, ntiles = dff // 128, _cdiv(R, 64)
    out = []
    for wg in range(ntiles * nslice):
        if nslice % 8 == 0:
            spx, j = nslice // 8, wg // 8
            out.append((j // spx, (wg % 8) * spx + j % spx))
        else:
            out.append((wg % ntiles, wg // ntiles))
    return out


# ---- dropout ---------------------------------------------------------------------------------------------------------------------
def drop_thresh(p):
    p = float(F32(p))
    return int(math.floor(p * 4294967296.0)) if p > 0.0 else 0


def drop_scale(p):
    """1 / (1 - p) as the host forms it, in float32"""
    return float(F32(1.0) / (F32(1.0) - F32(p)))


def keep_mask(R, ncols, stride, p, seed, counter=None, gt=False):
    """keep[r][c] iff hash32(r * stride + c, seed word) >= floor(float32(p) 2^32); the seed word is seed + counter * golden ratio"""
    th = drop_thresh(p)
    if th == 0:
        return np.ones((R, ncols), bool)
    idx = np.arange(R, dtype=np.uint64)[:, None] * np.uint64(stride) + np.arange(ncols, dtype=np.uint64)[None, :]
    h = hash32(idx, seed, counter)
    return h > np.uint32(th) if gt else h >= np.uint32(th)


def _unxorshift(h, s):
    x = h
    for _ in range(32 // s + 1):
        x = h ^ (x >> s)
    return x


def seed_hitting(idx, value):
    """a seed (below 2^32, no counter) under which hash32(idx) == value, idx < 2^32: the finaliser is a bijection"""
    M = 0xFFFFFFFF
    h = _unxorshift(value & M, 16)
    h = (h * pow(0xC2B2AE35, -1, 1 << 32)) & M
    h = _unxorshift(h, 13)
    h = (h * pow(0x85EBCA6B, -1, 1 << 32)) & M
    h = _unxorshift(h, 16)
    return h ^ (idx & M)


# ---- windows -----------------------------------------------------------------------------------------------------------------------
Window = collections.namedtuple("Window", "buf start shape")


def window(a, fill=np.nan):
    a = np.ascontiguousarray(a, F32)
    m = MARGIN_ROWS * a.shape[-1]
    assert m % 4 == 0
    buf = np.full(2 * m + a.size, fill, F32)
    buf[m:m + a.size] = a.ravel()
    return Window(buf, m, a.shape)


def out_window(*shape):
    return window(np.full(shape, SENTINEL, F32), SENTINEL)


def inside(win, buf=None):
    b = win.buf if buf is None else buf
    return np.asarray(b[win.start:win.start + int(np.prod(win.shape))]).reshape(win.shape)


def embed(win, dense, spill=None):
    """the allocation of ``win`` with ``dense`` (the window's shape) inside; ``spill``: values written right after the window"""
    buf = win.buf.copy()
    n = int(np.prod(win.shape))
    with np.errstate(over="ignore", invalid="ignore"):
        buf[win.start:win.start + n] = np.asarray(dense, F64).astype(F32).ravel()
        if spill is not None:
            s = np.asarray(spill, F64).astype(F32).ravel()
            buf[win.start + n:win.start + n + s.size] = s
    return buf


Result = collections.namedtuple("Result", "what ok line")


def hold(tag, what, got_buf, win, want, allowed=None, written=None):
    """One comparison of the device test.  got_buf: the whole allocation after the call; want: float64, the window's shape;
    allowed: the bar (None: exact equality); written: which elements of the window the call may write (default all).  True only
    if the written elements agree, every sentinel outside is intact, no NaN stands where the reference is finite and NaN, +Inf,
    -Inf stand where the reference has them."""
    got_buf = np.asarray(got_buf)
    assert got_buf.dtype == F32 and got_buf.shape == win.buf.shape, (tag, what)
    n = int(np.prod(win.shape))
    want = np.asarray(want, F64).reshape(-1)
    mask = np.zeros(got_buf.shape, bool)
    mask[win.start:win.start + n] = True if written is None else np.asarray(written, bool).reshape(-1)
    broken = int((got_buf[~mask] != win.buf[~mask]).sum())
    got = got_buf[win.start:win.start + n].astype(F64)
    w = mask[win.start:win.start + n]
    fin = w & np.isfinite(want)
    stray = int(np.isnan(got[fin]).sum())
    cls = lambda v: np.isnan(v) * 1 + np.isposinf(v) * 2 + np.isneginf(v) * 3
    misplaced = int((cls(got[w & ~fin]) != cls(want[w & ~fin])).sum())
    tail = f"sentinels broken={broken}/{int((~mask).sum())} NaN where the reference is finite={stray} non-finite misplaced={misplaced}/{int((w & ~fin).sum())}"
    if allowed is None:
        bad = int((got[fin] != want[fin]).sum())
        line = f"{tag} {what}: mismatches={bad}/{int(fin.sum())} {tail}"
        ok = bad == 0
    else:
        allowed = np.broadcast_to(np.asarray(allowed, F64), win.shape).reshape(-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(got[fin] - want[fin])
            ratio = np.where(err == 0.0, 0.0, err / allowed[fin])
        worst = 0.0 if not fin.any() else (math.inf if np.isnan(ratio).any() else float(ratio.max()))
        line = f"{tag} {what}: largest error / bar={worst:.3f} over {int(fin.sum())} {tail}"
        ok = worst <= 1.0
    return Result(what, bool(ok and broken == 0 and stray == 0 and misplaced == 0), line)


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 32 - 5)


def _values(rng, shape, kind):
    if kind == "real":
        return rng.standard_normal(shape).astype(F32)
    return (rng.integers(1, 4, shape) * rng.choice((-1, 1), shape)).astype(F32)


def _int_bound(name, *arrays):
    """the condition of exact comparison: every value an integer below 2^24"""
    for a in arrays:
        a = np.asarray(a, F64)
        assert (a == np.rint(a)).all() and float(np.abs(a).max(initial=0.0)) < 2 ** 24, name


def prod_bar(n_terms, magnitude):
    return (n_terms + 2) * U * np.asarray(magnitude, F64)


# ---- LayerNorm, forward and backward: float64, or plain float32 with every sum in index order ---------------------------------------
def _sum(v, dtype, axis=-1):
    v = np.asarray(v, dtype)
    if dtype is F64:
        return v.sum(axis)
    v = np.moveaxis(v, axis, 0)
    acc = np.zeros(v.shape[1:], F32)
    for i in range(v.shape[0]):
        acc = (acc + v[i]).astype(F32)
    return acc


def ln_fwd(x, a, b, eps, dtype=F64, mutant=""):
    """n = a (x - mu) r + b, mu, r = 1 / (std + eps), std unbiased.  Returns dict(n, mu, r) and, under "mag", the magnitudes."""
    t = dtype
    x, a, b, eps = np.asarray(x, t), np.asarray(a, t), np.asarray(b, t), t(F32(eps))
    mu = (_sum(x, t) / t(D)).astype(t)
    xc = (x - mu[:, None]).astype(t)
    var = (_sum(xc * xc, t) / t(D if mutant == "biased-std" else D - 1)).astype(t)
    r = (t(1.0) / (np.sqrt(var + eps) if mutant == "eps-under-root" else np.sqrt(var) + eps)).astype(t)
    n = (a * ((xc * r[:, None]).astype(t)) + b).astype(t)
    mag = {"n": np.abs(a) * np.abs(xc) * r[:, None] + np.abs(b), "mu": np.abs(x).mean(-1), "r": r}
    return {"n": n, "mu": mu, "r": r, "mag": mag}


def ln_bwd(dn, x, a, addend, eps, scale, keep, dtype=F64, stats=None):
    """dx = r dxh + c2 (x - mu) - c1 + addend with dxh = dn a, c1 = r mean(dxh), c2 = -(sum dxh (x - mu)) r^2 / (std 127), and
    c2 = 0 where std == 0 (autograd's masked gradient of the std);  dy = keep ? scale dx : 0;  pa = dn (x - mu) r, pb = dn per
    element (the tile sums are ``tile_sums``).  float64: mu, std from x itself.  float32: mu, r from ``stats`` as the kernel
    reads them, std = 1 / r - eps."""
    t = dtype
    dn, x, a, eps = np.asarray(dn, t), np.asarray(x, t), np.asarray(a, t), t(F32(eps))
    ad = np.zeros_like(dn) if addend is None else np.asarray(addend, t)
    if stats is None:
        mu = _sum(x, t) / t(D)
        xc = x - mu[:, None]
        sd = np.sqrt(_sum(xc * xc, t) / t(D - 1))
        r = t(1.0) / (sd + eps)
    else:
        mu, r = np.asarray(stats[:, 0], t), np.asarray(stats[:, 1], t)
        xc = (x - mu[:, None]).astype(t)
        sd = (t(1.0) / r - eps).astype(t)
    dxh = (dn * a).astype(t)
    s1, s2 = _sum(dxh, t), _sum((dxh * xc).astype(t), t)
    with np.errstate(invalid="ignore", divide="ignore"):
        c2 = np.where(sd == 0, t(0.0), -(s2 * r * r) / (sd * t(D - 1))).astype(t)
    c1 = (r * s1 / t(D)).astype(t)
    with np.errstate(invalid="ignore"):
        dx = (r[:, None] * dxh + c2[:, None] * xc - c1[:, None] + ad).astype(t)
        dy = np.where(keep, (dx * t(scale)).astype(t), t(0.0)).astype(t)
        pa = (dn * (xc * r[:, None]).astype(t)).astype(t)
        mdx = r[:, None] * np.abs(dxh) + np.abs(c2)[:, None] * np.abs(xc) + np.abs(c1)[:, None] + np.abs(ad)
        mag = {"dx": mdx, "dy": mdx * scale, "pa": np.abs(dn) * (np.abs(x) + np.abs(mu)[:, None]) * r[:, None]}
    return {"dx": dx, "dy": dy, "pa": pa, "pb": dn, "mag": mag, "r": r, "sd": sd, "xc": xc}


def dn_error_through_ln(e, a, xc, r, sd):
    """|d dx| for |d dn| <= e elementwise (see the docstring)"""
    ae = np.abs(a) * e
    with np.errstate(invalid="ignore", divide="ignore"):
        t3 = np.where(sd[:, None] > 0, np.abs(xc) * (r * r / (sd * (D - 1)))[:, None] * (ae * np.abs(xc)).sum(-1)[:, None], 0.0)
    return r[:, None] * ae + r[:, None] * ae.mean(-1)[:, None] + t3


def tile_sums(v, dtype=F64):
    """[tiles][128]: sums over the rows of each 16-row tile (rows past the end contribute nothing)"""
    R = v.shape[0]
    pad = np.zeros((rows_tiles(R) * BM, v.shape[1]), dtype)
    pad[:R] = v
    return _sum(pad.reshape(-1, BM, v.shape[1]), dtype, axis=1)


def delta_of(out2, attn, Lq, dtype=F64, mutant=""):
    """delta[b][head][q] = sum_d out2[b Lq + q][16 head + d] attn[same]; (delta, magnitude)"""
    R = out2.shape[0]
    pr = (np.asarray(out2, dtype) * np.asarray(attn, dtype)).astype(dtype).reshape(R // Lq, Lq, HEADS, DK)
    d = np.transpose(_sum(pr, dtype), (0, 2, 1)).astype(F64)
    mag = np.transpose(np.abs(pr.astype(F64)).sum(-1), (0, 2, 1))
    if mutant == "delta-head":      # both halves of a wave's 32 columns write head 2 w: the odd heads are never written
        d2 = np.full_like(d, float(SENTINEL))
        d2[:, 0::2] = d[:, 1::2]
        d = d2
    return d, mag


# ---- the row kernel: cases ---------------------------------------------------------------------------------------------------------------
RowsCase = collections.namedtuple("RowsCase", "name kind mode R K1 nparts bias1 res N2 bias2 p counter seed lq n_out special eps")
FIRST = ("none", "K128", "K256", "K384", "K512", "K640") + tuple(f"parts{n}" for n in (1, 2, 4, 5, 8, 9, 13, 16, 17, 24))
ROW_RS = (1, 15, 16, 17, 33)


def _first(f):
    return (0, 0) if f == "none" else ((int(f[1:]), 0) if f[0] == "K" else (0, int(f[5:])))


def _rows_table():
    t = []
    for kind in ("int", "real"):
        # forward: every first part x a cycling R, N2, bias1, bias2, dropout
        for i, f in enumerate(FIRST):
            K1, nparts = _first(f)
            for j in range(2):
                R, N2 = ROW_RS[(i + 2 * j) % 5], (0, 128, 256, 384, 512)[(i + 3 * j) % 5]
                bias1, bias2 = int((i + j) % 2 == 0 and f != "none"), int((i + j) % 3 != 0 and N2 > 0)
                p = 0.0 if f == "none" else ((0.5, 0.0)[(i + j) % 3 == 2] if kind == "int" else (0.1, 0.5, 0.0)[(i + j) % 3])
                cnt = (None, 3, 2 ** 33 + 5)[i % 3] if p else None
                name = f"fwd-{f}-R{R}-N2_{N2}{'-b1' if bias1 else ''}{'-b2' if bias2 else ''}{f'-p{p}' if p else ''}{'-counter' if cnt else ''}"
                t.append(RowsCase(f"{name}-{kind}", kind, 0, R, K1, nparts, bias1, 1, N2, bias2, p, cnt, 1000 + 7 * i + j, 0, 1, "", 1e-6))
        # forward: the column split of the second product on both sides of its 64-tile edge
        for R in (1024, 1025):
            for N2 in (384, 256):
                t.append(RowsCase(f"fwd-split-R{R}-N2_{N2}-ny{ny(R, N2, 0)}-{kind}", kind, 0, R, 128, 0, 1, 1, N2, 1, 0.5 if kind == "int" else 0.1, 7, 99,
                                  0, 1, "", 1e-6))
        # backward: g, products and sums of slices x a cycling R; addend, dy, second product on and off
        for i, f in enumerate(("g",) + FIRST[1:]):
            K1, nparts = (0, 0) if f == "g" else _first(f)
            for j in range(2):
                R = ROW_RS[(i + 2 * j + 1) % 5]
                res, n_out, N2 = int((i + j) % 2 == 0), int((i + j) % 3 != 0), 128 * int((i // 2 + j) % 2 == 0)
                p = 0.0 if (i + j) % 3 == 1 else (0.5 if kind == "int" else (0.1, 0.5)[i % 2])
                cnt = (None, 11)[(i + j) % 2] if p else None
                name = f"bwd-{f}-R{R}{'-addend' if res else ''}{'-dy' if n_out else ''}{'-out2' if N2 else ''}{f'-p{p}' if p else ''}{'-counter' if cnt else ''}"
                t.append(RowsCase(f"{name}-{kind}", kind, 1, R, K1, nparts, 0, res, N2, 0, p, cnt, 2000 + 7 * i + j, 0, n_out, "", 1e-6))
        # backward: the attention row term, rows of one batch element straddling tiles or not
        for R, Lq in ((16, 1), (48, 3), (51, 17), (32, 16)):
            t.append(RowsCase(f"bwd-delta-R{R}-Lq{Lq}-{kind}", kind, 1, R, 0, 2, 0, 1, 128, 0, 0.5 if kind == "int" else 0.1, None, 31 + Lq, Lq, 1, "", 1e-6))
    # the keep rule's edge: one element hashes to the threshold exactly (kept under >=, dropped under >)
    t.append(RowsCase("fwd-K128-R17-drop-edge-int", "int", 0, 17, 128, 0, 1, 1, 0, 0, 0.5, None, 0, 0, 1, "drop-edge", 1e-6))
    t.append(RowsCase("bwd-g-R17-drop-edge-int", "int", 1, 17, 0, 0, 0, 1, 0, 0, 0.5, None, 0, 0, 1, "drop-edge", 1e-6))
    return tuple(t)


EDGE_ELEMENT = (16, 5)      # (row, column) of the element whose hash equals the threshold in the "drop-edge" cases
ROWS_CASES = _rows_table()


def _spread_rows(rng, R, kind):
    """[R][128] rows whose std is at least 1e-3 (``real``: standard normal scaled per row by 2^-3 .. 2^3 and shifted; ``int``)"""
    v = _values(rng, (R, D), kind)
    if kind == "real":
        v = ((v + rng.standard_normal((R, 1))) * (2.0 ** rng.integers(-3, 4, (R, 1)))).astype(F32)
        assert v.astype(F64).std(-1, ddof=1).min() >= 1e-3
    return v


def rows_inputs(case):
    """dict of Windows: the operands (NaN margins), and the outputs (sentinel); an absent operand / a null output is None"""
    c, rng = case, np.random.default_rng(_seed(case.name))
    x = {k: None for k in "a1 w1 bias1 res ln_a ln_b x_ln g stats w2 bias2 attn_out x_out n_out stats_out part out2 delta_out".split()}
    R = c.R
    if c.nparts:
        x["a1"] = window(_values(rng, (c.nparts, R, D), c.kind))
    elif c.K1:
        x["a1"] = window(_values(rng, (R, c.K1), c.kind))
        x["w1"] = window(_values(rng, (D, c.K1) if c.mode == 0 else (c.K1, D), c.kind))
    if c.bias1:
        x["bias1"] = window(_values(rng, (1, D), c.kind))
    if c.res:
        x["res"] = window(_spread_rows(rng, R, c.kind) if c.mode == 0 and not (c.K1 or c.nparts) else _values(rng, (R, D), c.kind))
    x["ln_a"] = window(_values(rng, (1, D), c.kind) if c.kind == "int" else (rng.standard_normal((1, D)) * 0.3 + 1).astype(F32))
    if c.mode == 0:
        # (``real``: |b| >= 1/2, so that no element of n has a magnitude near zero, against which any error would be large)
        lb = _values(rng, (1, D), c.kind)
        x["ln_b"] = window(lb if c.kind == "int" else lb + np.sign(lb) * F32(0.5))
        x["x_out"], x["n_out"], x["stats_out"] = out_window(R, D), out_window(R, D), out_window(R, 2)
    else:
        xl = _spread_rows(rng, R, c.kind)
        f = ln_fwd(xl, np.ones(D), np.zeros(D), c.eps, F32)
        x["x_ln"], x["stats"] = window(xl), window(np.stack([f["mu"], f["r"]], 1))
        if not (c.K1 or c.nparts):
            x["g"] = window(_values(rng, (R, D), c.kind))
        x["x_out"], x["part"] = out_window(R, D), out_window(rows_tiles(R), 2 * D)
        x["n_out"] = out_window(R, D) if c.n_out else None
    if c.N2:
        x["w2"] = window(_values(rng, (c.N2, D), c.kind) if c.mode == 0 else _values(rng, (D, D), c.kind))
        x["out2"] = out_window(R, c.N2)
        if c.bias2:
            x["bias2"] = window(_values(rng, (1, c.N2), c.kind))
    if c.lq:
        x["attn_out"], x["delta_out"] = window(_values(rng, (R, D), c.kind)), out_window(R // c.lq, HEADS, c.lq)
    return x


def _v(win):
    return None if win is None else inside(win).astype(F64)


def rows_seed(case, x):
    """the host seed word of the call (``drop-edge``: the one under which EDGE_ELEMENT hashes to the threshold)"""
    if case.special != "drop-edge":
        return case.seed
    r, col = EDGE_ELEMENT
    return seed_hitting(r * D + col, drop_thresh(case.p))


def rows_first(case, x, mutant=""):
    """(first part [R][128] float64 or None, sum |a| |w| of it, number of terms)"""
    c = case
    if c.nparts:
        parts = _v(x["a1"])
        S = c.nparts - (1 if mutant == "nparts-skip" and c.nparts > 1 else 0)
        acc = parts[0].copy()
        for s in range(1, S):
            acc = acc + parts[s]
        if c.kind == "int":
            _int_bound(c.name, np.cumsum(parts, 0))
        return acc, np.abs(parts).sum(0), c.nparts
    if c.K1:
        A, W = _v(x["a1"]), _v(x["w1"])
        Wop = W.T if c.mode == 0 else W
        K = c.K1 - (128 if mutant == "k-chunk" and c.K1 > 128 and (c.K1 // 128) % 2 == 1 else 0)
        mag = np.abs(A) @ np.abs(Wop)
        if c.kind == "int":
            _int_bound(c.name, mag)
        return A[:, :K] @ Wop[:K], mag, c.K1
    return None, None, 0


def rows_keep(case, x, mutant=""):
    stride = 2 * D if mutant == "rows-drop-stride" else D
    return keep_mask(case.R, D, stride, case.p, rows_seed(case, x), case.counter, gt=mutant == "keep>")


def rows_fwd_x(case, x, mutant=""):
    """x' = res + dropout(first + bias1): (x', its bar, the keep mask or None without a first part)"""
    c = case
    acc, mag, nt = rows_first(c, x, mutant)
    res = _v(x["res"])
    if acc is None:
        return res, np.zeros_like(res), None
    b1 = _v(x["bias1"])[0] if (c.bias1 and mutant != "no-bias1") else np.zeros(D)
    scale, keep = drop_scale(c.p), rows_keep(c, x, mutant)
    dr = np.where(keep, (acc + b1) * scale, 0.0)
    xo = res + dr
    if c.kind == "int":
        _int_bound(c.name, dr, xo)
    # the product's bound through the scale, one rounding for the scaling, one for the addition
    bar = np.where(keep, scale * prod_bar(nt, mag + np.abs(b1)) + U * np.abs(dr), 0.0) + U * np.abs(xo)
    return xo, bar, keep


def rows_bwd_dn(case, x, mutant=""):
    """(dn [R][128], its a-priori error bound: zeros where dn is an operand)"""
    c = case
    acc, mag, nt = rows_first(c, x, mutant)
    if acc is None:
        g = _v(x["g"])
        return g, np.zeros_like(g)
    return acc, (np.zeros_like(acc) if c.kind == "int" else prod_bar(nt, mag))


def rows_emulate(case, x, mutant="", nulls=()):
    """{output name: the whole allocation, float32} as a kernel that follows the contract (or ``mutant``) leaves it: the float64
    chain from the operands, rounded once per output."""
    c, R = case, case.R
    out = {}
    spill = lambda v: (np.repeat(np.asarray(v, F64)[-1:], rows_tiles(R) * BM - R, 0) if mutant == "tail-rows" else None)
    if c.mode == 0:
        xo, _, _ = rows_fwd_x(c, x, mutant)
        f = ln_fwd(xo, _v(x["ln_a"])[0], _v(x["ln_b"])[0], c.eps, F64, mutant)
        out["x_out"], out["n_out"] = embed(x["x_out"], xo, spill(xo)), embed(x["n_out"], f["n"], spill(f["n"]))
        out["stats_out"] = embed(x["stats_out"], np.stack([f["mu"], f["r"]], 1))
        if c.N2:
            o2 = f["n"] @ _v(x["w2"]).T + (_v(x["bias2"])[0] if c.bias2 else 0.0)
            if mutant == "ny-overwrite" and ny(R, c.N2, 0) >= 3:
                o2[:, :D] = o2[:, D:2 * D]
                o2[:, D:2 * D] = float(SENTINEL)
            out["out2"] = embed(x["out2"], o2, spill(o2))
    else:
        dn, _ = rows_bwd_dn(c, x, mutant)
        keep = rows_keep(c, x, mutant)
        b = ln_bwd(dn, _v(x["x_ln"]), _v(x["ln_a"])[0], _v(x["res"]), c.eps, drop_scale(c.p), keep)
        out["x_out"] = embed(x["x_out"], b["dx"], spill(b["dx"]))
        with np.errstate(invalid="ignore", over="ignore"):      # dy is formed from the float32 dx, in float32
            dy = np.where(keep, b["dx"].astype(F32) * F32(drop_scale(c.p)), F32(0.0)).astype(F64)
        if c.n_out:
            out["n_out"] = embed(x["n_out"], dy, spill(dy))
        pa, pb = b["pa"], b["pb"]
        if mutant == "tail-rows" and R % BM:      # the clamped last row counted once per missing row
            k = rows_tiles(R) * BM - R
            pa, pb = np.concatenate([pa, np.repeat(pa[-1:], k, 0)]), np.concatenate([pb, np.repeat(pb[-1:], k, 0)])
        out["part"] = embed(x["part"], np.concatenate([tile_sums(pa), tile_sums(pb)], 1))
        if c.N2:
            o2 = dy @ _v(x["w2"])
            out["out2"] = embed(x["out2"], o2, spill(o2))
            if c.lq:
                out["delta_out"] = embed(x["delta_out"], delta_of(o2, _v(x["attn_out"]), c.lq, mutant=mutant)[0])
    for k in nulls:
        out.pop(k, None)
    return out


def rows_check(case, x, got, tag="TF-EDGES"):
    """The device test's comparisons of one row-kernel call: [Result].  ``got``: {output name: whole allocation after the call};
    an output missing from it was passed as null.  Stage by stage (see the docstring)."""
    c, R, res = case, case.R, []
    tag = f"{tag} spacap_tf_rows_f32 {c.name}"
    exact = c.kind == "int"
    la = _v(x["ln_a"])[0]
    if c.mode == 0:
        xo, xbar, keep = rows_fwd_x(c, x)
        if "x_out" in got:
            res.append(hold(tag, "x_out", got["x_out"], x["x_out"], xo, None if exact else xbar))
            if keep is not None and c.p:
                zeros = inside(x["x_out"], got["x_out"]).astype(F64) - _v(x["res"]) == 0.0
                want0 = ~keep | (xo - _v(x["res"]) == 0.0) if exact else ~keep
                bad = int((zeros != want0).sum())
                res.append(Result("dropout mask", bad == 0, f"{tag} dropout mask: zeros of x_out - res misplaced={bad}/{R * D} dropped={int((~keep).sum())}"))
            xs = inside(x["x_out"], got["x_out"]).astype(F64)
        else:
            xs = xo.astype(F32).astype(F64)
        f = ln_fwd(xs, la, _v(x["ln_b"])[0], c.eps)
        if "n_out" in got:
            res.append(hold(tag, "n_out (from the stored x_out)", got["n_out"], x["n_out"], f["n"], LN_BAR["n"] * U * f["mag"]["n"]))
        if "stats_out" in got:
            res.append(hold(tag, "stats (from the stored x_out)", got["stats_out"], x["stats_out"], np.stack([f["mu"], f["r"]], 1),
                            U * np.stack([LN_BAR["mu"] * f["mag"]["mu"], LN_BAR["r"] * f["mag"]["r"]], 1)))
        if c.N2:
            ns = inside(x["n_out"], got["n_out"]).astype(F64) if "n_out" in got else f["n"].astype(F32).astype(F64)
            W2, b2 = _v(x["w2"]), (_v(x["bias2"])[0] if c.bias2 else np.zeros(c.N2))
            bar = prod_bar(D, np.abs(ns) @ np.abs(W2).T + np.abs(b2))
            if "n_out" not in got:      # n itself only within its own bar: carried through the product
                bar = bar + (LN_BAR["n"] * U * f["mag"]["n"]) @ np.abs(W2).T
            res.append(hold(tag, f"out2 (from the stored n_out, ny={ny(R, c.N2, 0)})", got["out2"], x["out2"], ns @ W2.T + b2, bar))
        return res
    dn, e = rows_bwd_dn(c, x)
    keep, scale = rows_keep(c, x), drop_scale(c.p)
    b = ln_bwd(dn, _v(x["x_ln"]), la, _v(x["res"]), c.eps, scale, keep)
    through = dn_error_through_ln(e, la, b["xc"], b["r"], b["sd"])
    res.append(hold(tag, "dx", got["x_out"], x["x_out"], b["dx"], LN_BAR["dx"] * U * b["mag"]["dx"] + through))
    dxs = inside(x["x_out"], got["x_out"])
    with np.errstate(invalid="ignore", over="ignore"):
        dys = np.where(keep, (dxs * F32(scale)).astype(F32), F32(0.0))
    if "n_out" in got:
        res.append(hold(tag, "dy", got["n_out"], x["n_out"], b["dy"], LN_BAR["dy"] * U * b["mag"]["dy"] + scale * through))
        gy = inside(x["n_out"], got["n_out"])
        bad = int((~((gy == dys) | (np.isnan(gy) & np.isnan(dys)))).sum())
        res.append(Result("dy bits", bad == 0, f"{tag} dy against keep ? float32(scale) * stored dx : 0, bit for bit: mismatches={bad}/{R * D} dropped={int((~keep).sum())}"))
    want = np.concatenate([tile_sums(b["pa"]), tile_sums(b["pb"])], 1)
    pbar = np.concatenate([LN_BAR["part"] * U * tile_sums(b["mag"]["pa"]) + tile_sums(e * np.abs(b["xc"]) * b["r"][:, None]),
                           prod_bar(BM, tile_sums(np.abs(dn))) + tile_sums(e)], 1)
    if exact:      # the sum dn half alone, exactly (the other half stands as unwritten in this comparison)
        half = np.zeros((rows_tiles(R), 2 * D), bool)
        half[:, D:] = True
        res.append(hold(tag, "part, the sum dn half", embed(x["part"], np.where(half, inside(x["part"], got["part"]), SENTINEL)), x["part"], want, None, half))
    res.append(hold(tag, f"part ({rows_tiles(R)} tiles)", got["part"], x["part"], want, pbar))
    if c.N2:
        ys = dys.astype(F64)
        W2 = _v(x["w2"])
        o2 = ys @ W2
        res.append(hold(tag, "out2 (from the stored dx through the mask)", got["out2"], x["out2"], o2, prod_bar(D, np.abs(ys) @ np.abs(W2))))
        if c.lq:
            o2s = inside(x["out2"], got["out2"]).astype(F64)
            d, mag = delta_of(o2s, _v(x["attn_out"]), c.lq)
            res.append(hold(tag, f"delta (from the stored out2, Lq={c.lq})", got["delta_out"], x["delta_out"], d, LN_BAR["delta"] * U * mag))
    return res


def measure_ln():
    """{output: the float32 evaluation's largest error over the ``real`` row cases, in units of 2^-24 x magnitude}"""
    fig = dict.fromkeys(LN_FIGURE, 0.0)

    def take(key, got, want, mag):
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(np.asarray(got, F64) - want)
            fig[key] = max(fig[key], float(np.where(err == 0, 0.0, err / (U * np.asarray(mag, F64))).max()))

    for c in ROWS_CASES:
        if c.kind != "real":
            continue
        x = rows_inputs(c)
        la = _v(x["ln_a"])[0]
        if c.mode == 0:
            xs = rows_fwd_x(c, x)[0].astype(F32)
            f32, f64 = ln_fwd(xs, la, _v(x["ln_b"])[0], c.eps, F32), ln_fwd(xs, la, _v(x["ln_b"])[0], c.eps)
            for k in ("n", "mu", "r"):
                take(k, f32[k], f64[k], f64["mag"][k])
            continue
        dn = rows_bwd_dn(c, x)[0].astype(F32)
        keep, scale = rows_keep(c, x), drop_scale(c.p)
        args = (dn, inside(x["x_ln"]), la, None if x["res"] is None else inside(x["res"]), c.eps, scale, keep)
        b32, b64 = ln_bwd(*args, dtype=F32, stats=inside(x["stats"])), ln_bwd(*args)
        take("dx", b32["dx"], b64["dx"], b64["mag"]["dx"])
        take("dy", b32["dy"], b64["dy"], b64["mag"]["dy"])
        take("part", tile_sums(b32["pa"], F32), tile_sums(b64["pa"]), tile_sums(b64["mag"]["pa"]))
        if c.lq:
            o2 = (b32["dy"].astype(F64) @ _v(x["w2"])).astype(F32)
            d64, mag = delta_of(o2, inside(x["attn_out"]), c.lq)
            take("delta", delta_of(o2, inside(x["attn_out"]), c.lq, F32)[0], d64, mag)
    return fig


# ---- the split product and its epilogues (spacap_tf_gemm_f32, spacap_tf_ffn1_f32, spacap_tf_dgrad_mask_f32) ---------------------------
GemmCase = collections.namedtuple("GemmCase", "name kind entry R K N trans nsplit bias p counter seed")
GEMM_RS, GEMM_NS = (1, 63, 64, 65, 129), (128, 256, 384)


def _gemm_table():
    t = []
    for kind in ("int", "real"):
        i = 0
        for K in (128, 256, 1024):
            for ns in [s for s in range(1, K // 128 + 1) if (K // 128) % s == 0]:
                for trans in (1, 0):
                    R, N = GEMM_RS[i % 5], GEMM_NS[(i + i // 5) % 3]
                    i += 1
                    t.append(GemmCase(f"gemm-R{R}-K{K}-N{N}-{'wT' if trans else 'w'}-S{ns}-{kind}", kind, "gemm", R, K, N, trans, ns, 0, 0.0, None, 0))
        for i, R in enumerate(GEMM_RS):
            p = 0.5 if kind == "int" else (0.1, 0.0, 0.5)[i % 3]
            cnt = (None, 5)[i % 2] if p else None
            t.append(GemmCase(f"ffn1-R{R}-N{GEMM_NS[i % 3]}{'-bias' if i % 2 == 0 else ''}{f'-p{p}' if p else ''}{'-counter' if cnt else ''}-{kind}", kind, "ffn1", R, 128,
                              GEMM_NS[i % 3], 1, 1, int(i % 2 == 0), p, cnt, 300 + i))
            t.append(GemmCase(f"dgrad-mask-R{R}-N{GEMM_NS[(i + 1) % 3]}-{kind}", kind, "dgrad", R, 128, GEMM_NS[(i + 1) % 3], 0, 1, 0, 0.5 if kind == "int" else 0.2, None, 0))
    return tuple(t)


GEMM_CASES = _gemm_table()


def _gated(rng, shape, kind):
    """a saved activation: positive where the unit was active and kept, exact zeros elsewhere (about half)"""
    return (np.abs(_values(rng, shape, kind)) * rng.integers(0, 2, shape)).astype(F32)


def gemm_inputs(case):
    c, rng = case, np.random.default_rng(_seed(case.name))
    x = {"x": window(_values(rng, (c.R, c.K), c.kind)), "W": window(_values(rng, (c.N, c.K) if c.trans else (c.K, c.N), c.kind)), "bias": None, "y": None}
    if c.bias:
        x["bias"] = window(_values(rng, (1, c.N), c.kind))
    if c.entry == "dgrad":
        x["y"] = window(_gated(rng, (c.R, c.N), c.kind))
        assert (inside(x["y"]) == 0).any() and (inside(x["y"]) > 0).any()
    x["out"] = out_window(c.nsplit, c.R, c.N)
    return x


def gemm_reference(case, x, mutant=""):
    """(expected out [nsplit][R][N], its bar, the keep mask of EPI 1 or None, the pre-activation of EPI 1 or None)"""
    c = case
    A, W = _v(x["x"]), _v(x["W"])
    Wop = W.T if c.trans else W
    KS = c.K // c.nsplit
    out = np.stack([A[:, z * KS:(z + 1) * KS] @ Wop[z * KS:(z + 1) * KS] for z in range(c.nsplit)])
    mag = np.stack([np.abs(A[:, z * KS:(z + 1) * KS]) @ np.abs(Wop[z * KS:(z + 1) * KS]) for z in range(c.nsplit)])
    if c.kind == "int":
        _int_bound(c.name, mag.sum(0) * 2 + 3)
    if c.entry == "gemm":
        return out, prod_bar(KS, mag), None, None
    scale = drop_scale(c.p)
    if c.entry == "ffn1":
        b = _v(x["bias"])[0] if c.bias else np.zeros(c.N)
        pre = out[0] + b
        keep = keep_mask(c.R, c.N, D if (mutant == "ffn-drop-stride" and c.N != D) else c.N, c.p, c.seed, c.counter, gt=mutant == "keep>")
        o = np.where(keep, np.maximum(pre, 0.0) * scale, 0.0)
        return o[None], (scale * prod_bar(c.K, mag[0] + np.abs(b)) + U * np.abs(o))[None], keep, pre
    y = _v(x["y"])
    o = np.where((y >= 0) if mutant == "relu>=" else (y > 0), out[0] * scale, 0.0)
    return o[None], (scale * prod_bar(c.K, mag[0]) + U * np.abs(o))[None], None, None


def gemm_emulate(case, x, mutant=""):
    o = gemm_reference(case, x, mutant)[0]
    spill = None
    if mutant == "tail-rows" and case.R % FM:
        spill = np.repeat(o[-1, -1:], min(_cdiv(case.R, FM) * FM - case.R, MARGIN_ROWS), 0)
    return {"out": embed(x["out"], o, spill)}


def gemm_check(case, x, got, tag="TF-EDGES"):
    c, res = case, []
    entry = {"gemm": "spacap_tf_gemm_f32", "ffn1": "spacap_tf_ffn1_f32", "dgrad": "spacap_tf_dgrad_mask_f32"}[c.entry]
    tag = f"{tag} {entry} {c.name}"
    want, bar, keep, pre = gemm_reference(c, x)
    exact = c.kind == "int"
    g = inside(x["out"], got["out"])
    if c.nsplit > 1:
        per = [int((g[z].astype(F64) != want[z]).sum()) if exact else round(float((np.abs(g[z] - want[z]) / bar[z]).max()), 3) for z in range(c.nsplit)]
        print(f"{tag} per slice: {'mismatches' if exact else 'largest error / bar'}={per}")
    res.append(hold(tag, "values", got["out"], x["out"], want, None if exact else bar))
    if c.nsplit > 1:      # the slices added in order, on the host in float32
        acc = g[0].copy()
        for z in range(1, c.nsplit):
            acc = (acc + g[z]).astype(F32)
        w1 = window(np.full((c.R, c.N), SENTINEL), SENTINEL)
        A, W = _v(x["x"]), _v(x["W"])
        Wop = W.T if c.trans else W
        res.append(hold(tag, f"the {c.nsplit} slices added in order (host, float32)", embed(w1, acc), w1, A @ Wop,
                        None if exact else prod_bar(c.K + c.nsplit, np.abs(A) @ np.abs(Wop))))
    if c.entry == "ffn1" and c.p:
        g0 = g[0]
        bad = int((~keep & (g0 != 0)).sum()) + int((keep & (pre > bar[0]) & (g0 == 0)).sum())
        res.append(Result("dropout mask", bad == 0, f"{tag} dropout mask: dropped elements not zero + kept active elements zero={bad} dropped={int((~keep).sum())}/{keep.size}"))
    if c.entry == "dgrad":
        y = _v(x["y"])
        bad = int(((y <= 0) & (g[0] != 0)).sum())
        res.append(Result("relu mask", bad == 0, f"{tag} relu mask: non-zero where y is not positive={bad} exact zeros in y={int((y == 0).sum())}"))
    return res


# ---- the chained feed-forward block (spacap_tf_ffn_f32, spacap_tf_ffn_bf3_f32) and its piece images (spacap_tf_ffn_split_f32) -----------
FfnCase = collections.namedtuple("FfnCase", "name kind bf3 mode R dff bias hid p counter seed")
BF16_SENTINEL = F32(-768.0)       # (exact in bf16)


def _ffn_table():
    t = []
    for kind in ("int", "real"):
        for i, R in enumerate((1, 15, 16, 17, 511, 512, 513, 575, 576, 577)):
            for mode in (0, 1):
                dff = (128, 256, 384)[(i + mode) % 3]
                hid, bias = int(mode == 1 or i % 3 != 0), int(mode == 0 and i % 2 == 0)
                p = (0.5 if kind == "int" else (0.1, 0.5, 0.0)[i % 3]) if (mode == 1 or i % 4 != 3) else 0.0
                cnt = (None, 9)[i % 2] if (p and mode == 0) else None
                t.append(FfnCase(f"ffn-{'MT1' if ffn_small(R) else 'MT4'}-mode{mode}-R{R}-dff{dff}{'' if hid else '-nohid'}{'-bias' if bias else ''}{f'-p{p}' if p else ''}"
                                 f"{'-counter' if cnt else ''}-{kind}", kind, 0, mode, R, dff, bias, hid, p, cnt, 500 + i))
        for i, (R, dff) in enumerate(((1, 128), (63, 384), (64, 1024), (65, 1152), (513, 2048), (577, 128), (577, 1152), (65, 2048), (513, 384), (63, 1024))):
            for mode in (0, 1):
                hid, bias = int(mode == 1 or i % 2 == 0), int(mode == 0 and i % 3 != 1)
                p = 0.5 if kind == "int" else (0.1, 0.0)[i % 2]
                t.append(FfnCase(f"bf3-{'xcd' if (dff // 128) % 8 == 0 else 'slice-major'}-mode{mode}-R{R}-dff{dff}{'' if hid else '-nohid'}{'-bias' if bias else ''}"
                                 f"{f'-p{p}' if p else ''}-{kind}", kind, 1, mode, R, dff, bias, hid, p, None, 700 + i))
    return tuple(t)


FFN_CASES = _ffn_table()


def split_images(W1, W2, mutant=""):
    """[4][3][dff 128] float64: the piece images of one layer in operand order (image, piece, index); index = ((((slice c, wave w),
    t, kc), lane), e) <-> unit 32 w + 16 t + lane % 16, contraction index 32 kc + 8 (lane / 16) + e, + 128 c on the hidden axis"""
    W1, W2 = np.asarray(W1, F32), np.asarray(W2, F32)
    dff = W1.shape[0]
    idx = np.arange(dff * D)
    e, lane, kc, t, w, c = idx & 7, (idx >> 3) & 63, (idx >> 9) & 3, (idx >> 11) & 1, (idx >> 12) & 3, idx >> 14
    unit, kk = 32 * w + 16 * t + (lane & 15), 32 * kc + 8 * (lane >> 4) + e
    v = (W1[128 * c + unit, kk], W2[unit, 128 * c + kk], W2[kk, 128 * c + unit], W1[128 * c + kk, unit])
    out = np.stack([np.stack(split3(vi)) for vi in v])
    if mutant == "pieces-swapped":
        out[1, [1, 2]] = out[1, [2, 1]]
    return out


def bf3_bar(A, B):
    """the split-bf16 product's bound for A [M][K] B [K][N] (float32 operands): see the docstring"""
    a, b = split3(np.asarray(A, F32)), split3(np.asarray(B, F32))
    six = sum(np.abs(a[PA[q]]) @ np.abs(b[PB[q]]) for q in range(6))
    nine = (np.abs(a[0]) + np.abs(a[1]) + np.abs(a[2])) @ (np.abs(b[0]) + np.abs(b[1]) + np.abs(b[2]))
    A64, B64 = np.asarray(A, F64), np.asarray(B, F64)
    resid = np.abs(A64 - (a[0] + a[1] + a[2])) @ np.abs(B64) + np.abs(A64) @ np.abs(B64 - (b[0] + b[1] + b[2]))
    return (6 * A64.shape[1] + 2) * U * six + (nine - six) + resid


def ffn_inputs(case):
    c, rng = case, np.random.default_rng(_seed(case.name))
    x = {"x": window(_values(rng, (c.R, D), c.kind)), "W1": window(_values(rng, (c.dff, D), c.kind)), "W2": window(_values(rng, (D, c.dff), c.kind)),
         "bias": None, "y": None, "hid": None}
    if c.bias:
        x["bias"] = window(_values(rng, (1, c.dff), c.kind))
    if c.mode == 1:
        x["y"] = window(_gated(rng, (c.R, c.dff), c.kind))
        assert (inside(x["y"]) == 0).any()
    if c.hid:
        x["hid"] = out_window(c.R, c.dff)
    x["part"] = out_window(c.dff // 128, c.R, D)
    return x


def _prod(c, A, B):
    """(A B in float64, its bar) on the case's arithmetic"""
    if c.bf3 and c.kind == "real":
        return A @ B, bf3_bar(A, B)
    return A @ B, prod_bar(A.shape[1], np.abs(A) @ np.abs(B))


def ffn_hid(case, x, mutant=""):
    """(hid [R][dff], its bar, the keep mask (mode 0) or None, the pre-activation)"""
    c = case
    A, W1, W2 = _v(x["x"]), _v(x["W1"]), _v(x["W2"])
    scale = drop_scale(c.p)
    if c.mode == 0:
        b = _v(x["bias"])[0] if c.bias else np.zeros(c.dff)
        pre, bar = _prod(c, A, W1.T)
        pre, bar = pre + b, bar + 2 * U * np.abs(b)
        keep = keep_mask(c.R, c.dff, D if (mutant == "ffn-drop-stride" and c.dff != D) else c.dff, c.p, c.seed, c.counter, gt=mutant == "keep>")
        hid = np.where(keep, np.maximum(pre, 0.0) * scale, 0.0)
    else:
        pre, bar = _prod(c, A, W2)
        y, keep = _v(x["y"]), None
        hid = np.where((y >= 0) if mutant == "relu>=" else (y > 0), pre * scale, 0.0)
    if c.kind == "int":
        _int_bound(c.name, (np.abs(A) @ np.abs(W1.T if c.mode == 0 else W2) + 3) * scale)
    return hid, scale * bar + U * np.abs(hid), keep, pre


def ffn_part(case, x, hid):
    """(part [dff / 128][R][128] from ``hid``, its bar)"""
    c = case
    W1, W2 = _v(x["W1"]), _v(x["W2"])
    out, bar = [], []
    for s in range(c.dff // 128):
        sl = slice(128 * s, 128 * s + 128)
        o, b = _prod(c, hid[:, sl], W2[:, sl].T if c.mode == 0 else W1[sl])
        out.append(o), bar.append(b)
    if c.kind == "int":
        _int_bound(c.name, np.abs(hid) @ np.abs(W2.T if c.mode == 0 else W1))
    return np.stack(out), np.stack(bar)


def ffn_emulate(case, x, mutant=""):
    c = case
    hid = ffn_hid(c, x, mutant)[0]
    part = ffn_part(c, x, hid.astype(F32).astype(F64))[0]
    spill = None
    tile = BM if (ffn_small(c.R) and not c.bf3) else FM
    if mutant == "tail-rows" and c.R % tile:
        spill = np.repeat(part[-1, -1:], min(_cdiv(c.R, tile) * tile - c.R, MARGIN_ROWS), 0)
    out = {"part": embed(x["part"], part, spill)}
    if c.hid:
        out["hid"] = embed(x["hid"], hid)
    return out


def ffn_check(case, x, got, tag="TF-EDGES"):
    c, res = case, []
    tag = f"{tag} {'spacap_tf_ffn_bf3_f32' if c.bf3 else 'spacap_tf_ffn_f32'} {c.name}"
    exact = c.kind == "int"
    hid, hbar, keep, pre = ffn_hid(c, x)
    if c.hid:
        res.append(hold(tag, "hid", got["hid"], x["hid"], hid, None if exact else hbar))
        hs = inside(x["hid"], got["hid"])
        if c.mode == 0 and c.p:
            bad = int((~keep & (hs != 0)).sum()) + int((keep & (pre > hbar) & (hs == 0)).sum())
            res.append(Result("dropout mask", bad == 0, f"{tag} dropout mask: dropped elements not zero + kept active elements zero={bad} dropped={int((~keep).sum())}/{keep.size}"))
        if c.mode == 1:
            y = _v(x["y"])
            bad = int(((y <= 0) & (hs != 0)).sum())
            res.append(Result("relu mask", bad == 0, f"{tag} relu mask: non-zero where y is not positive={bad} exact zeros in y={int((y == 0).sum())}"))
        part, pbar = ffn_part(c, x, hs.astype(F64))
        what = "part (from the stored hid)"
    else:      # nothing stored: the hidden tile only within its own bar, carried through the second product
        part, pbar = ffn_part(c, x, hid.astype(F32).astype(F64))
        W2 = np.abs(_v(x["W2"]))
        pbar = pbar + np.stack([hbar[:, 128 * s:128 * s + 128] @ W2[:, 128 * s:128 * s + 128].T for s in range(c.dff // 128)])
        what = "part (hid not stored)"
    res.append(hold(tag, what, got["part"], x["part"], part, None if exact else pbar))
    return res


SplitCase = collections.namedtuple("SplitCase", "name kind nlayers dff")
SPLIT_CASES = tuple(SplitCase(f"split-L{n}-dff{dff}-{kind}", kind, n, dff) for kind in ("int", "real") for n, dff in ((1, 128), (16, 128), (17, 128), (1, 384), (2, 1152)))


def split_inputs(case):
    """the layers' weights, and per layer an output allocation of [4 images][3 pieces][dff 128] bf16 elements (held here as
    float32) between two margins of 64 elements"""
    c, rng = case, np.random.default_rng(_seed(case.name))
    n = 12 * c.dff * D
    assert n == pieces_elems(c.dff)
    return {"W1": [window(_values(rng, (c.dff, D), c.kind)) for _ in range(c.nlayers)], "W2": [window(_values(rng, (D, c.dff), c.kind)) for _ in range(c.nlayers)],
            "out": [Window(np.full(n + 128, BF16_SENTINEL, F32), 64, (12, c.dff * D)) for _ in range(c.nlayers)]}


def split_emulate(case, x, mutant=""):
    out = []
    for l in range(case.nlayers):
        img = split_images(inside(x["W1"][l]), inside(x["W2"][l]), mutant).reshape(12, -1)
        out.append(x["out"][l].buf.copy() if (mutant == "layer16" and l == 16) else embed(x["out"][l], img))
    return out


def split_check(case, x, got, tag="TF-EDGES"):
    """got: per layer, the whole allocation as float32 (from bf16)"""
    res = []
    for l in range(case.nlayers):
        want = split_images(inside(x["W1"][l]), inside(x["W2"][l])).reshape(12, -1)
        res.append(hold(f"{tag} spacap_tf_ffn_split_f32 {case.name}", f"layer {l}", got[l], x["out"][l], want, None))
    return res
