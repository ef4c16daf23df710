"""The contracts of csrc/dense_rows.hip restated in numpy on the host, in float64: the row product of any shape with its two-level
rows, zeroed skipped rows, split over K and batch mode (``rows``), the in-order sum of its slices (``sum_slices``), the weight +
bias gradient of a short, wide product (``wgrad_small``), the block-diagonal weight gradient (``wgrad_blocks``) and the weight
gradient of a tall, narrow product (``wgrad_tall``), the two last as per-slab partial results; the three host helpers that pick a
split, and the predicates by which the host code picks a kernel and allows 16-byte accesses.  With the case tables that reach
every edge of that dispatch, the seeded input builders, the a-priori bar of the ``real`` cases and the figures.  Not a test
module; tests/test_dense_rows_restated_cpu.py anchors the restatement to independent float64 compositions and states the
conditions the device test depends on, tests/test_dense_rows_edges_gpu.py runs the tables through the kernels.

Written from the addressing rules of include/spacap_hip.h and of the comments in csrc/dense_rows.hip, not from the kernels'
loops: every function here gathers its operands by index arithmetic into dense float64 matrices, multiplies them with ``@``, and
scatters the result by index arithmetic into a copy of the output allocation, with a boolean mask of what the call may write.

Two kinds of operand.  ``int``: values from {+-1, +-2, +-3}, never zero.  Everything in the file is fp32 arithmetic on exact
products (v_mfma_f32_16x16x4_f32, __builtin_fmaf), so on such operands every product and every partial sum is an integer below
2^24, exactly representable, and ANY order of summation gives the float64 result bit for bit: the device test compares with
``np.array_equal``, and a dropped, doubled or misplaced term at any k is a mismatch.  ``real``: standard normal, held
elementwise to the standard bound of a float32 sum of n exact products in any order,
    |got - ref64| <= (n + 2) 2^-24 (sum |a| |w| + |bias|),
n the number of terms added into the element (``bar``); nothing of it is measured.

Every operand and every output is a window inside a larger flat allocation with at least one row stride of margin on each
side.  Inputs: the margins and every float the contract does not name (columns beyond K, skipped rows, the gaps between groups,
rows beyond R of a group) hold NaN, so a read of padding shows as a NaN in the result.  Outputs: the allocation is pre-filled
with one finite sentinel, which must survive wherever the mask is off.  A window may start one float past a 16-byte boundary.

``mutant=`` plants one wrong rule at a time, for the test that the tables have teeth.  numpy only."""
import collections
import math

import numpy as np

F32, F64 = np.float32, np.float64
SENTINEL = F32(-777.25)                  # finite, exactly representable, no sum of small integers the tables produce
U = 2.0 ** -24                           # unit roundoff of float32
KC = 128                                 # the row product's K chunk (the unit of a split over K)
TALL_TILE = 32                           # rows per tile of the tall weight gradient (the unit of its slabs)
F64_BAR = 1e-12                          # two float64 computations of one formula, of the largest reference entry
MUTANTS = ("k-tail", "bias-every-slice", "a-skip", "gstride=grp*ld", "o-zero-unwritten", "skipped-zeroed", "slab-last-row",
           "slab-overlap", "co-1", "w-zstride", "db-block")
_cdiv = lambda a, b: -(-a // b)
_up4 = lambda n: (n + 3) // 4 * 4


# ---- the host helpers and the tier predicates, restated ----------------------------------------------------------------------
def rows_slices(R, K, CO):
    """spacap_dense_rows_slices: 1 unless the tile grid is small and the reduction long; then 256 / tiles, at most one slice per
    128-wide chunk and at most 16."""
    tiles, chunks = _cdiv(R, 32) * _cdiv(CO, 64), _cdiv(K, KC)
    if tiles >= 128 or chunks < 4:
        return 1
    return max(min(256 // max(tiles, 1), chunks, 16), 1)


def wgrad_blocks_slabs(R):
    """spacap_dense_wgrad_blocks_slabs: one slab per 128 rows, 1 .. 64"""
    return min(max(_cdiv(R, 128), 1), 64)


def wgrad_tall_slabs(R, M, N):
    """spacap_dense_wgrad_tall_slabs: 512 workgroups over the (m, n) blocks, at most 8 Mi floats of partial results, at least four
    32-row tiles per slab; 0 for an empty shape"""
    if R < 1 or M < 1 or N < 1:
        return 0
    yz = _cdiv(M, 64) * _cdiv(N, 16 if N <= 16 else 144)
    return max(min(512 // yz, (8 << 20) // (M * N), _cdiv(R, 32) // 4), 1)


def rows_tier(R):
    """rows per workgroup of the row product (and of its parent, csrc/linear_rows.hip): 32 up to 1024 rows, 64 beyond"""
    return "MT2" if R <= 1024 else "MT4"


def wgrad_small_tier(M, N):
    """m per thread of the small weight gradient: 8 once the 64 x 128 tiles alone make 200 workgroups, else 2"""
    return 8 if _cdiv(M, 64) * _cdiv(N, 128) >= 200 else 2


def wgrad_tall_tier(N):
    """16-column blocks per workgroup of the tall weight gradient"""
    return 1 if N <= 16 else 9


def rows_vec(a_aligned, lda, a_grp, a_gstride, w_aligned, ldw, o_aligned, ldo, o_grp, o_gstride, slices, slice_stride, batch,
             a_zstride, w_zstride):
    """(vec_a, vec_w, vec_o): 16-byte accesses need an aligned base and every stride that enters the address a multiple of 4
    floats; the z strides count in batch mode only, the slice stride whenever there is more than one slice."""
    az, wz = (a_zstride, w_zstride) if batch else (0, 0)
    return (bool(a_aligned and lda % 4 == 0 and (a_grp == 0 or a_gstride % 4 == 0) and az % 4 == 0),
            bool(w_aligned and ldw % 4 == 0 and wz % 4 == 0),
            bool(o_aligned and ldo % 4 == 0 and (o_grp == 0 or o_gstride % 4 == 0) and (slices == 1 or slice_stride % 4 == 0)))


# ---- addressing ---------------------------------------------------------------------------------------------------------------
def row_offsets(R, ld, grp=0, gstride=0, skip=0):
    """element offset of rows 0 .. R-1: r * ld, or with two-level rows (grp > 0) (r / grp) * gstride + (r % grp + skip) * ld"""
    r = np.arange(R, dtype=np.int64)
    return r * ld if grp <= 0 else (r // grp) * gstride + (r % grp + skip) * ld


def _gather(buf, offs, ncols):
    return np.asarray(buf, F64)[offs[:, None] + np.arange(ncols, dtype=np.int64)[None, :]]


def slice_chunks(K, slices):
    """[(k0, k1)] per slice of a split over K: slice z takes the 128-wide chunks [z per, min(nchunks, (z + 1) per)),
    per = ceil(nchunks / slices); a slice past the last chunk takes nothing"""
    n = _cdiv(K, KC)
    per = _cdiv(n, slices)
    return [(min(z * per, n) * KC, min(min(n, (z + 1) * per) * KC, K)) for z in range(slices)]


def slab_rows(R, nslab, unit=1):
    """[(r0, r1)] per slab: slab s covers the units [s per, min(n, (s + 1) per)), per = ceil(n / nslab), n = ceil(R / unit) units of
    ``unit`` rows (1 for the block-diagonal gradient, 32 for the tall one)"""
    n = _cdiv(R, unit)
    per = _cdiv(n, nslab)
    return [(min(s * per, n) * unit, min(min(n, (s + 1) * per) * unit, R)) for s in range(nslab)]


# ---- the restatements -----------------------------------------------------------------------------------------------------------
def rows(a, lda, a_grp, a_gstride, a_skip, W, ldw, trans_w, bias, R, K, CO, out, ldo, o_grp, o_gstride, o_skip, o_zero, slices,
         slice_stride, batch, a_zstride, w_zstride, mutant=""):
    """spacap_dense_rows_f32 on flat buffers that begin at the pointers the call is given.  Returns (the expected contents of
    ``out`` in float64, the mask of the elements the call may write)."""
    exp, mask = np.asarray(out, F64).copy(), np.zeros(len(out), bool)
    if R == 0:
        return exp, mask
    if mutant == "a-skip":
        a_skip = 0
    if mutant == "gstride=grp*ld" and a_grp > 0:
        a_gstride = a_grp * lda
    if mutant == "w-zstride":
        w_zstride = 0
    ao, oo = row_offsets(R, lda, a_grp, a_gstride, a_skip), row_offsets(R, ldo, o_grp, o_gstride, o_skip)
    cols = np.arange(CO if mutant != "co-1" else CO - 1, dtype=np.int64)
    b = np.zeros(CO) if bias is None else np.asarray(bias, F64)[:CO]
    for z in range(slices):
        az, wz = (z * a_zstride, z * w_zstride) if batch else (0, 0)
        k0, k1 = (0, K) if batch else slice_chunks(K, slices)[z]
        if mutant == "k-tail" and K % 4 and k1 == K:
            k1 = K - 1
        A = _gather(a[az:], ao, K)[:, k0:k1] if k1 > k0 else np.zeros((R, 0))
        if k1 <= k0:
            Wop = np.zeros((0, CO))
        elif trans_w:
            Wop = _gather(W[wz:], np.arange(CO, dtype=np.int64) * ldw, K)[:, k0:k1].T
        else:
            Wop = _gather(W[wz:], np.arange(k0, k1, dtype=np.int64) * ldw, CO)
        with np.errstate(invalid="ignore"):
            val = A @ Wop + (b if batch or z == 0 or mutant == "bias-every-slice" else 0.0)
        at = z * slice_stride + oo[:, None] + cols[None, :]
        exp[at], mask[at] = val[:, :len(cols)], True
        zero = (o_zero and mutant != "o-zero-unwritten") or (mutant == "skipped-zeroed" and not o_zero)
        if zero and o_grp > 0 and o_skip > 0:      # the skipped leading rows of every group that holds a row
            g = np.arange(_cdiv(R, o_grp), dtype=np.int64)[:, None, None] * o_gstride
            at = z * slice_stride + g + np.arange(o_skip, dtype=np.int64)[None, :, None] * ldo + cols[None, None, :]
            exp[at], mask[at] = 0.0, True
    return exp, mask


def sum_slices(parts, S, n, stride, out, dtype=F64):
    """spacap_dense_sum_slices_f32: out[e] = parts[e] + parts[stride + e] + ... in that order, e < n (``dtype`` float32: every
    addition rounded, which the kernel must match to the bit)"""
    exp, mask = np.asarray(out, dtype).copy(), np.zeros(len(out), bool)
    acc = np.asarray(parts[:n], dtype).copy()
    with np.errstate(invalid="ignore"):
        for z in range(1, S):
            acc = (acc + np.asarray(parts[z * stride:z * stride + n], dtype)).astype(dtype)
    exp[:n], mask[:n] = acc, True
    return exp, mask


def wgrad_small(G, ldg, X, ldx, x_grp, x_gstride, x_skip, R, M, N, dW, db, mutant=""):
    """spacap_dense_wgrad_small_f32: dW [M][N] dense = G^T X, db [M] = column sums of G (``db`` None: not asked for); X rows may
    be two-level.  R = 0 gives zeros.  Returns (expected dW, its mask, expected db or None, its mask or None)."""
    if mutant == "a-skip":
        x_skip = 0
    if mutant == "gstride=grp*ld" and x_grp > 0:
        x_gstride = x_grp * ldx
    Gm, Xm = _gather(G, row_offsets(R, ldg), M), _gather(X, row_offsets(R, ldx, x_grp, x_gstride, x_skip), N)
    if mutant == "slab-last-row" and R:
        Gm, Xm = Gm[:-1], Xm[:-1]
    ew, mw = np.asarray(dW, F64).copy(), np.zeros(len(dW), bool)
    with np.errstate(invalid="ignore"):
        val = Gm.T @ Xm
    ncol = N - 1 if mutant == "co-1" else N
    at = (np.arange(M, dtype=np.int64) * N)[:, None] + np.arange(ncol, dtype=np.int64)[None, :]
    ew[at], mw[at] = val[:, :ncol], True
    if db is None:
        return ew, mw, None, None
    eb, mb = np.asarray(db, F64).copy(), np.zeros(len(db), bool)
    s = Gm.sum(0)
    eb[:M], mb[:M] = (np.roll(s, 16 if M > 16 else 1) if mutant == "db-block" else s), True
    return ew, mw, eb, mb


def _slabs(R, nslab, unit, mutant):
    sl = slab_rows(R, nslab, unit)
    if mutant == "slab-last-row":
        sl = [(r0, max(r1 - 1, r0)) for r0, r1 in sl]
    if mutant == "slab-overlap":
        sl = [(r0 - 1 if s and r1 > r0 else r0, r1) for s, (r0, r1) in enumerate(sl)]
    return sl


def wgrad_blocks(G, ldg, X, ldx, R, Z, M, N, nslab, part, mutant=""):
    """spacap_dense_wgrad_blocks_f32: part [nslab][M][Z N], part[s][o][z N + n] = sum over the rows r of slab s of
    G[r][z M + o] X[r][z N + n]; an empty slab is zeros."""
    Gm, Xm = _gather(G, row_offsets(R, ldg), Z * M).reshape(R, Z, M), _gather(X, row_offsets(R, ldx), Z * N).reshape(R, Z, N)
    exp, mask = np.asarray(part, F64).copy(), np.zeros(len(part), bool)
    ncol = N - 1 if mutant == "co-1" else N
    for s, (r0, r1) in enumerate(_slabs(R, nslab, 1, mutant)):
        with np.errstate(invalid="ignore"):
            val = np.stack([Gm[r0:r1, z].T @ Xm[r0:r1, z] for z in range(Z)], 1)            # [M][Z][N]
        at = s * M * Z * N + (np.arange(M, dtype=np.int64) * Z * N)[:, None, None] + (np.arange(Z, dtype=np.int64) * N)[None, :, None] \
            + np.arange(ncol, dtype=np.int64)[None, None, :]
        exp[at], mask[at] = val[:, :, :ncol], True
    return exp, mask


def wgrad_tall(G, ldg, X, ldx, R, M, N, nslab, part, mutant=""):
    """spacap_dense_wgrad_tall_f32: part [nslab][M][N], part[s] = G^T X over the rows of slab s, slabs in whole tiles of 32 rows;
    an empty slab is zeros."""
    Gm, Xm = _gather(G, row_offsets(R, ldg), M), _gather(X, row_offsets(R, ldx), N)
    exp, mask = np.asarray(part, F64).copy(), np.zeros(len(part), bool)
    ncol = N - 1 if mutant == "co-1" else N
    for s, (r0, r1) in enumerate(_slabs(R, nslab, TALL_TILE, mutant)):
        with np.errstate(invalid="ignore"):
            val = Gm[r0:r1].T @ Xm[r0:r1]
        at = s * M * N + (np.arange(M, dtype=np.int64) * N)[:, None] + np.arange(ncol, dtype=np.int64)[None, :]
        exp[at], mask[at] = val[:, :ncol], True
    return exp, mask


def sum_parts(exp, n, count, stride=None):
    """the partial results of ``exp`` (``count`` of them, ``stride`` apart, n elements each) added in order, float64"""
    stride = n if stride is None else stride
    with np.errstate(invalid="ignore"):
        return sum_slices(exp, count, n, stride, np.zeros(n))[0]


# ---- the bar and the figures ------------------------------------------------------------------------------------------------------
def bar(n_terms, magnitude):
    """(n + 2) 2^-24 (sum |a| |w| + |bias|), elementwise: the bound of a float32 sum of n exact products in any order, plus one
    rounding for the bias and one for the store"""
    return (n_terms + 2) * U * np.asarray(magnitude, F64)


def figure(got, want, allowed):
    """the largest |got - want| / allowed over the elements whose reference is finite; where nothing is allowed (a reference of
    exact zeros) the result must be exact.  inf for a NaN where the reference is finite."""
    got, want, allowed = np.asarray(got, F64), np.asarray(want, F64), np.broadcast_to(np.asarray(allowed, F64), np.shape(want))
    ok = np.isfinite(want)
    if not ok.any():
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got[ok] - want[ok])
        ratio = np.where(err == 0.0, 0.0, err / allowed[ok])
    return math.inf if np.isnan(ratio).any() else float(ratio.max())


def mismatches(got, want):
    """elements that differ under exact comparison (a NaN on either side differs from everything)"""
    return int((np.asarray(got, F64) != np.asarray(want, F64)).sum())


def same_nonfinite(got, want):
    """True when got is NaN exactly where want is, and +Inf / -Inf exactly where want is."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
                and np.array_equal(np.isneginf(got), np.isneginf(want)))


# ---- windows and seeded operands ----------------------------------------------------------------------------------------------------
Window = collections.namedtuple("Window", "buf start")        # a flat float32 allocation and the index the operand begins at


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 32 - 5)


def _values(rng, n, kind):
    if kind == "real":
        return rng.standard_normal(n).astype(F32)
    return (rng.integers(1, 4, n) * rng.choice((-1, 1), n)).astype(F32)


def _window(extent, margin, off, fill):
    """an allocation of margin + off + extent + margin floats filled with ``fill``; the margin a multiple of 4, so ``off`` alone
    decides the window's alignment"""
    m = _up4(margin) + 4
    return Window(np.full(m + off + extent + m, fill, F32), m + off)


def _fill(win, rng, index, kind):
    index = np.unique(np.asarray(index, np.int64).ravel())
    win.buf[win.start + index] = _values(rng, len(index), kind)


def _rows_index(offs, ncols):
    return offs[:, None] + np.arange(ncols, dtype=np.int64)[None, :]


# ---- spacap_dense_rows_f32 (and its parent spacap_linear_rows_f32): cases --------------------------------------------------------
RowsCase = collections.namedtuple("RowsCase", "name kind R K CO trans bias lda ldw ldo a_rows o_rows o_zero slices sstride batch a_z w_z "
                                  "a_off w_off o_off tier vec poison")
RowsIn = collections.namedtuple("RowsIn", "a W bias out")       # three Windows and the bias (dense float32, or None)


def _extent(R, ncols, ld, rows3):
    return int(row_offsets(R, ld, *rows3)[-1]) + ncols if R else 0


def _r(name, kind, R, K, CO, trans=1, bias=0, lda=None, ldw=None, ldo=None, a_rows=(0, 0, 0), o_rows=(0, 0, 0), o_zero=0, slices=1,
       sstride=None, batch=0, a_z=0, w_z=0, a_off=0, w_off=0, o_off=0, vec="awo", poison=0):
    """defaults: padded rows (stride a multiple of 4 beyond the row), slices one padded result apart.  ``vec`` names the 16-byte
    switches the case is in the table to find ON, ``tier`` the kernel instance; the CPU test holds both to the predicates."""
    lda = _up4(K) + 4 if lda is None else lda
    ldw = _up4(K if trans else CO) + 4 if ldw is None else ldw
    ldo = _up4(CO) + 4 if ldo is None else ldo
    if sstride is None:
        sstride = 0 if slices == 1 else _up4(_extent(R, CO, ldo, o_rows)) + 8
    tier = name[:3] if name.startswith("MT") else None         # what the name claims
    return RowsCase(f"{name}-{kind}", kind, R, K, CO, trans, bias, lda, ldw, ldo, a_rows, o_rows, o_zero, slices, sstride, batch, a_z, w_z,
                    a_off, w_off, o_off, tier, vec, poison)


def _two(grp, skip, ld, extra):
    return (grp, (grp + skip) * ld + extra, skip)


def _rows_table():
    t = []
    Rs, Ks, COs = (1, 31, 32, 33, 1024, 1025), (1, 3, 4, 5, 127, 128, 129, 131, 257), (1, 3, 15, 16, 17, 63, 64, 65)
    for kind in ("int", "real"):
        # the shape sweep: every R, K, CO of the lists, both layouts of W, with and without bias; padded strides, all switches on
        for j, (trans, bias) in enumerate(((1, 1), (1, 0), (0, 1), (0, 0))):
            for i, K in enumerate(Ks):
                R, CO = Rs[(i + j) % 6], COs[(i + 2 * j + i // 8) % 8]
                t.append(_r(f"{'MT4' if R == 1025 else 'MT2'}-R{R}-K{K}-CO{CO}-{'wT' if trans else 'w'}{'-bias' if bias else ''}", kind, R, K, CO, trans, bias))
        # the tier edge once more with both column blocks and a K tail, dense rows of odd length (every switch off by its stride)
        for R in (1024, 1025):
            t.append(_r(f"{'MT4' if R == 1025 else 'MT2'}-R{R}-dense-odd", kind, R, 131, 65, 1, 1, lda=131, ldw=131, ldo=65, vec=""))
        # each switch off alone, by each of its causes (K % 4 != 0 and CO % 4 != 0 throughout)
        g5 = lambda ld, extra: _two(5, 1, ld, extra)
        for trans in (1, 0):
            w = "wT" if trans else "w"
            t += [_r(f"vec-a-off-base-{w}", kind, 33, 131, 17, trans, 1, a_off=1, vec="wo"),
                  _r(f"vec-a-off-row-stride-{w}", kind, 33, 131, 17, trans, 0, lda=133, vec="wo"),
                  _r(f"vec-a-off-group-stride-{w}", kind, 33, 131, 17, trans, 1, a_rows=g5(136, 6), vec="wo"),
                  _r(f"vec-a-off-z-stride-{w}", kind, 33, 131, 17, trans, 1, slices=3, batch=1, a_z=33 * 136 + 9, w_z=4 * 17 * 136, vec="wo"),
                  _r(f"vec-w-off-base-{w}", kind, 33, 131, 17, trans, 1, w_off=1, vec="ao"),
                  _r(f"vec-w-off-row-stride-{w}", kind, 33, 131, 17, trans, 0, ldw=133 if trans else 23, vec="ao"),
                  _r(f"vec-w-off-z-stride-{w}", kind, 33, 131, 17, trans, 1, slices=3, batch=1, a_z=33 * 136 + 8, w_z=4 * 132 * 136 + 2, vec="ao"),
                  _r(f"vec-o-off-base-{w}", kind, 33, 131, 17, trans, 1, o_off=1, vec="aw"),
                  _r(f"vec-o-off-row-stride-{w}", kind, 33, 131, 17, trans, 0, ldo=21, vec="aw"),
                  _r(f"vec-o-off-group-stride-{w}", kind, 33, 131, 17, trans, 1, o_rows=g5(24, 2), vec="aw"),
                  _r(f"vec-o-off-slice-stride-{w}", kind, 33, 300, 17, trans, 1, slices=2, sstride=33 * 24 + 10, vec="aw"),
                  _r(f"vec-o-off-batch-stride-{w}", kind, 33, 131, 17, trans, 1, slices=3, batch=1, a_z=33 * 136 + 8, w_z=4 * 132 * 136,
                     sstride=33 * 24 + 9, vec="aw")]
        # two-level A: rows per group x skipped rows, the group stride once exactly (grp + skip) lda and else larger; R = 33 leaves
        # the last group short
        for grp in (1, 5, 31):
            for skip in (0, 1, 2):
                K = (5, 129, 16)[skip]
                t.append(_r(f"a-grp{grp}-skip{skip}-K{K}", kind, 33, K, 17, skip != 1, 1, a_rows=_two(grp, skip, _up4(K) + 4, 0 if grp == 5 and skip == 1 else 8)))
        # two-level out: the skipped rows zeroed, or left alone
        for grp in (1, 5, 7):
            for skip in (0, 1, 2):
                for o_zero in (0, 1):
                    CO = 65 if grp == 7 else 17
                    t.append(_r(f"o-grp{grp}-skip{skip}-{'zeroed' if o_zero else 'kept'}", kind, 33, 16 if skip == 2 else 129, CO, grp != 5, 1,
                                o_rows=_two(grp, skip, _up4(CO) + 4, 8 * (skip != 1)), o_zero=o_zero))
        # split over K: 3 and 4 chunks over 1 .. 5 slices (counts that do not divide, slices without a chunk), bias in slice 0, the
        # last two under two-level output rows with zeroed skipped rows
        for K in (300, 401):
            for S in (1, 2, 3, 4, 5):
                two = S >= 4
                t.append(_r(f"split-K{K}-S{S}{'-zeroed' if two else ''}", kind, 33, K, 17, (K + S) % 2, 1, slices=S,
                            o_rows=_two(5, 2, 24, 8) if two else (0, 0, 0), o_zero=int(two)))
        # batch mode: three products, every z stride once a multiple of 4 and once not, bias in every z
        for trans in (1, 0):
            for odd in (0, 1):
                t.append(_r(f"batch-{'wT' if trans else 'w'}-{'odd' if odd else 'x4'}-strides", kind, 33, 16 if odd else 129, 17, trans, 1, slices=3,
                            batch=1, a_z=33 * 136 + 8 + odd, w_z=4 * 132 * 136 + 3 * odd, sstride=33 * 24 + 8 + 5 * odd, vec="" if odd else "awo"))
        # the relation head's value projection and its data gradient, H = 3, D = 5, C = 17 on B K = 2 x 9 rows: the heads' windows
        # of one packed q | k | v row and of one weight matrix, interleaved in one output row
        H, D, C, Rr = 3, 5, 17, 18
        t += [_r("relation-u", kind, Rr, D, C, 1, 0, lda=3 * H * D, ldw=H * D, ldo=H * C, slices=H, sstride=C, batch=1, a_z=D, w_z=D, a_off=2 * H * D,
                 vec=""),
              _r("relation-dv", kind, Rr, C, D, 0, 0, lda=H * C, ldw=H * D, ldo=H * D, slices=H, sstride=D, batch=1, a_z=C, w_z=D, vec="")]
    # non-finite: a +Inf at the K tail of one row, a NaN in another; a split, so that the slices differ
    t += [_r("nonfinite", "int", 33, 131, 17, 1, 1, poison=1), _r("nonfinite-split-w", "int", 33, 401, 17, 0, 1, slices=3, poison=1)]
    return tuple(t)


def _lin_table():
    """spacap_linear_rows_f32: dense operands, K in {128, 512}, CO in {64, 192}"""
    t = []
    for kind in ("int", "real"):
        for i, R in enumerate((1, 32, 33, 1024, 1025)):
            for trans in (1, 0):
                K, CO = ((128, 64), (512, 192), (128, 192), (512, 64))[(i + trans) % 4]
                t.append(_r(f"{'MT4' if R == 1025 else 'MT2'}-lin-R{R}-K{K}-CO{CO}-{'wT' if trans else 'w'}", kind, R, K, CO, trans, (i + trans) % 2, lda=K, ldw=K if trans else CO, ldo=CO))
    t.append(_r("lin-nonfinite", "int", 33, 128, 64, 1, 1, lda=128, ldw=128, ldo=64, poison=1))
    return tuple(t)


ROWS_CASES, LIN_CASES = _rows_table(), _lin_table()


def rows_inputs(case):
    c, rng = case, np.random.default_rng(_seed(case.name))
    Z = c.slices if c.batch else 1
    ao = row_offsets(c.R, c.lda, *c.a_rows)
    a = _window(_extent(c.R, c.K, c.lda, c.a_rows) + (Z - 1) * c.a_z, max(c.lda, c.a_rows[1]), c.a_off, np.nan)
    wrows, wcols = (c.CO, c.K) if c.trans else (c.K, c.CO)
    W = _window((wrows - 1) * c.ldw + wcols + (Z - 1) * c.w_z, c.ldw, c.w_off, np.nan)
    for z in range(Z):
        _fill(a, rng, z * c.a_z + _rows_index(ao, c.K), c.kind)
        _fill(W, rng, z * c.w_z + _rows_index(row_offsets(wrows, c.ldw), wcols), c.kind)
    if c.poison:      # +Inf at the last k (a K tail) of row 1, NaN at k = 0 of the last row
        a.buf[a.start + ao[1] + c.K - 1], a.buf[a.start + ao[-1]] = np.inf, np.nan
    bias = _values(rng, c.CO, c.kind) if c.bias else None
    # (the skipped rows of group 0 lie before row 0 and after the pointer: inside the window)
    out = _window(_extent(c.R, c.CO, c.ldo, c.o_rows) + (c.slices - 1) * c.sstride, max(c.ldo, c.o_rows[1]), c.o_off, SENTINEL)
    return RowsIn(a, W, bias, out)


def rows_call(case, x):
    """the argument list of ``rows`` (and, with pointers for the buffers, of spacap_dense_rows_f32)"""
    c = case
    return (x.a.buf[x.a.start:], c.lda, *c.a_rows, x.W.buf[x.W.start:], c.ldw, c.trans, x.bias, c.R, c.K, c.CO, x.out.buf[x.out.start:], c.ldo,
            *c.o_rows, c.o_zero, c.slices, c.sstride, c.batch, c.a_z, c.w_z)


def _whole(win, exp, mask):
    """(expected, mask) of the part after the window's start, extended over the whole allocation"""
    return np.concatenate([np.asarray(win.buf[:win.start], exp.dtype), exp]), np.concatenate([np.zeros(win.start, bool), mask])


def rows_reference(case, x, mutant=""):
    """(expected contents of the whole output allocation, mask of what may be written)"""
    return _whole(x.out, *rows(*rows_call(case, x), mutant=mutant))


def rows_magnitude(case, x):
    """sum |a| |w| + |bias| per written element, laid out as the output (for ``bar``)"""
    call = list(rows_call(case, x))
    call[0], call[5] = np.abs(call[0]), np.abs(call[5])
    call[8] = None if call[8] is None else np.abs(call[8])
    return _whole(x.out, *rows(*call))[0]


def rows_vec_of(case, x):
    c = case
    al = lambda w: w.start % 4 == 0
    return rows_vec(al(x.a), c.lda, c.a_rows[0], c.a_rows[1], al(x.W), c.ldw, al(x.out), c.ldo, c.o_rows[0], c.o_rows[1], c.slices, c.sstride,
                    c.batch, c.a_z, c.w_z)


def rows_summed(case, exp):
    """the slices of a split over K (expected contents from the window's start on) added in order: n = the slice stride"""
    return sum_parts(exp, case.sstride, case.slices)


# ---- spacap_dense_sum_slices_f32 ----------------------------------------------------------------------------------------------------
SumCase = collections.namedtuple("SumCase", "name kind n S stride poison")
SUM_CASES = tuple(SumCase(f"sum-n{n}-S{S}-stride{st}-{kind}", kind, n, S, st, 0)
                  for kind in ("int", "real")
                  for i, n in enumerate((1, 3, 4, 5, 1020, 1023, 1024, 1025))
                  for S in ((1, 2, 5)[i % 3], (1, 2, 5)[(i + 1) % 3])
                  for st in (_up4(n) + 4 * (i % 2) + 4 * (S == 5),)) + (SumCase("sum-nonfinite-int", "int", 1023, 5, 1032, 1),)
SumIn = collections.namedtuple("SumIn", "parts out")


def sum_inputs(case):
    rng = np.random.default_rng(_seed(case.name))
    parts = _window((case.S - 1) * case.stride + case.n, case.stride, 0, np.nan)
    _fill(parts, rng, (np.arange(case.S) * case.stride)[:, None] + np.arange(case.n)[None, :], case.kind)
    if case.poison:      # +Inf in the scalar tail of one slice, NaN in another, -Inf against +Inf in a third element
        s = parts.start
        parts.buf[s + 2 * case.stride + case.n - 1], parts.buf[s + case.stride + 5] = np.inf, np.nan
        parts.buf[s + 8], parts.buf[s + 4 * case.stride + 8] = np.inf, -np.inf
    return SumIn(parts, _window(case.n, case.stride, 0, SENTINEL))


def sum_reference(case, x, dtype=F64):
    return _whole(x.out, *sum_slices(x.parts.buf[x.parts.start:], case.S, case.n, case.stride, x.out.buf[x.out.start:], dtype))


# ---- the weight gradients ---------------------------------------------------------------------------------------------------------------
GradCase = collections.namedtuple("GradCase", "name entry kind R Z M N ldg ldx x_rows nslab db tier poison")
GradIn = collections.namedtuple("GradIn", "G X out db")        # Windows; ``db`` None where the entry point has none or it is not asked for


def _g(entry, name, kind, R, M, N, Z=1, ldg=None, ldx=None, x_rows=(0, 0, 0), nslab=1, db=1, poison=0):
    ldg, ldx = Z * M if ldg is None else ldg, Z * N if ldx is None else ldx
    tier = {"mt8": 8, "mt2": 2, "nt1": 1, "nt9": 9}.get(name[:3])         # what the name claims
    return GradCase(f"{name}-{kind}", entry, kind, R, Z, M, N, ldg, ldx, x_rows, nslab, db if entry == "small" else 0, tier, poison)


def _grad_tables():
    small, blocks, tall = [], [], []
    for kind in ("int", "real"):
        small += [_g("small", "mt8-R70-M1411-N1027", kind, 70, 1411, 1027), _g("small", "mt2-R70-M1347-N1027", kind, 70, 1347, 1027)]
        Ms, Ns = (1, 15, 16, 17), (1, 3, 127, 128, 129, 131)
        for i, R in enumerate((0, 1, 63, 64, 65, 129)):
            M, N = Ms[i % 4], Ns[i]
            small.append(_g("small", f"mt2-R{R}-M{M}-N{N}", kind, R, M, N))
            small.append(_g("small", f"mt2-R{R}-M{Ms[(i + 2) % 4]}-N{Ns[(i + 3) % 6]}-strided{'' if i % 2 else '-no-db'}", kind, R, Ms[(i + 2) % 4], Ns[(i + 3) % 6],
                            ldg=Ms[(i + 2) % 4] + 3, ldx=Ns[(i + 3) % 6] + 5, db=i % 2))
        for grp in (5, 31):
            for skip in (1, 2):
                N = 131 if grp == 5 else 16
                small.append(_g("small", f"mt2-x-grp{grp}-skip{skip}", kind, 65, 17, N, ldx=N + 1, x_rows=_two(grp, skip, N + 1, 3 * skip)))
        Zs, Ms, Ns, Rs = (1, 3, 8), (1, 16, 127, 128, 129), (1, 7, 8, 9, 16, 17), (1, 7, 8, 9, 130)
        for i in range(12):
            R, Z, M, N = Rs[i % 5], Zs[i % 3], Ms[(i + i // 5) % 5], Ns[i % 6]
            ns = (1, 2, 3, R + 1)[(i + i // 4) % 4]
            pad = 3 * (i % 2)
            blocks.append(_g("blocks", f"blocks-R{R}-Z{Z}-M{M}-N{N}-slabs{ns}{'-strided' if pad else ''}", kind, R, M, N, Z=Z, nslab=ns,
                             ldg=Z * M + pad, ldx=Z * N + 2 * pad))
        blocks.append(_g("blocks", "blocks-R130-Z8-M129-N17-slabs131", kind, 130, 129, 17, Z=8, nslab=131))
        Rs, Ms, Ns = (1, 31, 32, 33, 127, 129), (1, 63, 64, 65), (1, 15, 16, 17, 143, 144, 145)
        for i in range(14):
            R, M, N = Rs[i % 6], Ms[(i + i // 4) % 4], Ns[i % 7]
            ns = (1, 2, _cdiv(R, 32), _cdiv(R, 32) + 1)[(i + i // 6) % 4]
            pad = 5 * (i % 2)
            tall.append(_g("tall", f"{'nt1' if N in (1, 15, 16) else 'nt9'}-tall-R{R}-M{M}-N{N}-slabs{ns}{'-strided' if pad else ''}", kind, R, M, N, nslab=ns, ldg=M + pad, ldx=N + pad // 5 * 3))
        tall.append(_g("tall", "nt9-tall-R127-M65-N17-slabs4", kind, 127, 65, 17, nslab=4))          # one tile per slab, none empty
    # non-finite: +Inf in the last row of a slab (a chunk, a tile) whose length is no multiple of the unroll, a NaN elsewhere
    small.append(_g("small", "small-nonfinite", "int", 70, 17, 131, poison=1))
    blocks.append(_g("blocks", "blocks-nonfinite", "int", 13, 17, 9, Z=3, nslab=2, poison=1))
    tall.append(_g("tall", "tall-nonfinite", "int", 70, 65, 17, nslab=2, poison=1))
    return tuple(small), tuple(blocks), tuple(tall)


SMALL_CASES, BLOCKS_CASES, TALL_CASES = _grad_tables()
GRAD_CASES = SMALL_CASES + BLOCKS_CASES + TALL_CASES


def poison_rows(case):
    """(row of the +Inf, row of the NaN) in X.  Block-diagonal: the +Inf in the last row of slab 0, whose 7 rows are no multiple of
    the eight the kernel takes at a time, the NaN in the last row of all.  Small and tall: the +Inf in the last row of all, the
    sixth of its 64-row chunk or 32-row tile, the NaN in row 3 or in the last row of slab 0."""
    c = case
    if c.entry == "blocks":
        return slab_rows(c.R, c.nslab)[0][1] - 1, c.R - 1
    return c.R - 1, (slab_rows(c.R, c.nslab, TALL_TILE)[0][1] - 1 if c.entry == "tall" else 3)


def grad_inputs(case):
    c, rng = case, np.random.default_rng(_seed(case.name))
    xo = row_offsets(c.R, c.ldx, *c.x_rows)
    G = _window(_extent(c.R, c.Z * c.M, c.ldg, (0, 0, 0)), c.ldg, 0, np.nan)
    X = _window(_extent(c.R, c.Z * c.N, c.ldx, c.x_rows), max(c.ldx, c.x_rows[1]), 0, np.nan)
    _fill(G, rng, _rows_index(row_offsets(c.R, c.ldg), c.Z * c.M), c.kind)
    _fill(X, rng, _rows_index(xo, c.Z * c.N), c.kind)
    if c.poison:         # +Inf in the last column of its (z-th) block, NaN in the first column
        ri, rn = poison_rows(c)
        X.buf[X.start + xo[ri] + c.Z * c.N - 1], X.buf[X.start + xo[rn]] = np.inf, np.nan
    out = _window(c.nslab * c.M * c.Z * c.N, c.Z * c.N, 0, SENTINEL)
    return GradIn(G, X, out, _window(c.M, c.M, 0, SENTINEL) if c.db else None)


def grad_reference(case, x, mutant="", magnitude=False):
    """{'part' or 'dW': (expected whole allocation, mask), 'db': ...}; ``magnitude``: on the operands' absolute values (for ``bar``)"""
    c = case
    f = np.abs if magnitude else (lambda v: v)
    G, X, out = f(x.G.buf[x.G.start:]), f(x.X.buf[x.X.start:]), x.out.buf[x.out.start:]
    if c.entry == "small":
        ew, mw, eb, mb = wgrad_small(G, c.ldg, X, c.ldx, *c.x_rows, c.R, c.M, c.N, out, x.db.buf[x.db.start:] if c.db else None, mutant=mutant)
        ref = {"dW": _whole(x.out, ew, mw)}
        if c.db:
            ref["db"] = _whole(x.db, eb, mb)
        return ref
    if c.entry == "blocks":
        return {"part": _whole(x.out, *wgrad_blocks(G, c.ldg, X, c.ldx, c.R, c.Z, c.M, c.N, c.nslab, out, mutant=mutant))}
    return {"part": _whole(x.out, *wgrad_tall(G, c.ldg, X, c.ldx, c.R, c.M, c.N, c.nslab, out, mutant=mutant))}
