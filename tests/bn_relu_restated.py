"""The kernels of csrc/bn_relu.hip and csrc/group_max.hip restated in numpy on the host: train-mode BatchNorm -> ReLU (-> max over
the S samples of a group), its gradient, the running-buffer update, the eval form and the plain group max, with the case tables
that reach every edge of the kernels' dispatch, the seeded and conditioned input builders, the bars and the figures.  Not a test
module; tests/test_bn_relu_restated_cpu.py anchors the restatement to PyTorch's float64 composition and states the conditions
the device test depends on, tests/test_bn_relu_edges_gpu.py runs the tables through the kernels.

Semantics, from the composition the kernels replace (BatchNorm1d/2d(train) -> relu -> max_pool2d([1, S])): the biased variance
normalises, the unbiased one goes into running_var, eps sits inside the root, the first maximum wins, a NaN passes through the
ReLU and wins the max (the first NaN, where a group holds several), and the ReLU's gradient passes wherever the output is not
<= 0 (so also where it is NaN).

Two precisions.  dtype=float64 (the default) is the reference: plain two-pass float64 arithmetic on the float32 inputs.
dtype=float32 is "float32 done right": the kernels' expressions in their order, every product and sum rounded to float32
(numpy never contracts), the per-channel sums in float64 as the kernels take them.  The float32 variant sets the bars; its
``mutant`` argument plants one wrong expression at a time, for the test that the bars have teeth.

The arithmetic uses numpy only; torch appears in no formula here."""
import collections
import functools
import math

import numpy as np

F32, F64 = np.float32, np.float64
EPS, MOMENTUM = 1e-5, 0.1                 # torch.nn.BatchNorm's defaults, as every layer of the model uses them
MARGIN = 1e-4                             # conditioning: relative to |xhat gamma| + |beta| of the element

# ---- the bars --------------------------------------------------------------------------------------------------------------
# FIGURE_32[q]: the largest max |float32 variant - float64| / max |float64| over every case of the tables (the offset-channel
# cases apart), as tests/test_bn_relu_restated_cpu.py measures and prints it; the CPU test holds these constants to what it
# measures.  BAR[q] = min(16 FIGURE_32[q], CAP[q]): the factor covers what the variant does not model (the kernels' istd * gamma
# association against a library's, a device square root or reciprocal that is not correctly rounded, another order of the float64
# sums).  CAP[q] is what tests/test_ops_gpu.py allows for the quantity today, so nothing loosens: rtol 1e-4 for values, 2e-4 of
# scale for gradients, rtol 1e-5 for the running buffers (the statistics record has no bar there: it takes the running buffers').
QUANTITIES = ("y", "pooled", "dz", "dgamma", "dbeta", "running_mean", "running_var", "stats_mean", "stats_istd")
CAP = {"y": 1e-4, "pooled": 1e-4, "dz": 2e-4, "dgamma": 2e-4, "dbeta": 2e-4, "running_mean": 1e-5, "running_var": 1e-5,
       "stats_mean": 1e-5, "stats_istd": 1e-5}
FIGURE_32 = {"y": 4.8049e-07, "pooled": 1.3883e-07, "dz": 2.6338e-07, "dgamma": 3.4932e-07, "dbeta": 5.0499e-08,
             "running_mean": 4.3654e-08, "running_var": 5.3464e-08, "stats_mean": 5.8952e-08, "stats_istd": 5.4348e-08}
# the cases with a channel of mean / std = 1e3: float32 itself loses three digits in z - mean there
FIGURE_32_OFFSET = {"y": 5.5895e-06, "pooled": 3.7625e-06, "dz": 8.8012e-07, "dgamma": 5.6486e-06, "dbeta": 1.1435e-08,
                    "running_mean": 3.5548e-08, "running_var": 3.4568e-08, "stats_mean": 2.5233e-08, "stats_istd": 4.4311e-08}
FACTOR = 16.0
BAR = {q: min(FACTOR * FIGURE_32[q], CAP[q]) for q in QUANTITIES}
BAR_OFFSET = {q: min(FACTOR * FIGURE_32_OFFSET[q], CAP[q]) for q in QUANTITIES}
F64_BAR = 1e-12                           # two float64 computations of one formula, of the largest reference entry


def bars(case):
    return BAR_OFFSET if case.kind == "offset" else BAR


def figure(got, want):
    """max |got - want| / max |want| over the elements whose reference is finite; a reference that is identically zero must be
    reproduced exactly."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    ok = np.isfinite(want)
    if not ok.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        err, ref = np.abs(got[ok] - want[ok]).max(), np.abs(want[ok]).max()
    if np.isnan(err):
        return math.inf
    if ref == 0.0:
        return 0.0 if err == 0.0 else math.inf
    return float(err / ref)


def same_nonfinite(got, want):
    """True when got is NaN exactly where want is, and +Inf / -Inf exactly where want is."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
                and np.array_equal(np.isneginf(got), np.isneginf(want)))


def same_zeros(got, want):
    """True when got is exactly zero exactly where want is."""
    return bool(np.array_equal(np.asarray(got) == 0.0, np.asarray(want) == 0.0))


# ---- the host code's dispatch, restated (csrc/bn_relu.hip: bn_small, pick_split, grid_x) ------------------------------------
STAT_THREADS = 256


def bn_small(B, C, L, single_launch=True):
    return bool(single_launch and L % 4 == 0 and C >= 64 and B * L <= 32768)


def pick_split(C, elems_per_channel):
    want = max(4096 // max(C, 1), 1)
    return min(want, int(elems_per_channel / (STAT_THREADS * 8)) + 1, 256)


def grid_x(L):
    return min(max((L + 4095) // 4096, 1), 64)


def apply_trips(L):
    """trips of the busiest thread round the grid-stride loop of bn_relu_apply_kernel / bn_bwd_dz_kernel"""
    per_trip = grid_x(L) * (1024 if L % 4 == 0 else 256)
    return -(-L // per_trip)


# ---- group max ---------------------------------------------------------------------------------------------------------------
def group_max(x, last=False):
    """x (..., S) -> (max over the last axis, its index as uint8): the first maximum, a NaN before any number, the first NaN.
    last=True is the mutant in which the last maximum wins."""
    x = np.asarray(x)
    S = x.shape[-1]
    nan = np.isnan(x)
    with np.errstate(invalid="ignore"):
        key = np.where(nan, np.inf, x)                 # a NaN ranks above +Inf ...
        key_is_top = np.where(nan.any(-1, keepdims=True), nan, key == key.max(-1, keepdims=True))   # ... and only NaNs tie with it
    arg = (S - 1 - key_is_top[..., ::-1].argmax(-1)) if last else key_is_top.argmax(-1)
    val = np.take_along_axis(x, arg[..., None], -1)[..., 0]
    return val, arg.astype(np.uint8)


def group_max_grad(go, arg, S):
    """go (...), arg (...) -> (..., S): go at sample arg of each group, exact zeros elsewhere"""
    go = np.asarray(go)
    out = np.zeros(go.shape + (S,), go.dtype)
    np.put_along_axis(out, np.asarray(arg, np.int64)[..., None], go[..., None], -1)
    return out


# ---- BatchNorm -> ReLU (-> max) ----------------------------------------------------------------------------------------------
Fwd = collections.namedtuple("Fwd", "y pooled arg mean var istd xhat pre M")
Bwd = collections.namedtuple("Bwd", "dz dgamma dbeta")
MUTANTS = ("drop-one", "M-1", "eps-outside", "last-max", "mask-z>mean", "row/B", "biased-running")


def forward(z, gamma, beta, eps=EPS, S=None, dtype=F64, mutant=""):
    """z (B, C, ...) float32 -> Fwd.  y has z's shape; with S the last axis (of size S) is max-reduced into ``pooled`` with its
    ``arg``.  mean and var (biased) are float64 in both variants, as the kernels keep them; istd, xhat, pre and y have ``dtype``."""
    z, gamma, beta = np.asarray(z), np.asarray(gamma), np.asarray(beta)
    assert z.dtype == F32 and gamma.dtype == F32 and beta.dtype == F32
    B, C = z.shape[:2]
    zr = z.reshape(B, C, -1)
    L = zr.shape[2]
    M = B * L
    with np.errstate(invalid="ignore", over="ignore"):
        if dtype == F64:
            assert not mutant
            z64 = zr.astype(F64)
            mean = z64.mean((0, 2))
            var = ((z64 - mean[None, :, None]) ** 2).mean((0, 2))
            istd = 1.0 / np.sqrt(var + eps)
            xhat = (z64 - mean[None, :, None]) * istd[None, :, None]
            pre = xhat * gamma.astype(F64)[None, :, None] + beta.astype(F64)[None, :, None]
        else:
            # bn_stats_partial / bn_stats_final (spacap::bn_channel): float64 (sum, sum of squares), var = q / M - mean^2 clamped
            zc = zr.transpose(1, 0, 2).reshape(C, M).astype(F64)
            if mutant == "drop-one":
                zc = zc[:, :-1]
            Mn = F64(M - 1 if mutant == "M-1" else M)
            mean = zc.sum(1) / Mn
            var = (zc * zc).sum(1) / Mn - mean * mean
            var = np.where(var < 0.0, 0.0, var)
            e = F64(F32(eps))
            istd = (1.0 / (np.sqrt(var) + e) if mutant == "eps-outside" else 1.0 / np.sqrt(var + e)).astype(F32)
            # the apply kernels: rows = (b, c), c = row % C;  (z - mean) * (istd * gamma) + beta
            rows = np.arange(B * C)
            c = rows // B if mutant == "row/B" else rows % C
            mean32, sc = mean.astype(F32), istd * gamma
            zrow = zr.reshape(B * C, L)
            pre = ((zrow - mean32[c, None]) * sc[c, None] + beta[c, None]).reshape(B, C, L)
            xhat = ((zrow - mean32[c, None]) * istd[c, None]).reshape(B, C, L)       # as the backward kernels form it
            assert pre.dtype == F32 and xhat.dtype == F32
        y = np.maximum(pre, dtype(0)).reshape(z.shape)         # np.maximum hands a NaN on
    pooled = arg = None
    if S:
        assert z.shape[-1] == S
        pooled, arg = group_max(y, last=mutant == "last-max")
    return Fwd(y, pooled, arg, mean, var, istd, xhat.reshape(z.shape), pre.reshape(z.shape), M)


def backward(z, gamma, beta, f, up, S=None, arg=None, dtype=F64, mutant=""):
    """Gradient of sum(up * out) with respect to z, gamma and beta; f is forward()'s result of the same dtype.  With S, up has
    the pooled shape and goes to sample ``arg`` (f.arg unless given) of each group."""
    z, gamma, beta, up = np.asarray(z), np.asarray(gamma), np.asarray(beta), np.asarray(up)
    B, C = z.shape[:2]
    L = z.size // (B * C)
    M = F64(f.M - 1 if mutant == "M-1" else f.M)
    bc = lambda a: a.reshape((1, C) + (1,) * (z.ndim - 2))
    red = (0,) + tuple(range(2, z.ndim))
    with np.errstate(invalid="ignore", over="ignore"):
        d = up.astype(dtype)
        if S:
            d = group_max_grad(d, f.arg if arg is None else arg, S)
        assert d.shape == z.shape
        if dtype == F64:
            mask = ~(f.pre <= 0.0)
            dy = np.where(mask, d, 0.0)
            dbeta, dgamma = dy.sum(red), (dy * f.xhat).sum(red)
            dz = bc(gamma.astype(F64) * f.istd) * (dy - bc(dbeta / M) - f.xhat * bc(dgamma / M))
            return Bwd(dz, dgamma, dbeta)
        # bn_bwd_partial / bn_bwd_pooled_partial / bn_bwd_final / bn_bwd_dz: the mask from xhat * gamma + beta
        rows = np.arange(B * C)
        c = (rows // B if mutant == "row/B" else rows % C).reshape(B, C)
        par = lambda a: a[c].reshape((B, C) + (1,) * (z.ndim - 2))
        if mutant == "mask-z>mean":
            mask = z > par(f.mean.astype(F32))
        else:
            mask = ~(f.xhat * par(gamma) + par(beta) <= F32(0))
        dy = np.where(mask, d, F32(0))
        s1, s2 = dy.astype(F64).sum(red), (dy.astype(F64) * f.xhat.astype(F64)).sum(red)
        k1, k2, gr = (s1 / M).astype(F32), (s2 / M).astype(F32), gamma * f.istd
        dz = par(gr) * (dy - par(k1) - f.xhat * par(k2))
        assert dz.dtype == F32
        return Bwd(dz, s2.astype(F32), s1.astype(F32))


def running_update(running_mean, running_var, f, momentum=MOMENTUM, dtype=F64, mutant=""):
    """(running_mean, running_var) after one training forward: (1 - momentum) old + momentum (mean, UNBIASED variance)"""
    with np.errstate(invalid="ignore", over="ignore"):
        M = F64(f.M)
        unbiased = f.var if mutant == "biased-running" or f.M <= 1 else f.var * M / (M - 1.0)
        mom = F64(F32(momentum)) if dtype == F32 else F64(momentum)
        rm = (1.0 - mom) * running_mean.astype(F64) + mom * f.mean
        rv = (1.0 - mom) * running_var.astype(F64) + mom * unbiased
        return rm.astype(dtype), rv.astype(dtype)


def eval_forward(z, gamma, beta, running_mean, running_var, eps=EPS, dtype=F64):
    """relu(batch_norm(z)) on the running statistics"""
    z = np.asarray(z)
    bc = lambda a: np.asarray(a).astype(dtype).reshape((1, -1) + (1,) * (z.ndim - 2))
    with np.errstate(invalid="ignore", over="ignore"):
        if dtype == F64:
            return np.maximum((z.astype(F64) - bc(running_mean)) / np.sqrt(bc(running_var) + eps) * bc(gamma) + bc(beta), 0.0)
        istd = (F32(1) / np.sqrt(np.asarray(running_var, F32) + F32(eps))).astype(F32)    # fused_bn.bn_relu_eval's fold
        out = np.maximum((z - bc(running_mean)) * bc(istd * np.asarray(gamma, F32)) + bc(beta), F32(0))
        assert out.dtype == F32
        return out


# ---- case tables -----------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name shape S kind momentum track")


def _c(name, shape, kind="", momentum=MOMENTUM, track=True, pooled=False):
    return Case(name, tuple(shape), shape[3] if pooled else None, kind, momentum, track)


_KIND_DENSE, _KIND_POOLED = (2, 4, 52), (2, 4, 7, 32)
DENSE_CASES = (
    # bn_small: L % 4 == 0 and C >= 64 and B L <= 32768
    _c("small-last", (4, 64, 8192)), _c("small-one-group-over", (4, 64, 8196)), _c("small-C63", (2, 63, 4096)),
    _c("small-L-odd", (2, 64, 4098)), _c("small-tiny", (3, 64, 4)),
    # pick_split: min(4096 / C, M / 2048 + 1, 256)
    _c("split-256", (1, 16, 522240)), _c("split-C5000", (1, 5000, 8)), _c("split-scalar-ragged", (2, 5, 4099)),
    # grid_x: min(ceil(L / 4096), 64) workgroups of 256 threads, 4 elements a thread where L % 4 == 0
    _c("grid-L4096", (2, 3, 4096)), _c("grid-L4100", (2, 3, 4100)), _c("grid-64-full", (1, 3, 262144)),
    _c("grid-64-one-group-over", (1, 3, 262148)), _c("grid-scalar-trips", (1, 2, 16387)),
    # blockIdx.y = (b, c) row: at most 65535;  M = 2
    _c("rows-65535", (1, 65535, 4)), _c("M2", (2, 3, 1)),
    # parameter kinds
    _c("d-neg-gamma", _KIND_DENSE, "neg-gamma"), _c("d-gamma0-beta+", _KIND_DENSE, "gamma0+"),
    _c("d-gamma0-beta-", _KIND_DENSE, "gamma0-"), _c("d-const-channel", _KIND_DENSE, "const"),
    _c("d-offset-channel", _KIND_DENSE, "offset"), _c("d-momentum-none", _KIND_DENSE, momentum=None),
    _c("d-no-running-stats", _KIND_DENSE, track=False), _c("d-expanded-upstream", _KIND_DENSE, "expanded"),
    # one NaN / one +Inf in channel 1; 64 channels of 16 elements: both the single launch and the three passes serve it
    _c("d-nan", (2, 64, 8), "nan"), _c("d-inf", (2, 64, 8), "inf"),
)
POOLED_CASES = tuple(
    _c(f"p{S}-{n}", shape + (S,), pooled=True)
    for S in (16, 32, 64, 128) for n, shape in (("one-row", (1, 1, 1)), ("odd-rows", (1, 3, 5)), ("blocks", (2, 8, 131)))
) + tuple(_c(f"p{S}-tie", (2, 4, 7, S), "tie", pooled=True) for S in (16, 32, 64, 128)) + tuple(
    _c("p-" + k, _KIND_POOLED, k, pooled=True)
    for k in ("neg-gamma", "gamma0+", "gamma0-", "const", "clamped", "offset", "expanded", "nan", "inf"))
# pooled backward at an S the forward does not serve: only spacap_bn_relu_max_bwd_f32 itself takes these
CABI_CASES = (_c("c7-L28", (2, 3, 4, 7), pooled=True), _c("c7-L35", (2, 3, 5, 7), pooled=True), _c("c20", (2, 3, 5, 20), pooled=True),
              _c("c256", (2, 3, 3, 256), "top-index", pooled=True))
ALL_CASES = DENSE_CASES + POOLED_CASES + CABI_CASES
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)
POISON_CHANNEL = 1            # of the nan / inf cases
TIE_SLOTS = ((0, 1, 2, 5, -3), (1, 1, 3, 8, 10))    # (b, c, p, first, second): two lanes of a row; one lane's own float4

Inputs = collections.namedtuple("Inputs", "z gamma beta up running_mean running_var rounds")
_SCALE, _SHIFT = (1.0, 0.02, 3.0, 0.5, 2.0), (0.25, -0.5, 0.5)


def conditions(z, gamma, beta, S=None):
    """(smallest |pre| / margin, smallest gap / margin between the two largest distinct positive values of a group, the Fwd):
    both at least 1 for conditioned inputs.  margin = MARGIN (|xhat gamma| + |beta|) of the element (for a gap: the larger of the
    two).  Channels whose statistics are not finite are left out (every output there is NaN)."""
    f = forward(z, gamma, beta, S=S)
    C = z.shape[1]
    bc = lambda a: a.reshape((1, C) + (1,) * (z.ndim - 2))
    with np.errstate(invalid="ignore"):
        margin = MARGIN * (np.abs(f.xhat * bc(gamma.astype(F64))) + bc(np.abs(beta.astype(F64))))
        finite = bc(np.isfinite(f.istd)) & np.ones(z.shape, bool)
        kink = np.where(finite, np.abs(f.pre) / margin, np.inf)
        gap = None
        if S:
            v = np.where(finite & (f.pre > 0.0), f.pre, -np.inf)
            top = v.max(-1, keepdims=True)
            second = np.where(v < top, v, -np.inf)
            i2 = second.argmax(-1)[..., None]
            v2, m2 = np.take_along_axis(second, i2, -1), np.take_along_axis(margin, i2, -1)
            m1 = np.take_along_axis(margin, v.argmax(-1)[..., None], -1)
            gap = np.where(np.isfinite(v2), (top - v2) / np.maximum(m1, m2), np.inf)[..., 0]
    return kink, gap, f


@functools.lru_cache(maxsize=None)
def inputs(case):
    """Seeded inputs of a case, nudged until no pre-activation sits within the margin of the ReLU's kink and no runner-up of a
    group within the margin of its maximum (tests/test_bn_relu_restated_cpu.py asserts both for every case)."""
    rng = np.random.default_rng(20261020 + ALL_CASES.index(case))
    shape, S, kind = case.shape, case.S, case.kind
    B, C = shape[:2]
    ch = np.arange(C)
    bc = lambda a: np.asarray(a).reshape((1, C) + (1,) * (len(shape) - 2))
    scale, shift = np.asarray(_SCALE)[ch % 5], np.asarray(_SCALE)[ch % 5] * np.asarray(_SHIFT)[ch % 3]
    z = (rng.standard_normal(shape) * bc(scale) + bc(shift)).astype(F32)
    gamma = rng.uniform(0.5, 1.5, C).astype(F32)
    gamma[0] = -0.7                                  # a negative scale reverses the order inside a group
    beta = rng.normal(0.0, 0.3, C).astype(F32)
    beta[np.abs(beta) < 0.01] = 0.05
    if kind == "neg-gamma":
        gamma = -gamma
        gamma[0] = -0.7
    if kind in ("gamma0+", "gamma0-"):               # every sample of the channel is relu(beta): all tied
        gamma[1], beta[1] = 0.0, (0.4 if kind == "gamma0+" else -0.4)
    if kind == "const":
        z[:, 1] = 0.75
        beta[1] = 0.3
    if kind == "offset":
        z[:, 1] = (1000.0 + rng.standard_normal(z[:, 1].shape)).astype(F32)
    if kind == "clamped":                            # gamma[2] > 0: far below the channel's mean is far below zero
        z[0, 2, 0, :] = (-40.0 - rng.uniform(0.0, 1.0, S)).astype(F32)
        z[1, 3, 6, :] = (-40.0 - rng.uniform(0.0, 1.0, S)).astype(F32)
    if kind == "tie":                                # two equal samples above the rest of their group (gamma[1] > 0)
        for b, c, p, i, j in TIE_SLOTS:
            z[b, c, p, i] = z[b, c, p, j] = F32(z[b, c, p].max() + F32(1.0))
    if kind == "top-index":                          # the maximum at sample 255: the top of the uint8 arg-max
        z[0, 1, 0, S - 1] = F32(z[0, 1, 0].max() + F32(1.0))
    for r in range(32):
        kink, gap, f = conditions(z, gamma, beta, S)
        bad = kink < 1.0
        if S:
            v = np.where(f.pre > 0.0, f.pre, -np.inf)
            second = np.where(v < v.max(-1, keepdims=True), v, -np.inf)
            bad |= (gap < 1.0)[..., None] & (second == second.max(-1, keepdims=True)) & np.isfinite(second)
        if not bad.any():
            break
        # away from the kink (an element at the kink) or down, away from the maximum (a runner-up): 8 margins of pre, in z
        g64, b64 = bc(gamma.astype(F64)), bc(np.abs(beta.astype(F64)))
        with np.errstate(divide="ignore", invalid="ignore"):
            step = 8.0 * MARGIN * (np.abs(f.xhat * g64) + b64) / (np.abs(g64) * bc(f.istd))
            direction = np.where(kink < 1.0, np.where(f.pre >= 0.0, 1.0, -1.0), -1.0) * np.sign(g64)
            z = np.where(bad, (z.astype(F64) + direction * step).astype(F32), z)
    else:
        raise ValueError(f"{case.name}: the inputs did not settle")
    if kind == "nan":
        z[0, POISON_CHANNEL].flat[3] = np.nan
    if kind == "inf":
        z[0, POISON_CHANNEL].flat[3] = np.inf
    up = rng.standard_normal(shape[:3] if S else shape).astype(F32)
    if kind == "expanded":
        up = np.ones_like(up)                        # y.sum().backward(): an upstream gradient of ones that arrives expanded
    out = Inputs(z, gamma, beta, up, rng.normal(0.0, 1.0, C).astype(F32), rng.uniform(0.5, 2.0, C).astype(F32), r)
    for a in out[:-1]:
        a.setflags(write=False)                      # shared between the tests: nobody changes it
    return out


Ref = collections.namedtuple("Ref", "fwd bwd running_mean running_var")


def run(case, dtype=F64, mutant=""):
    x = inputs(case)
    f = forward(x.z, x.gamma, x.beta, S=case.S, dtype=dtype, mutant=mutant)
    b = backward(x.z, x.gamma, x.beta, f, x.up, S=case.S, dtype=dtype, mutant=mutant)
    rm, rv = running_update(x.running_mean, x.running_var, f, case.momentum or 0.0, dtype=dtype, mutant=mutant)
    return Ref(f, b, rm, rv)


@functools.lru_cache(maxsize=None)
def reference(case):
    return run(case)


def unpoisoned(case):
    """the case's z with the planted NaN / +Inf taken out again (what the conditioning saw)"""
    z = inputs(case).z
    if case.kind in ("nan", "inf"):
        z = z.copy()
        z[0, POISON_CHANNEL].flat[3] = 0.0
    return z


@functools.lru_cache(maxsize=None)
def eval_buffers(case):
    """(running_mean, running_var) for the eval form: the batch's own statistics in float32, so that the eval pre-activations
    are the conditioned ones to within float32's rounding of the buffers"""
    x = inputs(case)
    f = forward(unpoisoned(case), x.gamma, x.beta)
    return f.mean.astype(F32), f.var.astype(F32)


def figures(got, want, case):
    """{quantity: figure} of one run against another (Ref against Ref)"""
    out = {"y": figure(got.fwd.y, want.fwd.y), "dz": figure(got.bwd.dz, want.bwd.dz), "dgamma": figure(got.bwd.dgamma, want.bwd.dgamma),
           "dbeta": figure(got.bwd.dbeta, want.bwd.dbeta), "running_mean": figure(got.running_mean, want.running_mean),
           "running_var": figure(got.running_var, want.running_var), "stats_mean": figure(got.fwd.mean.astype(F32), want.fwd.mean),
           "stats_istd": figure(got.fwd.istd, want.fwd.istd)}
    if case.S:
        out["pooled"] = figure(got.fwd.pooled, want.fwd.pooled)
    return out


# ---- group_max cases -------------------------------------------------------------------------------------------------------
GmCase = collections.namedtuple("GmCase", "name shape offset")
GM_CASES = (
    GmCase("S1", (2, 3, 5, 1), 0), GmCase("S7-one-row", (1, 1, 1, 7), 0),
    GmCase("S16-odd-rows", (1, 3, 5, 16), 0), GmCase("S32-odd-rows", (1, 3, 5, 32), 0), GmCase("S64-odd-rows", (1, 3, 5, 64), 0),
    GmCase("S128-one-row", (1, 1, 1, 128), 0), GmCase("S128-odd-rows", (1, 3, 5, 128), 0), GmCase("S128-blocks", (2, 8, 131, 128), 0),
    GmCase("S256", (2, 3, 5, 256), 0),
    GmCase("S64-offset-one-float", (2, 3, 5, 64), 1), GmCase("S128-offset-one-float", (2, 3, 5, 128), 1),
)
GmInputs = collections.namedtuple("GmInputs", "x go")


@functools.lru_cache(maxsize=None)
def gm_inputs(case):
    """random rows with a run of exact ties at the top of every third row, one NaN, and (S = 256) a maximum at sample 255"""
    rng = np.random.default_rng(77 + GM_CASES.index(case))
    B, C, P, S = case.shape
    x = rng.standard_normal(case.shape).astype(F32)
    rows = x.reshape(-1, S)
    if S >= 7:
        rows[::3, 2:7] = rows[::3].max(1, keepdims=True) + F32(1.0)
    if S == 256:
        rows[1, 255] = F32(9.0)
    if rows.shape[0] > 1 and S > 1:
        rows[-1, S // 2] = np.nan
    x = rows.reshape(case.shape)
    go = rng.standard_normal(case.shape[:3]).astype(F32)
    x.setflags(write=False), go.setflags(write=False)
    return GmInputs(x, go)
