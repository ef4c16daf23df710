"""The loss kernels of csrc/losses.hip restated in numpy on the host: detection (vote, objectness, box and class losses),
relation loss and caption head, with the case tables that reach every dispatch edge of the kernels, the seeded input builders,
the bars and the figures.  Not a test module; tests/test_losses_restated_cpu.py anchors the restatement to
spacap3d_amd/loss_helper.py and states the conditions the device test depends on, tests/test_losses_edges_gpu.py runs the
tables through the kernels.

Two precisions, on purpose:
  * every DISCRETE decision is taken in float32 in the kernel's expression order, so that it is pinned bit for bit: squared
    distances as (dx*dx + dy*dy) + dz*dz with every operation rounded to float32, the first minimum (np.argmin),
    eu = sqrt(float32(d + float32(1e-6))), label = eu < near, mask = label | (eu > far) with float32 thresholds; the vote of a
    seed is the first minimum of (|a| + |b|) + |c| with vote_label + seed_xyz formed in float32 first; arg-max = first maximum;
  * every VALUE and GRADIENT is float64 arithmetic on the float32 inputs and those decisions (lib/loss_helper.py:35-289 as
    spacap3d_amd/loss_helper.py:60-160 restates it): denominators + 1e-6, Huber with delta 1, size residual averaged over 3,
    gradients written out by hand (softmax minus one-hot, the Huber clamp, 2 (c - g) both ways, the L1 sign).

The arithmetic uses numpy only; torch appears in no formula here."""
import collections
import functools
import math

import numpy as np

from spacap3d_amd import loss_helper as LH   # the thresholds and the objectness weights only (plain Python constants)

F32, F64 = np.float32, np.float64
NEAR, FAR, OBJ_W = LH.NEAR_THRESHOLD, LH.FAR_THRESHOLD, tuple(LH.OBJECTNESS_CLS_WEIGHTS)

# ---- the bars: the project's own (tests/test_engine_gpu.py, tests/test_fused_small_gpu.py), here against float64 -----------
DET_LOSS_RTOL, DET_LOSS_ATOL = 2e-5, 1e-6
DET_GRAD_BAR = 2e-5                      # max |error| / max |reference| for each of d net, d center, d vote_xyz
REL_LOSS_RTOL, REL_LOSS_ATOL = 1e-5, 1e-7
REL_GRAD_RTOL, REL_GRAD_ATOL = 1e-4, 1e-9
CAP_LOGP_ABS = 2e-5                      # max |log-probability error|
CAP_LOSS_REL = 1e-5                      # |error| <= CAP_LOSS_REL * max(1, |reference|)
CAP_ACC_ABS = 1e-6
CAP_GRAD_REL, CAP_GRAD_ABS = 2e-6, 1e-9  # max |error| <= CAP_GRAD_REL * max(max |reference|, 1e-6) + CAP_GRAD_ABS
F64_BAR = 1e-10                          # two float64 computations of one formula, relative to the largest reference entry

DET_UPSTREAM = (1.0, 0.5, 1.3, 0.1, 0.7, 0.2, 0.9, 0.3)   # eight distinct upstream gradients of the eight losses
REL_UPSTREAM = (0.3, 1.0, 2.0)
CAP_UPSTREAM = 1.7


def figure(got, want):
    """max |got - want| / max |want|; a reference that is identically zero must be reproduced exactly."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    if want.size == 0:
        return 0.0
    err, ref = float(np.abs(got - want).max()), float(np.abs(want).max())
    if ref == 0.0:
        return 0.0 if err == 0.0 else math.inf
    return err / ref


def excess(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): at most 1 inside the bar of allclose(rtol, atol)."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


def zero_where_reference_is(got, want):
    """True when every element whose reference is exactly 0.0 came out exactly zero (either sign)."""
    return bool((np.asarray(got)[np.asarray(want) == 0.0] == 0.0).all())


# ---- float32 decisions -----------------------------------------------------------------------------------------------------
def sqdist32(a, b):
    """(dx*dx + dy*dy) + dz*dz over the last axis of float32 a - b, every operation rounded to float32 (numpy adds and multiplies
    float32 arrays in float32 and never contracts them)."""
    assert a.dtype == F32 and b.dtype == F32
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def euclid32(d):
    return np.sqrt(d + F32(1e-6))


def threshold_hits(eu, near, far, tol):
    """How many proposals have eu within tol of a threshold (the comparison there could flip with one ulp of the square root)."""
    eu = np.asarray(eu, F64)
    return int(((np.abs(eu - F64(F32(near))) <= tol) | (np.abs(eu - F64(F32(far))) <= tol)).sum())


def tied(d, axis):
    """Where the minimum of d along axis is taken more than once."""
    return (d == d.min(axis, keepdims=True)).sum(axis) > 1


def exact_offset(threshold):
    """An x > 0 with sqrt(float32(x*x + 1e-6f)) == float32(threshold) bit for bit: the proposal (x, 0, 0) beside a box at the
    origin sits exactly ON the threshold.  Found by walking float32 neighbours of sqrt(threshold^2 - 1e-6)."""
    thr = F32(threshold)
    x0 = F32(math.sqrt(float(thr) ** 2 - 1e-6))
    for direction in (F32(np.inf), F32(-np.inf)):
        x = x0
        for _ in range(256):
            if euclid32(x * x) == thr:
                return x
            x = np.nextafter(x, direction)
    raise ValueError(f"no float32 offset lands on {threshold}")


# ---- float64 values ----------------------------------------------------------------------------------------------------------
def _ce(s, label):
    """s (..., C) float64, label (...) -> cross entropy (...), softmax - onehot (..., C)"""
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    z = e.sum(-1, keepdims=True)
    idx = label[..., None].astype(np.int64)
    loss = (m + np.log(z))[..., 0] - np.take_along_axis(s, idx, -1)[..., 0]
    g = e / z
    np.put_along_axis(g, idx, np.take_along_axis(g, idx, -1) - 1.0, -1)
    return loss, g


def _den(n):
    """n + 1e-6 as every denominator is formed: in float32, because n is a sum of float32 0/1 flags in the composition (whatever
    the type of the scores) and in the kernels alike -- n itself from 16 up, 1e-6 for an empty sum."""
    return F64(F32(n) + F32(1e-6))


def _huber(err):
    a = np.abs(err)
    q = np.minimum(a, 1.0)
    return 0.5 * q * q + (a - q), np.clip(err, -1.0, 1.0)


DetRef = collections.namedtuple("DetRef", "losses obj_label obj_mask assignment dnet dcenter dvote eu d_agg d_center ic i2 pick")


def detection(x, gout=DET_UPSTREAM):
    """Everything spacap_det_losses_fwd_f32 / _bwd_f32 return for the inputs x (a DetInputs): the eight losses, the three integer
    outputs and the gradients of sum_i gout_i loss_i with respect to net (B,K,CH), center and vote_xyz; plus the float32
    quantities the decisions were taken on (eu, the two distance matrices, the nearest indices, the vote picked per seed)."""
    B, K, CH = x.net.shape
    M, NH, NS = x.gt_center.shape[1], x.NH, x.NS
    G = np.asarray(gout, F64)
    bi, ak = np.arange(B)[:, None], np.arange(K)[None, :]
    # decisions (float32)
    d_agg = sqdist32(x.agg_xyz[:, :, None, :], x.gt_center[:, None, :, :])      # (B,K,M)
    oa = d_agg.argmin(2)
    eu = euclid32(d_agg.min(2))
    label = eu < F32(x.near)
    mask = label | (eu > F32(x.far))
    d_cen = sqdist32(x.center[:, :, None, :], x.gt_center[:, None, :, :])
    ic, i2 = d_cen.argmin(2), d_cen.argmin(1)                                  # (B,K) nearest box, (B,M) nearest proposal
    vl = x.vote_label[bi, x.seed_inds].reshape(B, -1, 3, 3)                     # (B,NSEED,3 votes,3)
    t32 = vl + x.seed_xyz[:, :, None, :]
    a32 = np.abs(x.vote_xyz[:, :, None, :] - t32)
    pick = ((a32[..., 0] + a32[..., 1]) + a32[..., 2]).argmin(-1)              # (B,NSEED)
    assert t32.dtype == F32 and a32.dtype == F32 and eu.dtype == F32
    # values (float64)
    net, cen, gt = x.net.astype(F64), x.center.astype(F64), x.gt_center.astype(F64)
    obj, msk, bm = label.astype(F64), mask.astype(F64), x.box_mask.astype(F64)
    n_obj, d_mask, d_box = _den(obj.sum()), _den(msk.sum()), _den(bm.sum())
    losses, dnet = np.zeros(8), np.zeros((B, K, CH))
    o_hs, o_hr, o_ss = 5, 5 + NH, 5 + 2 * NH
    o_sr, o_sem = o_ss + NS, o_ss + 4 * NS
    # vote
    m = x.vote_mask[bi, x.seed_inds].astype(F64)
    e = x.vote_xyz.astype(F64) - (np.take_along_axis(vl.astype(F64), pick[..., None, None].repeat(3, -1), 2)[:, :, 0]
                                  + x.seed_xyz.astype(F64))
    d_vote = _den(m.sum())
    losses[0] = (np.abs(e).sum(-1) * m).sum() / d_vote
    dvote = G[0] / d_vote * m[..., None] * np.sign(e)
    # objectness: weighted two-class cross entropy over the masked proposals
    w = np.asarray([F32(x.w0), F32(x.w1)], F64)[label.astype(np.int64)]
    ce, g = _ce(net[..., 0:2], label)
    losses[1] = (w * ce * msk).sum() / d_mask
    dnet[..., 0:2] = G[1] / d_mask * (w * msk)[..., None] * g
    # centre: proposal -> nearest box over the positives, box -> nearest proposal over the valid boxes
    diff1, diff2 = cen - gt[bi, ic], cen[bi, i2] - gt                           # (B,K,3), (B,M,3)
    losses[2] = ((diff1 ** 2).sum(-1) * obj).sum() / n_obj + ((diff2 ** 2).sum(-1) * bm).sum() / d_box
    dcenter = G[2] * 2.0 * diff1 * obj[..., None] / n_obj
    np.add.at(dcenter, (np.broadcast_to(bi, i2.shape), i2), G[2] * 2.0 * diff2 * bm[..., None] / d_box)
    # heading class and residual of the assigned box
    hl = x.heading_cls_label[bi, oa]
    ce, g = _ce(net[..., o_hs:o_hr], hl)
    losses[3] = (ce * obj).sum() / n_obj
    dnet[..., o_hs:o_hr] = G[3] / n_obj * obj[..., None] * g
    err = np.take_along_axis(net[..., o_hr:o_ss], hl[..., None], -1)[..., 0] - x.heading_res_label.astype(F64)[bi, oa] / (math.pi / NH)
    hv, hg = _huber(err)
    losses[4] = (hv * obj).sum() / n_obj
    np.put_along_axis(dnet[..., o_hr:o_ss], hl[..., None], (G[4] / n_obj * obj * hg)[..., None], -1)
    # size class and residual
    sl = x.size_cls_label[bi, oa]
    ce, g = _ce(net[..., o_ss:o_sr], sl)
    losses[5] = (ce * obj).sum() / n_obj
    dnet[..., o_ss:o_sr] = G[5] / n_obj * obj[..., None] * g
    res = net[..., o_sr:o_sem].reshape(B, K, NS, 3)[bi, ak, sl]                 # (B,K,3)
    err = res - x.size_res_label.astype(F64)[bi, oa] / x.mean_size.astype(F64)[sl]
    sv, sg = _huber(err)
    losses[6] = (sv.mean(-1) * obj).sum() / n_obj
    gsr = np.zeros((B, K, NS, 3))
    gsr[bi, ak, sl] = G[6] / n_obj * obj[..., None] * sg / 3.0
    dnet[..., o_sr:o_sem] = gsr.reshape(B, K, 3 * NS)
    # semantic class
    ce, g = _ce(net[..., o_sem:], x.sem_cls_label[bi, oa])
    losses[7] = (ce * obj).sum() / n_obj
    dnet[..., o_sem:] = G[7] / n_obj * obj[..., None] * g
    return DetRef(losses, label.astype(np.int64), mask.astype(F32), oa.astype(np.int64), dnet, dcenter, dvote, eu, d_agg, d_cen,
                  ic, i2, pick)


RelRef = collections.namedtuple("RelRef", "out dpred n_pairs")


def relation(x, gout=REL_UPSTREAM):
    """out (7,) = (x, y, z loss, x, y, z accuracy, 1 / max(#pairs, 1)) and d(sum_a gout_a loss_a) / d pred."""
    B, K = x.assignment.shape
    bi = np.arange(B)[:, None]
    sel = (x.box_mask_int[bi, x.assignment] & x.obj_label) != 0
    W = (sel[:, :, None] & sel[:, None, :]).astype(F64)
    n = max(W.sum(), 1.0)
    out, dpred = np.zeros(7), np.zeros(x.pred.shape)
    for a, lab_all in enumerate((x.x_label, x.y_label, x.z_label)):
        lab = lab_all[bi[..., None], x.assignment[:, :, None], x.assignment[:, None, :]]   # (B,K,K)
        s = x.pred[..., 3 * a:3 * a + 3]
        ce, g = _ce(s.astype(F64), lab)
        out[a] = (ce * W).sum() / n
        out[3 + a] = ((s.argmax(-1) == lab) * W).sum() / n                                # float32 comparison, first maximum
        dpred[..., 3 * a:3 * a + 3] = gout[a] / n * W[..., None] * g
    out[6] = 1.0 / n
    return RelRef(out, dpred, int(W.sum()))


CapRef = collections.namedtuple("CapRef", "logp loss acc dlogits target n_valid")


def caption(x, gout=CAP_UPSTREAM):
    """log-probabilities (B,W,V), cap_loss, cap_acc and d(gout cap_loss) / d logits; a target id outside [0, V) is ignored
    like the pad id 0."""
    B, W, V = x.logits.shape
    t = x.lang_ids[:, 1:W + 1].copy()
    t[(t < 0) | (t >= V)] = 0
    s = x.logits.astype(F64)
    m = s.max(-1, keepdims=True)
    lse = m + np.log(np.exp(s - m).sum(-1, keepdims=True))
    logp = s - lse
    gd = np.broadcast_to(x.good.astype(F64)[:, None], (B, W))
    valid = gd * (t != 0)
    den = _den(gd.sum())
    loss = (-np.take_along_axis(logp, t[..., None], -1)[..., 0] * valid).sum() / den
    acc = ((x.logits.argmax(-1) == t) * valid).sum() / max(valid.sum(), 1.0)
    g = np.exp(logp)
    np.put_along_axis(g, t[..., None], np.take_along_axis(g, t[..., None], -1) - 1.0, -1)
    return CapRef(logp, loss, acc, gout * (valid / den)[..., None] * g, t, int(valid.sum()))


# ---- detection cases -------------------------------------------------------------------------------------------------------
DetCase = collections.namedtuple("DetCase", "name B K M NH NS NC NSEED N kind positives")
_BASE = dict(B=2, K=256, M=128, NH=1, NS=18, NC=18, NSEED=256, N=1000, kind="", positives="some")


def _det(name, **kw):
    return DetCase(name=name, **{**_BASE, **kw})


def lds_bytes(K, M, NS):
    """dynamic LDS of det_proposal_kernel without the staged head output (spacap_det_losses_fwd_f32)"""
    return 4 * (12 * M + 6 * K + 3 * NS + 4)


def staged(K, M, NH, NS, NC):
    """whether the host code stages the K x CH head outputs of a scene in LDS (det_proposal_kernel<true>)"""
    return lds_bytes(K, M, NS) + 4 * K * (5 + 2 * NH + 4 * NS + NC) <= 150 * 1024


def last_staged_k(M=128, NH=1, NS=18, NC=18):
    k = 1
    while staged(k + 1, M, NH, NS, NC):
        k += 1
    return k


K_EDGE = last_staged_k()      # 357 at M = 128, CH = 97: tests/test_losses_restated_cpu.py holds it to the inequality

DET_CASES = (
    _det("K256"),
    _det("K1", K=1), _det("K3", K=3), _det("K7", K=7),
    _det("K41", K=41),
    _det("K257", K=257),
    _det("K-last-staged", K=K_EDGE), _det("K-first-unstaged", K=K_EDGE + 1),
    _det("K512", K=512),
    _det("K41-NC1000", K=41, NC=1000),
    _det("M1", M=1), _det("M3", M=3), _det("M129", M=129), _det("M256", M=256),
    _det("NH12", NH=12), _det("NS1", NS=1),
    _det("B1", B=1), _det("B12-K512", B=12, K=512),
    _det("scene0-no-valid-box", kind="scene0-no-valid-box"),
    _det("none-near", kind="none-near", positives="none"),
    _det("all-grey", kind="all-grey", positives="all-masked"),
    _det("dup-boxes", kind="dup-boxes"),
    _det("dup-proposals", kind="dup-proposals"),
    _det("exact-thresholds", kind="exact-thresholds"),
    _det("NSEED1", NSEED=1), _det("NSEED255", NSEED=255), _det("NSEED257", NSEED=257), _det("NSEED1024", NSEED=1024),
    _det("same-votes", kind="same-votes"),      # (which of three equal votes wins shows in no output: the sums must still be right)
    _det("scene1-no-vote-mask", kind="scene1-no-vote-mask"),
)
DET_BY_NAME = {c.name: c for c in DET_CASES}
DET_SEED = {}     # case name -> seed, for a row whose inputs miss a condition of tests/test_losses_restated_cpu.py

DetInputs = collections.namedtuple(
    "DetInputs", "net center vote_xyz agg_xyz gt_center box_mask heading_cls_label heading_res_label size_cls_label "
                 "size_res_label sem_cls_label mean_size seed_xyz seed_inds vote_label vote_mask NH NS near far w0 w1")

_N_VALID = (12, 20, 5, 9, 16, 3, 11, 7, 14, 2, 18, 6)


def n_valid(case, b):
    """valid boxes of scene b: the first n rows; above 128 boxes nearly all of them, so that the second pass has real ones"""
    if case.kind == "scene0-no-valid-box" and b == 0:
        return 0
    if case.M > 128:
        return case.M - 59 * (b % 2)
    return min(_N_VALID[b % len(_N_VALID)], case.M if b % 2 == 0 else max(case.M - 1, 1))


def _unit(rng, shape):
    v = rng.normal(size=shape + (3,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


_RADII = ((0.02, 0.27), (0.33, 0.57), (0.63, 1.5))    # near, grey, far: clear of both thresholds by construction


def _eu_of(agg, gt):
    return euclid32(sqdist32(agg[:, None, :], gt[None, :, :]).min(1))


@functools.lru_cache(maxsize=None)
def mean_sizes(NS):
    """the package's own array at NS = 18, else random in [0.3, 2]; cached: loss_helper keys its copy on the array's identity"""
    if NS == 18:
        from spacap3d_amd.synthetic import mean_size_arr
        return np.ascontiguousarray(mean_size_arr().numpy(), F32)
    return np.random.default_rng(NS).uniform(0.3, 2.0, (NS, 3)).astype(F32)


@functools.lru_cache(maxsize=None)
def detection_inputs(case):
    B, K, M, NH, NS, NC, NSEED, N = case.B, case.K, case.M, case.NH, case.NS, case.NC, case.NSEED, case.N
    CH = 5 + 2 * NH + 4 * NS + NC
    rng = np.random.default_rng(DET_SEED.get(case.name, 20261020 + DET_CASES.index(case)))
    nv = [n_valid(case, b) for b in range(B)]
    valid = (np.arange(M)[None, :] < np.asarray(nv)[:, None])
    gt = (rng.uniform(-2.0, 2.0, (B, M, 3)) * valid[..., None]).astype(F32)       # a 4 m cube; padded rows are all zero
    if case.kind == "exact-thresholds":      # a valid box at the origin, every other box of the scene at least 1.3 m from it
        gt[0, 0] = 0.0
        r = np.linalg.norm(gt[0, 1:nv[0]], axis=-1, keepdims=True)
        gt[0, 1:nv[0]] *= np.maximum(1.0, 1.3 / r).astype(F32)
    if case.kind == "dup-boxes":
        gt[:, 5] = gt[:, 2]
    hcl = rng.integers(0, NH, (B, M)) * valid
    scl = rng.integers(0, NS, (B, M)) * valid
    sem = rng.integers(0, NC, (B, M)) * valid
    hrl = (rng.uniform(-1.0, 1.0, (B, M)) * math.pi / (2 * NH) * valid).astype(F32)
    srl = (rng.normal(0.0, 0.3, (B, M, 3)) * valid[..., None]).astype(F32)
    if case.kind == "dup-boxes":             # the same centre under two different sets of labels
        scl[:, 5], sem[:, 5] = (scl[:, 2] + 1) % NS, (sem[:, 2] + 1) % NC
    # proposals: a box of the scene (the origin, where the padded rows sit, in a scene without one) plus noise of three scales
    target = np.stack([rng.integers(0, max(n, 1), K) for n in nv])
    cls = (np.arange(K)[None, :] + 2 * np.arange(B)[:, None]) % 3       # (K = 1: one near, one far)
    if case.kind == "none-near":
        cls = 1 + cls % 2
    if case.kind == "all-grey":
        cls = np.ones_like(cls)
    lo, hi = np.asarray(_RADII)[cls, 0], np.asarray(_RADII)[cls, 1]
    base = gt[np.arange(B)[:, None], target].astype(F64)
    agg = (base + _unit(rng, (B, K)) * rng.uniform(lo, hi)[..., None]).astype(F32)
    cen = (base + _unit(rng, (B, K)) * rng.uniform(0.05, 0.6, (B, K))[..., None]).astype(F32)
    if case.kind == "dup-boxes":             # eight proposals of every scene sit next to the doubled box
        k8 = min(8, K)
        agg[:, :k8] = (gt[:, 2:3].astype(F64) + _unit(rng, (B, k8)) * rng.uniform(0.02, 0.25, (B, k8, 1))).astype(F32)
        cen[:, :k8] = (gt[:, 2:3].astype(F64) + _unit(rng, (B, k8)) * rng.uniform(0.05, 0.25, (B, k8, 1))).astype(F32)
    if case.kind == "dup-proposals":         # proposals 4 and 9 share one centre, a centimetre from box 1: its nearest, twice
        cen[:, 4] = cen[:, 9] = gt[:, 1] + np.asarray([0.01, 0.0, 0.0], F32)
    if case.kind == "exact-thresholds":
        agg[0, 0] = (exact_offset(NEAR), 0.0, 0.0)
        agg[0, 1] = (exact_offset(FAR), 0.0, 0.0)
    if case.kind == "none-near":             # whoever came near another box (or the padded rows) leaves the cube
        for b in range(B):
            bad = _eu_of(agg[b], gt[b]) < F32(NEAR) + F32(0.02)
            agg[b, bad] = (3.0 + rng.uniform(0.0, 0.5, (int(bad.sum()), 3))).astype(F32)
    if case.kind == "all-grey":              # drawn again around another box until every one sits between the thresholds
        for b in range(B):
            for _ in range(200):
                eu = _eu_of(agg[b], gt[b])
                bad = (eu < F32(NEAR) + F32(0.02)) | (eu > F32(FAR) - F32(0.02))
                if not bad.any():
                    break
                nb = int(bad.sum())
                again = gt[b, rng.integers(0, max(nv[b], 1), nb)].astype(F64)
                agg[b, bad] = (again + _unit(rng, (nb,)) * rng.uniform(*_RADII[1], (nb, 1))).astype(F32)
            else:
                raise ValueError("all-grey: no placement found")
    net = rng.normal(0.0, 1.0, (B, K, CH)).astype(F32)
    seed_xyz = rng.uniform(-2.0, 2.0, (B, NSEED, 3)).astype(F32)
    seed_inds = rng.integers(0, N, (B, NSEED))
    vote_label = rng.normal(0.0, 0.5, (B, N, 9)).astype(F32)
    vote_mask = rng.integers(0, 2, (B, N))
    vote_mask[0, seed_inds[0, 0]] = 1
    if case.kind == "same-votes":            # the usual content of vote_label: one vote, three times
        vote_label[..., 3:6] = vote_label[..., 6:9] = vote_label[..., 0:3]
    if case.kind == "scene1-no-vote-mask":
        vote_mask[1] = 0
    which = rng.integers(0, 3, (B, NSEED))
    bi = np.arange(B)[:, None]
    chosen = np.take_along_axis(vote_label[bi, seed_inds].reshape(B, NSEED, 3, 3), which[..., None, None].repeat(3, -1), 2)[:, :, 0]
    vote_xyz = (seed_xyz + chosen + rng.normal(0.0, 0.1, (B, NSEED, 3))).astype(F32)
    out = DetInputs(net, cen, vote_xyz, agg, gt, valid.astype(F32), hcl.astype(np.int64), hrl, scl.astype(np.int64), srl,
                    sem.astype(np.int64), mean_sizes(NS), seed_xyz, seed_inds.astype(np.int64), vote_label,
                    vote_mask.astype(np.int64), NH, NS, NEAR, FAR, OBJ_W[0], OBJ_W[1])
    for a in out:
        if isinstance(a, np.ndarray) and a is not out.mean_size:
            a.setflags(write=False)      # shared between the tests: nobody changes it
    return out


@functools.lru_cache(maxsize=None)
def detection_reference(case):
    return detection(detection_inputs(case))


# ---- relation cases --------------------------------------------------------------------------------------------------------
RelCase = collections.namedtuple("RelCase", "name B K M select")
REL_CASES = (
    RelCase("1-5-7", 1, 5, 7, "some"),             # 25 pairs: one partial workgroup
    RelCase("3-17-20", 3, 17, 20, "some"),         # 289 pairs: the second workgroup of a scene holds 33
    RelCase("2-40-128", 2, 40, 128, "some"),
    RelCase("2-256-64", 2, 256, 64, "some"),       # 1 179 648 elements: above the 4 096 x 256 threads of rel_scale_kernel
    RelCase("3-17-20-all", 3, 17, 20, "all"),
    RelCase("3-17-20-none", 3, 17, 20, "none"),
)
RelInputs = collections.namedtuple("RelInputs", "pred assignment box_mask_int obj_label x_label y_label z_label")
# planted on four selected pairs of every scene, per axis: a three-way tie, then two-way ties in each position (first maximum
# 0, 0, 1, 0); the labels of those pairs name the first maximum, so another choice costs a hit
_REL_TIES = (((1.5, 1.5, 1.5), 0), ((2.0, 2.0, -1.0), 0), ((-1.0, 2.0, 2.0), 1), ((2.0, -1.0, 2.0), 0))


@functools.lru_cache(maxsize=None)
def relation_inputs(case):
    B, K, M = case.B, case.K, case.M
    rng = np.random.default_rng(4100 + REL_CASES.index(case))
    pred = (rng.normal(0.0, 2.0, (B, K, K, 9))).astype(F32)
    oa = rng.integers(0, M, (B, K))
    n_box = np.asarray([max(2, M // 2 + b) for b in range(B)])
    bmi = (np.arange(M)[None, :] < n_box[:, None]).astype(np.int64)
    ol = rng.integers(0, 2, (B, K))
    oa[:, 0], oa[:, 1] = 0, 1
    if case.select == "some":
        ol[:, 0:2], ol[:, -1] = 1, 0
    elif case.select == "all":
        ol[:], bmi[:] = 1, 1
    else:
        ol[:] = 0
    labels = [rng.integers(0, 3, (B, M, M)) for _ in range(3)]
    for b in range(B):
        for (vals, first), (i, j) in zip(_REL_TIES, ((0, 0), (0, 1), (1, 0), (1, 1))):
            for a in range(3):
                pred[b, i, j, 3 * a:3 * a + 3] = vals
                labels[a][b, oa[b, i], oa[b, j]] = first
    out = RelInputs(pred, oa.astype(np.int64), bmi, ol.astype(np.int64), *(l.astype(np.int64) for l in labels))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def relation_reference(case):
    return relation(relation_inputs(case))


# ---- caption cases ---------------------------------------------------------------------------------------------------------
CapCase = collections.namedtuple("CapCase", "B W V width good")
CAP_SHAPES = ((2, 5, 2, 6), (3, 7, 257, 9), (2, 31, 1000, 36))    # (B, W, V, columns of lang_ids): W + 1 is the least allowed
CAP_CASES = tuple(CapCase(*s, g) for s in CAP_SHAPES for g in ("all", "some", "none"))
CapInputs = collections.namedtuple("CapInputs", "logits lang_ids good")
CAP_FAR_ID = (1 << 40) + 7


def cap_ties(V):
    """(word row of scene 0, the two tied columns, the target column) planted for a vocabulary of V words.  The accuracy is
    the one place an arg-max shows, and it only counts hits: every target is the FIRST of its tied columns, so each row is a
    hit by the first-maximum rule and a miss by any other -- rows that pulled in both directions could cancel."""
    rows = []
    if V > 67:       # columns 3 and 3 + 64: two waves of the workgroup;  5 and 9: two lanes of one wave
        rows += [(1, (3, 67), 3), (2, (5, 9), 5)]
    if V > 266:      # columns 10 and 10 + 256: one thread, two trips of its loop;  700 and 956: the same, in the last wave
        rows += [(3, (10, 266), 10), (4, (700, 956), 700)]
    if V == 2:       # (the target cannot be the pad id 0: the one row that must miss)
        rows += [(1, (0, 1), 1)]
    return rows


@functools.lru_cache(maxsize=None)
def caption_inputs(case):
    B, W, V = case.B, case.W, case.V
    rng = np.random.default_rng(B * W + V)
    logits = (rng.normal(0.0, 3.0, (B, W, V))).astype(F32)
    ids = np.zeros((B, case.width), np.int64)
    ids[:, 0] = min(2, V - 1)
    for b in range(B):
        n = W if b == 0 else int(rng.integers(3, W + 1))
        ids[b, 1:1 + n] = rng.integers(1, V, n)                # word ids; 0 pads the rest
    top = lambda b, w: F32(logits[b, w].max() + F32(2.0))
    logits[0, 0, ids[0, 1]] = top(0, 0)                        # the maximum at the target: a hit
    for w, cols, t in cap_ties(V):
        logits[0, w, list(cols)] = top(0, w)                   # equal maxima: the first index is the arg-max
        ids[0, w + 1] = t
    ids[B - 1, 1], ids[B - 1, 2] = V, CAP_FAR_ID               # out of range: ignored like the pad id
    good = {"all": np.ones(B, bool), "some": np.arange(B) % 2 == 0, "none": np.zeros(B, bool)}[case.good]
    out = CapInputs(logits, ids, good)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def caption_reference(case):
    return caption(caption_inputs(case))
