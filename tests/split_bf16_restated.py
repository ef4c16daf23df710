"""The split-bf16 product of csrc/mfma.hpp, restated in numpy on the host, and the probe inputs that make
each of its three 2^-16 piece products visible.  Not a test module; tests/test_split_bf16_cpu.py checks that the probes
discriminate and tests/test_split_bf16_terms_gpu.py runs them through every kernel that owns a copy of the product loop.

x = x0 + x1 + x2 (three bf16 pieces, round to nearest even); a product is the six piece products of PA / PB, of which
a0 b2, a2 b0 and a1 b1 (q = 0, 1, 2) weigh 2^-16 of the leading one.  On randn operands a lost 2^-16 term is a zero-mean error
that averages out of a max-norm; ``probe`` chooses signs so that the probed term is POSITIVE in every summand and adds up
coherently, while the leading term keeps a random sign along the contraction (so the fp32 accumulation error stays at its
random level) and every mantissa stays independent (full rank: a lane or row mix-up in a low piece shows as well).

The bar of ``measures`` -- a quarter of the smallest share the probed term has in sum |a| |b| -- follows from the inputs alone."""
import numpy as np
import torch

PA = (0, 2, 1, 0, 1, 0)
PB = (2, 0, 1, 1, 0, 0)


def split3(x):
    """The three bf16 pieces of fp32 ``x`` as float64 arrays, by the arithmetic of mfma.hpp's split3."""
    v = torch.from_numpy(np.array(x, dtype=np.float32))
    h = v.bfloat16().float()
    r = v - h
    m = r.bfloat16().float()
    l = (r - m).bfloat16().float()
    return tuple(t.numpy().astype(np.float64) for t in (h, m, l))


def six_term_product(A, B, drop=None, chunk=32):
    """A [M,K] @ B [K,N] as the device computes it: per chunk of the contraction, the six piece products in PA / PB order, each
    exact (float64 holds a sum of 32 products of 8-bit mantissas), added into an fp32 accumulator.  ``drop=q`` leaves product
    q out.  This is what a correct kernel may err by; it never stands in for the float64 answer."""
    a, b = split3(A), split3(B)
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k0 in range(0, A.shape[1], chunk):
        for q in range(6):
            if q == drop:
                continue
            t = a[PA[q]][:, k0:k0 + chunk] @ b[PB[q]][k0:k0 + chunk]
            acc = (acc.astype(np.float64) + t).astype(np.float32)
    return acc


def _magnitudes(rng, shape, piece, want, floor=0.0):
    """|N(0,1)| + 0.05 fp32, single elements redrawn until piece ``piece`` has the sign ``want`` (broadcast against shape) and,
    with ``floor`` > 0, at least that fraction of the largest magnitude the piece can have next to x in [2^e, 2^(e+1)):
    2^(e-8) for piece 1 (half a bf16 ulp of x), 2^(e-17) for piece 2 (half a bf16 ulp of a piece 1 in its top binade)."""
    x = (np.abs(rng.standard_normal(shape)) + 0.05).astype(np.float32)
    want = np.broadcast_to(want, shape)
    while True:
        xp = split3(x)[piece]
        bad = np.sign(xp) != want
        if floor > 0 and piece > 0:
            bad |= np.abs(xp) < floor * np.ldexp(1.0, np.frexp(x)[1] - 1 - (8 if piece == 1 else 17))
        n = int(bad.sum())
        if n == 0:
            return x
        x[bad] = (np.abs(rng.standard_normal(n)) + 0.05).astype(np.float32)


def probe(q, M, K, N, seed, nonneg_a=False, floor=0.0):
    """(A [M,K], B [K,N]) fp32 for term q in {0, 1, 2} = (a0 b2, a2 b0, a1 b1): piece PA[q] of a_mk times piece PB[q] of b_kn is
    positive for every (m, k, n).  ``nonneg_a``: A >= 0 throughout (an operand behind a ReLU).  ``floor``: see _magnitudes."""
    assert q in (0, 1, 2)
    p, pp = PA[q], PB[q]
    rng = np.random.default_rng([seed, q, M, K, N])
    pm = lambda: rng.integers(0, 2, K) * 2.0 - 1.0
    # tau tau' is the sign of the leading term a0 b0: random along k, but BALANCED (as many + as -), or every element of A B
    # would share the offset E|a| E|b| sum_k tau tau' and a ReLU behind the product could hide most of them
    s = rng.permutation(np.where(np.arange(K) % 2 == 0, 1.0, -1.0))
    tau = np.ones(K) if p == 0 else (s if pp == 0 else pm())
    taup = np.ones(K) if pp == 0 else tau * s
    alpha = np.ones(K) if nonneg_a else pm()
    a = _magnitudes(rng, (M, K), p, tau[None, :], floor)
    b = _magnitudes(rng, (K, N), pp, taup[:, None], floor)
    A = (alpha[None, :] * a).astype(np.float32)
    B = ((alpha * tau * taup)[:, None] * b).astype(np.float32)
    return A, B


def measures(A, B, got, q):
    """All in float64: S = |A| |B|, err = |got - A B| / S elementwise, share = (A_p B_p') / S for the probed term, bar =
    share.min() / 4.  Returns a dict (plus ref = A B)."""
    A64, B64 = np.asarray(A, np.float64), np.asarray(B, np.float64)
    S = np.abs(A64) @ np.abs(B64)
    ref = A64 @ B64
    share = (split3(A)[PA[q]] @ split3(B)[PB[q]]) / S
    return {"S": S, "ref": ref, "err": np.abs(np.asarray(got, np.float64) - ref) / S, "share": share, "bar": float(share.min()) / 4}


def bias_probe(p, R, C, seed, floor=0.0):
    """G [R,C] fp32 for the column-sum loops (pieces 2, 1, 0 of g, each times ones): piece p in {1, 2} is positive in every
    element, the elements' own signs are random."""
    assert p in (1, 2)
    rng = np.random.default_rng([seed, p, R, C])
    sgn = rng.integers(0, 2, (R, C)) * 2.0 - 1.0
    return (sgn * _magnitudes(rng, (R, C), p, sgn, floor)).astype(np.float32)   # piece p of |g| has g's sign <=> piece p of g > 0


def bias_measures(G, got, p):
    """S = sum_r |g|, err = |got - sum_r g| / S, share = sum_r g_p / S, bar = share.min() / 4."""
    G64 = np.asarray(G, np.float64)
    S = np.abs(G64).sum(0)
    ref = G64.sum(0)
    share = split3(G)[p].sum(0) / S
    return {"S": S, "ref": ref, "err": np.abs(np.asarray(got, np.float64) - ref) / S, "share": share, "bar": float(share.min()) / 4}


def column_sum(G, drop=None, chunk=32):
    """The bias loop restated: pieces 2, 1, 0 of g times ones, chunk by chunk along the rows, into an fp32 accumulator."""
    g = split3(G)
    acc = np.zeros(G.shape[1], np.float32)
    for r0 in range(0, G.shape[0], chunk):
        for p in (2, 1, 0):
            if p != drop:
                acc = (acc.astype(np.float64) + g[p][r0:r0 + chunk].sum(0)).astype(np.float32)
    return acc


# ---- the probes the device tests run, by site (tests/test_split_bf16_terms_gpu.py); the CPU test checks every one of them ------
# name -> (M, K, N, nonneg_a, swapped).  ``swapped``: the kernel hands the product's RIGHT operand (a weight image held in
# registers) to PA and the left one to PB, so kernel term q is the probe's term SWAP[q] of (left, right).
# The device shapes have up to 150 000 output elements, against the 1 920 of the generic 48 x 40 probe: the largest fp32
# accumulation error among so many reaches a third of the bar (and numpy's own fp32 product the bar itself) for about every
# other seed.  Their probes therefore keep the probed pieces in the upper half of their range (floor = 1/2), which triples the
# probed term's share: the restated product then stays under 0.15 bar and an fp32 product under 0.45 bar for every seed tried.
SEED = 1
FLOOR = 0.5
SWAP = (1, 0, 2)
CASES = {
    "gemm_bf3/128x128": (131, 128, 128, False, False),
    "gemm_bf3/256x128": (131, 256, 128, False, False),
    "linear_wgrad/R129": (256, 129, 128, False, False),       # dW [CK, CP] = g^T x: left = g^T, contraction over the rows
    "linear_wgrad/R200": (256, 200, 128, False, False),
    "conv1x1_cm/128x97": (97, 128, 128, False, False),        # left = W [CO, CI], right = in [CI, B N]
    "conv1x1_cm/256x5": (5, 256, 128, False, False),
    "conv1x1_wgrad": (128, 192, 128, False, False),           # left = g [CO, B N], right = x^T [B N, CI]
    "sa/64x64": (77, 64, 64, True, False),
    "sa/64x128": (77, 64, 128, True, False),
    "sa/128x128": (77, 128, 128, True, False),
    "sa/128x256": (77, 128, 256, True, False),
    "sa_pool/64x128": (112, 64, 128, True, False),
    "sa_pool/128x128": (112, 128, 128, True, False),
    "sa_pool/128x256": (112, 128, 256, True, False),
    "sa_dgrad/128x64": (117, 128, 64, False, False),
    "sa_dgrad/128x128": (117, 128, 128, False, False),
    "sa_dgrad/256x128": (117, 256, 128, False, False),
    "tf_ffn/fwd/first": (583, 128, 256, False, True),
    "tf_ffn/fwd/second": (583, 128, 256, True, True),
    "tf_ffn/bwd/first": (583, 128, 256, False, True),
    "tf_ffn/bwd/second": (583, 128, 256, False, True),
    "decode": (37, 128, 40, False, False),
    "relation/hid2/K8": (8, 128, 128, True, True),
    "relation/hid2/K24": (24, 128, 128, True, True),
    "relation/dhid1": (9, 128, 128, False, True),             # left = the rows of W3 (dz2 = 2^e W3[o]), right = W2
}
BIAS_CASES = {"linear_wgrad/R129": (129, 256), "linear_wgrad/R200": (200, 256), "conv1x1_wgrad": (192, 128)}
_cache = {}


def case(name, q):
    """(A, B, qp) of case ``name`` for KERNEL term q: qp is the term of (A, B) to hand to ``measures``.  Cached; do not write."""
    if (name, q) not in _cache:
        M, K, N, nonneg, swapped = CASES[name]
        qp = SWAP[q] if swapped else q
        A, B = probe(qp, M, K, N, SEED + sorted(CASES).index(name), nonneg, FLOOR)
        A.setflags(write=False), B.setflags(write=False)
        _cache[name, q] = (A, B, qp)
    return _cache[name, q]


def bias_case(name, p):
    if (name, "bias", p) not in _cache:
        G = bias_probe(p, *BIAS_CASES[name], SEED + sorted(BIAS_CASES).index(name), FLOOR)
        G.setflags(write=False)
        _cache[name, "bias", p] = G
    return _cache[name, "bias", p]


def relu_measures(A, B, got, q):
    """``measures`` for a product followed by a ReLU: the error against relu(A B) on all elements, and ``visible`` = the fraction of
    elements with A B > 4 bar S, the only ones that can show a lost term."""
    m = measures(A, B, got, q)
    m["err"] = np.abs(np.asarray(got, np.float64) - np.maximum(m["ref"], 0)) / m["S"]
    m["visible"] = float((m["ref"] > 4 * m["bar"] * m["S"]).mean())
    return m


# ---- the decoders' logit tile: only differences of logits leave the kernels ------------------------------------------------------
DECODE_W = 8


def decode_case(q):
    """x [37,128], Wt [40,128] (bias 0).  A quarter of the words keep the probe's magnitude, the others are scaled by 1/4 (exact:
    a power of two): log-probabilities and arg-maxima are blind to an error all words of a row share, so the probed term must
    differ between the words that meet in a row's top W."""
    A, B, qp = case("decode", q)
    scale = np.where(np.arange(B.shape[1]) % 4 == 0, 1.0, 0.25).astype(np.float32)
    return A, np.ascontiguousarray((B * scale[None, :]).T), qp


def topw_check(x, Wt, q, top_logp, top_word):
    """spacap_beam_topw_f32's lists against float64.  Returns (ratio, decided): ratio = the largest error of
    top_logp[r,i] - top_logp[r,0] against the float64 logit difference of the same two words, over its tolerance
    bar S + 2^-22 max|logp| (S = the larger of the two words'; the second term: two fp32 subtractions of the row's log-sum-exp,
    2^-23 each, times 2); decided = the fraction of list positions whose float64 logit is more than 2 bar S away from both
    neighbours in the float64 ranking -- there the word must be the float64 one (asserted here)."""
    B = np.ascontiguousarray(Wt.T)
    m = measures(x, B, np.zeros((x.shape[0], B.shape[1])), q)
    ref, S, bar = m["ref"], m["S"], m["bar"]
    W = top_word.shape[1]
    order = np.argsort(-ref, axis=1, kind="stable")
    srt = np.take_along_axis(ref, order, 1)
    thr = 2 * bar * S.max(1, keepdims=True)
    gap = srt[:, :-1] - srt[:, 1:]                                   # gap[i]: between ranks i and i + 1
    clear = np.ones((x.shape[0], W), bool)
    clear[:, 1:] &= gap[:, :W - 1] > thr
    clear &= gap[:, :W] > thr
    assert (top_word[clear] == order[:, :W][clear]).all(), "a word differs from the float64 ranking where it is decided"
    lw = np.take_along_axis(ref, top_word, 1)
    Sw = np.take_along_axis(S, top_word, 1)
    got = top_logp.astype(np.float64)
    err = np.abs((got - got[:, :1]) - (lw - lw[:, :1]))
    tol = bar * np.maximum(Sw, Sw[:, :1]) + 2.0 ** -22 * np.abs(got).max()
    return float((err / tol).max()), float(clear.mean())


def topw_restated(logits, W):
    """What the kernel returns, given its logits: fp32 log-probabilities of the W best words (descending, ties: smaller word)."""
    l = np.asarray(logits, np.float32).astype(np.float64)
    order = np.argsort(-l, axis=1, kind="stable")[:, :W]
    mx = l.max(1, keepdims=True)
    lse = (mx + np.log(np.exp(l - mx).sum(1, keepdims=True))).astype(np.float32)
    return (np.take_along_axis(l, order, 1).astype(np.float32) - lse).astype(np.float32), order


def greedy_check(x, Wt, q, word):
    """spacap_decode_word_f32: the word is the float64 arg-max on every row whose best-to-second gap exceeds 2 bar S.  Returns the
    fraction of rows decided."""
    B = np.ascontiguousarray(Wt.T)
    m = measures(x, B, np.zeros((x.shape[0], B.shape[1])), q)
    srt = -np.sort(-m["ref"], axis=1)
    decided = (srt[:, 0] - srt[:, 1]) > 2 * m["bar"] * m["S"].max(1)
    assert (np.asarray(word)[decided] == m["ref"].argmax(1)[decided]).all(), "the greedy word differs from the float64 arg-max"
    return float(decided.mean())


# ---- the fused relation head's backward (csrc/relation_fused.hip): scenes whose fp32 stages are exact -----------------------------
# hid1[(i,j),:] = P[0,i,j] U[j,0,:] (P is 0 / 1 on head 0, 0 on the others, b1 = 0); dpred has ONE non-zero output o per pair, a
# signed power of two s, and hid2 > 0 everywhere: dz2[(i,j),:] = s W3[o,:] exactly.
def _pair_output(K):
    i, j = np.meshgrid(np.arange(K), np.arange(K), indexing="ij")
    return (i + 3 * j) % 9


def relation_dw2_scene(q, K, seed=SEED):
    """dW2 [c_out, c_in] = sum over the pairs of dz2[pair, c_out] hid1[pair, c_in], kernel term q = (piece PA[q] of dz2) x
    (piece PB[q] of hid1).  Row o of W3 is positive with piece PA[q] of sign t_o, key j's row of U positive with piece PB[q] of
    sign tau_j; the pair's s has the sign t_o tau_j, which makes the probed product positive in every summand and is also the
    (random) sign of the leading term.  Returns dict(W3 [9,128], U0 [K,128], dpred [K,K,9], A [128, K K], B [K K, 128])."""
    p, pp = PA[q], PB[q]
    rng = np.random.default_rng([seed, 77, q, K])
    pm = lambda n: rng.integers(0, 2, n) * 2.0 - 1.0
    t = np.ones(9) if p == 0 else pm(9)
    tau = np.ones(K) if pp == 0 else pm(K)
    W3 = _magnitudes(rng, (9, 128), p, t[:, None], FLOOR)
    U0 = _magnitudes(rng, (K, 128), pp, tau[:, None], FLOOR)
    o = _pair_output(K)
    s = t[o] * tau[None, :] * 2.0 ** rng.integers(-1, 2, (K, K))
    dpred = np.zeros((K, K, 9), np.float32)
    np.put_along_axis(dpred, o[..., None], s[..., None].astype(np.float32), 2)
    A = (s.reshape(-1)[None, :] * W3[o.reshape(-1)].T).astype(np.float32)             # [c_out, pair], pair = i K + j
    B = np.ascontiguousarray(np.broadcast_to(U0[None], (K, K, 128)).reshape(K * K, 128))
    return {"W3": W3, "U0": U0, "dpred": dpred, "A": A, "B": B}


def relation_db2_scene(p, K, seed=SEED):
    """db2 [c] = sum over the pairs of dz2[pair, c] through the ones loop: W3 = bias_probe (piece p positive in every element), s > 0.
    Returns dict(W3, dpred [K,K,9], G [K K, 128] = dz2)."""
    rng = np.random.default_rng([seed, 78, p, K])
    W3 = bias_probe(p, 9, 128, seed + 5, FLOOR)
    o = _pair_output(K)
    s = 2.0 ** rng.integers(-1, 2, (K, K))
    dpred = np.zeros((K, K, 9), np.float32)
    np.put_along_axis(dpred, o[..., None], s[..., None].astype(np.float32), 2)
    return {"W3": W3, "dpred": dpred, "G": (s.reshape(-1)[:, None] * W3[o.reshape(-1)]).astype(np.float32)}
