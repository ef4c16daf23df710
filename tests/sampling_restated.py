"""Sampled caption decoding restated in numpy float64 -- the contract the device kernels
(csrc/caption_decode.hip: vocab_gumbel_kernel / sample_next_kernel) and the generic path (spacap3d_amd/sampling.py) are held to.

Row rho, step i, word v, logits l of the row:
    idx  = (rho n_words + i) V + v                      (unsigned 64-bit)
    h    = hash32(idx, make_seed(seed, counter))        (csrc/dropout.hpp: the dropout keep mask's hash)
    u    = ((h >> 9) + 0.5) 2^-23                       (exact in float32; in [2^-24, 1 - 2^-24])
    g    = -log(-log u)
    z_v  = l_v / tau + g_v
    word = argmax z (the larger z, among equal z the smaller v) over the whole vocabulary (top_k = 0) or over the k words of
           largest l (equal l: the smaller word first)
    logp = l_word - logsumexp(l)
A row that was finished emits eos and keeps score and length; another adds logp, sets length = i + 1 and becomes finished when
it drew eos.  Here g is float64 of the exact u; the kernels form it in float32 (``gumbel32`` restates that)."""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15


def seed_words(seed, counter=None):
    s = np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    if counter is not None:
        with np.errstate(over="ignore"):
            s = s + np.array([int(counter) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64) * np.array([GOLDEN], dtype=np.uint64)
    return (s & np.uint64(0xFFFFFFFF)).astype(np.uint32), (s >> np.uint64(32)).astype(np.uint32)


def hash32(idx, seed, counter=None):
    """uint32 hash of the uint64 indices ``idx``, in uint32 / uint64 array arithmetic (which wraps as the device's does)"""
    idx = np.asarray(idx, dtype=np.uint64)
    s_lo, s_hi = seed_words(seed, counter)
    with np.errstate(over="ignore"):
        h = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32) ^ s_lo
        h = h + ((idx >> np.uint64(32)).astype(np.uint32) ^ s_hi) * np.uint32(0x9E3779B1)
        h = h ^ (h >> np.uint32(16))
        h = h * np.uint32(0x85EBCA6B)
        h = h ^ (h >> np.uint32(13))
        h = h * np.uint32(0xC2B2AE35)
        h = h ^ (h >> np.uint32(16))
    assert h.dtype == np.uint32
    return h


def uniform_of(h):
    return ((np.asarray(h, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel64(h):
    return -np.log(-np.log(uniform_of(h)))


def gumbel32(h):
    """the kernels' arithmetic: every step in float32"""
    u = ((np.asarray(h, dtype=np.uint32) >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    return -np.log(-np.log(u))


def noise(rho, step, n_words, V, seed, counter=None, words=None):
    """g (N, V) float64 of rows ``rho`` (N,) at ``step`` (or (N, C) for the word ids ``words`` (N, C))"""
    rho = np.asarray(rho, dtype=np.uint64).reshape(-1, 1)
    w = np.arange(V, dtype=np.uint64).reshape(1, -1) if words is None else np.asarray(words, dtype=np.uint64)
    idx = (rho * np.uint64(n_words) + np.uint64(step)) * np.uint64(V) + w
    return gumbel64(hash32(idx, seed, counter))


def draw(logits, rho, step, n_words, tau, top_k, seed, counter=None):
    """One step for rows ``rho`` (N,) with float64 ``logits`` (N, V).  Returns a dict of (N,) arrays: ``word``, ``second`` (the
    runner-up; -1 with one candidate), ``gap`` (z_word - z_second; inf with one candidate), ``logp``, and ``cut``: the k-th
    minus the (k+1)-th largest logit (inf for top_k = 0 or k = V) -- how firmly the candidate set itself is decided."""
    logits = np.asarray(logits, dtype=np.float64)
    N, V = logits.shape
    z = logits / tau + noise(rho, step, n_words, V, seed, counter)
    cut = np.full(N, np.inf)
    if top_k:
        order = np.argsort(-logits, axis=1, kind="stable")             # equal logits keep the smaller word first
        srt = np.take_along_axis(logits, order, 1)
        if top_k < V:
            cut = srt[:, top_k - 1] - srt[:, top_k]
        allowed = np.zeros((N, V), bool)
        np.put_along_axis(allowed, order[:, :top_k], True, 1)
        z = np.where(allowed, z, -np.inf)
    word = z.argmax(1)                                                  # numpy: the first maximum
    rows = np.arange(N)
    best = z[rows, word]
    z2 = z.copy()
    z2[rows, word] = -np.inf
    second = z2.argmax(1)
    gap = best - z2[rows, second]
    second = np.where(np.isfinite(z2[rows, second]), second, -1)
    m = logits.max(1)
    lse = m + np.log(np.exp(logits - m[:, None]).sum(1))
    return {"word": word, "second": second, "gap": gap, "logp": logits[rows, word] - lse, "cut": cut}


def advance(word, logp, step, eos, score, length, finished):
    """The row state after a step: returns (word emitted, score, length, finished) -- new arrays."""
    fin = np.asarray(finished, bool)
    out = np.where(fin, eos, word)
    score = np.where(fin, score, score + logp)
    length = np.where(fin, length, step + 1)
    return out, score, length, fin | (out == eos)


def tolerance(logits, tau):
    """A row-step whose best and second-best z are closer than this is open: 1e-4 max|l| / tau (the project's bound for the
    logit arithmetic, tests/test_beam_search_gpu.py::test_top_w_words_of_gaussian_logits) + 1e-5 (two float32 logs, |g| <= 17)"""
    return 1e-4 * float(np.abs(logits).max()) / tau + 1e-5


def chi_square(words, p):
    """Pearson's statistic of the drawn ``words`` against the probabilities ``p`` (V,) (zero entries must stay undrawn)"""
    n = len(words)
    cnt = np.bincount(words, minlength=len(p)).astype(np.float64)
    assert (cnt[p == 0] == 0).all()
    keep = p > 0
    return float((((cnt - n * p) ** 2)[keep] / (n * p[keep])).sum()), float((n * p[keep]).min())


# the one-step cases of tests/test_sampling_gpu.py (Gaussian inputs as in the top-W tests); checked without a GPU in tests/test_sampling.py
STEP_SHAPES = [(16, 64), (37, 40), (300, 1000), (33, 3001)]
STEP_TOP_K = [0, 1, 3, 8]
STEP_TAU = [1.0, 0.7]
STEP, N_WORDS, EOS, STEP_SEED = 5, 31, 1, 0x1234567890ABCDEF


def step_inputs(rows, V):
    """x (rows, 128), W (V, 128), bias (V,) float32 torch tensors on the CPU, and the float64 logits.  The generator seed was
    chosen by the restatement alone (tests/test_sampling.py::test_one_step_cases_have_few_open_rows): 16 rows allow no open
    row at all under the 2 % cap, and rows + V, the top-W tests' seed, has one."""
    import torch
    g = torch.Generator().manual_seed(rows + V + 2)
    x = torch.randn(rows, 128, generator=g)
    Wt, b = 0.3 * torch.randn(V, 128, generator=g), torch.randn(V, generator=g)
    logits = (x.double() @ Wt.double().t() + b.double()).numpy()
    return x, Wt, b, logits


def chi_cases():
    """(name, R, logits (V,), tau, top_k, bar): the distribution cases; bar = the 99.9 % quantile of chi-square with V - 1
    (k - 1) degrees of freedom.  Logits uniform in [-1.5, 1.5]: the smallest expected count stays above 5."""
    g = np.random.default_rng(0)
    l16, l40 = g.uniform(-1.5, 1.5, 16), g.uniform(-1.5, 1.5, 40)
    return [("V16", 4096, l16, 1.0, 0, 37.7), ("V40", 8192, l40, 1.0, 0, 72.1), ("V40_tau2", 8192, l40, 2.0, 0, 72.1),
            ("V16_top4", 4096, l16, 1.0, 4, 16.27)]


def target(logits, tau, top_k):
    """softmax(l / tau), over the top_k largest logits only when top_k >= 1"""
    logits = np.asarray(logits, np.float64)
    e = np.exp((logits - logits.max()) / tau)
    if top_k:
        keep = np.zeros(len(logits), bool)
        keep[np.argsort(-logits, kind="stable")[:top_k]] = True
        e = np.where(keep, e, 0.0)
    return e / e.sum()


def teacher_forced_logits(cap, d, tokens):
    """The logits (rows, n, V) that predict word i of every row of ``tokens`` (rows, n) from the row's own prefix, through the
    UNCACHED decoder in one pass (``forward_eval(use_cache=False)`` without the loop); row rho belongs to proposal
    rho // (rows / (B K)).  In the dtype of ``cap``'s parameters."""
    import torch
    from spacap3d_amd.transformer_captioner import subsequent_mask
    obj = d["aggregated_vote_features"]
    if cap.token_proj is not None:
        obj = cap.token_proj(obj)
    B, K, _ = obj.shape
    rows, n = tokens.shape
    S = rows // (B * K)
    src_pos = cap._src_pos(d)
    src_mask = d["bbox_mask"].unsqueeze(1)
    memory = cap.model.encode(obj, src_pos, src_mask)
    ys = torch.cat([torch.full((rows, 1), cap.word_to_idx["sos"], dtype=torch.long, device=tokens.device), tokens[:, :-1]], 1)
    outs = []
    for s in range(S):      # sample s of every proposal: one pass of B K rows, as the uncached greedy loop runs it
        out = cap.model(obj, ys[s::S], src_mask, subsequent_mask(n + 1, device=tokens.device), obj.reshape(B * K, -1).unsqueeze(1),
                        src_pos=src_pos, memory=memory)
        outs.append(cap.model.generator.proj(out[:, 1:, :]))             # position 1 + i predicts word i
    return torch.stack(outs, 1).reshape(rows, n, -1)


def replay(tokens, logits, tau, top_k, seed, eos, counter=None):
    """Every row's own prefix replayed: ``tokens`` (rows, n) as sampled, ``logits`` (rows, n, V) float64 teacher-forced on them.
    Through each row's first eos the restated draw must equal the sampled word unless the step is open (gap below
    ``tolerance``, then either of the two words; or, with top_k, the candidate set itself within 1e-4 max|l| of changing).
    Returns ``wrong`` [(row, step)], ``open_rows`` (set), ``open_steps`` of ``live_steps`` row-steps, and the float64 ``score`` / ``length`` of the sampled words, and
    ``padded``: whether eos repeats behind every first eos."""
    tokens, logits = np.asarray(tokens), np.asarray(logits, np.float64)
    rows, n = tokens.shape
    rho = np.arange(rows)
    fin = np.zeros(rows, bool)
    score, length = np.zeros(rows), np.zeros(rows, np.int64)
    wrong, open_rows, padded, open_steps, live_steps = [], set(), True, 0, 0
    for i in range(n):
        lg = logits[:, i]
        d = draw(lg, rho, i, n, tau, top_k, seed, counter)
        tol = tolerance(lg, tau)
        m = lg.max(1)
        lp = lg[rho, tokens[:, i]] - (m + np.log(np.exp(lg - m[:, None]).sum(1)))
        for r in np.flatnonzero(~fin):
            near = d["gap"][r] < tol
            loose = d["cut"][r] < 1e-4 * float(np.abs(lg).max())
            live_steps += 1
            if near or loose:
                open_rows.add(int(r))
                open_steps += 1
            ok = tokens[r, i] == d["word"][r] or (near and tokens[r, i] == d["second"][r]) or loose
            if not ok:
                wrong.append((int(r), i))
        padded = padded and bool((tokens[fin, i] == eos).all())
        _, score, length, fin = advance(tokens[:, i], lp, i, eos, score, length, fin)
    return {"wrong": wrong, "open_rows": open_rows, "open_steps": open_steps, "live_steps": live_steps, "score": score, "length": np.where(fin, length, n), "padded": padded}
