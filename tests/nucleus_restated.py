"""Nucleus (top-p) sampling restated in numpy float64 ("Top-p") -- the contract the device kernels
(csrc/caption_decode.hip: vocab_logits_kernel / nucleus_next_kernel) and the generic path (spacap3d_amd/sampling.py) are held to.

Row rho, step i, logits l of the row, temperature tau, 0 < p <= 1:
    q    = softmax(l / tau)                              (the tempered distribution)
    A_v  = sum of q_u over the words u with l_u > l_v    (the mass strictly more probable than v)
    N    = { v : A_v < p }                               (equal logits enter or stay out together; the best word is always in)
    word = the first maximum over v in N of z_v = l_v / tau + g_v, g the noise of tests/sampling_restated.py (same flat index)
    logp = l_word - logsumexp(l)                         (untempered, untruncated)
The row state advances as in sampling_restated.advance.  The kernels form l in split-bf16 arithmetic (within 1e-4 max|l| of
float64) and the mass in float32, so a set decided by less than that is not decided: ``draw`` reports as ``edge`` whether the word
changes when p moves by the relative amount ``delta``."""
import numpy as np

import sampling_restated as SR


def mass_above(logits, tau):
    """A (N, V) float64.  Summed along the logits in descending order; a run of equal logits takes the mass in front of it."""
    logits = np.asarray(logits, dtype=np.float64)
    order = np.argsort(-logits, axis=1, kind="stable")
    srt = np.take_along_axis(logits, order, 1)
    e = np.exp((srt - srt[:, :1]) / tau)
    q = e / e.sum(1, keepdims=True)
    front = np.cumsum(q, 1) - q
    starts = np.ones(srt.shape, bool)
    starts[:, 1:] = srt[:, 1:] != srt[:, :-1]
    front = np.maximum.accumulate(np.where(starts, front, 0.0), axis=1)          # (front never decreases along a row)
    A = np.empty_like(front)
    np.put_along_axis(A, order, front, 1)
    return A


def nucleus(logits, tau, p):
    """(N, V) bool: the words of every row's nucleus"""
    return mass_above(logits, tau) < p


def delta(logits, tau):
    """The relative width of p inside which the set is not decided: 2 x (1e-4 max|l| / tau) -- the project's logit bound on both
    sides of a probability ratio -- + 1e-5 for the float32 sum."""
    return 2.0 * (1e-4 * float(np.abs(logits).max()) / tau) + 1e-5


def _best_two(z):
    rows = np.arange(z.shape[0])
    word = z.argmax(1)                                                  # numpy: the first maximum
    z2 = z.copy()
    z2[rows, word] = -np.inf
    second = z2.argmax(1)
    gap = z[rows, word] - z2[rows, second]
    return word, np.where(np.isfinite(z2[rows, second]), second, -1), gap


def draw(logits, rho, step, n_words, tau, p, seed, counter=None):
    """One step for rows ``rho`` (N,) with float64 ``logits`` (N, V).  Returns a dict of (N,) arrays: ``word``, ``second`` (the
    runner-up inside the nucleus; -1 with one candidate), ``gap`` (inf with one candidate), ``logp``, ``lo`` / ``hi`` (the word
    when p is replaced by p (1 - delta) / by min(p (1 + delta), 1)), ``edge`` (one of those two differs from ``word``), ``free``
    (the unrestricted draw: top_k = 0) and ``size`` (words in the nucleus); and ``inside`` (N, V) bool, the nucleus."""
    logits = np.asarray(logits, dtype=np.float64)
    N, V = logits.shape
    z = logits / tau + SR.noise(rho, step, n_words, V, seed, counter)
    A = mass_above(logits, tau)
    inside = A < p
    word, second, gap = _best_two(np.where(inside, z, -np.inf))
    dl = delta(logits, tau)
    lo = _best_two(np.where(A < p * (1.0 - dl), z, -np.inf))[0]
    hi = _best_two(np.where(A < min(p * (1.0 + dl), 1.0), z, -np.inf))[0]
    m = logits.max(1)
    lse = m + np.log(np.exp(logits - m[:, None]).sum(1))
    return {"word": word, "second": second, "gap": gap, "logp": logits[np.arange(N), word] - lse, "lo": lo, "hi": hi,
            "edge": (lo != word) | (hi != word), "free": z.argmax(1),
            "size": inside.sum(1), "inside": inside}


def is_open(d, logits, tau):
    """(N,) bool: the row-steps of ``draw``'s result that may draw another restated word than ``word``"""
    return (d["gap"] < SR.tolerance(logits, tau)) | d["edge"]


def allowed(d, logits, tau, words):
    """(N,) bool: ``words`` are what the contract lets the rows draw -- the restated word; with a gap below ``SR.tolerance`` also
    the runner-up; on an edge row also the word at either moved p."""
    near = d["gap"] < SR.tolerance(logits, tau)
    return (words == d["word"]) | (near & (words == d["second"])) | (d["edge"] & ((words == d["lo"]) | (words == d["hi"])))


def replay(tokens, logits, tau, p, seed, eos, counter=None):
    """Every row's own prefix replayed, as sampling_restated.replay: ``tokens`` (rows, n) as sampled, ``logits`` (rows, n, V)
    float64 teacher-forced on them.  Through each row's first eos the restated draw must equal the sampled word unless the step
    is open (``allowed``).  Returns ``wrong`` [(row, step)], ``outside`` [(row, step)] -- live words that lie outside the nucleus of min(p (1 + delta), 1) --,
    ``open_rows`` (set), ``open_steps`` of ``live_steps`` row-steps, ``left`` -- live steps whose restated unrestricted draw is
    not in the nucleus --, the float64 ``score`` / ``length`` of the sampled words, and ``padded``."""
    tokens, logits = np.asarray(tokens), np.asarray(logits, np.float64)
    rows, n = tokens.shape
    rho = np.arange(rows)
    fin = np.zeros(rows, bool)
    score, length = np.zeros(rows), np.zeros(rows, np.int64)
    wrong, outside, open_rows, padded, open_steps, live_steps, left = [], [], set(), True, 0, 0, 0
    for i in range(n):
        lg = logits[:, i]
        d = draw(lg, rho, i, n, tau, p, seed, counter)
        near = d["gap"] < SR.tolerance(lg, tau)
        fine = allowed(d, lg, tau, tokens[:, i])
        wide = mass_above(lg, tau) < min(p * (1.0 + delta(lg, tau)), 1.0)
        m = lg.max(1)
        lp = lg[rho, tokens[:, i]] - (m + np.log(np.exp(lg - m[:, None]).sum(1)))
        for r in np.flatnonzero(~fin):
            live_steps += 1
            left += int(not d["inside"][r, d["free"][r]])
            if near[r] or d["edge"][r]:
                open_rows.add(int(r))
                open_steps += 1
            if not wide[r, tokens[r, i]]:
                outside.append((int(r), i))
            if not fine[r]:
                wrong.append((int(r), i))
        padded = padded and bool((tokens[fin, i] == eos).all())
        _, score, length, fin = SR.advance(tokens[:, i], lp, i, eos, score, length, fin)
    return {"wrong": wrong, "outside": outside, "open_rows": open_rows, "open_steps": open_steps, "live_steps": live_steps, "left": left,
            "score": score, "length": np.where(fin, length, n), "padded": padded}


# the one-step cases of tests/test_nucleus_gpu.py; checked without a GPU in tests/test_nucleus.py
STEP_SHAPES = SR.STEP_SHAPES + [(19, 257)]
STEP_TAU = [1.0, 0.7]
STEP_P = [0.25, 0.5, 0.9, 0.99]
OPEN_CAP = 0.05               # of the rows; and none in the 16-row shape


def step_inputs(rows, V):
    """``sampling_restated.step_inputs`` for its own shapes.  The added shape draws the same Gaussians from generator seed
    rows + V + 1, chosen by the restatement alone (tests/test_nucleus.py::test_one_step_cases_have_few_open_rows): 19 rows allow
    no open row under the 5 % cap, and rows + V + 2, the seed of the other shapes, has one edge row at tau = 1, p = 0.5."""
    if (rows, V) in SR.STEP_SHAPES:
        return SR.step_inputs(rows, V)
    import torch
    g = torch.Generator().manual_seed(rows + V + 1)
    x = torch.randn(rows, 128, generator=g)
    Wt, b = 0.3 * torch.randn(V, 128, generator=g), torch.randn(V, generator=g)
    return x, Wt, b, (x.double() @ Wt.double().t() + b.double()).numpy()


def tie_case():
    """(bias (V,) float32, p, tied words, tail words): two words at A = 0, three tied words at A ~ 0.6 whose inclusion carries the
    mass past p = 0.7, and a tail of five.  The cumulative masses are 0.6, 0.9 and then the tail's: p is 0.1 from the nearest.
    Entries 2..4 are ONE float32 (the caller duplicates the weight rows as well), so their logits are bit-identical."""
    q = np.array([0.3, 0.3, 0.1, 0.1, 0.1, 0.02, 0.02, 0.02, 0.02, 0.02])
    return np.log(q).astype(np.float32), 0.7, (2, 3, 4), (5, 6, 7, 8, 9)
