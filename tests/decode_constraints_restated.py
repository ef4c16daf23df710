"""Constrained caption decoding restated in numpy -- the contract the device kernels
(csrc/caption_decode.hip: decode_constraint_kernel and the *_constrained kernels) and the torch rule
(spacap3d_amd/decode_constraints.py) are held to.

A row has generated y_0 .. y_{i-1} (neither sos nor the object indicator).  The logits z of step i become z':
  1. every distinct word v of the history: z_v / theta when z_v > 0, else z_v * theta  (theta >= 1; one operation in z's dtype)
  2. z_v = -inf for v in bad_words, for eos while i < min_length, and with n = ngram >= 1 for every v for which
     (y_{i-n+1} .. y_{i-1}, v) equals some (y_j .. y_{j+n-1}), j + n - 1 <= i - 1  (n = 1: every used word)
Everything downstream -- arg-max, log_softmax, softmax / top-k / nucleus, the reported log-probability -- sees z'.
This file is written loop by loop from that text, not from the code under test."""
import numpy as np

import sampling_restated as SR

OFF = dict(min_length=0, ngram=0, theta=1.0, bad_words=())


def ngram_bans(h, n):
    """the words the no-repeat rule bans after the history h (a list): loops over every n-gram of the history"""
    i = len(h)
    out = set()
    if n < 1 or i < n - 1:
        return out
    tail = list(h[i - (n - 1):]) if n > 1 else []
    for j in range(0, i - n + 1):                       # the n-gram y_j .. y_{j+n-1} lies inside the history
        if list(h[j:j + n - 1]) == tail:
            out.add(int(h[j + n - 1]))
    return out


def banned_set(h, eos, min_length=0, ngram=0, theta=1.0, bad_words=()):
    out = {int(w) for w in bad_words}
    if len(h) < min_length:
        out.add(int(eos))
    return out | ngram_bans(h, ngram)


def constrain(z, h, eos, min_length=0, ngram=0, theta=1.0, bad_words=()):
    """z' of one row: z (V,) in float32 or float64 (the penalty is one operation in that dtype), h the row's history"""
    z = np.array(z, copy=True)
    th = z.dtype.type(theta)
    for v in sorted({int(w) for w in h}):
        z[v] = z[v] / th if z[v] > 0 else z[v] * th
    for v in banned_set(h, eos, min_length, ngram, theta, bad_words):
        z[v] = -np.inf
    return z


def constrain_rows(z, hist, step, eos, **c):
    """z' (N, V) for the histories hist (N, >= step), of which columns 0 .. step - 1 count"""
    return np.stack([constrain(z[r], list(hist[r, :step]), eos, **c) for r in range(z.shape[0])])


def image_words(V):
    return 2 * ((V + 63) // 64)


def images(hist, step, V, eos, **c):
    """uint32 (N, 2, nw): plane 0 the banned words, plane 1 the words of the history; bit v % 32 of word v // 32"""
    N, nw = hist.shape[0], image_words(V)
    out = np.zeros((N, 2, nw), np.uint32)
    for r in range(N):
        # a word outside the vocabulary counts as none: it sets no bit and matches nothing (a value of its own per position)
        row = [int(w) if 0 <= w < V else -1 - j for j, w in enumerate(hist[r, :step])]
        h = [w for w in row if w >= 0]
        for v in banned_set(row, eos, **c):
            if 0 <= v < V:
                out[r, 0, v // 32] |= np.uint32(1 << (v % 32))
        for v in h:
            out[r, 1, v // 32] |= np.uint32(1 << (v % 32))
    return out


def beam_histories(tr_word, anc, step, W):
    """(R W, step): hypothesis (r, w)'s own words.  tr_word (n_words, R, W); anc (R W, T): the ancestor table of position
    t = step + 1.  Word j was the input of position j + 2, computed in the slot the hypothesis occupied there: anc[row][j + 2]
    for j + 2 < t, the row's own slot at position t; an entry outside 0..W-1 reads the row's own slot."""
    RW = anc.shape[0]
    t = step + 1
    out = np.zeros((RW, step), np.int64)
    for row in range(RW):
        r, w = divmod(row, W)
        for j in range(step):
            p = j + 2
            slot = w
            if p < t:
                s = int(anc[row, p])
                slot = s if 0 <= s < W else w
            out[row, j] = tr_word[j, r, slot]
    return out


# ---- properties of finished captions ---------------------------------------------------------------------------------------------
def through_first_eos(tokens, eos):
    """the caption's words through its first eos (all of them when there is none)"""
    tokens = [int(t) for t in tokens]
    return tokens[:tokens.index(eos) + 1] if eos in tokens else tokens


def repeats_ngram(words, n):
    seen = set()
    for j in range(len(words) - n + 1):
        g = tuple(words[j:j + n])
        if g in seen:
            return True
        seen.add(g)
    return False


def caption_faults(tokens, eos, min_length=0, ngram=0, bad_words=(), **_):
    """[(row, what)] over the captions tokens (N, n) read through their first eos: a bad word, a repeated n-gram, an eos before
    min_length words"""
    out = []
    for r, row in enumerate(np.asarray(tokens)):
        w = through_first_eos(row, eos)
        if set(w) & set(bad_words):
            out.append((r, "bad word"))
        if ngram >= 1 and repeats_ngram(w, ngram):
            out.append((r, "repeated n-gram"))
        body = w[:-1] if w and w[-1] == eos else w
        if len(body) < min_length:
            out.append((r, "too short"))
    return out


# ---- the one-step cases of tests/test_decode_constraints_gpu.py; checked without a GPU in tests/test_decode_constraints_cpu.py ----
STEP_SHAPES = SR.STEP_SHAPES + [(1, 65), (17, 257)]
STEP, N_WORDS = SR.STEP, SR.N_WORDS
THETA = 1.3


def edge_words(V):
    """word 0 and V - 1 and both sides of every 64-word chunk edge (on the MI355X a vocabulary slice is one chunk at every
    shape above, so these are also the first and last word of every slice)"""
    e = [0, V - 1]
    for k in range(64, V, 64):
        e += [k - 1, k]
    return sorted(set(e))


# Per shape: {row: salt} moves the free words of a row's history (p, q and, for n <= 2, B).  Chosen by the restatement alone
# (tests/test_decode_constraints_cpu.py::test_one_step_cases_have_few_open_rows), as SR.step_inputs' generator seed was: the
# small shapes allow no open row at all under the 2 % cap.
ROW_SALT = {(37, 40): {6: 1}, (33, 3001): {0: 1, 17: 1, 21: 1}, (17, 257): {1: 1, 7: 1}}


def step_case(rows, V, ngram, salts=None):
    """The planted inputs of a shape: SR.step_inputs' x, W, bias and float64 logits, then
    eos        the unconstrained arg-max of the last row, banned by min_length = STEP + 1
    bad_words  word 0, V - 1 and as many chunk-edge words as fit a budget of min(64, V // 4)
    hist       (rows, STEP): every row's history bans, by the n-gram rule, its own unconstrained arg-max (even rows) or a
               chunk-edge word (odd rows) and one more edge word; the edge words cycle over the rows, so every edge is
               banned in some row, some through bad_words and the history at once.
    n = 1: the history is banned itself; n = 2: [p, A, p, B, p] bans A and B; n = 3: [p, q, A, p, q] bans A."""
    x, Wt, b, logits = SR.step_inputs(rows, V)
    order = np.argsort(-logits, axis=1, kind="stable")
    best = order[:, 0]
    eos = int(best[-1])
    edges = edge_words(V)
    budget = min(64, V // 4)
    bad = [w for w in [0, V - 1] + edges[1:-1] if w != eos][:budget]
    if len(bad) < 3:
        bad += [w for w in (V // 3, V // 2) if w != eos and w not in bad]
    edges = [w for w in edges if w not in bad] + [w for w in edges if w in bad]     # the histories take the others first
    hist = np.zeros((rows, STEP), np.int64)
    salts = ROW_SALT.get((rows, V), {}) if salts is None else salts
    for r in range(rows):
        salt = salts.get(r, 0)
        A = int(best[r]) if r % 2 == 0 else edges[(r // 2) % len(edges)]
        # salt >= 1 bans the row's salt-th runner-up as well or instead: in place of q under n = 1 (B stays an edge word), of B
        # under n = 2, of an odd row's A under n = 3
        B = edges[r % len(edges)] if salt == 0 or ngram == 1 else int(order[r, salt])
        if ngram == 3 and salt and r % 2:
            A = B
        free = [w for w in range(V) if w not in (A, B, eos)]
        p, q = free[(7 * r + 3 + 5 * salt) % len(free)], free[(11 * r + 5 + 3 * salt) % len(free)]
        if ngram == 1 and salt:
            q = int(order[r, salt])
        hist[r] = {1: [p, A, q, B, p], 2: [p, A, p, B, p], 3: [p, q, A, p, q]}[ngram]
    c = dict(min_length=STEP + 1, ngram=ngram, theta=1.0, bad_words=tuple(bad))
    return dict(x=x, Wt=Wt, b=b, logits=logits, eos=eos, hist=hist, c=c, z=constrain_rows(logits, hist, STEP, eos, **c),
                seed=SR.STEP_SEED)


NGRAM_OF = {shape: (1, 2, 3)[i % 3] for i, shape in enumerate(STEP_SHAPES)}     # the n of every shape's one-step case


def penalty_case(rows, V):
    """theta = 1.3 alone: an even row's history holds its unconstrained arg-max (the penalty must move it wherever the
    runner-up then leads), an odd row's history holds its five worst words (its best word stays)."""
    x, Wt, b, logits = SR.step_inputs(rows, V)
    order = np.argsort(-logits, axis=1, kind="stable")
    hist = np.zeros((rows, STEP), np.int64)
    for r in range(rows):
        hist[r] = [order[r, 0]] + list(order[r, -4:]) if r % 2 == 0 else list(order[r, -5:])
    c = dict(OFF, theta=THETA)
    eos = int(order[0, -1])
    return dict(x=x, Wt=Wt, b=b, logits=logits, eos=eos, hist=hist, c=c, z=constrain_rows(logits, hist, STEP, eos, **c))


def top2_gap(z):
    """best minus second best of every row (inf with one finite entry)"""
    s = np.sort(z, axis=1)[:, ::-1]
    return np.where(np.isfinite(s[:, 1]), s[:, 0] - s[:, 1], np.inf) if z.shape[1] > 1 else np.full(z.shape[0], np.inf)


def log_softmax(z):
    m = z.max(1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(1, keepdims=True)))


def top_w(z, W):
    """the W best (log-probability, word) of every row of z': value descending, equal ones the smaller word first"""
    order = np.argsort(-z, axis=1, kind="stable")[:, :W]
    return np.take_along_axis(log_softmax(z), order, 1), order


def lmax(z):
    """max |z'| over the finite entries: the scale of the project's 1e-4 bound for the logit arithmetic"""
    return float(np.abs(z[np.isfinite(z)]).max())


def tolerance(z, tau):
    """SR.tolerance on the finite entries of z'"""
    return 1e-4 * lmax(z) / tau + 1e-5


def list_gaps(z, W):
    """(N, W): entry k of a row's top-W list minus entry k + 1 (inf where both are -inf, or behind the last word): where it is
    below 1e-4 max|l| the float32 logits may order the two words the other way"""
    s = np.sort(z, axis=1)[:, ::-1][:, :W + 1]
    if s.shape[1] < W + 1:
        s = np.concatenate([s, np.full((s.shape[0], W + 1 - s.shape[1]), -np.inf)], 1)
    with np.errstate(invalid="ignore"):
        d = s[:, :-1] - s[:, 1:]
    return np.where(np.isnan(d), np.inf, d)


def list_open(z, W):
    """(N,) bool, the open rows of a top-W list: best and second best within the tolerance, or the W-th and (W + 1)-th entry
    within 1e-4 max|l| (the set itself may differ)"""
    g = list_gaps(z, W)
    return (top2_gap(z) < tolerance(z, 1.0)) | (g[:, W - 1] < 1e-4 * lmax(z))


def sample_draw(z, tau, top_k, top_p, seed=SR.STEP_SEED, step=STEP, n_words=N_WORDS):
    """The restated draw of every row from the constrained logits z' (N, V): SR.draw for top_k >= 0, the nucleus rule of
    tests/nucleus_restated.py for top_p (its tolerances taken from the finite entries).  Returns word, second, logp64 (N, V)
    and open (N,) bool: the best and second-best z within the tolerance, the top-k set within 1e-4 max|l| of changing, or
    the nucleus within its delta of changing the draw."""
    import nucleus_restated as NR
    N, V = z.shape
    rho = np.arange(N)
    tol = tolerance(z, tau)
    if top_p is None:
        with np.errstate(invalid="ignore"):
            d = SR.draw(z, rho, step, n_words, tau, top_k, seed)
        is_open = (d["gap"] < tol) | (np.nan_to_num(d["cut"], nan=np.inf) < 1e-4 * lmax(z))
        word, second = d["word"], d["second"]
    else:
        zz = z / tau + SR.noise(rho, step, n_words, V, seed)
        A = NR.mass_above(z, tau)
        dl = 2.0 * (1e-4 * lmax(z) / tau) + 1e-5
        word, second, gap = NR._best_two(np.where(A < top_p, zz, -np.inf))
        lo = NR._best_two(np.where(A < top_p * (1.0 - dl), zz, -np.inf))[0]
        hi = NR._best_two(np.where(A < min(top_p * (1.0 + dl), 1.0), zz, -np.inf))[0]
        is_open = (gap < tol) | (lo != word) | (hi != word)
    return dict(word=word, second=second, logp=log_softmax(z), open=is_open)


SAMPLE_MODES = [(tau, k, p) for tau in (1.0, 0.7) for k, p in ((0, None), (3, None), (0, 0.6))]
TOPW_WIDTHS = (1, 3, 8)
