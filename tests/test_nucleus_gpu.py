"""Nucleus (top-p) sampling on the MI355X (csrc/caption_decode.hip: vocab_logits_kernel / nucleus_next_kernel,
caption_decode.sample_decode(top_p=), forward_eval, Evaluator, SelfCritical) against the float64 restatement of the contract
(tests/nucleus_restated.py, DESIGN.md section 7i "Top-p"), the greedy decoder (p -> 0) and the unrestricted sampler (the same
noise).  The restatement itself, the generic path, the refusals and the open-row caps of the cases below: tests/test_nucleus.py."""
import copy
import math

import numpy as np
import pytest
import torch

import nucleus_restated as NR
import sampling_restated as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True, scope="module")
def _needs_a_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _lib():
    from spacap3d_amd._native import check, lib
    return lib, check, torch.cuda.current_stream().cuda_stream


class _Step:
    """One call of spacap_sample_word_nucleus_f32 (``top_p`` None: of spacap_sample_word_f32 at top_k = 0) on poisoned outputs;
    the state arrays are copies of the ones given."""

    def __init__(self, x, Wt, b, top_p, tau, seed, step, n_words, eos, fin=None, score=None, length=None, counter=None):
        from spacap3d_amd.linear import bf3_pieces
        lib, check, st = _lib()
        rows, V = x.shape[0], Wt.shape[0]
        g = torch.Generator().manual_seed(1)
        self.lut, self.pe = torch.randn(V, 128, generator=g).to(DEV), torch.randn(128, generator=g).to(DEV)
        self.scale = math.sqrt(128.0)
        self.ys = torch.full((rows, n_words), -7, dtype=torch.long, device=DEV)
        self.xw = torch.full((rows, 128), float("nan"), device=DEV)
        zero = torch.zeros(rows, dtype=torch.int32, device=DEV)
        self.fin = (zero if fin is None else fin).clone()
        self.score = (torch.zeros(rows, device=DEV) if score is None else score).clone()
        self.length = (zero if length is None else length).clone()
        cnt = None if counter is None else torch.tensor([counter], dtype=torch.int64, device=DEV)
        tail = (None if cnt is None else cnt.data_ptr(), n_words, step, eos, self.lut.data_ptr(), self.scale, self.pe.data_ptr(),
                self.ys.data_ptr(), self.score.data_ptr(), self.length.data_ptr(), self.fin.data_ptr(), self.xw.data_ptr())
        if top_p is None:
            ws = torch.empty(int(lib.spacap_sample_word_workspace_bytes(rows, V, 0)), dtype=torch.uint8, device=DEV)
            check(lib.spacap_sample_word_f32(x.data_ptr(), bf3_pieces(Wt).data_ptr(), b.data_ptr(), rows, V, 0, 1.0 / tau, seed, *tail,
                                             ws.data_ptr(), st), "spacap_sample_word_f32")
        else:
            ws = torch.empty(int(lib.spacap_sample_word_nucleus_workspace_bytes(rows, V)), dtype=torch.uint8, device=DEV)
            check(lib.spacap_sample_word_nucleus_f32(x.data_ptr(), bf3_pieces(Wt).data_ptr(), b.data_ptr(), rows, V, top_p, 1.0 / tau, seed,
                                                     *tail, ws.data_ptr(), st), "spacap_sample_word_nucleus_f32")
        torch.cuda.synchronize()

    def words(self, step):
        return self.ys[:, step].cpu().numpy()


@pytest.fixture(scope="module")
def step_case():
    """The inputs of a shape on the device, once (tests/nucleus_restated.py::step_inputs)."""
    made = {}

    def get(rows, V):
        if (rows, V) not in made:
            x, Wt, b, logits = NR.step_inputs(rows, V)
            made[(rows, V)] = (x.to(DEV), Wt.to(DEV), b.to(DEV), logits)
        return made[(rows, V)]
    return get


# ---- 1. one step through the C ABI -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", NR.STEP_P)
@pytest.mark.parametrize("tau", NR.STEP_TAU)
@pytest.mark.parametrize("rows,V", NR.STEP_SHAPES)
def test_one_step_against_the_restatement(step_case, rows, V, tau, p):
    """Step 5 of 31 with every third row finished on entry, outputs poisoned.  A row that is not open draws the restated word;
    an open one (best and second-best z within the tolerance, or the word changes when p moves by delta) a word the restatement
    allows (nucleus_restated.allowed); at most 5 % of the rows are open and none of 16.  The state as in
    tests/test_sampling_gpu.py: logp within 1e-4 max|l| of float64; finished rows write eos and keep score and length; a row
    that draws eos (eos is made the word of the first live row that is not open) becomes finished with length step + 1;
    xw = lut[word] sqrt(d) + pe_row; only column `step` of ys is written.  At p = 0.5, tau = 1 the restated word differs from
    the unrestricted draw in at least a quarter of the 300 x 1000 rows: an implementation that ignores top_p fails there."""
    x, Wt, b, logits = step_case(rows, V)
    n, step, seed = SR.N_WORDS, SR.STEP, SR.STEP_SEED
    d = NR.draw(logits, np.arange(rows), step, n, tau, p, seed)
    is_open = NR.is_open(d, logits, tau)
    fin0 = (torch.arange(rows) % 3 == 0)
    f0 = fin0.numpy()
    lmax = float(np.abs(logits).max())
    r_eos = int(np.flatnonzero(~f0 & ~is_open)[0])
    eos = int(d["word"][r_eos])
    score0 = -0.25 * torch.arange(rows, dtype=torch.float32) - 1.0
    len0 = torch.where(fin0, torch.full((rows,), 3), torch.full((rows,), step)).to(torch.int32)
    got = _Step(x, Wt, b, p, tau, seed, step, n, eos, fin0.to(torch.int32).to(DEV), score0.to(DEV), len0.to(DEV))
    word = got.words(step)
    fin, score, length = got.fin.cpu().numpy(), got.score.cpu().numpy(), got.length.cpu().numpy()
    n_open = int(is_open.sum())
    moved = int((d["word"] != d["free"]).sum())
    print(f"open rows: {n_open} of {rows}; nucleus sizes {d['size'].min()}..{d['size'].max()}; the restriction moves {moved} rows")
    assert n_open <= NR.OPEN_CAP * rows and (rows != 16 or n_open == 0)
    if (rows, V, tau, p) == (300, 1000, 1.0, 0.5):
        assert moved >= 75
    assert bool((got.ys[:, :step] == -7).all()) and bool((got.ys[:, step + 1:] == -7).all())
    assert ((word >= 0) & (word < V)).all()
    live = ~f0
    exact = live & ~is_open
    assert np.array_equal(word[exact], d["word"][exact])
    assert NR.allowed(d, logits, tau, word)[live].all()
    # finished rows
    assert (word[f0] == eos).all() and np.array_equal(score[f0], score0.numpy()[f0]) and np.array_equal(length[f0], len0.numpy()[f0])
    assert (fin[f0] == 1).all()
    # live rows: logp of the word the device drew (untempered, untruncated), length, finished
    m = logits.max(1)
    logp = logits[np.arange(rows), word] - (m + np.log(np.exp(logits - m[:, None]).sum(1)))
    err = float(np.abs((score.astype(np.float64) - score0.numpy().astype(np.float64)) - logp)[live].max())
    print(f"largest |logp - float64| = {err:.3g} (bound {1e-4 * lmax:.3g} + the rounding of the float32 sum)")
    assert err <= 1e-4 * lmax + 2.0 ** -24 * float(np.abs(score[live]).max())
    assert (length[live] == step + 1).all() and np.array_equal(fin[live] == 1, word[live] == eos)
    assert fin[r_eos] == 1 and word[r_eos] == eos and length[r_eos] == step + 1  # that row drew eos now
    wd = torch.from_numpy(word).to(DEV)
    assert torch.equal(got.xw, got.lut[wd] * got.scale + got.pe)


def test_the_largest_vocabulary_the_entry_takes():
    """V = 16 384: the row fills 128 KB of LDS.  Three rows against the restatement."""
    rows, V, tau, p = 3, 16384, 1.0, 0.9
    g = torch.Generator().manual_seed(9)
    x = torch.randn(rows, 128, generator=g)
    Wt, b = 0.3 * torch.randn(V, 128, generator=g), torch.randn(V, generator=g)
    logits = (x.double() @ Wt.double().t() + b.double()).numpy()
    d = NR.draw(logits, np.arange(rows), 0, SR.N_WORDS, tau, p, SR.STEP_SEED)
    got = _Step(x.to(DEV), Wt.to(DEV), b.to(DEV), p, tau, SR.STEP_SEED, 0, SR.N_WORDS, SR.EOS)
    word = got.words(0)
    print(f"nucleus sizes {d['size'].tolist()}, words {word.tolist()}, restated {d['word'].tolist()}, open {NR.is_open(d, logits, tau).tolist()}")
    assert NR.allowed(d, logits, tau, word).all()


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------------
def test_tied_words_enter_the_nucleus_together():
    """Every word has the same weight row and words 0-1, 2-4 and 5-9 one bias each, so the logits of a group are bit-identical in
    every row (the rows differ by one constant).  q = (.3 .3 .1 .1 .1 .02 x 5), p = 0.7: the three tied words at A = 0.6 carry the
    mass to 0.9 together -- all three are drawn, at their share of the renormalised nucleus, and no tail word ever."""
    bias, p, tied, tail = NR.tie_case()
    R, V = 400, len(bias)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(R, 128, generator=g)
    Wt = (0.3 * torch.randn(1, 128, generator=g)).expand(V, 128).contiguous()
    b = torch.from_numpy(bias)
    logits = (x.double() @ Wt.double().t() + b.double()).numpy()
    inside = NR.nucleus(logits, 1.0, p)
    assert (inside == (np.arange(V) < 5)).all()                              # by the restatement: words 0..4 in every row
    A = NR.mass_above(logits, 1.0)
    assert (np.abs(A - p) >= 0.05).all() and (np.abs(np.array([0.0, 0.6, 0.9, 1.0]) - p) >= 0.05).all()
    got = _Step(x.to(DEV), Wt.to(DEV), b.to(DEV), p, 1.0, SR.STEP_SEED, SR.STEP, SR.N_WORDS, SR.EOS)
    cnt = np.bincount(got.words(SR.STEP), minlength=V)
    print(f"draws per word: {cnt.tolist()}")
    assert cnt[list(tail)].sum() == 0 and (cnt[list(tied)] >= 20).all() and (cnt[:2] >= 80).all()      # expected 44 and 133 each
    d = NR.draw(logits, np.arange(R), SR.STEP, SR.N_WORDS, 1.0, p, SR.STEP_SEED)
    sure = ~NR.is_open(d, logits, 1.0)
    assert sure.mean() > 0.95 and np.array_equal(got.words(SR.STEP)[sure], d["word"][sure])


# ---- 3. p -> 0 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,V", [(300, 1000), (33, 3001)])
def test_a_vanishing_nucleus_is_the_greedy_word(step_case, rows, V):
    """top_p = 1e-6 keeps the most probable word alone: spacap_decode_word_f32's word on every row whose two best logits are
    further apart than 1e-4 max|l|, whatever the noise and the temperature."""
    from spacap3d_amd.linear import bf3_pieces
    lib, check, st = _lib()
    x, Wt, b, logits = step_case(rows, V)
    got = _Step(x, Wt, b, 1e-6, 0.7, SR.STEP_SEED, SR.STEP, SR.N_WORDS, SR.EOS)
    ys = torch.full((rows, 1), -7, dtype=torch.long, device=DEV)
    xn = torch.empty(rows, 128, device=DEV)
    ws = torch.empty(int(lib.spacap_decode_word_workspace_bytes(rows, V)), dtype=torch.uint8, device=DEV)
    check(lib.spacap_decode_word_f32(x.data_ptr(), bf3_pieces(Wt).data_ptr(), b.data_ptr(), rows, V, got.lut.data_ptr(), got.scale,
                                     got.pe.data_ptr(), ys.data_ptr(), 1, 0, xn.data_ptr(), ws.data_ptr(), st), "spacap_decode_word_f32")
    top = np.sort(logits, 1)[:, -2:]
    clear = top[:, 1] - top[:, 0] > 1e-4 * float(np.abs(logits).max())
    assert clear.mean() > 0.9
    assert np.array_equal(got.words(SR.STEP)[clear], ys[:, 0].cpu().numpy()[clear])
    assert np.array_equal(got.words(SR.STEP)[clear], logits.argmax(1)[clear])


# ---- 4. containment --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau,p", [(1.0, 0.5), (0.7, 0.9)])
def test_an_unrestricted_draw_inside_the_nucleus_is_kept(step_case, tau, p):
    """The noise is spacap_sample_word_f32's: a row whose top_k = 0 word (on the device, same seed) lies in the restated nucleus
    draws that same word.  Open rows (by either restatement) are left out; a good share of the rows is on each side."""
    rows, V = 300, 1000
    x, Wt, b, logits = step_case(rows, V)
    free = _Step(x, Wt, b, None, tau, SR.STEP_SEED, SR.STEP, SR.N_WORDS, SR.EOS).words(SR.STEP)
    got = _Step(x, Wt, b, p, tau, SR.STEP_SEED, SR.STEP, SR.N_WORDS, SR.EOS).words(SR.STEP)
    d = NR.draw(logits, np.arange(rows), SR.STEP, SR.N_WORDS, tau, p, SR.STEP_SEED)
    f = SR.draw(logits, np.arange(rows), SR.STEP, SR.N_WORDS, tau, 0, SR.STEP_SEED)
    sure = ~NR.is_open(d, logits, tau) & (f["gap"] >= SR.tolerance(logits, tau))
    kept = d["inside"][np.arange(rows), free] & sure
    print(f"{int(kept.sum())} of {rows} unrestricted draws lie in the nucleus; {int((sure & ~kept).sum())} do not")
    assert kept.sum() >= 0.2 * rows and (sure & ~kept).sum() >= 0.05 * rows
    assert np.array_equal(got[kept], free[kept])
    assert (got[sure & ~kept] != free[sure & ~kept]).all() and d["inside"][np.arange(rows), got][sure].all()


# ---- 5. the distribution ---------------------------------------------------------------------------------------------------------
def test_device_draws_follow_the_renormalised_nucleus():
    """As tests/test_sampling_gpu.py's chi-square cases: 4 096 rows share one x row (zero: the logits are the bias) and differ
    through rho only.  p lies mid-way between the cumulative masses of the 7 and the 8 most probable of 16 words: every draw is
    one of the 8 (chi_square asserts it) and Pearson's statistic against q renormalised on them stays under the 99.9 %
    quantile of chi-square with 7 degrees of freedom."""
    name, R, logits, tau, _, _ = SR.chi_cases()[0]
    b = torch.from_numpy(logits).float()
    l32 = b.double().numpy()
    cum = np.cumsum(np.sort(SR.target(l32, tau, 0))[::-1])
    p = float(0.5 * (cum[6] + cum[7]))
    inside = NR.nucleus(l32[None, :], tau, p)[0]
    assert inside.sum() == 8
    q = np.where(inside, SR.target(l32, tau, 0), 0.0)
    q /= q.sum()
    V = len(logits)
    x, Wt = torch.zeros(R, 128, device=DEV), (0.3 * torch.randn(V, 128, generator=torch.Generator().manual_seed(2))).to(DEV)
    got = _Step(x, Wt, b.to(DEV), p, tau, SR.STEP_SEED, SR.STEP, SR.N_WORDS, 0)
    chi, least = SR.chi_square(got.words(SR.STEP), q)
    print(f"{name}, p = {p:.4f}: chi-square {chi:.1f} (bar 24.32), smallest expected count {least:.1f}")
    assert least >= 5 and chi < 24.32


# ---- 6. the seed's device word, and capture --------------------------------------------------------------------------------------
def test_the_device_word_of_the_seed_is_mixed_in(step_case):
    """seed_dev as for spacap_sample_word_f32: the restated draws at that counter, and others than without it."""
    rows, V, tau, p = 37, 40, 1.0, 0.9
    x, Wt, b, logits = step_case(rows, V)
    words = {}
    for counter in (None, 3):
        got = _Step(x, Wt, b, p, tau, SR.STEP_SEED, 0, SR.N_WORDS, SR.EOS, counter=counter)
        d = NR.draw(logits, np.arange(rows), 0, SR.N_WORDS, tau, p, SR.STEP_SEED, counter)
        sure = ~NR.is_open(d, logits, tau)
        words[counter] = got.words(0)
        assert sure.sum() >= 0.9 * rows and np.array_equal(words[counter][sure], d["word"][sure])
    assert (words[None] != words[3]).mean() > 0.25


def test_one_captured_call_replays_on_new_inputs_and_an_advanced_counter(step_case):
    """The entry reads no value back and launches into the capturing stream: one captured call, replayed after x and the device
    word of the seed were rewritten in place, gives the eager call's words, scores and next input rows, bit for bit."""
    from spacap3d_amd.linear import bf3_pieces
    lib, check, _ = _lib()
    rows, V, tau, p, n = 37, 40, 0.7, 0.5, SR.N_WORDS
    x0, Wt, b, _ = step_case(rows, V)
    Wp = bf3_pieces(Wt)
    g = torch.Generator().manual_seed(1)
    lut, pe = torch.randn(V, 128, generator=g).to(DEV), torch.randn(128, generator=g).to(DEV)
    ws = torch.empty(int(lib.spacap_sample_word_nucleus_workspace_bytes(rows, V)), dtype=torch.uint8, device=DEV)

    def state():
        return (torch.full((rows, n), -7, dtype=torch.long, device=DEV), torch.zeros(rows, device=DEV),
                torch.zeros(rows, dtype=torch.int32, device=DEV), torch.zeros(rows, dtype=torch.int32, device=DEV),
                torch.full((rows, 128), float("nan"), device=DEV))

    def call(x, cnt, ys, score, length, fin, xw):
        check(lib.spacap_sample_word_nucleus_f32(x.data_ptr(), Wp.data_ptr(), b.data_ptr(), rows, V, p, 1.0 / tau, SR.STEP_SEED, cnt.data_ptr(),
                                                 n, 2, SR.EOS, lut.data_ptr(), 1.0, pe.data_ptr(), ys.data_ptr(), score.data_ptr(),
                                                 length.data_ptr(), fin.data_ptr(), xw.data_ptr(), ws.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream), "spacap_sample_word_nucleus_f32")

    x, cnt = x0.clone(), torch.tensor([0], dtype=torch.int64, device=DEV)
    static = state()
    call(x, cnt, *state())                                  # the first call of the process happens outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(x, cnt, *static)
    seen = []
    for counter, xs in ((0, x0), (5, x0), (5, x0.flip(0).contiguous())):
        x.copy_(xs)
        cnt.fill_(counter)
        for t in static[1:4]:                               # score, length, finished: a fresh row state, as the eager call's
            t.zero_()
        graph.replay()
        eager = state()
        call(x, cnt, *eager)
        torch.cuda.synchronize()
        assert torch.equal(static[0], eager[0]) and torch.equal(static[1], eager[1]) and torch.equal(static[4], eager[4])
        assert bool((static[0][:, 2] >= 0).all())
        seen.append(static[0][:, 2].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ---- 7. the decoder --------------------------------------------------------------------------------------------------------------
SEED = 0
SAMPLE_SEED = 20261021
TOP_P, N_SAMPLES = 0.8, 3


@pytest.fixture(scope="module")
def scene():
    """The model and the two scenes of tests/test_sampling_gpu.py (shared, not modified)."""
    from spacap3d_amd.engine import synthetic_batch
    from spacap3d_amd.spacapnet import build_default
    torch.manual_seed(SEED)
    model = build_default(vocab_size=120, num_proposal=32, N=2, d_ff=256).to(DEV).eval()
    data = synthetic_batch(2, 4096, DEV, seed=1, vocab=120)
    with torch.no_grad():
        d = model(dict(data), is_eval=True)
    return model, data, d


def _float64_logits(cap, d, tokens):
    """sampling_restated.teacher_forced_logits of ``tokens`` (rows, n) on the CPU oracle backend in double precision"""
    from oracle.attention_ref import OracleBackend
    from spacap3d_amd import backend
    cap64 = copy.deepcopy(cap).cpu().double()
    d64 = {k: (v.cpu().double() if v.is_floating_point() else v.cpu()) for k, v in d.items() if torch.is_tensor(v)}
    with backend.use_backend(OracleBackend()), torch.no_grad():
        return SR.teacher_forced_logits(cap64, d64, tokens.cpu()).numpy()


KEYS = ("lang_cap", "lang_cap_score", "lang_cap_samples", "lang_cap_sample_scores", "lang_cap_sample_lengths")


def test_forward_eval_draws_from_every_rows_own_nucleus(scene):
    """forward_eval(num_samples=3, top_p=0.8) takes the fused path; every row's own prefix, teacher-forced in float64 and
    replayed (nucleus_restated.replay): every step that is not open reproduces the sampled word, no word lies outside the nucleus
    of p (1 + delta), and at most 1 % of the live row-steps are open, the bar of tests/test_sampling.py's replay (so that the
    replay checks something.  A bar per ROW would have to allow for 31 steps each: an untrained model's 120 logits are nearly
    flat, about a hundred cumulative masses lie in (0, 1) and the window p (1 +- delta) is about 1e-3 wide, so a row meets a
    boundary inside it every few hundred steps -- 12 of these 192 rows hold an open step, by the restatement alone); lengths, eos padding and the scores (the float64 sums, within
    1e-3) as for every other mode; a second call is bit-equal; and the restriction matters: in a good share of the live steps
    the unrestricted draw would have left the nucleus."""
    model, data, d = scene
    cap = model.caption
    eos = cap.word_to_idx["eos"]
    kw = dict(num_samples=N_SAMPLES, top_p=TOP_P, sample_seed=SAMPLE_SEED)
    try:
        with torch.no_grad():
            cap.last_sample_trace = {"untouched": True}
            out = {k: v.clone() for k, v in cap.forward_eval(dict(d), **kw).items() if k in KEYS}
            assert cap.last_sample_trace is None, "forward_eval did not take caption_decode.sample_decode"
            again = cap.forward_eval(dict(d), **kw)
    finally:
        cap.__dict__.pop("last_sample_trace", None)
    B, K, n = d["lang_cap"].shape
    s = out["lang_cap_samples"]
    assert s.shape == (B, K, N_SAMPLES, n) and s.dtype == torch.long and torch.equal(out["lang_cap"], s[:, :, 0])
    assert out["lang_cap_sample_scores"].shape == (B, K, N_SAMPLES) and out["lang_cap_sample_lengths"].dtype == torch.int32
    assert torch.equal(out["lang_cap_score"], out["lang_cap_sample_scores"][:, :, 0])
    for k in KEYS:
        assert torch.equal(again[k], out[k]), k
    rows = B * K * N_SAMPLES
    logits = _float64_logits(cap, d, s.reshape(rows, n))
    rp = NR.replay(s.reshape(rows, n).cpu().numpy(), logits, 1.0, TOP_P, SAMPLE_SEED, eos)
    print(f"replay: wrong {rp['wrong']}; outside {rp['outside']}; rows with an open step: {len(rp['open_rows'])} of {rows}; open steps: "
          f"{rp['open_steps']} of {rp['live_steps']}; {rp['left']} unrestricted draws would have left the nucleus")
    assert not rp["wrong"] and not rp["outside"] and rp["padded"]
    assert rp["open_steps"] <= 0.01 * rp["live_steps"]
    assert rp["left"] >= 0.1 * rp["live_steps"]
    assert np.array_equal(out["lang_cap_sample_lengths"].reshape(-1).cpu().numpy(), rp["length"])
    err = float(np.abs(out["lang_cap_sample_scores"].reshape(-1).double().cpu().numpy() - rp["score"]).max())
    print(f"largest |score - float64 teacher-forced score| = {err:.3g} (scores down to {rp['score'].min():.1f})")
    assert err < 1e-3


def test_no_top_p_and_top_p_one_are_the_unrestricted_sampler_bit_for_bit(scene):
    """sample_decode called as before the argument existed, with top_p=None and with top_p=1.0: the same words, scores and
    lengths, at top_k = 0 and at top_k = 3."""
    from spacap3d_amd import caption_decode as cd
    model, data, d = scene
    cap = model.caption
    sos, eos = cap.word_to_idx["sos"], cap.word_to_idx["eos"]
    te, dec, gen = cap.model.tgt_embed, cap.model.decoder, cap.model.generator
    feat = d["aggregated_vote_features"]
    ind = feat.reshape(-1, feat.shape[-1])[:48].contiguous()
    for k in (3, 0):
        old = cd.sample_decode(dec, gen, te[0], te[1].pe, ind, sos, eos, 31, 2, 0.8, k, SAMPLE_SEED)
        for p in (None, 1.0):
            new = cd.sample_decode(dec, gen, te[0], te[1].pe, ind, sos, eos, 31, 2, 0.8, k, SAMPLE_SEED, top_p=p)
            assert all(torch.equal(a, b) for a, b in zip(old, new)), (k, p)
    narrow = cd.sample_decode(dec, gen, te[0], te[1].pe, ind, sos, eos, 31, 2, 0.8, 0, SAMPLE_SEED, top_p=0.5)
    assert narrow[0].shape == old[0].shape and not torch.equal(narrow[0], old[0])      # (another mode: other words than top_k = 0)
    with pytest.raises(ValueError):
        cd.sample_decode(dec, gen, te[0], te[1].pe, ind, sos, eos, 31, 2, 0.8, 3, SAMPLE_SEED, top_p=0.5)


def test_evaluator_pipeline_with_top_p(scene):
    """Evaluator(..., sample=dict(num_samples=2, top_p=0.8, seed=5)) under graph capture: the sample outputs keep their names
    and shapes, lang_cap is sample 0, and a second call repeats the seeded draws."""
    from spacap3d_amd.engine import Evaluator, synthetic_batch
    model = scene[0]
    cap = model.caption
    batch = {"point_clouds": synthetic_batch(2, 4096, DEV, seed=1, vocab=120)["point_clouds"]}
    try:
        ev = Evaluator(model, graph=True, sample=dict(num_samples=2, top_p=TOP_P, seed=5))
        assert cap.top_p == TOP_P and cap.top_k == 0
        first = {k: v.clone() for k, v in ev(dict(batch)).items() if k in KEYS}
        second = ev(dict(batch))
        torch.cuda.synchronize()
        assert first["lang_cap_samples"].shape == (2, 32, 2, 31) and first["lang_cap"].shape == (2, 32, 31)
        assert torch.equal(first["lang_cap"], first["lang_cap_samples"][:, :, 0])
        assert bool(torch.isfinite(first["lang_cap_sample_scores"]).all()) and bool((first["lang_cap_sample_scores"] <= 0).all())
        for k in KEYS:
            assert torch.equal(first[k], second[k]), k
    finally:
        for k in ("num_samples", "temperature", "top_k", "top_p", "sample_seed"):
            cap.__dict__.pop(k, None)


# ---- 8. self-critical training ---------------------------------------------------------------------------------------------------
def _random_corpus(cap, keys):
    idx2word = {i: w for w, i in cap.word_to_idx.items()}
    rng = np.random.default_rng(3)
    return {"k%d" % i: ["sos " + " ".join(idx2word[int(t)] for t in rng.integers(4, 120, 12)) + " eos" for _ in range(2)] for i in range(keys)}


def test_self_critical_step_samples_from_the_nucleus(scene):
    """SelfCritical(top_p=0.6), one eager training forward + backward on a copy of the captioner (train() mode, dropout 0): the
    loss is finite, gradients reach the generator, and scst_samples -- replayed on their own float64 teacher-forced logits at
    the matched proposals -- are the restated nucleus draws: nothing wrong, nothing outside the nucleus, while a good share of
    the unrestricted draws would have left it."""
    from spacap3d_amd.caption_eval import CaptionCorpus
    from spacap3d_amd.self_critical import SelfCritical
    model, data, d = scene
    cap = copy.deepcopy(model.caption).train()
    for m in cap.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    twin = copy.deepcopy(cap)          # train() mode as well: the source embedding normalises with the batch's statistics
    B, K, _ = d["aggregated_vote_features"].shape
    ep = {k: v.detach() for k, v in d.items() if torch.is_tensor(v) and not k.startswith("lang_cap")}
    ep["dataset_idx"] = torch.arange(B, device=DEV).view(B, 1)
    ep["object_id"] = torch.arange(B, device=DEV) + 3
    sos, eos = cap.word_to_idx["sos"], cap.word_to_idx["eos"]
    table = np.full((B, B + 3), -1, np.int32)
    for b in range(B):
        table[b, b + 3] = b
    p, S, seed = 0.6, 3, 77
    cap.self_critical = SelfCritical(CaptionCorpus(_random_corpus(cap, B), cap.word_to_idx, key_of=table), sos, eos, num_samples=S, seed=seed,
                                     top_p=p)
    out = cap.forward_train(dict(ep))
    loss = out["_cap_loss"][0]
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(cap.model.generator.proj.weight.grad).all())
    samples = out["scst_samples"]
    n = samples.shape[-1]
    assert samples.shape == (B, S, n)
    allrows = torch.full((B, K, S, n), sos, dtype=torch.long)
    mi = out["match_idx"].cpu()
    for b in range(B):
        allrows[b, mi[b]] = samples[b].cpu()
    tf = _float64_logits(twin, ep, allrows.view(-1, n)).reshape(B, K, S, n, -1)
    logits = np.stack([tf[b, int(mi[b])] for b in range(B)]).reshape(B * S, n, -1)
    # the noise index of a sample row is its row among the B S rows that were drawn
    rp = NR.replay(samples.reshape(B * S, n).cpu().numpy(), logits, 1.0, p, seed, eos)
    print(f"loss {float(loss.detach()):.4f}; replay: wrong {rp['wrong']}; outside {rp['outside']}; open rows {sorted(rp['open_rows'])}; "
          f"{rp['left']} of {rp['live_steps']} unrestricted draws would have left the nucleus")
    assert not rp["wrong"] and not rp["outside"] and rp["padded"]
    assert rp["left"] >= 0.1 * rp["live_steps"]


def test_self_critical_hands_top_p_to_its_sampler_in_matched_mode(monkeypatch):
    """proposals="matched": one eager Trainer step with finite losses, and sample_decode received the sampler's top_p."""
    from spacap3d_amd import caption_decode as cd
    from spacap3d_amd import synthetic as SY
    from spacap3d_amd.caption_eval import CaptionCorpus
    from spacap3d_amd.engine import Trainer, synthetic_batch
    from spacap3d_amd.self_critical import SelfCritical
    from spacap3d_amd.spacapnet import build_default
    torch.manual_seed(0)
    model = build_default(vocab_size=120, num_proposal=32, N=2, d_ff=256).to(DEV).train()
    data = synthetic_batch(2, 4096, DEV, seed=0, vocab=120)
    with torch.no_grad():
        probe = model(dict(data))
    data = SY.anchor_boxes_on_proposals(data, probe["aggregated_vote_xyz"])
    B, G = data["box_label_mask"].shape
    off = 5
    data["dataset_idx"] = torch.arange(B, device=DEV)
    data["scene_object_ids"] = (torch.arange(G, device=DEV) + off).repeat(B, 1)
    cap = model.caption
    table = np.full((B, G + off), -1, np.int32)
    for i in range(2 * B):
        table[i % B, off + 2 * (i // B)] = i
    cap.self_critical = SelfCritical(CaptionCorpus(_random_corpus(cap, 2 * B), cap.word_to_idx, key_of=table), cap.word_to_idx["sos"],
                                     cap.word_to_idx["eos"], num_samples=3, seed=11, proposals="matched", max_proposals=3, top_p=0.5)
    seen = []
    real = cd.sample_decode

    def spy(*a, **kw):
        seen.append(a[12] if len(a) > 12 else kw.get("top_p"))
        return real(*a, **kw)
    monkeypatch.setattr(cd, "sample_decode", spy)
    tr = Trainer(model, SY.mean_size_arr().numpy())
    tr.step(data)
    losses = {k: float(v) for k, v in tr.last_losses.items()}
    print(f"one eager matched self-critical step at top_p = 0.5: {losses}")
    assert seen and all(v == 0.5 for v in seen) and tr.graph is None       # (every decode of the step)
    assert all(np.isfinite(v) for v in losses.values())
