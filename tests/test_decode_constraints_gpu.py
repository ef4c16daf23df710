"""Constrained caption decoding on the MI355X (csrc/caption_decode.hip: decode_constraint_kernel and the
*_constrained word kernels, caption_decode.*_decode(constraints=), transformer_captioner.forward_eval) against the numpy restatement
(tests/decode_constraints_restated.py), the generic path (decode_constraints.apply inside beam_search / sampling) and itself with
everything off.  The restatement, the refusals and the generic path on the CPU: tests/test_decode_constraints_cpu.py, which also
holds the inputs of the one-step tests below to at most 2 % open rows."""
import ctypes
import math

import numpy as np
import pytest
import torch

import decode_constraints_restated as CR
import sampling_restated as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEP, N = CR.STEP, CR.N_WORDS


@pytest.fixture(autouse=True, scope="module")
def _needs_a_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _lib():
    from spacap3d_amd._native import check, lib
    return lib, check, torch.cuda.current_stream().cuda_stream


def _ys_of(hist, rows):
    """ys (rows, N) poisoned with -7 behind the history's columns"""
    ys = torch.full((rows, N), -7, dtype=torch.long)
    ys[:, :hist.shape[1]] = torch.from_numpy(hist)
    return ys.to(DEV)


def _images(ys, V, eos, c, step=STEP, trace_word=None, anc=None, R=None, W=1, T=N + 1):
    """spacap_decode_constraints into a poisoned buffer -> uint32 (rows, 2, nw) on the host"""
    lib, check, st = _lib()
    rows = ys.shape[0] if ys is not None else anc.shape[0]
    R = rows // W if R is None else R
    nw = CR.image_words(V)
    assert int(lib.spacap_decode_constraints_bytes(rows, V)) == rows * 2 * nw * 4
    bits = torch.full((rows * 2 * nw,), -1, dtype=torch.int32, device=DEV)
    bad = (ctypes.c_int32 * max(len(c["bad_words"]), 1))(*c["bad_words"])
    check(lib.spacap_decode_constraints(None if ys is None else ys.data_ptr(), 0 if ys is None else ys.shape[1],
                                        None if trace_word is None else trace_word.data_ptr(), None if anc is None else anc.data_ptr(),
                                        R, W, T, V, step, eos, c["min_length"], c["ngram"], bad, len(c["bad_words"]), bits.data_ptr(), st),
          "spacap_decode_constraints")
    torch.cuda.synchronize()
    return bits


def _host(bits, rows, V):
    return bits.cpu().numpy().view(np.uint32).reshape(rows, 2, CR.image_words(V))


class _Env:
    """A case on the device: x, the weight's pieces, bias, a random embedding table and sinusoid row, ys with the planted
    history, the images (checked against the restatement bit for bit) -- once per shape and case."""

    def __init__(self, case):
        from spacap3d_amd.linear import bf3_pieces
        self.case = case
        self.rows, self.V = case["logits"].shape
        self.x, self.b = case["x"].to(DEV), case["b"].to(DEV)
        self.Wp = bf3_pieces(case["Wt"].to(DEV))
        g = torch.Generator().manual_seed(1)
        self.lut, self.pe = torch.randn(self.V, 128, generator=g).to(DEV), torch.randn(128, generator=g).to(DEV)
        self.scale = math.sqrt(128.0)
        self.ys0 = _ys_of(case["hist"], self.rows)
        self.bits = _images(self.ys0, self.V, case["eos"], case["c"])
        want = CR.images(case["hist"], STEP, self.V, case["eos"], **case["c"])
        assert np.array_equal(_host(self.bits, self.rows, self.V), want)
        self.theta = float(case["c"]["theta"])

    def word(self):
        """spacap_decode_word_constrained_f32 on poisoned outputs -> (ys, xw)"""
        lib, check, st = _lib()
        ys, xw = self.ys0.clone(), torch.full((self.rows, 128), float("nan"), device=DEV)
        ws = torch.empty(int(lib.spacap_decode_word_workspace_bytes(self.rows, self.V)), dtype=torch.uint8, device=DEV)
        check(lib.spacap_decode_word_constrained_f32(self.x.data_ptr(), self.Wp.data_ptr(), self.b.data_ptr(), self.rows, self.V,
                                                     self.bits.data_ptr(), self.theta, self.lut.data_ptr(), self.scale, self.pe.data_ptr(),
                                                     ys.data_ptr(), N, STEP, xw.data_ptr(), ws.data_ptr(), st),
              "spacap_decode_word_constrained_f32")
        torch.cuda.synchronize()
        return ys, xw

    def topw(self, W):
        lib, check, st = _lib()
        lp = torch.full((self.rows, W), float("nan"), device=DEV)
        wd = torch.full((self.rows, W), -7, dtype=torch.int32, device=DEV)
        ws = torch.empty(int(lib.spacap_beam_topw_workspace_bytes(self.rows, self.V, W)), dtype=torch.uint8, device=DEV)
        check(lib.spacap_beam_topw_constrained_f32(self.x.data_ptr(), self.Wp.data_ptr(), self.b.data_ptr(), self.rows, self.V, W,
                                                   self.bits.data_ptr(), self.theta, lp.data_ptr(), wd.data_ptr(), ws.data_ptr(), st),
              "spacap_beam_topw_constrained_f32")
        torch.cuda.synchronize()
        return lp.cpu().numpy().astype(np.float64), wd.cpu().numpy()

    def sample(self, tau, top_k, top_p, seed, fin, score, length):
        lib, check, st = _lib()
        ys, xw = self.ys0.clone(), torch.full((self.rows, 128), float("nan"), device=DEV)
        fin, score, length = fin.clone(), score.clone(), length.clone()
        tail = (seed, None, N, STEP, self.case["eos"], self.bits.data_ptr(), self.theta, self.lut.data_ptr(), self.scale, self.pe.data_ptr(),
                ys.data_ptr(), score.data_ptr(), length.data_ptr(), fin.data_ptr(), xw.data_ptr())
        if top_p is None:
            ws = torch.empty(int(lib.spacap_sample_word_workspace_bytes(self.rows, self.V, top_k)), dtype=torch.uint8, device=DEV)
            check(lib.spacap_sample_word_constrained_f32(self.x.data_ptr(), self.Wp.data_ptr(), self.b.data_ptr(), self.rows, self.V, top_k,
                                                         1.0 / tau, *tail, ws.data_ptr(), st), "spacap_sample_word_constrained_f32")
        else:
            ws = torch.empty(int(lib.spacap_sample_word_nucleus_workspace_bytes(self.rows, self.V)), dtype=torch.uint8, device=DEV)
            check(lib.spacap_sample_word_nucleus_constrained_f32(self.x.data_ptr(), self.Wp.data_ptr(), self.b.data_ptr(), self.rows, self.V,
                                                                 top_p, 1.0 / tau, *tail, ws.data_ptr(), st),
                  "spacap_sample_word_nucleus_constrained_f32")
        torch.cuda.synchronize()
        return ys, xw, fin, score, length


@pytest.fixture(scope="module")
def env():
    made = {}

    def get(rows, V, kind="ngram"):
        if (rows, V, kind) not in made:
            case = CR.step_case(rows, V, CR.NGRAM_OF[(rows, V)]) if kind == "ngram" else CR.penalty_case(rows, V)
            made[(rows, V, kind)] = _Env(case)
        return made[(rows, V, kind)]
    return get


# ---- 1. one step through the C ABI: the arg-max variant --------------------------------------------------------------------------
def _check_words(word, z, exact_only=None):
    """every row takes the best allowed word of z'; a row whose two best lie within the tolerance one of the two"""
    rows = z.shape[0]
    near = CR.top2_gap(z) < CR.tolerance(z, 1.0)
    order = np.argsort(-z, axis=1, kind="stable")
    assert np.isfinite(z[np.arange(rows), word]).all(), "a banned word was chosen"
    assert np.array_equal(word[~near], order[~near, 0])
    assert ((word[near] == order[near, 0]) | (word[near] == order[near, 1])).all()
    return int(near.sum())


@pytest.mark.parametrize("rows,V", CR.STEP_SHAPES)
def test_constrained_argmax_against_the_restatement(env, rows, V):
    """Step 5 of 31, planted histories (CR.step_case): the unconstrained arg-max of every even row is banned by the n-gram rule,
    eos by min_length, word 0, V - 1 and both sides of every 64-word chunk edge (= slice edge) through bad_words or a history.
    Every row that is not open takes the restated word -- the first maximum of z' --, an open one one of the two best; only
    column `step` of ys is written and xw = lut[word] sqrt(d) + pe."""
    e = env(rows, V)
    ys, xw = e.word()
    word = ys[:, STEP].cpu().numpy()
    n_open = _check_words(word, e.case["z"])
    print(f"open rows: {n_open} of {rows}; rows whose unconstrained arg-max is banned: "
          f"{int(np.isneginf(e.case['z'][np.arange(rows), e.case['logits'].argmax(1)]).sum())}")
    assert n_open <= 0.02 * rows
    keep = torch.ones(N, dtype=torch.bool)
    keep[STEP] = False
    assert torch.equal(ys[:, keep], e.ys0[:, keep])
    assert torch.equal(xw, e.lut[ys[:, STEP]] * e.scale + e.pe)


def test_all_but_one_word_banned_and_equal_logits():
    """V = 40, x = 0 so that the logits are the bias.  Row 0: every word but word 17 is banned -- 33 bad words, five history
    words under n = 1 and eos under min_length -- and must choose it although it has the smallest logit.  The other rows: equal
    logits at words 3, 9, 12 and 30 above every other allowed word, word 3 a bad word, word 9 in the history of the odd rows:
    the smaller allowed index wins (9 on even rows, 12 on odd ones)."""
    rows, V, eos = 19, 40, 39
    b = torch.linspace(-1.0, 1.0, V)
    b[17] = -5.0
    b[[3, 9, 12, 30]] = 2.5
    b[[0, 1, 2, 4, 5]] = 3.0                              # the largest of all: bad words
    bad = tuple(w for w in range(V) if w not in (17, eos, 9, 12, 30, 6, 7))
    assert len(bad) == 33 and 3 in bad and 0 in bad        # 33 bad words + 5 history words + eos = 39 < V
    hist = np.zeros((rows, STEP), np.int64)
    hist[0] = [9, 12, 30, 6, 7]
    hist[1::2] = [9, 6, 7, 6, 9]
    hist[2::2] = [6, 7, 6, 7, 6]
    c = dict(min_length=STEP + 1, ngram=1, theta=1.0, bad_words=bad)
    z = CR.constrain_rows(b.double().numpy()[None].repeat(rows, 0), hist, STEP, eos, **c)
    assert np.isfinite(z[0]).sum() == 1 and np.isfinite(z[0, 17])
    case = dict(x=torch.zeros(rows, 128), Wt=0.3 * torch.randn(V, 128, generator=torch.Generator().manual_seed(5)), b=b,
                logits=b.double().numpy()[None].repeat(rows, 0), eos=eos, hist=hist, c=c, z=z)
    word = _Env(case).word()[0][:, STEP].cpu().numpy()
    assert word[0] == 17
    assert (word[1::2] == 12).all() and (word[2::2] == 9).all()


@pytest.mark.parametrize("rows,V", CR.STEP_SHAPES)
def test_repetition_penalty_moves_the_argmax_where_it_must(env, rows, V):
    """theta = 1.3 alone (CR.penalty_case): an even row's history holds its unconstrained arg-max, an odd row's only its five
    worst words.  Every row takes the arg-max of the penalised logits; the odd rows that of the plain logits."""
    e = env(rows, V, "penalty")
    word = e.word()[0][:, STEP].cpu().numpy()
    z, plain = e.case["z"], e.case["logits"].argmax(1)
    n_open = _check_words(word, z)
    assert n_open <= 0.02 * rows
    moved = z.argmax(1) != plain
    print(f"the penalty moves the arg-max of {int(moved.sum())} of {(rows + 1) // 2} planted rows")
    sure = CR.top2_gap(e.case["logits"]) >= CR.tolerance(z, 1.0)
    assert np.array_equal(word[1::2][sure[1::2]], plain[1::2][sure[1::2]])
    assert rows < 16 or (moved & (word != plain)).any()


# ---- 2. the top-W variant --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", CR.TOPW_WIDTHS)
@pytest.mark.parametrize("rows,V", CR.STEP_SHAPES)
def test_constrained_top_w_against_the_restatement(env, rows, V, W):
    """The (log-probability, word) lists are those of log_softmax(z'): values within 1e-4 max|l| (the project's bound for this
    kernel's log-probabilities), no banned word in any list, W = 1 the constrained arg-max word.  A row is open when its two
    best lie within the tolerance or its W-th and (W + 1)-th entry within 1e-4 max|l| (CR.list_open): at most 2 % of the rows.
    Every other row lists exactly the restated words in the restated order.  An open row lists no word twice, and an entry
    that differs from the restated one is the restated word of a neighbouring position (the (W + 1)-th included)."""
    e = env(rows, V)
    z = e.case["z"]
    lp, wd = e.topw(W)
    want_lp, want_wd = CR.top_w(z, W)
    bound = 1e-4 * CR.lmax(z)
    n_open = int(CR.list_open(z, W).sum())
    assert n_open <= 0.02 * rows
    r = np.arange(rows)[:, None]
    real = wd != 0x7fffffff
    assert np.array_equal(real, np.isfinite(want_lp))                       # (fewer than W allowed words: -inf entries behind)
    assert np.isfinite(z[r, np.where(real, wd, 0)])[real].all(), "a banned word in a list"
    lse = CR.log_softmax(z)
    err = float(np.abs(lp[real] - lse[r, np.where(real, wd, 0)][real]).max())
    print(f"largest |logp - float64| = {err:.3g} (bound {bound:.3g}); open rows {n_open} of {rows}")
    assert err <= bound and np.isneginf(lp[~real]).all()
    is_open = CR.list_open(z, W)
    assert np.array_equal(wd[~is_open][real[~is_open]], want_wd[~is_open][real[~is_open]])
    more = CR.top_w(z, min(W + 1, V))[1]                                    # the restated order, one entry further
    for row in np.flatnonzero(is_open):
        got = wd[row][real[row]].tolist()
        assert len(set(got)) == len(got), (row, got)
        for k, word in enumerate(got):
            assert word in more[row, max(k - 1, 0):k + 2], (row, k, got, more[row].tolist())
    if W == 1:
        assert np.array_equal(wd[:, 0], e.word()[0][:, STEP].cpu().numpy())


# ---- 3. the Gumbel and nucleus variants ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau,top_k,top_p", CR.SAMPLE_MODES)
@pytest.mark.parametrize("rows,V", CR.STEP_SHAPES)
def test_constrained_draw_against_the_restatement(env, rows, V, tau, top_k, top_p):
    """Every third row finished on entry.  A live row that is not open draws the restated word from z' (an open one: see
    CR.sample_draw; at most 2 % of the rows); no row ever draws a banned word; the log-probability is log_softmax(z')[word]
    within 1e-4 max|l|; finished rows write eos and keep score and length; xw and the other columns of ys as specified."""
    e = env(rows, V)
    z, eos, seed = e.case["z"], e.case["eos"], e.case["seed"]
    d = CR.sample_draw(z, tau, top_k, top_p, seed=seed)
    fin0 = (torch.arange(rows) % 3 == 0)
    score0 = -0.25 * torch.arange(rows, dtype=torch.float32) - 1.0
    len0 = torch.where(fin0, torch.full((rows,), 3), torch.full((rows,), STEP)).to(torch.int32)
    ys, xw, fin, score, length = e.sample(tau, top_k, top_p, seed, fin0.to(torch.int32).to(DEV), score0.to(DEV), len0.to(DEV))
    word = ys[:, STEP].cpu().numpy()
    fin, score, length, f0 = fin.cpu().numpy(), score.cpu().numpy(), length.cpu().numpy(), fin0.numpy()
    live = ~f0
    n_open = int(d["open"].sum())
    print(f"open rows: {n_open} of {rows}")
    assert n_open <= 0.02 * rows
    assert np.isfinite(z[np.arange(rows), word])[live].all(), "a banned word was drawn"
    sure = live & ~d["open"]
    assert np.array_equal(word[sure], d["word"][sure])
    assert (word[f0] == eos).all() and np.array_equal(score[f0], score0.numpy()[f0]) and np.array_equal(length[f0], len0.numpy()[f0])
    assert (fin[f0] == 1).all()
    logp = d["logp"][np.arange(rows), word]
    err = float(np.abs((score.astype(np.float64) - score0.numpy().astype(np.float64)) - logp)[live].max()) if live.any() else 0.0
    bound = 1e-4 * CR.lmax(z)
    print(f"largest |logp - float64| = {err:.3g} (bound {bound:.3g} + the rounding of the float32 sum)")
    assert err <= bound + 2.0 ** -24 * float(np.abs(score).max())
    assert (length[live] == STEP + 1).all() and np.array_equal(fin[live] == 1, word[live] == eos)
    keep = torch.ones(N, dtype=torch.bool)
    keep[STEP] = False
    assert torch.equal(ys[:, keep], e.ys0[:, keep])
    assert torch.equal(xw, e.lut[ys[:, STEP]] * e.scale + e.pe)


# ---- 4. the constraint kernel alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step,n", [(0, 2), (1, 1), (2, 3), (5, 2), (9, 3), (30, 1), (30, 4)])
def test_images_of_row_histories(step, n):
    """Greedy / sampled histories (rows of ys): few distinct words, so that n-grams repeat; a vocabulary one past a chunk; 64
    bad words; rows that are no multiple of the four per workgroup.  Bit for bit, and nothing behind the buffer's words."""
    rows, V, eos = 23, 193, 7
    g = np.random.default_rng(step * 10 + n)
    hist = g.integers(0, 5, size=(rows, max(step, 1))) * 48          # words 0, 48, 96, 144, 192: every image word
    c = dict(min_length=6, ngram=n, theta=1.0, bad_words=tuple(range(100, 164)))
    got = _host(_images(_ys_of(hist[:, :step], rows), V, eos, c, step=step), rows, V)
    assert np.array_equal(got, CR.images(hist, step, V, eos, **c))


def test_a_history_word_outside_the_vocabulary_counts_as_none():
    """ys columns below `step` holding -7, V and V + 3: such a word sets no bit and matches nothing in an n-gram -- two equal
    out-of-range words are not a repeated context -- while the valid words around them keep their rule."""
    V, eos, step = 70, 1, 4
    hist = np.array([[-7, 5, -7, 9], [5, -7, 5, 9], [4, 5, 4, 9], [V, 6, V, V], [V + 3, V + 3, V + 3, V + 3], [9, 5, 9, 8], [9, 5, -7, 9]])
    for n in (1, 2, 3):
        c = dict(min_length=0, ngram=n, theta=1.0, bad_words=(69,))
        got = _host(_images(_ys_of(hist, hist.shape[0]), V, eos, c, step=step), hist.shape[0], V)
        assert np.array_equal(got, CR.images(hist, step, V, eos, **c)), n
    c = dict(min_length=0, ngram=2, theta=1.0, bad_words=())
    want = CR.images(np.array([[-7, 5, -7], [4, 5, 4]]), 3, V, eos, **c)
    assert want[0, 0].sum() == 0 and want[1, 0, 0] == 1 << 5                  # (-7, 5) after -7 bans nothing; (4, 5) after 4 bans 5
    got = _host(_images(_ys_of(np.array([[-7, 5, -7], [4, 5, 4]]), 2), V, eos, c, step=3), 2, V)
    assert np.array_equal(got, want)


def test_images_of_beam_histories_through_the_ancestor_table():
    """Beam histories: word j of hypothesis (r, w) is trace_word[j][r][slot] with the slot read from a hand-built ancestor
    table -- one hypothesis crosses slots at every position, entries outside 0..W-1 read the row's own slot -- and equal the
    images of the histories the restatement backtracks."""
    R, W, T, step, V, eos = 5, 3, N + 1, 9, 130, 2
    g = np.random.default_rng(3)
    tr = g.integers(0, 6, size=(N, R, W)).astype(np.int32) * 25                  # few words: repeats along every ancestry
    anc = g.integers(0, W, size=(R * W, T)).astype(np.int8)
    anc[4, :] = (np.arange(T) + 1) % W                                            # crosses slots at every position
    anc[7, 3], anc[7, 5], anc[8, 2] = -1, W, 100                                  # outside 0..W-1
    c = dict(min_length=0, ngram=2, theta=1.0, bad_words=(129,))
    hist = CR.beam_histories(tr, anc, step, W)
    assert (anc[4, 2:step] != anc[4, 3:step + 1]).all()
    got = _host(_images(None, V, eos, c, step=step, trace_word=torch.from_numpy(tr).to(DEV), anc=torch.from_numpy(anc).to(DEV),
                        R=R, W=W, T=T), R * W, V)
    want = CR.images(hist, step, V, eos, **c)
    assert np.array_equal(got, want) and want[:, 0].any() and want[:, 1].any()


def test_refusals_launch_nothing():
    lib, check, st = _lib()
    rows, V = 16, 40
    ys = torch.full((rows, N), 3, dtype=torch.long, device=DEV)
    bits = torch.full((rows * 2 * CR.image_words(V),), -1, dtype=torch.int32, device=DEV)
    bad = (ctypes.c_int32 * 64)(*range(64))
    ok = dict(ys=ys.data_ptr(), ys_ld=N, tr=None, anc=None, R=rows, W=1, T=N + 1, V=V, step=5, eos=1, ml=0, n=2, bad=bad, n_bad=2,
              bits=bits.data_ptr(), st=st)
    for over in (dict(step=31), dict(step=-1), dict(n_bad=65), dict(n_bad=34), dict(n=-1), dict(ml=-1), dict(eos=V), dict(W=2), dict(T=33)):
        assert lib.spacap_decode_constraints(*dict(ok, **over).values()) == -1, over
        assert b"spacap_decode_constraints" in lib.spacap_last_error()
    x, Wp, b = torch.zeros(rows, 128, device=DEV), torch.zeros(3 * V * 128, dtype=torch.bfloat16, device=DEV), torch.zeros(V, device=DEV)
    lut, pe = torch.zeros(V, 128, device=DEV), torch.zeros(128, device=DEV)
    xw, ws = torch.full((rows, 128), 5.0, device=DEV), torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    score, ln, fin = torch.full((rows,), 5.0, device=DEV), torch.full((rows,), -7, dtype=torch.int32, device=DEV), torch.zeros(
        rows, dtype=torch.int32, device=DEV)
    for theta in (0.5, float("nan")):
        assert lib.spacap_decode_word_constrained_f32(x.data_ptr(), Wp.data_ptr(), b.data_ptr(), rows, V, bits.data_ptr(), theta,
                                                      lut.data_ptr(), 1.0, pe.data_ptr(), ys.data_ptr(), N, 5, xw.data_ptr(), ws.data_ptr(), st) == -1
        assert lib.spacap_sample_word_constrained_f32(x.data_ptr(), Wp.data_ptr(), b.data_ptr(), rows, V, 0, 1.0, 7, None, N, 5, 1,
                                                      bits.data_ptr(), theta, lut.data_ptr(), 1.0, pe.data_ptr(), ys.data_ptr(), score.data_ptr(),
                                                      ln.data_ptr(), fin.data_ptr(), xw.data_ptr(), ws.data_ptr(), st) == -1
    assert lib.spacap_beam_topw_constrained_f32(x.data_ptr(), Wp.data_ptr(), b.data_ptr(), rows, V, 3, None, 1.2, xw.data_ptr(), ys.data_ptr(),
                                                ws.data_ptr(), st) == -1
    torch.cuda.synchronize()
    assert bool((bits == -1).all()) and bool((ys == 3).all()) and bool((xw == 5.0).all()) and bool((ws == 0).all())
    assert bool((score == 5.0).all()) and bool((ln == -7).all())


# ---- 5. full decodes ----------------------------------------------------------------------------------------------------------------
from test_beam_search_gpu import SCORE_TOL as BEAM_TOL, _differing  # noqa: E402
from test_sampling_gpu import SAMPLE_SEED, SCORE_TOL as SAMPLE_TOL, _first_difference  # noqa: E402

OFF = dict(min_length=0, no_repeat_ngram=0, repetition_penalty=1.0, bad_words=())
MODES = {"greedy": {}, "beam": dict(beam_size=3), "sample": dict(num_samples=3, sample_seed=SAMPLE_SEED),
         "sample_top_k": dict(num_samples=3, top_k=3, sample_seed=SAMPLE_SEED),
         "sample_top_p": dict(num_samples=3, top_p=0.6, sample_seed=SAMPLE_SEED)}


@pytest.fixture(scope="module")
def scene():
    """The model and scenes of the decoder tests (tests/test_beam_search_gpu.py / tests/test_sampling_gpu.py; shared, not modified)"""
    from spacap3d_amd.engine import synthetic_batch
    from spacap3d_amd.spacapnet import build_default
    torch.manual_seed(0)
    model = build_default(vocab_size=120, num_proposal=32, N=2, d_ff=256).to(DEV).eval()
    data = synthetic_batch(2, 4096, DEV, seed=1, vocab=120)
    with torch.no_grad():
        d = model(dict(data), is_eval=True)
    return model, data, d


def _bite(cap):
    w = cap.word_to_idx
    return dict(bad_words=(0, w["sos"], w["unk"]), min_length=4, no_repeat_ngram=2)


def _captions(out, mode):
    t = out["lang_cap_samples" if mode.startswith("sample") else "lang_cap"]
    return t.reshape(-1, t.shape[-1]).cpu().numpy()


@pytest.fixture(scope="module")
def decoded(scene):
    """forward_eval per mode, once: without the arguments, with every constraint at its off value, and with the constraints
    that bite, fused and (beam / sampling) through the generic path with its trace."""
    model, data, d = scene
    cap = model.caption
    c = _bite(cap)
    got = {}
    try:
        with torch.no_grad():
            for mode, kw in MODES.items():
                keep = lambda o: {k: v.clone() for k, v in o.items() if k.startswith("lang_cap")}  # noqa: E731
                e = dict(free=keep(cap.forward_eval(dict(d), **kw)), off=keep(cap.forward_eval(dict(d), **OFF, **kw)))
                cap.last_beam_trace = cap.last_sample_trace = None
                e["fused"] = keep(cap.forward_eval(dict(d), **c, **kw))
                if mode == "beam":
                    e["fused_trace"] = {k: v.cpu() for k, v in cap.last_beam_trace.items()}
                    assert "gap" not in e["fused_trace"], "forward_eval did not take caption_decode.beam_decode"
                    cap.beam_generic = True
                    e["generic"] = keep(cap.forward_eval(dict(d), **c, **kw))
                    e["generic_trace"] = {k: v.cpu() for k, v in cap.last_beam_trace.items()}
                    cap.beam_generic = False
                elif mode != "greedy":
                    assert cap.last_sample_trace is None, "forward_eval did not take caption_decode.sample_decode"
                    cap.sample_generic = True
                    e["generic"] = keep(cap.forward_eval(dict(d), **c, **kw))
                    e["gap"] = cap.last_sample_trace["gap"].cpu()
                    cap.sample_generic = False
                got[mode] = e
    finally:
        for k in ("beam_generic", "sample_generic", "last_beam_trace", "last_sample_trace"):
            cap.__dict__.pop(k, None)
    return got, c


@pytest.mark.parametrize("mode", list(MODES))
def test_off_is_off(decoded, mode):
    """Every constraint given at its off value: every output key bit-identical to the call without the arguments."""
    e = decoded[0][mode]
    assert set(e["free"]) == set(e["off"])
    for k in e["free"]:
        assert torch.equal(e["free"][k], e["off"][k]), k


@pytest.mark.parametrize("mode", list(MODES))
def test_constrained_captions_hold_the_invariants(scene, decoded, mode):
    """bad_words = {0, sos, unk}, min_length = 4, no_repeat_ngram = 2: read through its first eos no caption holds a bad word,
    repeats a bigram or has fewer than four words -- exactly, whatever the rounding --, and the constraints bite: the
    unconstrained captions break them and differ."""
    e, c = decoded[0][mode], decoded[1]
    eos = scene[0].caption.word_to_idx["eos"]
    kw = dict(min_length=c["min_length"], ngram=c["no_repeat_ngram"], bad_words=c["bad_words"])
    faults = CR.caption_faults(_captions(e["fused"], mode), eos, **kw)
    before = CR.caption_faults(_captions(e["free"], mode), eos, **kw)
    print(f"{mode}: {len(before)} faults without the constraints, {len(faults)} with")
    assert not faults
    assert before and not np.array_equal(_captions(e["fused"], mode), _captions(e["free"], mode))
    if mode != "greedy":
        assert bool(torch.isfinite(e["fused"]["lang_cap_score"]).all()) and bool((e["fused"]["lang_cap_score"] <= 0).all())
        assert not CR.caption_faults(_captions(e["generic"], mode), eos, **kw)


def test_fused_beam_against_the_generic_path(decoded):
    """The rule of tests/test_beam_search_gpu.py: the (parent, word) traces agree at every step, or at the first differing step
    the generic path's gap between its W-th and (W + 1)-th candidate is below that test's SCORE_TOL; scores within SCORE_TOL."""
    e = decoded[0]["beam"]
    R = e["fused"]["lang_cap"].shape[0] * e["fused"]["lang_cap"].shape[1]
    diff = _differing(e["fused_trace"], e["generic_trace"])
    print(f"fused vs generic: {len(diff)} of {R} sequences differ; gaps at the first differing step: "
          f"{[float(e['generic_trace']['gap'][s, r]) for r, s in diff]}")
    for r, s in diff:
        assert float(e["generic_trace"]["gap"][s, r]) < BEAM_TOL, (r, s)
    assert len(diff) <= 0.05 * R
    if not diff:
        assert torch.equal(e["fused"]["lang_cap"], e["generic"]["lang_cap"])
        dev_ = float((e["fused"]["lang_cap_score"] - e["generic"]["lang_cap_score"]).abs().max())
        print(f"largest |fused score - generic score| = {dev_:.3g}")
        assert dev_ <= BEAM_TOL


@pytest.mark.parametrize("mode", ["sample", "sample_top_k", "sample_top_p"])
def test_fused_sampler_against_the_generic_path(decoded, mode):
    """The rule of tests/test_sampling_gpu.py (e): rows are identical, or the first differing step is open by the generic
    path's recorded gap; at most 5 % of the rows differ; scores within 1e-3 when none does (that test's score bound)."""
    e = decoded[0][mode]
    a, b = _captions(e["fused"], mode), _captions(e["generic"], mode)
    diff = _first_difference(a, b)
    tol = SAMPLE_TOL
    print(f"{mode}: fused vs generic: {len(diff)} of {a.shape[0]} rows differ; gaps: {[float(e['gap'][s, r]) for r, s in diff]}")
    for r, s in diff:
        assert float(e["gap"][s, r]) < tol, (r, s)
    assert len(diff) <= 0.05 * a.shape[0]
    if not diff:
        assert torch.equal(e["fused"]["lang_cap_sample_lengths"], e["generic"]["lang_cap_sample_lengths"])
        assert float((e["fused"]["lang_cap_sample_scores"] - e["generic"]["lang_cap_sample_scores"]).abs().max()) <= 1e-3


def test_width_one_and_top_k_one_choose_the_constrained_greedy_words(scene, decoded):
    """A beam of width 1 and top_k = 1, both constrained, against the constrained greedy decoder: bit for bit through each
    row's first eos (behind it the greedy loop goes on; the others repeat eos)."""
    from spacap3d_amd import caption_decode as cd
    model, data, d = scene
    cap = model.caption
    c = dict(_bite(cap), repetition_penalty=1.2)
    eos, sos = cap.word_to_idx["eos"], cap.word_to_idx["sos"]
    with torch.no_grad():
        g = cap.forward_eval(dict(d), **c)["lang_cap"]
        s = cap.forward_eval(dict(d), num_samples=1, top_k=1, temperature=0.7, **c)["lang_cap"]
    n = g.shape[-1]
    g, s = g.reshape(-1, n), s.reshape(-1, n)
    is_eos = g == eos
    keep = (torch.cumsum(is_eos.long(), 1) - is_eos.long()) == 0
    assert torch.equal(s[keep], g[keep]) and bool((s[~keep] == eos).all())
    # the beam of width 1 through caption_decode on the rows the greedy decoder saw
    seen = {}
    real = cd.greedy_decode
    try:
        cd.greedy_decode = lambda *a, **k: (seen.update(a=a, k=k), real(*a, **k))[1]
        with torch.no_grad():
            g2 = cap.forward_eval(dict(d), **c)["lang_cap"].reshape(-1, n)
    finally:
        cd.greedy_decode = real
    assert torch.equal(g2, g)
    dec, gen, embed, pe, indicator, _, n_words = seen["a"]
    ys, score = cd.beam_decode(dec, gen, embed, pe, indicator, sos, eos, n_words, 1, constraints=seen["k"]["constraints"])
    assert torch.equal(ys[keep], g[keep]) and bool((ys[~keep] == eos).all())
    assert bool(torch.isfinite(score).all())


def _greedy_fused_against_generic(scene, c):
    """forward_eval with the constraints ``c``: the fused greedy decoder against the cached per-operator greedy loop
    (``_decode_rows`` with ``decode_constraints.apply``), taken on the GPU by answering ``decode_supported`` with no.  Rows
    are compared through the generic row's first eos; the greedy decoder records no gap, so a row that differs is judged by the
    gap between the two best constrained logits at its first differing step, recomputed by teacher forcing the generic
    path's prefix through the uncached decoder: below the SCORE_TOL of tests/test_beam_search_gpu.py, as its rule asks.
    Returns the fused words and the number of rows that differ (at most 5 %, that test's cap)."""
    from spacap3d_amd import caption_decode as cd
    from spacap3d_amd.decode_constraints import DecodeConstraints, apply
    model, data, d = scene
    cap = model.caption
    eos = cap.word_to_idx["eos"]
    real = cd.decode_supported
    with torch.no_grad():
        fused = cap.forward_eval(dict(d), **c)["lang_cap"]
        try:
            cd.decode_supported = lambda *a, **k: False
            gen = cap.forward_eval(dict(d), **c)["lang_cap"]
        finally:
            cd.decode_supported = real
        n = fused.shape[-1]
        a, b = fused.reshape(-1, n), gen.reshape(-1, n)
        is_eos = b == eos
        keep = (torch.cumsum(is_eos.long(), 1) - is_eos.long()) == 0
        diff = _first_difference(torch.where(keep, a, b).cpu().numpy(), b.cpu().numpy())
        if diff:
            cons = DecodeConstraints(c.get("min_length", 0), c.get("no_repeat_ngram", 0), c.get("repetition_penalty", 1.0), c.get("bad_words", ()))
            logits = SR.teacher_forced_logits(cap, d, b)
            for r, s_ in diff:
                z = apply(cons, logits[r:r + 1, s_], b[r:r + 1], s_, eos)
                top = torch.topk(z, 2, dim=1).values
                assert float(top[0, 0] - top[0, 1]) < BEAM_TOL, (r, s_)
    print(f"greedy {sorted(c)}: fused vs generic: {len(diff)} of {a.shape[0]} rows differ")
    assert len(diff) <= 0.05 * a.shape[0]
    return fused, len(diff)


def test_fused_greedy_against_the_generic_path(scene, decoded):
    """The example constraints through both greedy roads (see _greedy_fused_against_generic)."""
    fused, _ = _greedy_fused_against_generic(scene, decoded[1])
    assert torch.equal(fused, decoded[0]["greedy"]["fused"]["lang_cap"])


@pytest.mark.parametrize("mode", list(MODES))
def test_repetition_penalty_alone_fused_against_generic(scene, mode):
    """theta = 1.2 and nothing else, in every mode: the penalty changes captions, and fused equals generic under the rules
    above (beam: the trace rule; sampled modes: the recorded gap; greedy: _greedy_fused_against_generic)."""
    model, data, d = scene
    cap = model.caption
    kw = dict(MODES[mode], repetition_penalty=1.2)
    try:
        with torch.no_grad():
            free = cap.forward_eval(dict(d), **MODES[mode])
            if mode == "greedy":
                fused = {"lang_cap": _greedy_fused_against_generic(scene, dict(repetition_penalty=1.2))[0]}
            else:
                fused = cap.forward_eval(dict(d), **kw)
                ft = cap.last_beam_trace
                setattr(cap, "beam_generic" if mode == "beam" else "sample_generic", True)
                gen = cap.forward_eval(dict(d), **kw)
        assert not np.array_equal(_captions(fused, mode), _captions(free, mode))            # the penalty bites
        if mode == "beam":
            gt = {k: v.cpu() for k, v in cap.last_beam_trace.items()}
            diff = _differing({k: v.cpu() for k, v in ft.items()}, gt)
            for r, s in diff:
                assert float(gt["gap"][s, r]) < BEAM_TOL, (r, s)
            assert len(diff) <= 0.05 * gt["gap"].shape[1]
            print(f"{mode}, theta = 1.2: {len(diff)} sequences differ between fused and generic")
        elif mode != "greedy":
            gap = cap.last_sample_trace["gap"].cpu()
            diff = _first_difference(_captions(fused, mode), _captions(gen, mode))
            for r, s in diff:
                assert float(gap[s, r]) < SAMPLE_TOL, (r, s)
            assert len(diff) <= 0.05 * gap.shape[1]
            print(f"{mode}, theta = 1.2: {len(diff)} rows differ between fused and generic")
    finally:
        for k in ("beam_generic", "sample_generic", "last_beam_trace", "last_sample_trace"):
            cap.__dict__.pop(k, None)


def test_graph_capture_of_constrained_decoding(scene):
    """A constrained greedy call and a constrained sampled call (seed None) captured: replays on new inputs equal eager calls;
    the sampled replay draws new captions after advance_rng."""
    from spacap3d_amd.attention import advance_rng, rng_state
    model, data, d = scene
    cap = model.caption
    c = _bite(cap)
    eos = cap.word_to_idx["eos"]
    rng_state(torch.device(DEV))
    feats = d["aggregated_vote_features"]
    other = feats.flip(1).contiguous()
    static = dict(d)
    static["aggregated_vote_features"] = feats.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        cap.forward_eval(dict(static), **c)
        cap.forward_eval(dict(static), num_samples=2, **c)
    torch.cuda.current_stream().wait_stream(s)
    g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g1):
        out_g = cap.forward_eval(dict(static), **c)["lang_cap"]
    with torch.no_grad(), torch.cuda.graph(g2):
        out_s = cap.forward_eval(dict(static), num_samples=2, **c)["lang_cap_samples"]
    static["aggregated_vote_features"].copy_(other)
    g1.replay()
    with torch.no_grad():
        eager = cap.forward_eval(dict(d, aggregated_vote_features=other), **c)["lang_cap"]
    assert torch.equal(out_g, eager)
    assert not CR.caption_faults(out_g.reshape(-1, out_g.shape[-1]).cpu().numpy(), eos, min_length=4, ngram=2, bad_words=c["bad_words"])
    g2.replay()
    a = out_s.clone()
    g2.replay()
    b = out_s.clone()
    advance_rng(torch.device(DEV))
    g2.replay()
    cc = out_s.clone()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    changed = float((a != cc).any(-1).float().mean())
    print(f"after advance_rng {changed:.2f} of the rows changed")
    assert changed >= 0.5
    for t in (a, cc):
        assert not CR.caption_faults(t.reshape(-1, t.shape[-1]).cpu().numpy(), eos, min_length=4, ngram=2, bad_words=c["bad_words"])


def test_evaluator_with_kept_decoding_and_constraints(scene):
    """Evaluator(..., postprocess, decode="kept", constraints=...): the pred_* captions hold the invariants and lang_cap_decoded
    is that of the unconstrained run."""
    from spacap3d_amd.engine import Evaluator, synthetic_batch
    from test_postprocess_gpu import POST_DICT
    model = scene[0]
    cap = model.caption
    sos, eos = cap.word_to_idx["sos"], cap.word_to_idx["eos"]
    c = _bite(cap)
    post = dict(POST_DICT, dataset_config=None)
    batch = {"point_clouds": synthetic_batch(2, 4096, DEV, seed=1, vocab=120)["point_clouds"]}
    try:
        plain = Evaluator(model, graph=False, postprocess=post, predictions=(sos, eos), decode="kept")(dict(batch))
        plain = {k: v.clone() for k, v in plain.items() if torch.is_tensor(v)}
        out = Evaluator(model, graph=False, postprocess=post, predictions=(sos, eos), decode="kept", constraints=c)(dict(batch))
        torch.cuda.synchronize()
        assert torch.equal(out["lang_cap_decoded"], plain["lang_cap_decoded"]) and bool(out["lang_cap_decoded"].any())
        count = out["pred_count"].cpu().numpy()
        toks, ln = out["pred_tokens"].cpu().numpy(), out["pred_length"].cpu().numpy()
        n_caps = 0
        for bidx in range(toks.shape[0]):
            for j in range(int(count[bidx])):
                words = [int(t) for t in toks[bidx, j, :int(ln[bidx, j])]]
                body = [t for t in words if t not in (sos, eos)]
                assert not set(body) & set(c["bad_words"]) and not CR.repeats_ngram(body, 2) and len(body) >= c["min_length"], (bidx, j, words)
                n_caps += 1
        print(f"{n_caps} predicted captions checked")
        assert n_caps > 0
    finally:
        for k in ("min_length", "no_repeat_ngram", "repetition_penalty", "bad_words"):
            cap.__dict__.pop(k, None)
