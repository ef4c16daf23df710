"""Sampled caption decoding on the MI355X (csrc/caption_decode.hip: vocab_gumbel_kernel / sample_next_kernel,
caption_decode.sample_decode, transformer_captioner.forward_eval) against the float64 restatement of the contract
(tests/sampling_restated.py), the greedy decoder (top_k = 1) and the generic path
(spacap3d_amd/sampling.py).  The restatement itself, the C ABI's refusals and the generic path on the CPU: tests/test_sampling.py."""
import copy
import math

import numpy as np
import pytest
import torch

import sampling_restated as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HASH_SEED = 0x1234567890ABCDEF


@pytest.fixture(autouse=True, scope="module")
def _needs_a_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _lib():
    from spacap3d_amd._native import check, lib
    return lib, check, torch.cuda.current_stream().cuda_stream


class _Step:
    """One call of spacap_sample_word_f32 on poisoned outputs; the state arrays are copies of the ones given."""

    def __init__(self, x, Wt, b, top_k, tau, seed, step, n_words, eos, fin, score, length, counter=None):
        from spacap3d_amd.linear import bf3_pieces
        lib, check, st = _lib()
        rows, V = x.shape[0], Wt.shape[0]
        g = torch.Generator().manual_seed(1)
        self.lut, self.pe = torch.randn(V, 128, generator=g).to(DEV), torch.randn(128, generator=g).to(DEV)
        self.scale = math.sqrt(128.0)
        self.ys = torch.full((rows, n_words), -7, dtype=torch.long, device=DEV)
        self.xw = torch.full((rows, 128), float("nan"), device=DEV)
        self.fin, self.score, self.length = fin.clone(), score.clone(), length.clone()
        ws = torch.empty(int(lib.spacap_sample_word_workspace_bytes(rows, V, top_k)), dtype=torch.uint8, device=DEV)
        cnt = None if counter is None else torch.tensor([counter], dtype=torch.int64, device=DEV)
        check(lib.spacap_sample_word_f32(x.data_ptr(), bf3_pieces(Wt).data_ptr(), b.data_ptr(), rows, V, top_k, 1.0 / tau, seed,
                                         None if cnt is None else cnt.data_ptr(), n_words, step, eos, self.lut.data_ptr(), self.scale,
                                         self.pe.data_ptr(), self.ys.data_ptr(), self.score.data_ptr(), self.length.data_ptr(),
                                         self.fin.data_ptr(), self.xw.data_ptr(), ws.data_ptr(), st), "spacap_sample_word_f32")
        torch.cuda.synchronize()


# ---- 5. one step through the C ABI -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_case():
    """The inputs of a shape on the device, once (tests/sampling_restated.py::step_inputs)."""
    made = {}

    def get(rows, V):
        if (rows, V) not in made:
            x, Wt, b, logits = SR.step_inputs(rows, V)
            made[(rows, V)] = (x.to(DEV), Wt.to(DEV), b.to(DEV), logits)
        return made[(rows, V)]
    return get


@pytest.mark.parametrize("tau", SR.STEP_TAU)
@pytest.mark.parametrize("top_k", SR.STEP_TOP_K)
@pytest.mark.parametrize("rows,V", SR.STEP_SHAPES)
def test_one_step_against_the_restatement(step_case, rows, V, top_k, tau):
    """Step 5 of 31 with every third row finished on entry.  A row that is not open draws the restated word; an open one (best
    and second-best z within the tolerance) one of the two; with top_k a row whose k-th and (k+1)-th float64 logits are within
    1e-4 max|l| is open as well (the candidate set itself may differ); at most 2 % of the rows are open.  logp within
    1e-4 max|l| of float64; finished rows write eos and keep score and length; a row that draws eos (eos is made the word
    the restatement draws for the first live row that is not open) becomes finished with length step + 1 and its logp added; xw = lut[word] sqrt(d) + pe_row;
    only column `step` of ys is written; top_k = 1 is spacap_decode_word_f32's word."""
    x, Wt, b, logits = step_case(rows, V)
    n, step, seed = SR.N_WORDS, SR.STEP, SR.STEP_SEED
    d = SR.draw(logits, np.arange(rows), step, n, tau, top_k, seed)
    fin0 = (torch.arange(rows) % 3 == 0)
    lmax = float(np.abs(logits).max())
    near = d["gap"] < SR.tolerance(logits, tau)
    loose = d["cut"] < 1e-4 * lmax
    r_eos = int(np.flatnonzero(~fin0.numpy() & ~near & ~loose)[0])             # the first row that is neither finished nor open
    eos = int(d["word"][r_eos])
    score0 = -0.25 * torch.arange(rows, dtype=torch.float32) - 1.0
    len0 = torch.where(fin0, torch.full((rows,), 3), torch.full((rows,), step)).to(torch.int32)
    got = _Step(x, Wt, b, top_k, tau, seed, step, n, eos, fin0.to(torch.int32).to(DEV), score0.to(DEV), len0.to(DEV))
    word = got.ys[:, step].cpu().numpy()
    fin, score, length = got.fin.cpu().numpy(), got.score.cpu().numpy(), got.length.cpu().numpy()
    f0 = fin0.numpy()
    n_open = int((near | loose).sum())
    print(f"open rows: {n_open} of {rows}")
    assert n_open <= 0.02 * rows
    assert bool((got.ys[:, :step] == -7).all()) and bool((got.ys[:, step + 1:] == -7).all())
    assert ((word >= 0) & (word < V)).all()
    live = ~f0
    exact = live & ~near & ~loose
    assert np.array_equal(word[exact], d["word"][exact])
    either = live & near & ~loose
    assert ((word[either] == d["word"][either]) | (word[either] == d["second"][either])).all()
    # finished rows
    assert (word[f0] == eos).all() and np.array_equal(score[f0], score0.numpy()[f0]) and np.array_equal(length[f0], len0.numpy()[f0])
    assert (fin[f0] == 1).all()
    # live rows: logp of the word the device drew, length, finished
    m = logits.max(1)
    logp = logits[np.arange(rows), word] - (m + np.log(np.exp(logits - m[:, None]).sum(1)))
    err = float(np.abs((score.astype(np.float64) - score0.numpy().astype(np.float64)) - logp)[live].max())
    print(f"largest |logp - float64| = {err:.3g} (bound {1e-4 * lmax:.3g} + the rounding of the float32 sum)")
    assert err <= 1e-4 * lmax + 2.0 ** -24 * float(np.abs(score[live]).max())
    assert (length[live] == step + 1).all() and np.array_equal(fin[live] == 1, word[live] == eos)
    assert fin[r_eos] == 1 and word[r_eos] == eos and length[r_eos] == step + 1  # that row drew eos now
    wd = torch.from_numpy(word).to(DEV)
    assert torch.equal(got.xw, got.lut[wd] * got.scale + got.pe)
    if top_k == 1:
        from spacap3d_amd.linear import bf3_pieces
        lib, check, st = _lib()
        ys = torch.full((rows, 1), -7, dtype=torch.long, device=DEV)
        xn = torch.empty(rows, 128, device=DEV)
        ws = torch.empty(int(lib.spacap_decode_word_workspace_bytes(rows, V)), dtype=torch.uint8, device=DEV)
        check(lib.spacap_decode_word_f32(x.data_ptr(), bf3_pieces(Wt).data_ptr(), b.data_ptr(), rows, V, got.lut.data_ptr(), got.scale,
                                         got.pe.data_ptr(), ys.data_ptr(), 1, 0, xn.data_ptr(), ws.data_ptr(), st), "spacap_decode_word_f32")
        assert np.array_equal(word[live], ys[:, 0].cpu().numpy()[live])


def test_the_device_word_of_the_seed_is_mixed_in(step_case):
    """seed_dev as for dropout: seed + counter * golden ratio (mod 2^64): the restated draws at that counter, and others than
    without it in at least a quarter of the rows."""
    rows, V = 37, 40
    x, Wt, b, logits = step_case(rows, V)
    z = torch.zeros(rows, dtype=torch.int32, device=DEV)
    words = {}
    for counter in (None, 3):
        got = _Step(x, Wt, b, 0, 1.0, SR.STEP_SEED, 0, SR.N_WORDS, SR.EOS, z, torch.zeros(rows, device=DEV), z, counter=counter)
        d = SR.draw(logits, np.arange(rows), 0, SR.N_WORDS, 1.0, 0, SR.STEP_SEED, counter)
        sure = d["gap"] >= SR.tolerance(logits, 1.0)
        words[counter] = got.ys[:, 0].cpu().numpy()
        assert sure.sum() >= 0.9 * rows and np.array_equal(words[counter][sure], d["word"][sure])
    assert (words[None] != words[3]).mean() > 0.25          # (peaked rows draw their best word under any noise)


def test_sample_word_refusals_launch_nothing():
    from spacap3d_amd.linear import bf3_pieces
    lib, check, st = _lib()
    rows, V = 16, 40
    x, Wt, b = torch.zeros(rows, 128, device=DEV), torch.zeros(V, 128, device=DEV), torch.zeros(V, device=DEV)
    Wp = bf3_pieces(Wt)
    lut, pe = torch.zeros(V, 128, device=DEV), torch.zeros(128, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    ys = torch.full((rows, 31), -7, dtype=torch.long, device=DEV)
    score, xw = torch.full((rows,), 5.0, device=DEV), torch.full((rows, 128), 5.0, device=DEV)
    length, fin = torch.full((rows,), -7, dtype=torch.int32, device=DEV), torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    ok = dict(rows=rows, V=V, top_k=0, inv_tau=1.0, step=5)
    for bad in (dict(rows=-1), dict(V=0), dict(top_k=9), dict(top_k=-1), dict(V=3, top_k=4), dict(inv_tau=0.0), dict(inv_tau=float("nan")),
                dict(inv_tau=float("inf")), dict(step=31), dict(step=-1)):
        a = dict(ok, **bad)
        rc = lib.spacap_sample_word_f32(x.data_ptr(), Wp.data_ptr(), b.data_ptr(), a["rows"], a["V"], a["top_k"], a["inv_tau"], 7, None, 31,
                                        a["step"], 1, lut.data_ptr(), 1.0, pe.data_ptr(), ys.data_ptr(), score.data_ptr(), length.data_ptr(),
                                        fin.data_ptr(), xw.data_ptr(), ws.data_ptr(), st)
        assert rc == -1 and b"spacap_sample_word_f32" in lib.spacap_last_error(), bad
    rc = lib.spacap_sample_word_f32(x.data_ptr(), Wp.data_ptr(), b.data_ptr(), rows, V, 0, 1.0, 7, None, 31, 5, 1, lut.data_ptr(), 1.0,
                                    pe.data_ptr(), None, score.data_ptr(), length.data_ptr(), fin.data_ptr(), xw.data_ptr(), ws.data_ptr(), st)
    assert rc == -1
    torch.cuda.synchronize()
    assert bool((ys == -7).all()) and bool((score == 5.0).all()) and bool((xw == 5.0).all()) and bool((length == -7).all())
    assert bool((fin == -7).all()) and bool((ws == 0).all())                                      # nothing was launched


# ---- 6. the distribution on the device -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SR.chi_cases(), ids=lambda c: c[0])
def test_device_draws_follow_the_softmax(case):
    """The chi-square cases of tests/test_sampling.py on the device: R rows share one x row (zero, so the logits are the bias
    -- the case's logits rounded to float32) and differ through rho only."""
    name, R, logits, tau, top_k, bar = case
    V = len(logits)
    b = torch.from_numpy(logits).float()
    x, Wt = torch.zeros(R, 128, device=DEV), (0.3 * torch.randn(V, 128, generator=torch.Generator().manual_seed(2))).to(DEV)
    z = torch.zeros(R, dtype=torch.int32, device=DEV)
    got = _Step(x, Wt, b.to(DEV), top_k, tau, HASH_SEED, SR.STEP, SR.N_WORDS, 0, z, torch.zeros(R, device=DEV), z)
    words = got.ys[:, SR.STEP].cpu().numpy()
    chi, least = SR.chi_square(words, SR.target(b.double().numpy(), tau, top_k))
    print(f"{name}: chi-square {chi:.1f} (bar {bar}), smallest expected count {least:.1f}")
    assert least >= 5 and chi < bar


# ---- 7. the decoder --------------------------------------------------------------------------------------------------------------
SEED = 0          # weight seed of the model below; see test_replay_and_generic_path (d)
SAMPLE_SEED = 20261020
SCORE_TOL = 4 * 3.67e-5    # (c): four times the largest deviation measured on the MI355X (3.67e-5, see the test); must stay below 1e-3


@pytest.fixture(scope="module")
def scene():
    """The model of the decoder tests and one detector + encoder forward of two scenes of 4 096 points (shared, not modified):
    the construction of tests/test_beam_search_gpu.py."""
    from spacap3d_amd.engine import synthetic_batch
    from spacap3d_amd.spacapnet import build_default
    torch.manual_seed(SEED)
    model = build_default(vocab_size=120, num_proposal=32, N=2, d_ff=256).to(DEV).eval()
    data = synthetic_batch(2, 4096, DEV, seed=1, vocab=120)
    with torch.no_grad():
        d = model(dict(data), is_eval=True)
    return model, data, d


@pytest.fixture(scope="module")
def drawn(scene):
    """S = 3, tau = 1, top_k = 0 at SAMPLE_SEED: the fused outputs, the generic path's on the GPU and on the CPU oracle backend
    (with their recorded gaps), and the float64 teacher-forced logits of the fused samples (the uncached decoder on the CPU
    oracle backend in double precision).  Computed once for (b) to (e)."""
    from oracle.attention_ref import OracleBackend
    from spacap3d_amd import backend
    model, data, d = scene
    cap = model.caption
    kw = dict(num_samples=3, temperature=1.0, top_k=0, sample_seed=SAMPLE_SEED)
    keys = ("lang_cap", "lang_cap_score", "lang_cap_samples", "lang_cap_sample_scores", "lang_cap_sample_lengths")
    try:
        with torch.no_grad():
            cap.last_sample_trace = {"untouched": True}
            fused = {k: v.clone() for k, v in cap.forward_eval(dict(d), **kw).items() if k in keys}
            assert cap.last_sample_trace is None, "forward_eval did not take caption_decode.sample_decode"
            cap.sample_generic = True
            gen = {k: v.clone() for k, v in cap.forward_eval(dict(d), **kw).items() if k in keys}
            gap_gpu = cap.last_sample_trace["gap"].cpu()
            cpu_cap = copy.deepcopy(cap).cpu()
            d_cpu = {k: v.cpu() for k, v in d.items() if torch.is_tensor(v)}
            with backend.use_backend(OracleBackend()):
                cpu = {k: v.clone() for k, v in cpu_cap.forward_eval(dict(d_cpu), **kw).items() if k in keys}
                cap64 = copy.deepcopy(cpu_cap).double()
                d64 = {k: (v.double() if v.is_floating_point() else v) for k, v in d_cpu.items()}
                n = fused["lang_cap_samples"].shape[-1]
                logits = SR.teacher_forced_logits(cap64, d64, fused["lang_cap_samples"].reshape(-1, n).cpu()).numpy()
    finally:
        cap.__dict__.pop("sample_generic", None)
        cap.__dict__.pop("last_sample_trace", None)
    return fused, gen, gap_gpu, cpu, logits


def _through_first_eos(tokens, eos):
    is_eos = tokens == eos
    before = torch.cumsum(is_eos.long(), 1) - is_eos.long()
    return before == 0


def test_top_k_one_is_the_greedy_decoder(scene):
    """(a) top_k = 1, S = 1 at two temperatures against the greedy captions, word for word through each row's first eos, and
    eos behind it.  Exact: the candidates are spacap_beam_topw_f32's, whose first entry is the greedy kernel's arg-max."""
    model, data, d = scene
    eos = model.caption.word_to_idx["eos"]
    g = d["lang_cap"].reshape(-1, d["lang_cap"].shape[-1])
    keep = _through_first_eos(g, eos)
    print(f"rows with an eos: {int((g == eos).any(1).sum())} of {g.shape[0]}")
    for tau in (1.0, 0.5):
        with torch.no_grad():
            out = model.caption.forward_eval(dict(d), num_samples=1, temperature=tau, top_k=1)
        ys = out["lang_cap"].reshape(g.shape)
        assert torch.equal(ys[keep], g[keep]) and bool((ys[~keep] == eos).all())
        assert torch.equal(out["lang_cap_samples"][:, :, 0], out["lang_cap"])
        want_len = torch.where((g == eos).any(1), (g == eos).long().argmax(1) + 1, torch.full_like(g[:, 0], g.shape[1]))
        assert torch.equal(out["lang_cap_sample_lengths"].reshape(-1).long(), want_len)


def test_samples_shapes_seeds_and_variety(scene, drawn):
    """(b) S = 3, tau = 1, top_k = 0 at a fixed seed: shapes and dtypes, lang_cap is sample 0, a second call is bit-equal,
    another seed changes at least half of the rows, and in at least half of the proposals the three samples are not all equal."""
    model, data, d = scene
    fused = drawn[0]
    B, K, n = d["lang_cap"].shape
    s = fused["lang_cap_samples"]
    assert s.shape == (B, K, 3, n) and s.dtype == torch.long
    assert fused["lang_cap_sample_scores"].shape == (B, K, 3) and fused["lang_cap_sample_scores"].dtype == torch.float32
    assert fused["lang_cap_sample_lengths"].shape == (B, K, 3) and fused["lang_cap_sample_lengths"].dtype == torch.int32
    assert fused["lang_cap"].shape == (B, K, n) and torch.equal(fused["lang_cap"], s[:, :, 0])
    assert torch.equal(fused["lang_cap_score"], fused["lang_cap_sample_scores"][:, :, 0])
    kw = dict(num_samples=3, temperature=1.0, top_k=0)
    with torch.no_grad():
        again = model.caption.forward_eval(dict(d), sample_seed=SAMPLE_SEED, **kw)
        other = model.caption.forward_eval(dict(d), sample_seed=SAMPLE_SEED + 1, **kw)
    for k in ("lang_cap_samples", "lang_cap_sample_scores", "lang_cap_sample_lengths"):
        assert torch.equal(again[k], fused[k]), k
    changed = float((other["lang_cap_samples"] != s).any(-1).float().mean())
    varied = float(((s[:, :, 0] != s[:, :, 1]).any(-1) | (s[:, :, 0] != s[:, :, 2]).any(-1)).float().mean())
    print(f"another seed changes {changed:.2f} of the rows; {varied:.2f} of the proposals have samples that differ")
    assert changed >= 0.5 and varied >= 0.5


def test_sampled_scores_against_teacher_forcing(scene, drawn):
    """(c) lang_cap_sample_scores against the float64 teacher-forced sum of the sampled words' log-probabilities through the
    first eos, within SCORE_TOL = 4 x the largest deviation measured on the MI355X (3.67e-5 on scores down to -148: fp32
    accumulation of 31 terms; the factor is headroom for other seeds); lengths and eos padding as specified."""
    model, data, d = scene
    fused, logits = drawn[0], drawn[4]
    eos = model.caption.word_to_idx["eos"]
    n = logits.shape[1]
    rp = SR.replay(fused["lang_cap_samples"].reshape(-1, n).cpu().numpy(), logits, 1.0, 0, SAMPLE_SEED, eos)
    dev_ = float(np.abs(fused["lang_cap_sample_scores"].reshape(-1).double().cpu().numpy() - rp["score"]).max())
    print(f"largest |lang_cap_sample_scores - float64 teacher-forced score| = {dev_:.3g} (scores down to {rp['score'].min():.1f})")
    assert rp["padded"] and np.array_equal(fused["lang_cap_sample_lengths"].reshape(-1).cpu().numpy(), rp["length"])
    assert SCORE_TOL < 1e-3 and dev_ <= SCORE_TOL


def _first_difference(a, b):
    """[(row, first differing step)] of two (rows, n) word arrays"""
    diff = a != b
    return [(int(r), int(np.flatnonzero(diff[r])[0])) for r in np.flatnonzero(diff.any(1))]


def test_replay_and_generic_path(scene, drawn):
    """(d) the device's own prefixes replayed in float64 (tests/test_sampling.py, test 3): every step that is not open
    reproduces the sampled word, and at most 5 % of the rows contain an open step.  The weight seed (SEED) was chosen so that
    the generic path ALONE -- fp32 on the GPU against fp32 on the CPU oracle backend -- stays within that cap; checked first.
    (e) fused against sample_generic=True at the same seed: rows are identical, or the first differing step is open by the
    generic path's recorded gap; at most 5 % of the rows differ."""
    model, data, d = scene
    fused, gen, gap_gpu, cpu, logits = drawn
    eos = model.caption.word_to_idx["eos"]
    n = logits.shape[1]
    rows = logits.shape[0]
    host = lambda o: o["lang_cap_samples"].reshape(-1, n).cpu().numpy()  # noqa: E731
    alone = _first_difference(host(gen), host(cpu))
    print(f"generic GPU vs generic CPU: {len(alone)} of {rows} rows differ")
    assert len(alone) <= 0.05 * rows
    rp = SR.replay(host(fused), logits, 1.0, 0, SAMPLE_SEED, eos)
    print(f"replay: wrong {rp['wrong']}; rows with an open step: {len(rp['open_rows'])} of {rows}")
    assert not rp["wrong"]
    assert len(rp["open_rows"]) <= 0.05 * rows
    diff = _first_difference(host(fused), host(gen))
    tol = 1e-4 * float(np.abs(logits).max()) / 1.0 + 1e-5
    print(f"fused vs generic: {len(diff)} of {rows} rows differ; gaps at the first differing step: "
          f"{[float(gap_gpu[s, r]) for r, s in diff]} (open below {tol:.3g})")
    for r, s in diff:
        assert float(gap_gpu[s, r]) < tol, (r, s)
    assert len(diff) <= 0.05 * rows
    if not diff:
        assert torch.equal(fused["lang_cap_sample_lengths"], gen["lang_cap_sample_lengths"])
        assert float((fused["lang_cap_sample_scores"] - gen["lang_cap_sample_scores"]).abs().max()) <= 1e-3


def test_captured_graph_draws_new_captions_after_advance_rng(scene):
    """(f) forward_eval with sampling and no explicit seed, captured once: two replays without advance_rng give equal captions,
    two with it in between different ones."""
    from spacap3d_amd.attention import advance_rng, rng_state
    model, data, d = scene
    cap = model.caption
    rng_state(torch.device(DEV))                      # the device word exists before the capture
    kw = dict(num_samples=2, temperature=1.0, top_k=0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        cap.forward_eval(dict(d), **kw)               # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        static = cap.forward_eval(dict(d), **kw)["lang_cap_samples"]
    g.replay()
    a = static.clone()
    g.replay()
    b = static.clone()
    advance_rng(torch.device(DEV))
    g.replay()
    c = static.clone()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    changed = float((a != c).any(-1).float().mean())
    print(f"after advance_rng {changed:.2f} of the rows changed")
    assert changed >= 0.5


def test_evaluator_pipeline_with_sampling(scene):
    """(g) Evaluator(..., sample=dict(num_samples=2, top_k=5)) with post-processing and predictions: pred_tokens are sample 0's
    words (by the restatement of tests/dense_caption_restated.py)."""
    import dense_caption_restated as D
    from spacap3d_amd.engine import Evaluator, synthetic_batch
    from test_postprocess_gpu import POST_DICT
    model = scene[0]
    cap = model.caption
    sos, eos = cap.word_to_idx["sos"], cap.word_to_idx["eos"]
    post = dict(POST_DICT, dataset_config=None)
    batch = {"point_clouds": synthetic_batch(2, 4096, DEV, seed=1, vocab=120)["point_clouds"]}
    try:
        ev = Evaluator(model, graph=True, postprocess=post, predictions=(sos, eos), sample=dict(num_samples=2, top_k=5))
        out = ev(dict(batch))
        torch.cuda.synchronize()
        assert out["lang_cap_samples"].shape == (2, 32, 2, 31) and out["lang_cap"].shape == (2, 32, 31)
        assert torch.equal(out["lang_cap"], out["lang_cap_samples"][:, :, 0])
        assert bool(torch.isfinite(out["lang_cap_sample_scores"]).all()) and bool((out["lang_cap_sample_scores"] <= 0).all())
        h = {k: out[k].cpu().numpy() for k in ("post_valid", "post_obj_prob", "sem_cls", "bbox_corner", "lang_cap")}
        want = D.select(h["post_valid"], h["post_obj_prob"], h["sem_cls"], h["bbox_corner"], h["lang_cap"], sos, eos)
        np.testing.assert_array_equal(out["pred_tokens"].cpu().numpy(), want["tokens"])
        np.testing.assert_array_equal(out["pred_length"].cpu().numpy(), want["length"])
    finally:
        for k in ("num_samples", "temperature", "top_k", "sample_seed"):
            cap.__dict__.pop(k, None)
