"""Sampled caption decoding without a GPU: the float64 restatement of the contract
(tests/sampling_restated.py) against the existing keep-mask hash and against the distribution it claims, the generic path
(spacap3d_amd/sampling.py) against the restatement on the CPU oracle backend, the C ABI of csrc/caption_decode.hip, and the
argument errors of the public interface."""
import copy
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sampling_restated as SR  # noqa: E402

SEED = 0x1234567890ABCDEF


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter", [None, 3])
def test_hash_is_the_keep_masks_hash(counter):
    """keep = hash >= floor(p 2^32) of the keep-mask restatement (tests/test_dropout_mask_gpu.py::expected_keep), at thresholds
    that cut the 32-bit range in many places; and the generic path's integer-tensor hash, also above 2^32."""
    from test_dropout_mask_gpu import expected_keep
    n = 5000
    h = SR.hash32(np.arange(n), SEED, counter)
    for p in (0.001, 0.1, 0.25, 0.5, 0.75, 0.9, 0.999):
        thresh = int(float(np.float32(p)) * 4294967296.0)
        assert np.array_equal(h >= np.uint32(thresh), expected_keep(n, p, SEED, counter)), p
    from spacap3d_amd import sampling
    idx = np.concatenate([np.arange(n), (1 << 32) - 3 + np.arange(7), (5 << 32) + 11 * np.arange(n), [(1 << 62) + 12345]]).astype(np.uint64)
    lo, hi = sampling.seed_words(SEED, None if counter is None else torch.tensor([counter]))
    got = sampling.hash32(torch.from_numpy(idx.astype(np.int64)), lo, hi).numpy()
    assert np.array_equal(got.astype(np.uint32), SR.hash32(idx, SEED, counter))
    g = sampling.gumbel_noise(torch.from_numpy(idx.astype(np.int64)), lo, hi).numpy()
    assert g.dtype == np.float32 and np.abs(g - SR.gumbel64(SR.hash32(idx, SEED, counter))).max() < 1e-5


def test_gumbel_noise_in_float32_is_within_1e5_of_float64():
    """u = ((h >> 9) + 0.5) 2^-23 over a stride-7 sweep of the 2^23 values of h >> 9, both ends included"""
    k = np.unique(np.concatenate([np.arange(0, 1 << 23, 7), [(1 << 23) - 1]])).astype(np.uint32)
    h = k << np.uint32(9)
    u = SR.uniform_of(h)
    assert u.min() == 2.0 ** -24 and u.max() == 1 - 2.0 ** -24
    u32 = ((k.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23))
    assert np.array_equal(u32.astype(np.float64), u)                                  # exact in float32
    g64, g32 = SR.gumbel64(h), SR.gumbel32(h)
    err = float(np.abs(g32.astype(np.float64) - g64).max())
    print(f"g in [{g64.min():.3f}, {g64.max():.3f}]; max |float32 - float64| = {err:.3g}")
    assert g32.dtype == np.float32 and err < 1e-5
    assert -2.83 < g64.min() and g64.max() < 16.64


@pytest.mark.parametrize("case", SR.chi_cases(), ids=lambda c: c[0])
def test_restated_draws_follow_the_softmax(case):
    """chi-square of R restated draws from one logit row (the rows differ through rho only) against softmax(l / tau), or the
    renormalised top-k; bar: the 99.9 % quantile."""
    name, R, logits, tau, top_k, bar = case
    d = SR.draw(np.broadcast_to(logits, (R, len(logits))), np.arange(R), SR.STEP, SR.N_WORDS, tau, top_k, SEED)
    chi, least = SR.chi_square(d["word"], SR.target(logits, tau, top_k))
    print(f"{name}: chi-square {chi:.1f} (bar {bar}), smallest expected count {least:.1f}")
    assert least >= 5 and chi < bar


@pytest.mark.parametrize("rows,V", SR.STEP_SHAPES)
def test_one_step_cases_have_few_open_rows(rows, V):
    """The inputs tests/test_sampling_gpu.py uses for the one-step test: by the restatement alone at most 2 % of the rows of a
    case are open (best and second-best z within the tolerance, or the top-k candidate set within 1e-4 max|l| of changing)."""
    _, _, _, logits = SR.step_inputs(rows, V)
    for tau in SR.STEP_TAU:
        for k in SR.STEP_TOP_K:
            if k > V:
                continue
            d = SR.draw(logits, np.arange(rows), SR.STEP, SR.N_WORDS, tau, k, SR.STEP_SEED)
            n_open = int(((d["gap"] < SR.tolerance(logits, tau)) | (d["cut"] < 1e-4 * np.abs(logits).max())).sum())
            assert n_open <= 0.02 * rows, (tau, k, n_open)
            if k == 1:
                assert np.array_equal(d["word"], logits.argmax(1))


def test_generic_sampler_equals_the_restatement_on_a_table():
    """sampling.sample over a table of exactly representable logits (multiples of 1/8; the noise makes ties vanishingly rare):
    words, lengths and eos padding equal the restatement's, scores within float32 accumulation, for tau and top_k."""
    from spacap3d_amd.sampling import sample
    R, S, V, n, sos, eos = 3, 4, 11, 9, 0, 1
    g = np.random.default_rng(2)
    table = g.integers(-16, 17, size=(V, n, V)).astype(np.float64) / 8         # logits[previous word][step]
    table[:, :, eos] = -1.0
    table[:, 3:, eos] = 0.5                                                     # eos: likely from step 3 on only
    tt = torch.from_numpy(table).float()
    ends = set()
    for tau, k in ((1.0, 0), (0.7, 0), (1.3, 3), (1.0, 1), (2.0, 8)):
        got = sample(lambda i, words: tt[words, i], R, S, n, sos, eos, tau, k, SEED)
        rows = R * S
        words = np.full(rows, sos)
        fin, score, length = np.zeros(rows, bool), np.zeros(rows), np.zeros(rows, np.int64)
        ys = []
        for i in range(n):
            lg = table[words, i]
            d = SR.draw(lg, np.arange(rows), i, n, tau, k, SEED)
            assert (d["gap"] > SR.tolerance(lg, tau)).all()
            assert np.allclose(got["gap"][i].numpy(), d["gap"], atol=1e-4)
            words, score, length, fin = SR.advance(d["word"], d["logp"], i, eos, score, length, fin)
            ys.append(words)
        ys = np.stack(ys, 1)
        ends |= set(np.where(fin, length, -1).tolist())
        assert got["ys"].shape == (R, S, n) and np.array_equal(got["ys"].numpy().reshape(rows, n), ys), (tau, k)
        assert got["length"].dtype == torch.int32 and np.array_equal(got["length"].numpy().reshape(-1), np.where(fin, length, n))
        assert got["score"].dtype == torch.float32 and np.abs(got["score"].numpy().reshape(-1) - score).max() < 1e-4
        if k == 1:
            assert len({tuple(r) for r in ys[:S].tolist()}) == 1               # top_k = 1: the greedy words, whatever the noise
    assert -1 in ends and len(ends) > 3            # the fixture does what it says: rows finish at different steps, some never


# ---- 2. the C ABI ----------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    from spacap3d_amd import _native
    header = open(os.path.join(os.path.dirname(HERE), "include", "spacap_hip.h")).read()
    for name, ret in (("spacap_sample_word_workspace_bytes", "size_t"), ("spacap_sample_word_f32", "int")):
        m = re.search(r"\b%s %s\(([^;]*)\);" % (ret, name), header)
        assert m, name
        assert name in _native.SIGNATURES and hasattr(_native.lib, name)
        assert len(m.group(1).split(",")) == len(_native.SIGNATURES[name][1]), name      # as many arguments on both sides


def _call(**over):
    """spacap_sample_word_f32 with small non-null fake pointers (16-byte aligned; a refused call never touches them)"""
    from spacap3d_amd import _native
    a = dict(x=0x1000, Wp=0x2000, bias=0x3000, rows=4, V=40, top_k=0, inv_tau=1.0, seed=7, seed_dev=None, n_words=31, step=5, eos=1,
             lut=0x4000, scale=1.0, pe_row=0x5000, ys=0x6000, score=0x7000, length=0x8000, finished=0x9000, xw=0xA000,
             workspace=0xB000, stream=None)
    a.update(over)
    return _native.lib.spacap_sample_word_f32(*a.values()), _native.lib.spacap_last_error()


@pytest.mark.parametrize("over", [dict(rows=-1), dict(V=0), dict(top_k=-1), dict(top_k=9), dict(V=3, top_k=4), dict(inv_tau=0.0),
                                  dict(inv_tau=-1.0), dict(inv_tau=float("inf")), dict(inv_tau=float("nan")), dict(step=-1),
                                  dict(step=31), dict(x=None), dict(Wp=None), dict(bias=None), dict(lut=None), dict(pe_row=None),
                                  dict(ys=None), dict(score=None), dict(length=None), dict(finished=None), dict(xw=None),
                                  dict(workspace=None)], ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_sample_word_refuses_before_any_device_call(over):
    rc, msg = _call(**over)
    assert rc == -1 and b"spacap_sample_word_f32" in msg


def test_sample_word_with_no_rows_does_nothing():
    from spacap3d_amd import _native
    assert _call(rows=0)[0] == 0
    assert _native.lib.spacap_sample_word_workspace_bytes(0, 40, 0) == 0


# ---- 3. the generic path on the CPU oracle backend -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    """A tiny captioner on the CPU oracle backend and hand-made detector outputs (2 scenes x 8 proposals)."""
    from spacap3d_amd.spacapnet import build_default
    torch.manual_seed(3)
    model = build_default(vocab_size=40, num_proposal=8, N=1, d_ff=128).eval()
    g = torch.Generator().manual_seed(4)
    ep = {"aggregated_vote_features": torch.randn(2, 8, 128, generator=g), "aggregated_vote_xyz": torch.randn(2, 8, 3, generator=g),
          "bbox_mask": torch.ones(2, 8)}
    return model, ep


@pytest.mark.parametrize("tau,top_k", [(1.0, 0), (0.7, 5)])
def test_generic_path_on_the_cpu_oracle_backend(tiny, tau, top_k):
    """forward_eval(num_samples=3) through sampling.sample over decode_incremental.  Every row's own sampled prefix is
    teacher-forced through the uncached decoder in float64 and the restated noise applied: the restated choice is the sampled
    word wherever the step is not open; scores are the float64 sums through the first eos; lengths and eos padding as
    specified; the same seed gives the same captions, another seed others."""
    from oracle.attention_ref import OracleBackend
    from spacap3d_amd import backend
    model, ep = tiny
    cap = model.caption
    eos = cap.word_to_idx["eos"]
    S = 3
    with backend.use_backend(OracleBackend()), torch.no_grad():
        out = cap.forward_eval(dict(ep), num_samples=S, temperature=tau, top_k=top_k, sample_seed=SEED)
        again = cap.forward_eval(dict(ep), num_samples=S, temperature=tau, top_k=top_k, sample_seed=SEED)
        other = cap.forward_eval(dict(ep), num_samples=S, temperature=tau, top_k=top_k, sample_seed=SEED + 1)
        cap64 = copy.deepcopy(cap).double()
        samples = out["lang_cap_samples"]
        B, K, _, n = samples.shape
        logits = SR.teacher_forced_logits(cap64, {k: v.double() for k, v in ep.items()}, samples.reshape(B * K * S, n))
    assert logits.dtype == torch.float64
    assert samples.shape == (2, 8, S, n) and samples.dtype == torch.long and n == 31
    assert out["lang_cap_sample_scores"].shape == (2, 8, S) and out["lang_cap_sample_scores"].dtype == torch.float32
    assert out["lang_cap_sample_lengths"].shape == (2, 8, S) and out["lang_cap_sample_lengths"].dtype == torch.int32
    assert torch.equal(out["lang_cap"], samples[:, :, 0]) and torch.equal(out["lang_cap_score"], out["lang_cap_sample_scores"][:, :, 0])
    for k in ("lang_cap_samples", "lang_cap_sample_scores", "lang_cap_sample_lengths"):
        assert torch.equal(out[k], again[k]), k
    assert not torch.equal(out["lang_cap_samples"], other["lang_cap_samples"])
    rp = SR.replay(samples.reshape(-1, n).numpy(), logits.numpy(), tau, top_k, SEED, eos)
    print(f"rows with an open step: {len(rp['open_rows'])} of {B * K * S}; wrong: {rp['wrong']}")
    assert not rp["wrong"] and rp["padded"]
    # so that the replay checks something: few open row-steps (an untrained model's logits are nearly flat, so with top_k the
    # candidate set itself is within 1e-4 max|l| of changing now and then), and for top_k = 0 at most 5 % of the rows
    print(f"open row-steps: {rp['open_steps']} of {rp['live_steps']}")
    assert rp["open_steps"] <= 0.01 * rp["live_steps"]
    assert top_k or len(rp["open_rows"]) <= 0.05 * B * K * S
    assert np.array_equal(out["lang_cap_sample_lengths"].reshape(-1).numpy(), rp["length"])
    assert (rp["length"] < n).any()                                                  # some row did draw eos
    err = float(np.abs(out["lang_cap_sample_scores"].reshape(-1).double().numpy() - rp["score"]).max())
    print(f"largest |score - float64 teacher-forced score| = {err:.3g} (scores down to {rp['score'].min():.1f})")
    assert err < 1e-3
    gap = cap.last_sample_trace["gap"]
    assert gap.shape == (n, B * K * S)


# ---- 4. argument errors ----------------------------------------------------------------------------------------------------------
def test_forward_eval_and_evaluator_refuse_bad_sampling_arguments(tiny):
    from spacap3d_amd.engine import Evaluator
    from spacap3d_amd.spacapnet import build_default
    model = build_default(vocab_size=40, num_proposal=8, N=1, d_ff=128)
    cap = model.caption
    keys = set(model.state_dict())
    assert cap.num_samples == 0 and cap.temperature == 1.0 and cap.top_k == 0 and cap.sample_generic is False
    for kw in (dict(num_samples=2, beam_size=2), dict(num_samples=0), dict(num_samples=-1), dict(num_samples=1, temperature=0.0),
               dict(num_samples=1, temperature=-1.0), dict(num_samples=1, temperature=float("inf")),
               dict(num_samples=1, temperature=float("nan")), dict(num_samples=1, top_k=-1), dict(num_samples=1, top_k=9),
               dict(num_samples=1, use_cache=False)):
        with pytest.raises(ValueError):
            cap.forward_eval({}, **kw)
    small = build_default(vocab_size=5, num_proposal=8, N=1, d_ff=128)
    V = small.caption.model.generator.proj.out_features
    if V < 8:
        with pytest.raises(ValueError):
            small.caption.forward_eval({}, num_samples=1, top_k=V + 1)
    for kw in (dict(sample=dict(num_samples=2), beam_size=2), dict(sample=dict(num_samples=0)), dict(sample=dict(temperature=0.0)),
               dict(sample=dict(temperature=float("nan"))), dict(sample=dict(top_k=9)), dict(sample=dict(top_k=-1)),
               dict(sample=dict(samples=2))):
        with pytest.raises(ValueError):
            Evaluator(model, **kw)
        cap.__dict__.pop("beam_size", None)
    assert cap.num_samples == 0                                                        # a refused argument sets nothing
    try:
        Evaluator(model, sample=dict(num_samples=2, temperature=0.8, top_k=5, seed=11))
        assert (cap.num_samples, cap.temperature, cap.top_k, cap.sample_seed) == (2, 0.8, 5, 11) and set(model.state_dict()) == keys
        Evaluator(model, sample=dict(num_samples=4))
        assert (cap.num_samples, cap.temperature, cap.top_k, cap.sample_seed) == (4, 1.0, 0, None)
    finally:
        for k in ("num_samples", "temperature", "top_k", "sample_seed", "beam_size"):
            cap.__dict__.pop(k, None)
