"""Nucleus (top-p) sampling without a GPU ("Top-p"): the float64 restatement (tests/nucleus_restated.py)
against a brute-force sorted-prefix definition and hand-written tie cases, the generic path (spacap3d_amd/sampling.py) against
the restatement, the argument errors of the public interface, the C ABI of csrc/caption_decode.hip, and the open-row caps of the
one-step cases tests/test_nucleus_gpu.py runs."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nucleus_restated as NR  # noqa: E402
import sampling_restated as SR  # noqa: E402

SEED = 0x1234567890ABCDEF


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------
def _sorted_prefix(logits, tau, p):
    """The textbook definition on a tie-free row: walk the words by descending probability and take each while the mass taken
    so far is below p."""
    e = np.exp((logits - logits.max()) / tau)
    q = e / e.sum()
    inside, taken = np.zeros(len(logits), bool), 0.0
    for v in np.argsort(-logits):
        if not taken < p:
            break
        inside[v] = True
        taken += q[v]
    return inside


@pytest.mark.parametrize("tau", [1.0, 0.7, 2.0])
def test_restatement_is_the_sorted_prefix_on_tie_free_rows(tau):
    g = np.random.default_rng(5)
    logits = g.normal(0.0, 2.0, size=(40, 97))
    assert all(len(np.unique(r)) == 97 for r in logits)
    sizes = set()
    for p in (1e-6, 0.1, 0.5, 0.9, 0.999, 1.0):
        got = NR.nucleus(logits, tau, p)
        for r in range(len(logits)):
            assert np.array_equal(got[r], _sorted_prefix(logits[r], tau, p)), (p, r)
        assert got[np.arange(40), logits.argmax(1)].all()                   # the most probable word is always in
        sizes |= set(got.sum(1).tolist())
    assert np.array_equal(NR.nucleus(logits, tau, 1e-6).sum(1), np.ones(40))
    assert NR.nucleus(logits, tau, 1.0).all()
    assert len(sizes) > 10                                                   # the set adapts to the row


def test_restatement_on_hand_written_ties():
    """q = (.3 .3 .1 .1 .1 .05 .05): A = (0 0 .6 .6 .6 .9 .9).  Equal logits enter or stay out together, in any word order."""
    q = np.array([0.3, 0.3, 0.1, 0.1, 0.1, 0.05, 0.05])
    perm = np.array([4, 0, 6, 2, 1, 5, 3])
    for order in (np.arange(7), perm):
        logits = np.log(q)[order][None, :]
        A = NR.mass_above(logits, 1.0)[0]
        assert np.allclose(A, np.array([0, 0, 0.6, 0.6, 0.6, 0.9, 0.9])[order], atol=1e-12)
        for p, want in ((0.05, 2), (0.59, 2), (0.61, 5), (0.7, 5), (0.89, 5), (0.91, 7), (1.0, 7)):
            inside = NR.nucleus(logits, 1.0, p)[0]
            assert np.array_equal(inside, (np.arange(7) < want)[order]), (p, order)       # q is sorted: the first `want` words
    # the temperature acts before the set is formed: at tau = 0.5 q is proportional to (9 9 1 1 1 .25 .25): A = (0 0 .847 ..)
    A = NR.mass_above(np.log(q)[None, :], 0.5)[0]
    assert np.allclose(A[2:5], 18 / 21.5) and np.allclose(A[5:], 21 / 21.5)
    # all equal: one run, everything in at any p
    assert NR.nucleus(np.zeros((1, 9)), 1.0, 1e-6).all()


def test_restated_draw_keeps_the_unrestricted_word_inside_the_nucleus():
    """The noise is the unrestricted sampler's: where that draw lies in the nucleus it IS the nucleus draw; elsewhere the word
    is in the nucleus, and logp is the untempered, untruncated one."""
    _, _, _, logits = SR.step_inputs(300, 1000)
    rho = np.arange(300)
    free = SR.draw(logits, rho, SR.STEP, SR.N_WORDS, 0.7, 0, SEED)
    d = NR.draw(logits, rho, SR.STEP, SR.N_WORDS, 0.7, 0.5, SEED)
    assert np.array_equal(d["free"], free["word"])
    kept = d["inside"][rho, free["word"]]
    assert 0.2 < kept.mean() < 0.9
    assert np.array_equal(d["word"][kept], free["word"][kept]) and (d["word"][~kept] != free["word"][~kept]).all()
    assert d["inside"][rho, d["word"]].all()
    m = logits.max(1)
    assert np.allclose(d["logp"], logits[rho, d["word"]] - m - np.log(np.exp(logits - m[:, None]).sum(1)))
    one = NR.draw(logits, rho, SR.STEP, SR.N_WORDS, 0.7, 1e-6, SEED)
    assert np.array_equal(one["word"], logits.argmax(1)) and (one["second"] == -1).all() and np.isinf(one["gap"]).all()


@pytest.mark.parametrize("rows,V", NR.STEP_SHAPES)
def test_one_step_cases_have_few_open_rows(rows, V):
    """The inputs of tests/test_nucleus_gpu.py's one-step test: by the restatement alone at most 5 % of the rows of a case are
    open, none in the 16-row shape; and the nucleus matters: at p = 0.5, tau = 1 more than a quarter of the 300 x 1000 rows draw
    another word than the unrestricted sampler."""
    _, _, _, logits = NR.step_inputs(rows, V)
    for tau in NR.STEP_TAU:
        for p in NR.STEP_P:
            d = NR.draw(logits, np.arange(rows), SR.STEP, SR.N_WORDS, tau, p, SR.STEP_SEED)
            n_open = int(NR.is_open(d, logits, tau).sum())
            assert n_open <= NR.OPEN_CAP * rows and (rows != 16 or n_open == 0), (tau, p, n_open)
            if (rows, V, tau, p) == (300, 1000, 1.0, 0.5):
                assert (d["word"] != d["free"]).sum() >= 75


# ---- 2. the generic path ---------------------------------------------------------------------------------------------------------
def test_generic_nucleus_mask_equals_the_restatement():
    from spacap3d_amd.sampling import nucleus_mask
    g = np.random.default_rng(6)
    logits = g.integers(-16, 17, size=(50, 40)).astype(np.float64) / 8      # many ties
    for tau, p in ((1.0, 0.3), (0.7, 0.62), (1.3, 0.9), (1.0, 1e-6)):
        A = NR.mass_above(logits, tau)
        assert (np.abs(A - p) > 1e-9).all()                                   # no row sits on the boundary
        got = nucleus_mask(torch.from_numpy(logits).float(), tau, p).numpy()
        assert np.array_equal(got, A < p), (tau, p)


def test_generic_sampler_equals_the_restatement_on_a_table():
    """sampling.sample(top_p=) over the table of tests/test_sampling.py (logits in multiples of 1/8: ties in every row):
    words, lengths and eos padding equal the restatement's, scores within float32 accumulation; None and 1.0 are the
    unrestricted sampler."""
    from spacap3d_amd.sampling import sample
    R, S, V, n, sos, eos = 3, 4, 11, 9, 0, 1
    g = np.random.default_rng(2)
    table = g.integers(-16, 17, size=(V, n, V)).astype(np.float64) / 8         # logits[previous word][step]
    table[:, :, eos] = -1.0
    table[:, 3:, eos] = 0.5
    tt = torch.from_numpy(table).float()
    rows = R * S
    narrowed = 0
    for tau, p in ((1.0, 0.5), (0.7, 0.9), (1.3, 0.25)):
        got = sample(lambda i, words: tt[words, i], R, S, n, sos, eos, tau, 0, SEED, top_p=p)
        words = np.full(rows, sos)
        fin, score, length = np.zeros(rows, bool), np.zeros(rows), np.zeros(rows, np.int64)
        ys = []
        for i in range(n):
            lg = table[words, i]
            d = NR.draw(lg, np.arange(rows), i, n, tau, p, SEED)
            assert not NR.is_open(d, lg, tau).any()
            narrowed += int((d["word"] != d["free"]).sum())
            assert np.allclose(got["gap"][i].numpy(), d["gap"], atol=1e-4)
            words, score, length, fin = SR.advance(d["word"], d["logp"], i, eos, score, length, fin)
            ys.append(words)
        ys = np.stack(ys, 1)
        assert got["ys"].shape == (R, S, n) and np.array_equal(got["ys"].numpy().reshape(rows, n), ys), (tau, p)
        assert np.array_equal(got["length"].numpy().reshape(-1), np.where(fin, length, n))
        assert np.abs(got["score"].numpy().reshape(-1) - score).max() < 1e-4
    assert narrowed > 20
    plain = sample(lambda i, words: tt[words, i], R, S, n, sos, eos, 0.7, 0, SEED)
    for p in (None, 1.0):
        same = sample(lambda i, words: tt[words, i], R, S, n, sos, eos, 0.7, 0, SEED, top_p=p)
        assert all(torch.equal(plain[k], same[k]) for k in plain)


def test_forward_eval_takes_the_generic_path_on_the_cpu_oracle_backend():
    """forward_eval(num_samples=3, top_p=0.8) through sampling.sample over decode_incremental (the tiny captioner of
    tests/test_sampling.py): every row's own prefix, teacher-forced in float64 and replayed, reproduces the sampled words
    wherever the step is not open; no word lies outside its nucleus; the restriction matters; the same seed repeats the draws."""
    import copy
    from oracle.attention_ref import OracleBackend
    from spacap3d_amd import backend
    from spacap3d_amd.spacapnet import build_default
    torch.manual_seed(3)
    model = build_default(vocab_size=40, num_proposal=8, N=1, d_ff=128).eval()
    g = torch.Generator().manual_seed(4)
    ep = {"aggregated_vote_features": torch.randn(2, 8, 128, generator=g), "aggregated_vote_xyz": torch.randn(2, 8, 3, generator=g),
          "bbox_mask": torch.ones(2, 8)}
    cap = model.caption
    eos, S, p = cap.word_to_idx["eos"], 3, 0.8
    with backend.use_backend(OracleBackend()), torch.no_grad():
        out = cap.forward_eval(dict(ep), num_samples=S, top_p=p, sample_seed=SEED)
        again = cap.forward_eval(dict(ep), num_samples=S, top_p=p, sample_seed=SEED)
        free = cap.forward_eval(dict(ep), num_samples=S, sample_seed=SEED)
        samples = out["lang_cap_samples"]
        B, K, _, n = samples.shape
        logits = SR.teacher_forced_logits(copy.deepcopy(cap).double(), {k: v.double() for k, v in ep.items()}, samples.reshape(B * K * S, n))
    assert torch.equal(samples, again["lang_cap_samples"]) and torch.equal(out["lang_cap_sample_scores"], again["lang_cap_sample_scores"])
    assert not torch.equal(samples, free["lang_cap_samples"]) and cap.last_sample_trace["gap"].shape == (n, B * K * S)
    rp = NR.replay(samples.reshape(-1, n).numpy(), logits.numpy(), 1.0, p, SEED, eos)
    print(f"wrong {rp['wrong']}; outside {rp['outside']}; open steps {rp['open_steps']} of {rp['live_steps']}; left {rp['left']}")
    assert not rp["wrong"] and not rp["outside"] and rp["padded"]
    assert rp["open_steps"] <= 0.01 * rp["live_steps"] and rp["left"] >= 0.1 * rp["live_steps"]
    assert np.array_equal(out["lang_cap_sample_lengths"].reshape(-1).numpy(), rp["length"])
    assert float(np.abs(out["lang_cap_sample_scores"].reshape(-1).double().numpy() - rp["score"]).max()) < 1e-3


# ---- 3. argument errors ----------------------------------------------------------------------------------------------------------
BAD_P = [0.0, -0.1, 1.0001, 2.0, float("nan"), float("inf"), float("-inf")]


def test_bad_top_p_raises_everywhere():
    from spacap3d_amd.engine import Evaluator
    from spacap3d_amd.sampling import check_arguments, sample
    from spacap3d_amd.self_critical import SelfCritical
    from spacap3d_amd.spacapnet import build_default
    model = build_default(vocab_size=40, num_proposal=8, N=1, d_ff=128)
    cap = model.caption
    assert cap.top_p is None and "top_p" not in "".join(model.state_dict())
    for p in BAD_P:
        with pytest.raises(ValueError):
            check_arguments("t", 1, 1.0, 0, top_p=p)
        with pytest.raises(ValueError):
            cap.forward_eval({}, num_samples=1, top_p=p)
        with pytest.raises(ValueError):
            Evaluator(model, sample=dict(top_p=p))
        with pytest.raises(ValueError):
            sample(lambda i, w: torch.zeros(2, 5), 2, 1, 3, 0, 1, top_p=p)
    # one restriction at a time
    for k in (1, 8):
        with pytest.raises(ValueError):
            check_arguments("t", 1, 1.0, k, top_p=0.9)
        with pytest.raises(ValueError):
            cap.forward_eval({}, num_samples=1, top_k=k, top_p=0.9)
        with pytest.raises(ValueError):
            Evaluator(model, sample=dict(top_k=k, top_p=0.9))
        with pytest.raises(ValueError):
            sample(lambda i, w: torch.zeros(2, 20), 2, 1, 3, 0, 1, top_k=k, top_p=0.9)
    assert cap.num_samples == 0 and cap.top_p is None                       # a refused argument sets nothing
    check_arguments("t", 1, 1.0, 8, top_p=1.0)                                # 1.0 and None restrict nothing
    check_arguments("t", 1, 1.0, 8, top_p=None)
    check_arguments("t", 1, 1.0, 8)                                           # the trailing keyword: earlier callers unchanged
    try:
        Evaluator(model, sample=dict(num_samples=2, top_p=0.9, seed=3))
        assert (cap.num_samples, cap.top_k, cap.top_p, cap.sample_seed) == (2, 0, 0.9, 3)
        Evaluator(model, sample=dict(num_samples=2))
        assert cap.top_p is None
    finally:
        for k in ("num_samples", "temperature", "top_k", "top_p", "sample_seed"):
            cap.__dict__.pop(k, None)
    # SelfCritical checks its sampler's settings before it looks at anything else but the corpus' type
    import inspect
    assert inspect.signature(SelfCritical.__init__).parameters["top_p"].default is None
    assert list(inspect.signature(check_arguments).parameters)[-1] == "top_p"


# ---- 4. the C ABI ----------------------------------------------------------------------------------------------------------------
NAMES = (("spacap_sample_word_nucleus_workspace_bytes", "size_t"), ("spacap_sample_word_nucleus_f32", "int"))


def test_symbols_are_declared_and_exported():
    from spacap3d_amd import _native
    header = open(os.path.join(os.path.dirname(HERE), "include", "spacap_hip.h")).read()
    for name, ret in NAMES:
        m = re.search(r"\b%s %s\(([^;]*)\);" % (ret, name), header)
        assert m, name
        assert name in _native.SIGNATURES and hasattr(_native.lib, name)
        assert len(m.group(1).split(",")) == len(_native.SIGNATURES[name][1]), name      # as many arguments on both sides
    old = re.search(r"\bint spacap_sample_word_f32\(([^;]*)\);", header).group(1)
    new = re.search(r"\bint spacap_sample_word_nucleus_f32\(([^;]*)\);", header).group(1)
    norm = lambda s: [" ".join(a.split()) for a in s.split(",")]  # noqa: E731
    assert norm(new) == [a if a != "int top_k" else "float top_p" for a in norm(old)]      # the existing entry with top_p for top_k


def _call(**over):
    """spacap_sample_word_nucleus_f32 with small non-null fake pointers (16-byte aligned; a refused call never touches them)"""
    from spacap3d_amd import _native
    a = dict(x=0x1000, Wp=0x2000, bias=0x3000, rows=4, V=40, top_p=0.5, inv_tau=1.0, seed=7, seed_dev=None, n_words=31, step=5, eos=1,
             lut=0x4000, scale=1.0, pe_row=0x5000, ys=0x6000, score=0x7000, length=0x8000, finished=0x9000, xw=0xA000,
             workspace=0xB000, stream=None)
    a.update(over)
    return _native.lib.spacap_sample_word_nucleus_f32(*a.values()), _native.lib.spacap_last_error()


@pytest.mark.parametrize("over", [dict(rows=-1), dict(V=0), dict(V=16385), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.5),
                                  dict(top_p=float("nan")), dict(top_p=float("inf")), dict(inv_tau=0.0), dict(inv_tau=-1.0),
                                  dict(inv_tau=float("inf")), dict(inv_tau=float("nan")), dict(step=-1), dict(step=31), dict(eos=40),
                                  dict(eos=-1), dict(x=None), dict(Wp=None), dict(bias=None), dict(lut=None), dict(pe_row=None),
                                  dict(ys=None), dict(score=None), dict(length=None), dict(finished=None), dict(xw=None),
                                  dict(workspace=None), dict(workspace=0xB004), dict(xw=0xA008)],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_nucleus_entry_refuses_before_any_device_call(over):
    rc, msg = _call(**over)
    assert rc == -1 and b"spacap_sample_word_nucleus_f32" in msg


def test_nucleus_entry_with_no_rows_does_nothing_and_sizes_its_workspace():
    from spacap3d_amd import _native
    size = _native.lib.spacap_sample_word_nucleus_workspace_bytes
    assert _call(rows=0)[0] == 0
    assert size(0, 40) == 0 and size(5, 0) == 0 and size(5, 16385) == 0
    assert size(5, 40) == 5 * 64 * 4 and size(5, 64) == 5 * 64 * 4 and size(7, 65) == 7 * 128 * 4 and size(2048, 3500) == 2048 * 3520 * 4
    assert size(3, 16384) == 3 * 16384 * 4
