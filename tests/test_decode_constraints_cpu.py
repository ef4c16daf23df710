"""Constrained caption decoding without a GPU: the numpy restatement against hand-written cases, the torch
rule (spacap3d_amd/decode_constraints.py) against the restatement, the refusals, the generic beam search / sampler / greedy loop
on the CPU oracle backend, and the condition on the inputs of the one-step GPU tests (tests/test_decode_constraints_gpu.py)."""
import os
import re

import numpy as np
import pytest
import torch

import decode_constraints_restated as CR
import sampling_restated as SR

HERE = os.path.dirname(os.path.abspath(__file__))
INF = float("inf")


# ---- 1. the restatement on hand-written cases ------------------------------------------------------------------------------------
def test_ngram_rule_by_hand():
    h = [5, 7, 5, 7, 5]                                   # overlapping repeats
    assert CR.ngram_bans(h, 1) == {5, 7}
    assert CR.ngram_bans(h, 2) == {7}                     # (5, 7) occurred; (5, 5) did not
    assert CR.ngram_bans(h, 3) == {7}                     # the tail (7, 5) was followed by 7
    assert CR.ngram_bans([5, 7, 5, 7], 3) == {5}          # the tail (5, 7) was followed by 5
    assert CR.ngram_bans([1, 2, 3, 1, 2], 3) == {3}
    assert CR.ngram_bans([1, 2, 3, 4, 2], 3) == set()
    assert CR.ngram_bans([4, 4, 4], 2) == {4} and CR.ngram_bans([4, 4, 4], 3) == {4}
    assert CR.ngram_bans([4, 4], 3) == set()              # two words hold no trigram yet
    # i < n - 1, and i = n - 1: nothing to repeat
    assert CR.ngram_bans([], 1) == set() and CR.ngram_bans([], 2) == set() and CR.ngram_bans([3], 3) == set()
    assert CR.ngram_bans([3], 2) == set() and CR.ngram_bans([3, 3], 2) == {3}
    assert CR.ngram_bans(h, 0) == set()


def test_penalty_min_length_and_bad_words_by_hand():
    z = np.array([2.0, -2.0, 0.0, 1.0, -1.0, 3.0], np.float32)
    out = CR.constrain(z, [0, 1, 2, 0], eos=5, theta=2.0)
    assert out.dtype == np.float32 and out.tolist() == [1.0, -4.0, 0.0, 1.0, -1.0, 3.0]      # positive / 2, negative * 2, zero stays; once per word
    th = np.float32(1.3)
    out = CR.constrain(z, [0, 1], eos=5, theta=1.3)
    assert out[0] == np.float32(2.0) / th and out[1] == np.float32(-2.0) * th                 # one float32 operation
    # min_length: eos banned at i = min_length - 1, allowed at i = min_length
    assert CR.constrain(z, [3, 4], eos=5, min_length=3)[5] == -INF
    assert CR.constrain(z, [3, 4, 3], eos=5, min_length=3)[5] == 3.0
    # a bad word that is also in the history: penalised, then banned
    out = CR.constrain(z, [0, 3], eos=5, theta=2.0, bad_words=(0, 4))
    assert out.tolist() == [-INF, -2.0, 0.0, 0.5, -INF, 3.0]
    # the order: the penalty acts on z, the ban on the result (a banned word stays -inf whatever its sign)
    assert CR.constrain(z, [1], eos=5, ngram=1, theta=2.0).tolist() == [2.0, -INF, 0.0, 1.0, -1.0, 3.0]


def test_images_and_beam_histories_by_hand():
    hist = np.array([[3, 64, 3, 0, 0]])
    img = CR.images(hist, 3, 70, eos=1, min_length=4, ngram=1, theta=1.0, bad_words=(69,))
    assert img.shape == (1, 2, 4)
    assert img[0, 1].tolist() == [1 << 3, 0, 1, 0]                                            # seen: 3 and 64
    assert img[0, 0].tolist() == [(1 << 3) | (1 << 1), 0, 1 | (1 << 5), 0]                    # banned: 3, 64 (n = 1), eos = 1, 69
    # a hypothesis that changed slots at every position: words are read from the slot it sat in when they were its input
    W, T, step = 3, 6, 3
    tr = np.arange(5 * 2 * W).reshape(5, 2, W)
    anc = np.zeros((2 * W, T), np.int8)
    anc[4] = [0, 0, 2, 0, 9, 1]                            # row 4 = (r 1, w 1): positions 2, 3 in slots 2, 0; position 4 is its own
    got = CR.beam_histories(tr, anc, step, W)
    assert got[4].tolist() == [tr[0, 1, 2], tr[1, 1, 0], tr[2, 1, 1]]
    anc[4, 3] = -1                                         # outside 0..W-1: the row's own slot
    assert CR.beam_histories(tr, anc, step, W)[4].tolist() == [tr[0, 1, 2], tr[1, 1, 1], tr[2, 1, 1]]


def test_caption_faults_by_hand():
    eos = 1
    toks = np.array([[4, 5, 4, 5, 1, 1], [4, 5, 6, 1, 4, 5], [1, 0, 0, 0, 0, 0], [4, 5, 6, 7, 8, 9]])
    assert CR.caption_faults(toks, eos, ngram=2) == [(0, "repeated n-gram")]
    assert CR.caption_faults(toks, eos, min_length=4) == [(1, "too short"), (2, "too short")]
    assert CR.caption_faults(toks, eos, bad_words=(6, 0)) == [(1, "bad word"), (3, "bad word")]   # row 2's zeros lie behind its eos


# ---- 2. the torch rule against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_apply_equals_the_restatement(n):
    from spacap3d_amd.decode_constraints import DecodeConstraints, apply, banned_and_seen
    g = np.random.default_rng(n)
    N, V, eos = 64, 23, 1
    z = g.normal(size=(N, V)) * 3
    z[:, 4] = 0.0
    hist = g.integers(0, 6, size=(N, 9))                   # few distinct words: many repeats
    for step in (0, 1, 2, 5, 9):
        for theta, ml, bad in ((1.0, 0, ()), (1.3, 3, (0, 2, 22)), (2.0, 6, (5,))):
            c = DecodeConstraints(min_length=ml, no_repeat_ngram=n, repetition_penalty=theta, bad_words=bad)
            want = CR.constrain_rows(z, hist, step, eos, min_length=ml, ngram=n, theta=theta, bad_words=bad)
            got = apply(c, torch.from_numpy(z), torch.from_numpy(hist), step, eos)
            assert got.dtype == torch.float32
            got = got.numpy().astype(np.float64)
            assert np.array_equal(np.isneginf(got), np.isneginf(want)), (step, theta)
            fin = np.isfinite(want)
            # float64 in: z and theta are rounded to float32 (2^-24 each), then the one float32 operation (2^-24)
            assert (np.abs(got[fin] - want[fin]) <= 3.001 * 2.0 ** -24 * np.abs(want[fin])).all()
            ban, seen = banned_and_seen(c, torch.from_numpy(hist), step, eos, V)
            img = CR.images(hist, step, V, eos, min_length=ml, ngram=n, theta=theta, bad_words=bad)
            bits = lambda m: np.array([[(int(img[r, m, v // 32]) >> (v % 32)) & 1 for v in range(V)] for r in range(N)], bool)  # noqa: E731
            assert np.array_equal(ban.numpy(), bits(0)) and np.array_equal(seen.numpy(), bits(1))
            # float32 in, float32 restatement: the same bits
            z32 = z.astype(np.float32)
            want32 = CR.constrain_rows(z32, hist, step, eos, min_length=ml, ngram=n, theta=theta, bad_words=bad)
            assert np.array_equal(apply(c, torch.from_numpy(z32), torch.from_numpy(hist), step, eos).numpy(), want32)


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------
def test_constraints_refuse_what_cannot_hold():
    from spacap3d_amd.decode_constraints import DecodeConstraints, resolve
    for kw in (dict(min_length=-1), dict(no_repeat_ngram=-1), dict(repetition_penalty=0.9), dict(repetition_penalty=float("nan")),
               dict(repetition_penalty=float("inf")), dict(bad_words=range(65))):
        with pytest.raises(ValueError):
            DecodeConstraints(**kw)
    with pytest.raises(TypeError):
        resolve(dict(minimum=3))
    V, n, eos = 120, 31, 1
    DecodeConstraints(min_length=30, no_repeat_ngram=2, repetition_penalty=1.2, bad_words=(0, 2, 3)).check("t", V, n, eos)
    for kw in (dict(bad_words=(eos,)), dict(bad_words=(V,)), dict(bad_words=(-1,)), dict(min_length=31)):
        with pytest.raises(ValueError):
            DecodeConstraints(**kw).check("t", V, n, eos)
    with pytest.raises(ValueError):
        DecodeConstraints(bad_words=(0, 2, 3)).check("t", 35, n, eos)      # 3 + 31 + 1 >= 35
    DecodeConstraints(bad_words=(0, 2, 3)).check("t", 36, n, eos)
    assert not DecodeConstraints().active() and resolve(None) is None and resolve(dict(repetition_penalty=1.0)) is None
    assert all(DecodeConstraints(**kw).active() for kw in (dict(min_length=1), dict(no_repeat_ngram=1), dict(repetition_penalty=1.1),
                                                           dict(bad_words=(0,))))


@pytest.fixture(scope="module")
def tiny():
    """The tiny captioner of tests/test_sampling.py on hand-made detector outputs (2 scenes x 8 proposals)."""
    from spacap3d_amd.spacapnet import build_default
    torch.manual_seed(3)
    model = build_default(vocab_size=40, num_proposal=8, N=1, d_ff=128).eval()
    g = torch.Generator().manual_seed(4)
    ep = {"aggregated_vote_features": torch.randn(2, 8, 128, generator=g), "aggregated_vote_xyz": torch.randn(2, 8, 3, generator=g),
          "bbox_mask": torch.ones(2, 8)}
    return model, ep


def test_forward_eval_and_evaluator_refuse_bad_constraints(tiny):
    from spacap3d_amd.engine import Evaluator
    from spacap3d_amd.spacapnet import build_default
    model = build_default(vocab_size=40, num_proposal=8, N=1, d_ff=128)
    cap = model.caption
    keys = set(model.state_dict())
    assert cap.min_length == 0 and cap.no_repeat_ngram == 0 and cap.repetition_penalty == 1.0 and cap.bad_words == ()
    V, eos = cap.model.generator.proj.out_features, cap.word_to_idx["eos"]
    for kw in (dict(min_length=-1), dict(min_length=31), dict(no_repeat_ngram=-2), dict(repetition_penalty=0.5), dict(bad_words=(eos,)),
               dict(bad_words=(V,)), dict(bad_words=tuple(w for w in range(V) if w != eos)[:V - 32]), dict(min_length=2, use_cache=False),
               dict(repetition_penalty=1.2, use_cache=False)):
        with pytest.raises(ValueError):
            cap.forward_eval({}, **kw)
    for c in (dict(min_length=31), dict(bad_words=(eos,)), dict(repetition_penalty=0.0)):
        with pytest.raises(ValueError):
            Evaluator(model, constraints=c)
    with pytest.raises(TypeError):
        Evaluator(model, constraints=dict(ngram=2))
    assert cap.min_length == 0 and cap.bad_words == ()                      # a refused Evaluator sets nothing
    Evaluator(model, constraints=dict(min_length=4, no_repeat_ngram=2, bad_words=[0]))
    assert (cap.min_length, cap.no_repeat_ngram, cap.repetition_penalty, cap.bad_words) == (4, 2, 1.0, (0,))
    assert set(model.state_dict()) == keys                                  # attributes, not parameters


# ---- 4. the C ABI ----------------------------------------------------------------------------------------------------------------
NAMES = (("spacap_decode_constraints_bytes", "size_t"), ("spacap_decode_constraints", "int"), ("spacap_decode_word_constrained_f32", "int"),
         ("spacap_beam_topw_constrained_f32", "int"), ("spacap_sample_word_constrained_f32", "int"),
         ("spacap_sample_word_nucleus_constrained_f32", "int"))


def test_symbols_are_declared_and_exported():
    from spacap3d_amd import _native
    header = open(os.path.join(os.path.dirname(HERE), "include", "spacap_hip.h")).read()
    for name, ret in NAMES:
        m = re.search(r"\b%s %s\(([^;]*)\);" % (ret, name), header)
        assert m, name
        assert name in _native.SIGNATURES and hasattr(_native.lib, name)
        assert len(m.group(1).split(",")) == len(_native.SIGNATURES[name][1]), name
    assert _native.lib.spacap_decode_constraints_bytes(33, 3001) == 33 * 2 * 94 * 4         # 376 bytes a row and image
    assert _native.lib.spacap_decode_constraints_bytes(0, 40) == 0


def _constraints_call(**over):
    """spacap_decode_constraints with fake non-null pointers (a refused call never touches them)"""
    import ctypes
    from spacap3d_amd import _native
    bad = (ctypes.c_int32 * 64)(*range(2, 66))
    a = dict(ys=0x1000, ys_ld=31, trace_word=None, anc=None, R=4, W=1, T=32, V=3001, step=5, eos=1, min_length=0, ngram=2, bad=bad,
             n_bad=3, bits=0x2000, stream=None)
    a.update(over)
    return _native.lib.spacap_decode_constraints(*a.values()), _native.lib.spacap_last_error()


@pytest.mark.parametrize("over", [dict(R=-1), dict(W=0), dict(W=9), dict(V=0), dict(T=33), dict(T=1), dict(step=-1), dict(step=31),
                                  dict(T=6, step=5), dict(eos=-1), dict(eos=3001), dict(min_length=-1), dict(ngram=-1), dict(n_bad=-1),
                                  dict(n_bad=65), dict(bad=None), dict(V=40, n_bad=34), dict(bits=None), dict(ys=None),
                                  dict(ys=None, trace_word=0x3000), dict(W=2), dict(ys_ld=4)],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_constraint_images_refuse_before_any_device_call(over):
    rc, msg = _constraints_call(**over)
    assert rc == -1 and b"spacap_decode_constraints" in msg


def test_constrained_word_choices_refuse_a_missing_image_or_penalty():
    from spacap3d_amd._native import lib
    f = 0x1000
    for bits, theta in ((None, 1.2), (f, 0.9), (f, float("nan")), (f, float("inf"))):
        assert lib.spacap_decode_word_constrained_f32(f, f, f, 4, 40, bits, theta, f, 1.0, f, f, 31, 5, f, f, None) == -1
        assert b"spacap_decode_word_constrained_f32" in lib.spacap_last_error()
        assert lib.spacap_beam_topw_constrained_f32(f, f, f, 4, 40, 3, bits, theta, f, f, f, None) == -1
        assert b"spacap_beam_topw_constrained_f32" in lib.spacap_last_error()
        for k in (0, 3):
            assert lib.spacap_sample_word_constrained_f32(f, f, f, 4, 40, k, 1.0, 7, None, 31, 5, 1, bits, theta, f, 1.0, f, f, f, f, f, f, f,
                                                          None) == -1
            assert b"spacap_sample_word_constrained_f32" in lib.spacap_last_error()
        assert lib.spacap_sample_word_nucleus_constrained_f32(f, f, f, 4, 40, 0.6, 1.0, 7, None, 31, 5, 1, bits, theta, f, 1.0, f, f, f, f, f,
                                                              f, f, None) == -1
        assert b"spacap_sample_word_nucleus_constrained_f32" in lib.spacap_last_error()
    assert _constraints_call(R=0)[0] == 0
    # the unconstrained arguments are still checked, under the constrained entry's name
    assert lib.spacap_beam_topw_constrained_f32(f, f, f, 4, 40, 9, f, 1.2, f, f, f, None) == -1
    assert b"spacap_beam_topw_constrained_f32" in lib.spacap_last_error()


# ---- 5. the generic paths on the CPU oracle backend ------------------------------------------------------------------------------
def _bite(cap):
    sos, eos, unk = cap.word_to_idx["sos"], cap.word_to_idx["eos"], cap.word_to_idx["unk"]
    return dict(bad_words=(0, sos, unk), min_length=4, no_repeat_ngram=2), eos


@pytest.mark.parametrize("mode", ["greedy", "beam", "sample", "sample_top_k", "sample_top_p"])
def test_generic_paths_hold_the_invariants_on_the_cpu_oracle_backend(tiny, mode):
    """forward_eval with bad_words = {0, sos, unk}, min_length = 4, no_repeat_ngram = 2 through the cached per-operator decoder:
    no caption holds a bad word, repeats a bigram or ends before four words -- exactly --, some caption differs from the
    unconstrained run, and the constraints at their off values change nothing."""
    from oracle.attention_ref import OracleBackend
    from spacap3d_amd import backend
    model, ep = tiny
    cap = model.caption
    c, eos = _bite(cap)
    kw = {"greedy": {}, "beam": dict(beam_size=3), "sample": dict(num_samples=3, sample_seed=11),
          "sample_top_k": dict(num_samples=2, top_k=3, temperature=0.7, sample_seed=11),
          "sample_top_p": dict(num_samples=2, top_p=0.6, sample_seed=11)}[mode]
    key = "lang_cap_samples" if mode.startswith("sample") else "lang_cap"
    with backend.use_backend(OracleBackend()), torch.no_grad():
        free = cap.forward_eval(dict(ep), **kw)
        off = cap.forward_eval(dict(ep), min_length=0, no_repeat_ngram=0, repetition_penalty=1.0, bad_words=(), **kw)
        out = cap.forward_eval(dict(ep), **c, **kw)
    for k in free:
        if torch.is_tensor(free[k]):
            assert torch.equal(free[k], off[k]), k
    n = out[key].shape[-1]
    toks = out[key].reshape(-1, n).numpy()
    faults = CR.caption_faults(toks, eos, min_length=c["min_length"], ngram=c["no_repeat_ngram"], bad_words=c["bad_words"])
    before = CR.caption_faults(free[key].reshape(-1, n).numpy(), eos, min_length=c["min_length"], ngram=c["no_repeat_ngram"],
                               bad_words=c["bad_words"])
    print(f"{mode}: {len(before)} faults without constraints, {len(faults)} with")
    assert not faults
    assert before and not np.array_equal(toks, free[key].reshape(-1, n).numpy())      # the constraints bite on this model
    if mode != "greedy":
        assert bool(torch.isfinite(out["lang_cap_score"]).all()) and bool((out["lang_cap_score"] <= 0).all())


def test_generic_beam_width_one_and_top_k_one_are_the_constrained_greedy_words(tiny):
    from oracle.attention_ref import OracleBackend
    from spacap3d_amd import backend
    model, ep = tiny
    cap = model.caption
    c, eos = _bite(cap)
    c = dict(c, repetition_penalty=1.2)
    try:
        with backend.use_backend(OracleBackend()), torch.no_grad():
            greedy = cap.forward_eval(dict(ep), **c)["lang_cap"]
            cap.beam_generic = True
            beam = cap.forward_eval(dict(ep), beam_size=1, **c)["lang_cap"]
            cap.beam_generic = False
            samp = cap.forward_eval(dict(ep), num_samples=1, top_k=1, **c)["lang_cap"]
    finally:
        cap.__dict__.pop("beam_generic", None)
    n = greedy.shape[-1]
    for other in (beam, samp):
        for a, b in zip(greedy.reshape(-1, n).tolist(), other.reshape(-1, n).tolist()):
            assert CR.through_first_eos(a, eos) == CR.through_first_eos(b, eos)


# ---- 6. the inputs of the one-step GPU tests -------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,V", CR.STEP_SHAPES)
def test_one_step_cases_have_few_open_rows(rows, V):
    """By the restatement alone, for every parametrisation of tests/test_decode_constraints_gpu.py's one-step tests: at most
    2 % of the rows are open.  A condition on the inputs (the planted histories and bad words), not a measurement."""
    case = CR.step_case(rows, V, CR.NGRAM_OF[(rows, V)])
    z = case["z"]
    assert np.isfinite(z).sum(1).min() >= 1
    banned_best = int(np.isneginf(z[np.arange(rows), case["logits"].argmax(1)]).sum())
    assert banned_best >= (rows + 1) // 2                                    # the even rows' unconstrained arg-max is banned
    n_open = int((CR.top2_gap(z) < CR.tolerance(z, 1.0)).sum())
    assert n_open <= 0.02 * rows, ("arg-max", n_open)
    for W in CR.TOPW_WIDTHS:
        if W <= V:
            n_open = int(CR.list_open(z, W).sum())
            assert n_open <= 0.02 * rows, ("top-W", W, n_open)
    for tau, k, p in CR.SAMPLE_MODES:
        n_open = int(CR.sample_draw(z, tau, k, p, seed=case["seed"])["open"].sum())
        assert n_open <= 0.02 * rows, ("sample", tau, k, p, n_open)
    pen = CR.penalty_case(rows, V)
    n_open = int((CR.top2_gap(pen["z"]) < CR.tolerance(pen["z"], 1.0)).sum())
    assert n_open <= 0.02 * rows, ("penalty", n_open)
    moved = pen["z"].argmax(1) != pen["logits"].argmax(1)
    assert not moved[1::2].any() and (rows < 16 or moved[0::2].any())        # odd rows keep their word; some even row must move


def test_every_chunk_edge_is_banned_in_some_row():
    for rows, V in CR.STEP_SHAPES:
        case = CR.step_case(rows, V, CR.NGRAM_OF[(rows, V)])
        banned = np.isneginf(case["z"]).any(0)
        edges = CR.edge_words(V)
        want = [w for w in edges if w != case["eos"]]
        assert banned[want].all(), (rows, V)
        assert banned[0] and banned[V - 1] or case["eos"] in (0, V - 1)
        both = set(case["c"]["bad_words"]) & set(case["hist"].reshape(-1).tolist())
        assert both or rows == 1                                             # a bad word that is also in a history
