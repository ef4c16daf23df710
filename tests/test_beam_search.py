"""Beam search without a GPU: spacap3d_amd.beam_search (the generic path) against the float64 restatement of the contract
(tests/beam_search_restated.py), the width-1 beam against the reference's recorded greedy captions, and
the C ABI of csrc/caption_decode.hip."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from beam_search_restated import beam_search_restated  # noqa: E402

V, R, N_WORDS, SOS, EOS = 7, 5, 6, 0, 1


def _table():
    """logp[r][previous word][step] -> (V,) log-probabilities: multiples of 2^-10 (coarse ones: 1/4), so every fp32 sum is
    exact and equal scores abound; on top of those, planted: two equal words, two previous words with the same continuation
    (equal scores across beams), and eos made the best word at a different step for each sequence (the last never finishes)."""
    g = np.random.default_rng(5)
    t = -g.integers(1, 9, size=(R, V, N_WORDS, V)).astype(np.float64) / 4 - g.integers(0, 4, size=(R, V, N_WORDS, V)) / 1024.0
    t[:, :, :, EOS] = -6.0                           # eos: unattractive ...
    for r in range(R - 1):
        t[r, :, r + 1, EOS] = -1.0 / 1024            # ... except at step r + 1 of sequence r < R - 1
    t[0, :, 0, 2] = t[0, :, 0, 3] = -0.25            # equal words at the first step
    t[1, :, 0, 4] = t[1, :, 0, 5] = -0.5
    t[1, 4, 1] = t[1, 5, 1]                          # beams 4.. and 5.. continue identically: equal scores across beams
    t[2, :, 3] = t[2, 2, 3]                          # every beam of sequence 2 sees the same step 3
    assert np.array_equal(t * 1024, np.round(t * 1024))
    return t


@pytest.mark.parametrize("alpha", [0.0, 0.7])
@pytest.mark.parametrize("W", [1, 2, 3, 7])
def test_generic_beam_search_equals_the_restatement(W, alpha):
    from spacap3d_amd.beam_search import beam_search
    table = _table()
    want = beam_search_restated(lambda s, r, j, last, toks: table[r, last, s], R, W, N_WORDS, SOS, EOS, alpha)
    tt = torch.from_numpy(table).float()
    rows = torch.arange(R * W) // W
    seen = []

    def step_fn(s, words, parents):
        seen.append(None if parents is None else parents.clone())
        return tt[rows, words, s]

    got = beam_search(step_fn, R, W, N_WORDS, SOS, EOS, alpha)
    for k in ("ys", "beams", "lengths", "parent", "word"):
        assert np.array_equal(got[k].numpy(), want[k]), k
    for k in ("score", "scores"):
        assert got[k].dtype == torch.float32 and np.array_equal(got[k].numpy(), want[k].astype(np.float32)), k
    fin = np.isfinite(want["gap"])
    assert np.array_equal(got["gap"].numpy()[fin], want["gap"][fin].astype(np.float32))
    # the step function is told the ROW every hypothesis continues
    assert seen[0] is None
    for s in range(1, N_WORDS):
        assert np.array_equal(seen[s].view(R, W).numpy(), np.arange(R)[:, None] * W + want["parent"][s - 1])
    # the fixture does what it says: sequences finish at different steps, one never does, and ties were there to break
    if W == 3:
        first = [(list(y) + [EOS]).index(EOS) for y in want["ys"]]
        assert len(set(first[:R - 1])) > 1 and EOS not in want["ys"][R - 1]
        assert (want["gap"] == 0).any()


def test_selection_breaks_ties_by_index():
    from spacap3d_amd.beam_search import select_top
    cand = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0, -float("inf")], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    vals, idx = select_top(cand, 4)
    assert vals.tolist() == [[3.0, 3.0, 3.0, 2.0], [0.0] * 4] and idx.tolist() == [[1, 2, 4, 3], [0, 1, 2, 3]]


def test_width_one_through_the_generic_path_reproduces_the_reference_captions():
    """The one place the reference pins beam search: a beam of width 1 is its greedy decoder.  The cfg1 model on the CPU oracle
    backend, ``beam_size=1`` sent through beam_search.beam_search: the recorded ``lang_cap`` of the reference's own run
    (tests/golden/eval_greedy_cfg1.npz), compared through each row's first eos (behind it a beam repeats eos, the greedy loop
    goes on choosing words), or all words where there is none."""
    from oracle.attention_ref import OracleBackend
    from spacap3d_amd import backend
    from test_golden import G, _build, _inputs
    fx = np.load(os.path.join(G, "train_step_cfg1.npz"))
    ev = np.load(os.path.join(G, "eval_greedy_cfg1.npz"))
    with backend.use_backend(OracleBackend()), torch.no_grad():
        model = _build(fx, "cpu").eval()
        model.caption.beam_generic = True
        assert "beam_size" not in model.state_dict() and model.caption.beam_size == 1 and model.caption.length_penalty == 0.0
        d = model(_inputs(fx, "cpu"), is_eval=True)
    caps, ref = d["lang_cap"].numpy(), ev["lang_cap"]
    assert caps.shape == ref.shape and d["lang_cap_score"].shape == ref.shape[:2]
    eos = model.caption.word_to_idx["eos"]
    n = ref.shape[-1]
    for got, want in zip(caps.reshape(-1, n), ref.reshape(-1, n)):
        hit = np.flatnonzero(want == eos)
        upto = int(hit[0]) + 1 if hit.size else n
        assert np.array_equal(got[:upto], want[:upto])
        assert (got[upto:] == eos).all()
    assert np.isfinite(d["lang_cap_score"].numpy()).all()


def test_symbols_are_declared_and_exported():
    from spacap3d_amd import _native
    header = open(os.path.join(os.path.dirname(HERE), "include", "spacap_hip.h")).read()
    for name, ret in (("spacap_beam_topw_workspace_bytes", "size_t"), ("spacap_beam_topw_f32", "int"),
                      ("spacap_decode_attn_beam_f32", "int"), ("spacap_beam_step_f32", "int"), ("spacap_beam_finish_f32", "int")):
        m = re.search(r"\b%s %s\(([^;]*)\);" % (ret, name), header)
        assert m, name
        assert name in _native.SIGNATURES and hasattr(_native.lib, name)
        assert len(m.group(1).split(",")) == len(_native.SIGNATURES[name][1]), name      # as many arguments on both sides
    # invalid widths are refused before anything is launched (no device needed to say so)
    assert _native.lib.spacap_beam_topw_f32(None, None, None, 4, 3, 5, None, None, None, None) != 0
    assert b"W <= V" in _native.lib.spacap_last_error()
    assert _native.lib.spacap_beam_topw_f32(None, None, None, 4, 100, 9, None, None, None, None) != 0
    assert _native.lib.spacap_decode_attn_beam_f32(None, None, None, None, 4, 9, 8, 16, 32, 0, 0.25, None, None) != 0


def test_evaluator_sets_the_decoding_attributes():
    from spacap3d_amd.engine import Evaluator
    from spacap3d_amd.spacapnet import build_default
    model = build_default(vocab_size=40, num_proposal=8, N=1, d_ff=128)
    keys = set(model.state_dict())
    Evaluator(model)
    assert model.caption.beam_size == 1 and model.caption.length_penalty == 0.0
    Evaluator(model, beam_size=3, length_penalty=0.7)
    assert model.caption.beam_size == 3 and model.caption.length_penalty == 0.7 and set(model.state_dict()) == keys
    with pytest.raises(ValueError):
        Evaluator(model, beam_size=0)
    with pytest.raises(ValueError):
        model.caption.forward_eval({}, use_cache=False, beam_size=2)
