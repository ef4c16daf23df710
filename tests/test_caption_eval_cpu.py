"""No-GPU checks of the caption metrics (spacap3d_amd/caption_eval.py): the numpy restatement
(tests/caption_eval_restated.py) reproduces the reference's recorded results (tests/golden/caption_eval_ref.npz, made by
tests/golden/make_fixtures_caption.py from lib/capeval's Bleu / Cider / Rouge and lib/eval_helper.py's feed_scene_cap),
``CaptionCorpus`` tokenises, numbers words outside the vocabulary, builds the key table and the document-frequency tables
and refuses what does not fit, the C entry points reject bad arguments without touching a device, and the Python layer
refuses CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import caption_eval_restated as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "caption_eval_ref.npz"))
SCORE_CASES = ("edge", "random")
SELECT_INPUTS = ("tokens", "nms_masks", "good_bbox_masks", "dataset_idx", "scene_object_ids", "object_assignment")
_RESTATED = {}


def corpus_of(case):
    """(corpus dict of word strings, word2idx) of a fixture case; keys ``k<i>`` (``select``: the recorded keys)."""
    refs = R.refs_of(FIX, case)
    keys = [str(k) for k in FIX["select/keys"]] if case == "select" else ["k%d" % i for i in range(len(refs))]
    return {k: [R.sentence(r) for r in rs] for k, rs in zip(keys, refs)}, R.vocabulary(int(FIX[f"{case}/vocab"]))


def restated(case):
    if case not in _RESTATED:   # computed once, shared, never modified
        _RESTATED[case] = R.score_all(FIX[f"{case}/cand_tok"], FIX[f"{case}/cand_len"], R.refs_of(FIX, case))
    return _RESTATED[case]


def select_organized():
    org = {}
    for s, o, n in FIX["select/organized"]:
        org.setdefault(str(s), {})[str(o)] = {"0": {"object_name": str(n)}, "1": {"object_name": str(n) + "_other"}}
    return org


@pytest.mark.parametrize("case", SCORE_CASES)
def test_restatement_reproduces_the_reference(case):
    got = restated(case)
    np.testing.assert_array_equal(got["bleu_comp"], FIX[f"{case}/bleu_comp"])
    assert got["bleu"] == list(FIX[f"{case}/bleu"])
    assert got["rouge_scores"].tobytes() == FIX[f"{case}/rouge_scores"].tobytes()
    assert got["rouge"] == float(FIX[f"{case}/rouge"])
    assert np.max(np.abs(got["cider_scores"] - FIX[f"{case}/cider_scores"])) <= 1e-12
    assert abs(got["cider"] - float(FIX[f"{case}/cider"])) <= 1e-12


def test_restated_selection_reproduces_feed_scene_cap():
    d = {k: FIX[f"select/{k}"] for k in SELECT_INPUTS}
    table = R.new_table(len(FIX["select/keys"]), R.SOS, R.EOS)
    for s, suffix in ((0, "_step1"), (1, "")):
        R.select(table, *(d[k][s] for k in SELECT_INPUTS), FIX["select/key_table"], R.SOS, R.EOS)
        np.testing.assert_array_equal(table[0], FIX[f"select/cand_tok{suffix}"])
        np.testing.assert_array_equal(table[1], FIX[f"select/cand_len{suffix}"])


def test_fixture_holds_the_cases_it_is_for():
    for case in SCORE_CASES:
        comp, cd, rg = FIX[f"{case}/bleu_comp"], FIX[f"{case}/cider_scores"], FIX[f"{case}/rouge_scores"]
        assert (cd > 0).any() and ((rg > 0) & (rg < 1)).any() and (comp[:, 0] < comp[:, 1]).any()
        assert (FIX[f"{case}/cand_len"] == 2).any()                                   # a placeholder
    comp = FIX["edge/bleu_comp"]
    assert list(comp[0, 2:6]) == [2, 1, 0, 0]                                          # the placeholder's guesses
    assert list(comp[3, :2]) == [6, 5]                                                 # closest-length tie -> the shorter
    assert comp[4, 6] == 4 and comp[4, 7] == 3                                         # sos a a eos: a clipped to 2 of 4
    assert comp[11, 0] == 64 and FIX["edge/ref_len"].max() == 64
    assert sorted(set(FIX["edge/key_nref"])) [0] == 1 and FIX["edge/key_nref"].max() == 9
    assert (FIX["edge/ref_tok"] >= int(FIX["edge/vocab"])).sum() == 4                  # words outside the vocabulary
    assert FIX["edge/rouge_scores"][10] == 1.0
    assert FIX["edge/cider_scores"][12] == 0 and 0 < FIX["edge/rouge_scores"][12] < 1  # only sos / eos shared: idf 0, LCS 2
    assert len(FIX["random/cand_len"]) == 300
    t = FIX["select/tokens"]
    assert t.shape == (2, 2, 64, 31) and FIX["select/cand_len"].max() == 33 and (FIX["select/cand_len"] == 2).sum() >= 3
    assert (FIX["select/cand_tok_step1"] != FIX["select/cand_tok"]).any()


def test_corpus_tokenisation_oov_ids_and_tables():
    from spacap3d_amd.caption_eval import CaptionCorpus
    corpus, w2i = corpus_of("edge")
    V = len(w2i)
    c = CaptionCorpus(corpus, w2i, key_of=np.arange(len(corpus), dtype=np.int64)[None])
    refs = R.refs_of(FIX, "edge")
    assert c.keys == list(corpus) and c.nkeys == 16 and c.key_table.dtype == np.int32 and c.key_table.shape == (1, 16)
    np.testing.assert_array_equal(c.ref_len, FIX["edge/ref_len"])
    np.testing.assert_array_equal(c.key_ref_off, np.concatenate([[0], np.cumsum(FIX["edge/key_nref"])]))
    np.testing.assert_array_equal(c.ref_off, np.concatenate([[0], np.cumsum(FIX["edge/ref_len"])])[:-1])
    # words of the vocabulary keep their ids; the two other words get V and V + 1 in order of appearance
    want = FIX["edge/ref_tok"].copy()
    fresh = {}
    for i, t in enumerate(want):
        if t >= V:
            want[i] = fresh.setdefault(int(t), V + len(fresh))
    np.testing.assert_array_equal(c.ref_tok, want)
    assert len(fresh) == 2 and c.n_ids == V + 2
    # document frequencies against the restatement's dict (over the fixture's own ids: a renaming of the same words)
    df = R.doc_freq(refs)
    rename = {**{i: i for i in range(V)}, **fresh}
    packed = {}
    for g, n in df.items():
        code = 0
        for t in g:
            code = (code << 16) | rename[t]
        packed[len(g), code] = n
    assert c.df_off[0] == 0 and c.df_off[4] == len(c.df_code) == len(packed)
    for n in range(1, 5):
        codes = c.df_code[c.df_off[n - 1]:c.df_off[n]]
        assert codes.dtype == np.uint64 and np.all(codes[1:] > codes[:-1])
        for code, d in zip(codes, c.df[c.df_off[n - 1]:c.df_off[n]]):
            assert packed[n, int(code)] == d
    assert c.log_nkeys == np.log(16.0)
    for d, idf in zip(c.df, c.df_idf):
        assert idf == np.log(16.0) - np.log(max(1.0, float(d)))
    assert c.df_idf[c.df == 16].tolist() == [0.0] * int((c.df == 16).sum()) and (c.df == 16).sum() >= 2   # sos, eos


def test_corpus_refuses_what_does_not_fit():
    from spacap3d_amd.caption_eval import CaptionCorpus
    kt = np.zeros((1, 1), np.int32)
    with pytest.raises(ValueError, match="65 tokens"):
        CaptionCorpus({"k": ["sos " + "a " * 63 + "eos"]}, {"sos": 0, "eos": 1, "a": 2}, key_of=kt)
    CaptionCorpus({"k": ["sos " + "a " * 62 + "eos"]}, {"sos": 0, "eos": 1, "a": 2}, key_of=kt)          # 64 fit
    big = {"w%d" % i: i for i in range(65535)}
    CaptionCorpus({"k": ["w1 w2"]}, big, key_of=kt)                                                   # 65 535 ids fit
    with pytest.raises(ValueError, match="16 bits"):
        CaptionCorpus({"k": ["w1 stranger"]}, big, key_of=kt)                                         # the 65 536th does not
    with pytest.raises(ValueError, match="key_of"):
        CaptionCorpus({"k": ["a"]}, {"a": 0})


def test_key_table_from_organized():
    from spacap3d_amd.caption_eval import CaptionCorpus
    corpus, w2i = corpus_of("select")
    c = CaptionCorpus(corpus, w2i, organized=select_organized(), scene_ids=[str(s) for s in FIX["select/scene_ids"]])
    want = FIX["select/key_table"]
    got = c.key_table
    assert got.shape[0] == want.shape[0] and got.shape[1] <= want.shape[1]     # (columns past the last known object are -1)
    np.testing.assert_array_equal(got, want[:, :got.shape[1]])
    assert (want[:, got.shape[1]:] == -1).all() and (want == -1).any() and want[1, 9] == -1   # sB|9|lamp: not a corpus key


def test_entry_points_reject_bad_arguments_without_a_device():
    from spacap3d_amd._native import lib
    s = lambda B=1, K=64, L=31, M=8, items=1, nobj=1, nkeys=1, sos=2, eos=3: lib.spacap_caption_select_i32(
        None, None, None, None, None, None, B, K, L, M, None, items, nobj, nkeys, sos, eos, None, None, None, None, None)
    for bad in (dict(B=-1), dict(K=0), dict(L=0), dict(L=63), dict(M=0), dict(items=0), dict(nobj=0), dict(nkeys=0),
                dict(sos=-1), dict(eos=65536)):
        assert s(**bad) == -1, bad
        assert b"bad sizes" in lib.spacap_last_error()
    assert s() == -1 and b"null" in lib.spacap_last_error()
    assert s(B=0) == 0 and s(L=62, B=0) == 0
    off = (ctypes.c_int64 * 5)(0, 1, 2, 3, 4)
    c = lambda nkeys=1, n_tok=1, n_ref=1, o=off: lib.spacap_caption_score_f64(
        None, None, nkeys, None, n_tok, None, None, n_ref, None, None, None, o, 0.0, None, None, None, None)
    for bad in (dict(nkeys=-1), dict(n_tok=-1), dict(n_ref=-1)):
        assert c(**bad) == -1, bad
        assert b"bad sizes" in lib.spacap_last_error()
    assert c() == -1 and b"null" in lib.spacap_last_error()
    assert c(nkeys=0) == 0


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    from spacap3d_amd.caption_eval import CaptionCorpus, CaptionEval, corpus_bleu
    from spacap3d_amd.engine import Evaluator
    corpus, w2i = corpus_of("select")
    c = CaptionCorpus(corpus, w2i, key_of=FIX["select/key_table"])
    ce = CaptionEval(c, R.SOS, R.EOS)
    d = {k: torch.from_numpy(FIX[f"select/{k}"][0]) for k in SELECT_INPUTS}
    d["lang_cap"] = d["tokens"]
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ce.step(d, masks=d)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ce.set_candidates(torch.zeros(8, 64, dtype=torch.int32), torch.zeros(8, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="before any step"):
        ce.compute_metrics()
    assert ce.candidates({str(i): R.word(i) for i in range(50)}) == {k: ["sos eos"] for k in corpus}
    with pytest.raises(TypeError):
        CaptionEval(corpus, R.SOS, R.EOS)
    with pytest.raises(ValueError):
        Evaluator(None, caption_eval=ce)
    for case in SCORE_CASES:
        assert corpus_bleu([int(x) for x in FIX[f"{case}/bleu_comp"].sum(0)]) == list(FIX[f"{case}/bleu"])


def test_symbols_are_declared_and_exported():
    from spacap3d_amd import _native, caption_eval
    header = open(os.path.join(os.path.dirname(HERE), "include", "spacap_hip.h")).read()
    for name in ("spacap_caption_select_i32", "spacap_caption_score_f64"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _native.SIGNATURES and hasattr(_native.lib, name)
    assert caption_eval.LMAX == R.LMAX == 64
