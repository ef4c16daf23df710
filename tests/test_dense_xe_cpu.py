"""Cross-entropy caption training over every matched object of a scene without a GPU: the restated row
construction (tests/dense_xe_restated.py) against the reference's own rule for one sentence, the properties of the restated
draw -- distinct references inside a group, empty rows behind an object's last sentence, uniformity of the first reference --
over the corpus the kernel test runs, and the argument refusals of ``DenseCaptionXE``.  That the new entry point is declared and
bound is tests/test_capi_cpu.py's check of every symbol."""
import numpy as np
import pytest

import dense_xe_restated as DX

UNIFORM_SEED = 20261021          # chosen once, before the counts below were looked at, and kept


def _corpus(sentences_per_key, w2i):
    from spacap3d_amd.caption_eval import CaptionCorpus
    corpus = {"k%d" % i: list(s) for i, s in enumerate(sentences_per_key)}
    return CaptionCorpus(corpus, w2i, key_of=np.arange(len(corpus), dtype=np.int32).reshape(1, -1))


def _sentence(n_words, oov):
    """n_words vocabulary words, those at the positions ``oov`` replaced by words outside the vocabulary"""
    words = [f"w{4 + (3 * i) % (DX.N_VOCAB - 4)}" for i in range(n_words)]
    for i in oov:
        words[i] = f"out{i}"
    return "sos " + " ".join(words) + " eos"


@pytest.mark.parametrize("n_words", (1, 29, 30, 31, 45))
def test_the_two_roads_agree_on_one_sentence(n_words):
    """The kernel's rule over the corpus's ids and the reference's rule over the words give one row: outside words first, last,
    adjacent (and, for the long sentences, on both sides of the cut)."""
    variants = [(), (0,), (n_words - 1,), (0, n_words - 1)]
    if n_words >= 4:
        variants += [(1, 2), (n_words - 2, n_words - 1), (0, 1, n_words - 1)]
    if n_words > 30:
        variants += [(29, 30), (28, 29), (30,)]
    sents = [_sentence(n_words, v) for v in variants]
    cc = _corpus([sents], DX.W2I)
    assert cc.n_vocab == DX.N_VOCAB
    for j, s in enumerate(sents):
        ids = cc.ref_tok[cc.ref_off[j]:cc.ref_off[j] + cc.ref_len[j]]
        assert len(ids) == n_words + 2 and (len(variants[j]) == 0 or ids.max() >= DX.N_VOCAB)
        row, length = DX.id_row(ids, DX.T_IDS, DX.N_VOCAB, DX.UNK, DX.EOS)
        want = DX.sentence_row(s, DX.W2I)
        np.testing.assert_array_equal(np.array(row), want, err_msg=f"{n_words} words, outside at {variants[j]}")
        assert length == min(n_words, 30) + 1 == int((want != 0).sum()) - 1
        assert row[length] == DX.EOS and all(t == 0 for t in row[length + 1:])


def test_hand_corpus_holds_what_it_is_built_for():
    corpus, w2i = DX.hand_corpus()
    cc = _corpus(list(corpus.values()), w2i)
    assert tuple(np.diff(cc.key_ref_off)) == DX.REFS_PER_KEY
    assert {32, 33, 64, 3} <= set(cc.ref_len.tolist()) and cc.ref_len.max() == 64
    assert (cc.ref_tok == DX.N_VOCAB - 1).any() and (cc.ref_tok == DX.N_VOCAB).any() and cc.ref_tok[-2] == cc.ref_tok.max() > DX.N_VOCAB
    for case in DX.TARGET_CASES:
        key = DX.key_array(case)
        assert key.shape == case[:2]
        if case[0] > 1:
            assert (key[-1] == -1).all() and (key[:-1] >= 0).any()
        if case[0] > 2:
            assert (key[0] == 4).any() and (key[1] == 4).any()
    assert (DX.key_array((5, 128, 2)) == len(DX.REFS_PER_KEY)).sum() == 1
    assert set(np.unique(DX.key_array((5, 128, 2)))) == set(range(-1, len(DX.REFS_PER_KEY) + 1))


@pytest.mark.parametrize("case", DX.TARGET_CASES, ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("word", DX.DEVICE_WORDS, ids=lambda w: f"dev{w}")
def test_restated_rows_distinct_references_and_empty_rows(case, word):
    B, M, r = case
    corpus, w2i = DX.hand_corpus()
    cc = _corpus(list(corpus.values()), w2i)
    key = DX.key_array(case)
    t = DX.targets(key, cc.ref_tok, cc.ref_off, cc.ref_len, cc.key_ref_off, cc.n_vocab, DX.UNK, DX.SOS, DX.EOS, r, DX.T_IDS,
                   DX.HOST_SEED, word)
    sents = [s for v in corpus.values() for s in v]
    for g, k in enumerate(key.reshape(-1)):
        n = DX.REFS_PER_KEY[k] if 0 <= k < len(DX.REFS_PER_KEY) else 0
        ref = t.ref[g * r:(g + 1) * r]
        live = ref >= 0
        np.testing.assert_array_equal(live, np.arange(r) < n)                       # rows s >= n are empty
        np.testing.assert_array_equal(t.good[g * r:(g + 1) * r], live)
        assert len(set(ref[live])) == live.sum()                                     # distinct inside a group (all n when n < r)
        if n:
            assert (ref[live] >= cc.key_ref_off[k]).all() and (ref[live] < cc.key_ref_off[k + 1]).all()
            np.testing.assert_array_equal((ref[live] - cc.key_ref_off[k]), (ref[0] - cc.key_ref_off[k] + np.arange(live.sum())) % n)
        for s in range(r):
            row = g * r + s
            if live[s]:
                np.testing.assert_array_equal(t.ids[row], DX.sentence_row(sents[ref[s]], w2i))
                assert t.length[row] == (t.ids[row] != 0).sum() - 1
            else:
                assert t.ids[row].tolist() == [DX.SOS, DX.EOS] + [0] * (DX.T_IDS - 2) and t.length[row] == 0
    assert (t.tok[:, 0] == 1).all() and (t.tok[:, 1:] == t.ids).all() and t.ids.max() < DX.N_VOCAB


def test_another_device_word_draws_other_references():
    corpus, w2i = DX.hand_corpus()
    cc = _corpus(list(corpus.values()), w2i)
    key = DX.key_array((5, 128, 2))
    run = lambda seed, word: DX.targets(key, cc.ref_tok, cc.ref_off, cc.ref_len, cc.key_ref_off, cc.n_vocab, DX.UNK, DX.SOS, DX.EOS,
                                        2, DX.T_IDS, seed, word).ref
    a, b, c, d = run(DX.HOST_SEED, None), run(DX.HOST_SEED, 0), run(DX.HOST_SEED, 1), run(DX.HOST_SEED + 1, None)
    np.testing.assert_array_equal(a, b)          # a device word of 0 adds nothing
    assert (a != c).any() and (a != d).any() and ((a >= 0) == (c >= 0)).all()
    assert DX.make_seed(2 ** 64 - 1, 1) == ((DX.GOLDEN - 1) & DX.M32, (DX.GOLDEN - 1) >> 32)       # the sum wraps at 2^64


@pytest.mark.parametrize("n", (3, 7))
def test_first_reference_is_uniform(n):
    """6 000 groups over n references: every reference is the first one N/n +- 5 sigma times, sigma the binomial's."""
    N = 6000
    sd = DX.make_seed(UNIFORM_SEED)
    count = np.bincount([DX.first_reference(g, n, sd) for g in range(N)], minlength=n)
    bound = 5.0 * np.sqrt(N * (1.0 / n) * (1.0 - 1.0 / n))
    print(f"n = {n}: counts {count.tolist()}, expected {N / n:.1f} +- {bound:.1f}")
    assert count.sum() == N and len(count) == n
    assert (np.abs(count - N / n) <= bound).all()
    if n == 3:
        assert int(bound) == 182                  # 2000 +- 183, rounded outward


def test_constructor_refusals():
    from spacap3d_amd.dense_xe import DenseCaptionXE
    corpus, w2i = DX.hand_corpus()
    cc = _corpus(list(corpus.values()), w2i)
    ok = DenseCaptionXE(cc, DX.SOS, DX.EOS, DX.UNK)
    assert (ok.max_proposals, ok.near_threshold, ok.refs_per_object, ok.seed) == (16, 0.3, 1, None)
    assert ok.near2 == float(np.float32(0.3) * np.float32(0.3))
    assert DenseCaptionXE(cc, DX.SOS, DX.EOS, DX.UNK, max_proposals=128, refs_per_object=8, seed=5).seed == 5
    with pytest.raises(TypeError):
        DenseCaptionXE(corpus, DX.SOS, DX.EOS, DX.UNK)
    for kw in ({"max_proposals": 0}, {"max_proposals": 129}, {"near_threshold": 0.0}, {"near_threshold": -1.0},
               {"near_threshold": float("nan")}, {"refs_per_object": 0}, {"refs_per_object": 9}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            DenseCaptionXE(cc, DX.SOS, DX.EOS, DX.UNK, **kw)
    for words in ((65536, DX.EOS, DX.UNK), (DX.SOS, -1, DX.UNK), (DX.SOS, DX.EOS, 65536)):
        with pytest.raises(ValueError, match="65536"):
            DenseCaptionXE(cc, *words)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ok.targets(np.zeros((1, 16), np.int32))
    import torch
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ok.targets(torch.zeros(1, 16, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ok.select(torch.zeros(1, 4, 3), torch.zeros(1, 16, 3), torch.zeros(1, 16), torch.zeros(1, 16, dtype=torch.long), torch.zeros(1))
