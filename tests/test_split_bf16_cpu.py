"""The probes of tests/split_bf16_restated.py discriminate: on the host, with fixed seeds, a product that has all six piece
products sits at most a third of the bar, one that lost the probed 2^-16 term at least three bars out, and a plain fp32 product
within the bar -- for the generic shapes and for every probe tests/test_split_bf16_terms_gpu.py runs on the device.  These are
conditions on the INPUTS: if one fails for a seed, the construction changes, not the factor."""
import numpy as np
import pytest

import split_bf16_restated as R


def _five_conditions(A, B, q):
    a, b = R.split3(A), R.split3(B)
    for x, px in ((A, a), (B, b)):
        assert (np.abs(px[0] + px[1] + px[2] - x) <= 2.0 ** -24 * np.abs(x)).all()           # the pieces reproduce the operand
    sk = np.sign(a[R.PA[q]][0])                                                              # the probed product is positive in
    assert (sk != 0).all() and (np.sign(a[R.PA[q]]) == sk[None, :]).all() and (np.sign(b[R.PB[q]]) == sk[:, None]).all()   # every summand
    m6 = R.measures(A, B, R.six_term_product(A, B), q)
    m5 = R.measures(A, B, R.six_term_product(A, B, drop=q), q)
    mf = R.measures(A, B, A @ B, q)
    bar = m6["bar"]
    assert m6["err"].max() <= bar / 3, (m6["err"].max(), bar)
    assert m5["err"].min() >= 3 * bar, (m5["err"].min(), bar)
    assert mf["err"].max() <= bar, (mf["err"].max(), bar)
    return m6


def _bias_conditions(G, p):
    g = R.split3(G)
    assert (np.abs(g[0] + g[1] + g[2] - G) <= 2.0 ** -24 * np.abs(G)).all()
    assert (g[p] > 0).all() and (G > 0).any() and (G < 0).any()
    m = R.bias_measures(G, R.column_sum(G), p)
    bar = m["bar"]
    assert m["err"].max() <= bar / 3
    assert R.bias_measures(G, R.column_sum(G, drop=p), p)["err"].min() >= 3 * bar
    assert R.bias_measures(G, G.sum(0, dtype=np.float32), p)["err"].max() <= bar


@pytest.mark.parametrize("nonneg_a", [False, True])
@pytest.mark.parametrize("K", [64, 128, 256, 512])
@pytest.mark.parametrize("q", [0, 1, 2])
def test_probe_isolates_its_term(q, K, nonneg_a):
    A, B = R.probe(q, 48, K, 40, 0, nonneg_a)
    assert A.dtype == B.dtype == np.float32 and A.shape == (48, K) and B.shape == (K, 40)
    assert not nonneg_a or (A >= 0).all()
    m = _five_conditions(A, B, q)
    assert 0.9e-6 < m["share"].min() < 1.8e-6                                                # 2^-16-ish of sum |a| |b|
    assert np.linalg.matrix_rank(A.astype(np.float64)) == min(48, K) and np.linalg.matrix_rank(B.astype(np.float64)) == 40


@pytest.mark.parametrize("rows", [129, 512])
@pytest.mark.parametrize("p", [1, 2])
def test_bias_probe_isolates_its_piece(p, rows):
    _bias_conditions(R.bias_probe(p, rows, 128, 0), p)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_every_device_probe_meets_the_five_conditions(name):
    M, K, N, nonneg, swapped = R.CASES[name]
    assert K <= 512
    for q in range(3):
        A, B, qp = R.case(name, q)
        assert qp == (R.SWAP[q] if swapped else q) and (not nonneg or (A >= 0).all())
        m = _five_conditions(A, B, qp)
        if nonneg or name == "tf_ffn/fwd/first":
            # a ReLU follows (or may follow) the product: a quarter of the elements must still be able to show a lost term, and
            # the restated product meets the bar against relu(float64) as well
            r = R.relu_measures(A, B, np.maximum(R.six_term_product(A, B), 0), qp)
            assert r["visible"] >= 0.25 and r["err"].max() <= m["bar"] / 3
            lost = R.relu_measures(A, B, np.maximum(R.six_term_product(A, B, drop=qp), 0), qp)
            assert lost["err"].max() >= 3 * m["bar"]


def test_why_the_device_probes_keep_their_pieces_large():
    """The plain construction (floor = 0) misses the conditions at the device shapes: with the seeds in use, the restated
    six-term product -- exact arithmetic, the same on every host -- exceeds bar / 3 in these six of the cases, and with
    R.FLOOR the bar is two to five times the plain one.  Whoever removes the floor has to deal with this first."""
    names, over = sorted(R.CASES), set()
    for name in names:
        M, K, N, nonneg, swapped = R.CASES[name]
        for q in range(3):
            qp = R.SWAP[q] if swapped else q
            A, B = R.probe(qp, M, K, N, R.SEED + names.index(name), nonneg)
            m = R.measures(A, B, R.six_term_product(A, B), qp)
            if m["err"].max() > m["bar"] / 3:
                over.add((name, q))
            assert 2 < R.measures(*R.case(name, q)[:2], 0.0, qp)["bar"] / m["bar"] < 5
    assert over == {("linear_wgrad/R129", 0), ("sa/64x64", 2), ("sa_pool/128x256", 2), ("sa_pool/64x128", 2), ("tf_ffn/bwd/first", 0),
                    ("tf_ffn/fwd/first", 0)}, over


@pytest.mark.parametrize("name", sorted(R.BIAS_CASES))
def test_every_device_bias_probe(name):
    for p in (1, 2):
        _bias_conditions(R.bias_case(name, p), p)


@pytest.mark.parametrize("K", [8, 16])
def test_relation_backward_scenes(K):
    for q in range(3):
        s = R.relation_dw2_scene(q, K)
        assert (s["W3"] > 0).all() and (s["U0"] > 0).all() and ((s["dpred"] != 0).sum(-1) == 1).all()
        nz = np.abs(s["dpred"][s["dpred"] != 0])
        assert (np.log2(nz) == np.round(np.log2(nz))).all()                                  # powers of two: dz2 is exact
        assert K * K >= 64
        _five_conditions(s["A"], s["B"], q)
    for p in (1, 2) if K == 8 else ():                                                        # (the device test sums db2 at K = 8)
        s = R.relation_db2_scene(p, K)
        assert (s["dpred"] >= 0).all() and ((s["dpred"] != 0).sum(-1) == 1).all()
        _bias_conditions(s["G"], p)


def test_decoder_probes_show_a_lost_term_through_logit_differences():
    """Only differences of a row's logits leave spacap_beam_topw_f32 and spacap_decode_word_f32.  With the restated logits in
    place of the kernel's: all six terms pass, any five fail the log-probability check; the ranking and the greedy word are
    decided on (far) more than 3/4 of the rows."""
    for q in range(3):
        x, Wt, qp = R.decode_case(q)
        B = np.ascontiguousarray(Wt.T)
        _five_conditions(x, B, qp)
        lp, wd = R.topw_restated(R.six_term_product(x, B), R.DECODE_W)
        ratio, decided = R.topw_check(x, Wt, qp, lp, wd)
        assert ratio < 1 and decided >= 0.75, (ratio, decided)
        lp5, wd5 = R.topw_restated(R.six_term_product(x, B, drop=qp), R.DECODE_W)
        assert R.topw_check(x, Wt, qp, lp5, wd5)[0] > 1
        assert R.greedy_check(x, Wt, qp, wd[:, 0]) >= 0.75


def test_randn_operands_hide_a_lost_term_from_the_max_norm():
    """Why the device tests use probes: on randn operands, scored as max |got - ref| / max |ref| (the measure of the older
    tests, bars 1e-5 and looser), every five-term product passes."""
    g = np.random.default_rng(0)
    for K in (128, 512):
        A, B = g.standard_normal((48, K)).astype(np.float32), g.standard_normal((K, 40)).astype(np.float32)
        ref = A.astype(np.float64) @ B.astype(np.float64)
        old = lambda got: np.abs(got - ref).max() / np.abs(ref).max()
        assert old(R.six_term_product(A, B)) < 1e-6
        for q in range(3):
            assert 1e-6 < old(R.six_term_product(A, B, drop=q)) < 1e-5
