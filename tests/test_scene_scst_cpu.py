"""Self-critical training over every matched object of a scene without a GPU: the restated selection
(tests/scene_scst_restated.py) against a brute-force formulation over the cases the kernel test runs, the properties those
cases are built to contain, the restated row-indexed decoder input against plain numpy expressions, and the argument refusals
of ``SelfCritical``.  That the new entry points are declared and bound is tests/test_capi_cpu.py's check of every symbol."""
import numpy as np
import pytest

import scene_scst_restated as SS


@pytest.mark.parametrize("case", SS.SELECT_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_restated_selection_equals_the_brute_force(case):
    x, ref = SS.select_inputs(case), SS.select_reference(case)
    brute = SS.select_brute(x.xyz, x.center, x.label_mask, x.object_ids, x.dataset_idx, x.key_table, SS.SELECT_NKEYS, SS.SELECT_NEAR,
                            case[3])
    for name, a, b in zip(ref._fields, ref, brute):
        np.testing.assert_array_equal(a, b, err_msg=name)
    B, K, G, M = case
    filled = np.arange(M)[None, :] < ref.n_sel[:, None]
    assert ((ref.prop >= 0) == filled).all() and ((ref.key >= 0) == filled).all() and (np.isinf(ref.dist) == ~filled).all()
    for b in range(B):
        n = ref.n_sel[b]
        order = list(zip(ref.dist[b, :n], ref.slot_of[b, :n]))
        assert order == sorted(order) and len(set(ref.slot_of[b, :n])) == n
        assert (ref.obj[b, :n] == x.object_ids[b, ref.slot_of[b, :n]]).all() and (ref.prop[b, :n] < K).all()


def test_selection_cases_contain_what_they_are_built_for():
    found = set()
    for case in SS.SELECT_CASES:
        f = SS.select_features(case)
        print(case, sorted(f))
        found |= f
    assert found == set(SS.FEATURES), set(SS.FEATURES) - found
    assert SS.near2_of(SS.SELECT_NEAR) == np.float32(0.5625)


@pytest.mark.parametrize("case", SS.PREP_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_restated_row_indexed_input(case):
    B, K, M, S, D, T, V = case
    x = SS.prep_inputs(case)
    pe = SS.pe_table(max(T - 2, 1), D)
    x0, mask = SS.prep_rows_fwd(x.src, x.memory, x.prop, x.tok, x.emb, pe, M, S)
    R, L = B * M * S, T - 1
    prop = x.prop.reshape(-1)
    assert x0.dtype == np.float32 and x0.shape == (R, L, D) and mask.shape == (R, L, L)
    # what the cases are built to contain
    if M > 1:
        assert max(np.bincount(x.prop[0][x.prop[0] >= 0])) in (2, 3) and (prop < 0).any()
    if B > 1:
        assert (x.prop[B - 1] < 0).all() and (x.prop[:B - 1] >= 0).any()
    assert len({tuple(p) for b in range(B) for p in x.xyz[b]}) == B * K
    # the indicator rows by fancy indexing, the empty groups exact zeros
    grp = np.arange(R) // S
    scene, k = grp // M, prop[grp]
    want = np.where((k >= 0)[:, None], x.src[scene, np.maximum(k, 0)] + x.memory[scene, np.maximum(k, 0)], np.float32(0))
    np.testing.assert_array_equal(x0[:, 0], want)
    if L > 1:
        t = np.clip(x.tok[:, 1:L], 0, V - 1)
        np.testing.assert_array_equal(x0[:, 1:], x.emb[t] * np.float32(np.sqrt(np.float64(D))) + pe[None, :L - 1])
    np.testing.assert_array_equal(mask, (np.tril(np.ones((L, L), bool))[None] & (x.tok[:, None, :L] > 0)).astype(np.uint8))
    # the backward: sequential float32 sums, exact zeros where nobody points, within the bound of an n-term sum of float64
    d, n = SS.prep_rows_bwd(x.g, x.prop, B, K, M, S)
    g0 = x.g[:, 0].astype(np.float64)
    d64, sabs = np.zeros((B, K, D)), np.zeros((B, K, D))
    for r in range(R):
        if k[r] >= 0:
            d64[scene[r], k[r]] += g0[r]
            sabs[scene[r], k[r]] += np.abs(g0[r])
    assert (n == np.bincount(scene[k >= 0] * K + k[k >= 0], minlength=B * K).reshape(B, K)).all()
    assert (d[n == 0] == 0).all() and d.dtype == np.float32
    assert (np.abs(d - d64) <= np.maximum(n - 1, 0)[..., None] * 2.0 ** -24 * sabs).all()
    one = n == S
    if one.any():     # one group: the plain sequential sum of its S rows
        b1, k1 = np.argwhere(one)[0]
        rows = np.flatnonzero((scene == b1) & (k == k1))
        acc = np.zeros(D, np.float32)
        for r in rows:
            acc = acc + x.g[r, 0]
        np.testing.assert_array_equal(d[b1, k1], acc)


def test_self_critical_refuses_bad_arguments():
    from spacap3d_amd.caption_eval import CaptionCorpus
    from spacap3d_amd.self_critical import SelfCritical
    cc = CaptionCorpus({"k0": ["sos a eos"]}, {"pad_": 0, "unk": 1, "sos": 2, "eos": 3, "a": 4}, key_of=np.zeros((1, 1), np.int32))
    with pytest.raises(ValueError, match="proposals"):
        SelfCritical(cc, 2, 3, proposals="all")
    for m in (0, 129):
        with pytest.raises(ValueError, match="max_proposals"):
            SelfCritical(cc, 2, 3, proposals="matched", max_proposals=m)
    for t in (0.0, -0.3, float("nan")):
        with pytest.raises(ValueError, match="near_threshold"):
            SelfCritical(cc, 2, 3, proposals="matched", near_threshold=t)
    sc = SelfCritical(cc, 2, 3, proposals="matched", max_proposals=128, near_threshold=0.3)
    assert sc.max_proposals == 128 and sc.near2 == float(np.float32(0.3) * np.float32(0.3))
    assert SelfCritical(cc, 2, 3).proposals == "referred"
    SelfCritical(cc, 2, 3, max_proposals=0, near_threshold=-1.0)          # the default mode does not read the two arguments
