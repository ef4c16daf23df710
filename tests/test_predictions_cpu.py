"""No-GPU checks of the dense-caption predictions (spacap3d_amd/predictions.py): the numpy restatement
(tests/dense_caption_restated.py) reproduces the reference's recorded results (tests/golden/predictions_ref.npz, made by
tests/golden/make_fixtures_predictions.py from lib/ap_helper.py's parse_predictions with per_class_proposal=False and
lib/eval_helper.py's decode_caption), the order is the specified one, the fixture holds the cases it is for, header and
binding agree on the new symbol, the C entry point rejects bad arguments without touching a device, and the Python layer
refuses CPU tensors."""
import os
import re

import numpy as np
import pytest
import torch

import dense_caption_restated as D
from caption_eval_restated import EOS, SOS, word

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "predictions_ref.npz"))
CASES = ("k5", "k64", "k65", "k512")
INPUTS = ("valid", "obj_prob", "sem_cls", "bbox_corner", "tokens")
EMPTY, TIES = ("k64", 1), ("k64", 2)          # (case, scene)
_RESTATED = {}


def inputs(case):
    return {k: FIX[f"{case}/{k}"] for k in INPUTS}


def restated(case):
    if case not in _RESTATED:   # computed once, shared, never modified
        _RESTATED[case] = D.select(*(FIX[f"{case}/{k}"] for k in INPUTS), SOS, EOS)
        for a in _RESTATED[case].values():
            a.setflags(write=False)
    return _RESTATED[case]


def reference_rows(case, scene):
    """proposal -> (class, score f32, corners f64, string) of the reference's list of one scene."""
    sel = np.nonzero(FIX[f"{case}/ref_scene"] == scene)[0]
    return {int(FIX[f"{case}/ref_proposal"][i]): (int(FIX[f"{case}/ref_cls"][i]), FIX[f"{case}/ref_score"][i],
                                                   FIX[f"{case}/ref_corners"][i], str(FIX[f"{case}/ref_caption"][i]))
            for i in sel}


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference(case):
    got = restated(case)
    B = got["count"].shape[0]
    for b in range(B):
        ref = reference_rows(case, b)
        recs = D.records(got, b)
        assert sorted(r[0] for r in recs) == sorted(ref) and len(recs) == len(ref)        # the same set of kept proposals
        for j, c, p, box, text in recs:
            assert c == ref[j][0]
            assert p.dtype == np.float32 and p.tobytes() == ref[j][1].tobytes()           # bit-equal f32
            assert box.dtype == np.float64 and box.tobytes() == ref[j][2].tobytes()       # bit-equal f64
            assert text == ref[j][3]


@pytest.mark.parametrize("case", CASES)
def test_order_and_padding(case):
    got, d = restated(case), inputs(case)
    B, K, L = d["tokens"].shape
    assert got["tokens"].shape == (B, K, L + 2) and got["tokens"].dtype == np.int32 and got["index"].dtype == np.int32
    for b in range(B):
        n = int(got["count"][b])
        assert n == int(d["valid"][b].sum())
        idx, sc = got["index"][b, :n], got["score"][b, :n]
        assert sorted(idx) == list(np.nonzero(d["valid"][b])[0])                           # dense from 0, each kept box once
        for r in range(n - 1):                                                           # non-increasing, ties by index
            assert sc[r] > sc[r + 1] or (sc[r] == sc[r + 1] and idx[r] < idx[r + 1])
        assert (got["index"][b, n:] == -1).all()
        for k in ("score", "cls", "corners", "tokens", "length"):
            assert not got[k][b, n:].any(), k
        ln = got["length"][b, :n]
        assert ((ln >= 2) & (ln <= L + 2)).all() and (got["tokens"][b, :n, 0] == SOS).all()
        for r in range(n):
            t = got["tokens"][b, r]
            assert t[ln[r] - 1] == EOS and (t[1:ln[r] - 1] != EOS).all() and not t[ln[r]:].any()


def test_nan_scores_rank_last_and_zero_signs_tie():
    valid = np.ones((1, 6), np.uint8)
    valid[0, 4] = 0
    prob = np.array([[0.5, np.nan, -0.0, 0.9, 0.99, 0.0]], np.float32)
    got = D.select(valid, prob, np.arange(6)[None], np.zeros((1, 6, 8, 3)), np.full((1, 6, 2), 7), SOS, EOS)
    assert list(got["index"][0]) == [3, 0, 2, 5, 1, -1]


def test_fixture_holds_the_cases_it_is_for():
    shapes = {c: FIX[f"{c}/tokens"].shape for c in CASES}
    assert shapes == {"k5": (2, 5, 1), "k64": (3, 64, 31), "k65": (2, 65, 62), "k512": (2, 512, 12)}
    for c in CASES:
        for b in range(shapes[c][0]):
            assert (FIX[f"{c}/valid"][b].sum() == 0) == ((c, b) == EMPTY)                  # the reference keeps a box elsewhere
            assert not FIX[f"{c}/valid"][b].all() or c == "k5"
        # scene 0: eos at position 0, no eos, eos only at the last position
        ln = restated(c)["length"][0]
        L = shapes[c][2]
        tok, kept = FIX[f"{c}/tokens"][0], np.nonzero(FIX[f"{c}/valid"][0])[0]
        assert tok[kept[0], 0] == EOS and (tok[kept[1]] != EOS).all()
        assert 2 in ln and L + 2 in ln
        if L > 1:
            assert list(np.nonzero(tok[kept[2]] == EOS)[0]) == [L - 1]
    c, b = TIES
    p, v = FIX[f"{c}/obj_prob"][b], FIX[f"{c}/valid"][b].astype(bool)
    same = p[:, None] == p[None, :]
    assert (same & v[:, None] & v[None, :] & ~np.eye(len(p), dtype=bool)).sum() >= 2       # ties between kept boxes
    assert (same & v[:, None] & ~v[None, :]).any()                                         # a kept and a dropped box
    idx = restated(c)["index"][b]
    sc = restated(c)["score"][b]
    tied = [r for r in range(int(restated(c)["count"][b]) - 1) if sc[r] == sc[r + 1]]
    assert tied and all(idx[r] < idx[r + 1] for r in tied)


def test_symbol_is_declared_and_exported():
    from spacap3d_amd import _native, predictions
    header = open(os.path.join(os.path.dirname(HERE), "include", "spacap_hip.h")).read()
    name = "spacap_dense_caption_select"
    assert re.search(r"\bint %s\(" % name, header), name
    assert name in _native.SIGNATURES and hasattr(_native.lib, name)
    decl = re.search(r"\bint %s\((.*?)\);" % name, header, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_native.SIGNATURES[name][1]) == 18                  # as many arguments on both sides
    assert predictions.KEYS == D.KEYS and predictions.MAX_TOKENS == 62


def test_entry_point_rejects_bad_arguments_without_a_device():
    from spacap3d_amd._native import lib
    s = lambda B=1, K=64, L=31, sos=2, eos=3: lib.spacap_dense_caption_select(
        None, None, None, None, None, B, K, L, sos, eos, None, None, None, None, None, None, None, None)
    for bad in (dict(B=-1), dict(K=0), dict(K=513), dict(L=0), dict(L=63), dict(sos=-1), dict(eos=-1)):
        assert s(**bad) == -1, bad
        assert b"bad sizes" in lib.spacap_last_error()
    assert s() == -1 and b"null" in lib.spacap_last_error()
    assert s(B=0) == 0 and s(B=0, K=512, L=62) == 0


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    from spacap3d_amd.engine import Evaluator
    from spacap3d_amd.predictions import dense_caption_predictions, to_records
    d = {k: torch.from_numpy(v) for k, v in inputs("k5").items()}
    post = {"valid": d["valid"].bool(), "obj_prob": d["obj_prob"]}
    out = {"bbox_corner": d["bbox_corner"], "sem_cls": d["sem_cls"], "lang_cap": d["tokens"]}
    with pytest.raises(RuntimeError, match=r"predictions: .*: CPU not supported"):
        dense_caption_predictions(post, out, SOS, EOS)
    with pytest.raises(RuntimeError, match=r"predictions: .*: CPU not supported"):
        to_records({k: torch.from_numpy(np.array(v)) for k, v in restated("k5").items()}, {str(i): word(i) for i in range(50)})
    with pytest.raises(ValueError, match="predictions needs postprocess"):
        Evaluator(None, predictions=(SOS, EOS))
