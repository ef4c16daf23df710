"""Grouped / clipped Adam and torch-format optimizer state, the parts that need no GPU:
the numpy restatement (tests/optim_restated.py) against ``torch.optim.Adam`` + ``clip_grad_norm_``, the flat <-> per-parameter
state mapping on CPU tensors, and the reference optimizer's numbering (tests/golden/optimizer_layout_ref.npz, recorded by
running the reference: tests/golden/make_fixtures_optim.py)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import optim_restated as R  # noqa: E402
from detweights import fill_  # noqa: E402

from spacap3d_amd import optim as O  # noqa: E402

G_DIR = os.path.join(HERE, "golden")
SHAPES = [(128, 128), (7,), (3, 5, 2), (2048, 128), (1,), (259, 128, 1, 1)]
GROUP_OF = [0, 1, 0, 1, 1, 0]
RTOL, ATOL = 2e-6, 2e-7      # the project's Adam tolerance (tests/test_engine_gpu.py: FlatAdam against torch)


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) for s in SHAPES], g


@pytest.mark.parametrize("max_norm", [None, 1.0, 1e9])
def test_restatement_matches_torch_adam_with_groups_and_clipping(max_norm):
    init, g = _params()
    lrs, wds = [1e-3, 5e-4], [1e-5, 1e-4]
    tp = [torch.nn.Parameter(p.clone()) for p in init]
    dicts = [{"params": [p for p, k in zip(tp, GROUP_OF) if k == j], "lr": lrs[j], "weight_decay": wds[j]} for j in range(2)]
    # With clipping Adam's eps is 1e-3, as in this project's trajectory tests: torch forms the norm in float32, the
    # restatement (and the kernel) in float64, so the two coefficients differ by an ulp, i.e. g*coef by ~1e-10.  Where
    # g*coef + wd*p cancels to ~eps = 1e-8 the first update lr * g' / (|g'| + eps) amplifies that by lr / eps = 1e5: a
    # handful of the 560 000 elements would sit at 2e-6, a property of the default eps and not of either implementation.
    eps = 1e-8 if max_norm is None else 1e-3
    ref = torch.optim.Adam(dicts, lr=lrs[0], eps=eps)
    mine = R.RestatedAdam([p.numpy() for p in init], GROUP_OF, lrs, wds, eps=eps, max_norm=max_norm)
    for step in range(5):
        grads = [torch.randn(*s, generator=g) * (10.0 ** (step - 2)) for s in SHAPES]
        for p, gr in zip(tp, grads):
            p.grad = gr.clone()
        if max_norm is not None:
            norm = torch.nn.utils.clip_grad_norm_(tp, max_norm)
            assert abs(float(norm) - float(mine_norm(grads))) <= 1e-5 * float(norm)
        ref.step()
        assert mine.step([gr.numpy() for gr in grads])
        if max_norm == 1.0 and step >= 2:
            assert mine.coef < 1.0
        if max_norm == 1e9:
            assert mine.coef == 1.0
        for p, q in zip(tp, mine.p):
            np.testing.assert_allclose(q, p.detach().numpy(), rtol=RTOL, atol=ATOL, err_msg=str(step))


def mine_norm(grads):
    sq = R.sqnorms([gr.numpy() for gr in grads], GROUP_OF, 2)
    return np.sqrt(sq[2])


def test_restated_skip_leaves_everything_alone():
    init, g = _params(1)
    a = R.RestatedAdam([p.numpy() for p in init], GROUP_OF, [1e-3, 5e-4], [1e-5, 0.0], max_norm=2.0)
    b = R.RestatedAdam([p.numpy() for p in init], GROUP_OF, [1e-3, 5e-4], [1e-5, 0.0], max_norm=2.0)
    for step in range(5):
        grads = [torch.randn(*s, generator=g).numpy() for s in SHAPES]
        if step == 2:
            bad = [x.copy() for x in grads]
            bad[3][5, 7] = np.nan
            before = [x.copy() for x in a.p + a.m + a.v]
            assert not a.step(bad) and a.t == 2 and a.skipped == 1
            assert all(np.array_equal(x, y) for x, y in zip(before, a.p + a.m + a.v))
            continue
        a.step(grads)
        b.step(grads)
    assert a.t == b.t == 4 and all(np.array_equal(x, y) for x, y in zip(a.p, b.p))


# ---- flat <-> per-parameter state, torch's format ---------------------------------------------------------------------------
def _layout():
    """Six bucket parameters (odd sizes: padded offsets), interleaved over two groups, plus one parameter per group that is
    NOT in the bucket (no gradient: no state, but it counts in the numbering)."""
    init, g = _params(2)
    ps = [torch.nn.Parameter(p) for p in init]
    out0, out1 = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))
    groups = [{"params": [ps[0], out0, ps[2], ps[5]], "lr": 1e-3},
              {"params": [ps[1], ps[3], out1, ps[4]], "lr": 5e-4, "weight_decay": 1e-4}]
    offsets, total = R.padded_offsets([p.numel() for p in ps])
    return ps, groups, offsets, total, g


def test_flat_state_round_trip_and_torch_accepts_it():
    from spacap3d_amd.distributed import FlatGradBucket
    ps, groups, offsets, total, g = _layout()
    bucket = FlatGradBucket(ps, views=False)            # the layout under test is the bucket's own
    assert bucket.offsets == offsets and bucket.flat.numel() == total and any(o % 4 == 0 and (o + p.numel()) % 4 for o, p in zip(offsets, ps))
    pgs, group_of = O.normalise_groups(ps, groups, 1e-3, 1e-5)
    assert group_of == GROUP_OF
    seg_off, seg_group = O.segment_table(offsets, total, group_of)
    assert seg_off == offsets + [total] and seg_group == GROUP_OF
    m, v = torch.randn(total, generator=g), torch.rand(total, generator=g)
    # gather / scatter are inverse on everything but the padding
    ms = O.gather_state(ps, offsets, m)
    want = R.flat_to_params(m.numpy(), offsets, SHAPES)
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(ms, want))
    back = torch.zeros(total)
    O.scatter_state(ps, offsets, back, ms)
    assert np.array_equal(back.numpy(), R.params_to_flat(want, offsets, total))
    # torch's format and numbering
    sd = O.pack_state_dict(pgs, (0.9, 0.999), 1e-8, ps, offsets, m, v, step=7)
    names = {id(p): f"p{i}" for i, p in enumerate(ps)}
    group_names = [[names.get(id(p), "outside") for p in grp["params"]] for grp in groups]
    want_idx = R.state_indices(group_names, names.values())
    assert sorted(sd["state"]) == sorted(want_idx.values()) == [0, 2, 3, 4, 5, 7]
    for i, p in enumerate(ps):
        e = sd["state"][want_idx[f"p{i}"]]
        assert float(e["step"]) == 7 and torch.equal(e["exp_avg"], ms[i]) and e["exp_avg_sq"].shape == p.shape
    twin = torch.optim.Adam([dict(grp) for grp in groups], lr=1e-3, weight_decay=1e-5)
    ref_sd = twin.state_dict()
    assert [set(a) for a in sd["param_groups"]] == [set(a) for a in ref_sd["param_groups"]]      # every key torch writes
    assert [a["params"] for a in sd["param_groups"]] == [a["params"] for a in ref_sd["param_groups"]] == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert [(a["lr"], a["weight_decay"]) for a in sd["param_groups"]] == [(1e-3, 1e-5), (5e-4, 1e-4)]
    twin.load_state_dict(sd)
    assert sorted(twin.state_dict()["state"]) == [0, 2, 3, 4, 5, 7]
    # ... and back into fresh flat buffers
    m2, v2 = torch.full((total,), 9.0), torch.full((total,), 9.0)
    step, hyper = O.unpack_state_dict(twin.state_dict(), pgs, ps, offsets, m2, v2)
    assert step == 7 and hyper == [(1e-3, 1e-5), (5e-4, 1e-4)]
    assert all(torch.equal(a, b) for a, b in zip(O.gather_state(ps, offsets, m2), ms))
    assert all(torch.equal(a, b) for a, b in zip(O.gather_state(ps, offsets, v2), O.gather_state(ps, offsets, v)))
    # before the first update torch holds no state at all
    assert O.pack_state_dict(pgs, (0.9, 0.999), 1e-8, ps, offsets, m, v, step=0)["state"] == {}


def test_group_validation():
    ps, groups, offsets, total, _ = _layout()
    with pytest.raises(ValueError, match="appears in groups"):
        O.normalise_groups(ps, [groups[0], {"params": groups[1]["params"] + [ps[0]]}], 1e-3, 0.0)
    with pytest.raises(ValueError, match="in no group"):
        O.normalise_groups(ps, [groups[0]], 1e-3, 0.0)
    with pytest.raises(ValueError, match="parameter groups"):
        O.normalise_groups(ps, [{"params": [p]} for p in ps] + [{"params": []}] * 3, 1e-3, 0.0)
    with pytest.raises(ValueError, match="multiples of 4"):
        O.segment_table([0, 7], 9, [0, 1])


def test_load_state_dict_checks():
    ps, groups, offsets, total, g = _layout()
    pgs, _ = O.normalise_groups(ps, groups, 1e-3, 1e-5)
    m, v = torch.randn(total, generator=g), torch.rand(total, generator=g)
    good = O.pack_state_dict(pgs, (0.9, 0.999), 1e-8, ps, offsets, m, v, step=3)
    m2, v2 = torch.zeros(total), torch.zeros(total)

    def variant(edit):
        sd = {"state": {k: dict(e) for k, e in good["state"].items()}, "param_groups": [dict(a) for a in good["param_groups"]]}
        edit(sd)
        return sd

    # an int step (the torch of the reference's era) is accepted
    sd = variant(lambda s: [e.__setitem__("step", 3) for e in s["state"].values()])
    assert O.unpack_state_dict(sd, pgs, ps, offsets, m2, v2)[0] == 3 and torch.equal(m2[:16384], m[:16384])
    # entries of parameters outside the bucket are left alone, whatever they hold
    sd = variant(lambda s: s["state"].__setitem__(1, {"step": 99, "exp_avg": torch.zeros(5), "exp_avg_sq": torch.zeros(5)}))
    assert O.unpack_state_dict(sd, pgs, ps, offsets, m2, v2)[0] == 3
    with pytest.raises(ValueError, match="steps differ"):
        O.unpack_state_dict(variant(lambda s: s["state"][4].__setitem__("step", torch.tensor(4.0))), pgs, ps, offsets, m2, v2)
    with pytest.raises(ValueError, match="shape"):
        O.unpack_state_dict(variant(lambda s: s["state"][2].__setitem__("exp_avg", torch.zeros(5, 3, 2))), pgs, ps, offsets, m2, v2)
    with pytest.raises(ValueError, match="parameter groups"):
        O.unpack_state_dict(variant(lambda s: s["param_groups"].pop()), pgs, ps, offsets, m2, v2)
    with pytest.raises(ValueError, match="some bucket parameters only"):
        O.unpack_state_dict(variant(lambda s: s["state"].pop(5)), pgs, ps, offsets, m2, v2)


# ---- the reference optimizer's numbering ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    """Our model at the configuration of train_step_cfg1.npz and the parameters its loss reaches (CPU oracle backend)."""
    from oracle.attention_ref import OracleBackend
    from spacap3d_amd import backend, synthetic as S
    from spacap3d_amd.distributed import used_parameters
    from spacap3d_amd.loss_helper import get_scene_cap_loss
    from spacap3d_amd.spacapnet import SpaCapNet
    fx = np.load(os.path.join(G_DIR, "train_step_cfg1.npz"))
    model = SpaCapNet(num_class=S.NUM_CLASS, vocabulary=S.make_vocabulary(int(fx["cfg_V"])), num_heading_bin=1,
                      num_size_cluster=18, mean_size_arr=fx["mean_size_arr"], input_feature_dim=1,
                      num_proposal=int(fx["cfg_P"]), N=int(fx["cfg_layers"]), h=8, d_model=128, d_ff=int(fx["cfg_d_ff"]),
                      transformer_dropout=0.0, src_pos_type="xyz", use_transformer_encoder=True, early_guide=True,
                      check_relation=True)
    fill_(model, seed=1)
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    model.train()
    d = {"point_clouds": torch.from_numpy(fx["point_clouds"])}
    d.update({k[6:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("label_")})
    with backend.use_backend(OracleBackend()):
        d = get_scene_cap_loss(model(d), use_relation=True, mean_size_arr=fx["mean_size_arr"])
        used = used_parameters(model, d["loss"])
    return model, used


def test_reference_order_and_state_indices_match_the_reference(tiny):
    model, used = tiny
    fx = np.load(os.path.join(G_DIR, "optimizer_layout_ref.npz"))
    names, boundary = O.reference_order(model)
    assert names == [str(n) for n in fx["names"]] and boundary == int(fx["boundary"])
    groups = O.reference_groups(model, 1e-3, 5e-4)
    assert [g["lr"] for g in groups] == list(fx["group_lr"]) and [len(g["params"]) for g in groups] == [boundary, len(names) - boundary]
    idx = O.state_index(groups)
    assert sorted(idx[id(p)] for p in used) == list(fx["state_index"])
    assert int(fx["step"]) == 2
    # the same through the restated numbering, by name
    name_of = {id(p): n for n, p in model.named_parameters()}
    want = R.state_indices([names[:boundary], names[boundary:]], [name_of[id(p)] for p in used])
    assert sorted(want.values()) == list(fx["state_index"])
