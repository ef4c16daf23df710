"""engine.Trainer with the grouped optimizer: the reference's two parameter groups, gradient clipping
inside the captured step, rate changes without a re-capture, and optimizer checkpoints in the reference's numbering.
Model and batch are those of tests/test_engine_gpu.py (tiny learning rate: see there)."""
import copy
import functools
import math

import pytest
import torch

from spacap3d_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR = 1e-6


def _model(seed=0):
    from spacap3d_amd.spacapnet import build_default
    torch.manual_seed(seed)
    model = build_default(vocab_size=200, num_proposal=64, N=2, d_ff=256).to(DEV).train()
    for m in model.modules():  # dropout off: the comparison must be deterministic
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model


def _data():
    from spacap3d_amd.engine import synthetic_batch
    return synthetic_batch(2, 4096, DEV, seed=3, vocab=200)


def _snapshot(model):
    return {n: p.detach().clone() for n, p in model.named_parameters()}


def _moved(before, after, caption):
    return sum(float((after[n] - before[n]).abs().sum()) for n in before if ("caption" in n) == caption)


def _run(mode="eager", steps=6, **kw):
    """As tests/test_engine_gpu.py::_run; returns the losses (None for enable_graph's warm-up steps), the per-step telemetry,
    the parameters before / after, and the Trainer."""
    from spacap3d_amd.engine import Trainer
    model = _model()
    start = _snapshot(model)
    tr = Trainer(model, S.mean_size_arr().numpy(), lr=LR, split_optimizer=(mode == "graph-split"), **kw)
    data = _data()
    nxt = data if mode != "eager" else None
    losses, tele = [], []

    def one():
        losses.append(float(tr.step(data, next_data=nxt)))
        tele.append({k: float(v) for k, v in tr.last_losses.items() if k in ("grad_norm", "clip_coef", "skipped_updates")})
    one()
    if mode != "eager":
        assert tr.enable_graph(data, warmup=2), tr.graph_error
        losses += [None, None]
        tele += [None, None]
    while len(losses) < steps:
        one()
    torch.cuda.synchronize()
    return dict(losses=losses, tele=tele, start=start, end=_snapshot(model), tr=tr)


@functools.lru_cache(maxsize=None)
def _first_norm():
    """The first step's gradient norm (a one-step run with clipping far away): the clipped runs take half of it."""
    r = _run(steps=1, max_grad_norm=1e30)
    assert r["tele"][0]["clip_coef"] == 1.0 and math.isfinite(r["tele"][0]["grad_norm"]) and r["tele"][0]["grad_norm"] > 0
    return r["tele"][0]["grad_norm"]


@functools.lru_cache(maxsize=None)
def _clipped(mode, transformer_lr=5e-7):
    return _run(mode, transformer_lr=transformer_lr, max_grad_norm=0.5 * _first_norm())


def test_equal_rates_and_no_clipping_change_placement_only():
    a = _run(steps=4)
    b = _run(steps=4, transformer_lr=LR)
    assert not a["tr"].optimizer.grouped and b["tr"].optimizer.grouped and "grad_norm" not in a["tr"].last_losses
    for i, (x, y) in enumerate(zip(a["losses"], b["losses"])):
        assert abs(x - y) <= 1e-5 * abs(x) + 1e-6, (i, a["losses"], b["losses"])
    for n in a["end"]:
        d = float((a["end"][n] - b["end"][n]).abs().max())
        assert d <= 2 * LR * 4 + 1e-5 * float(a["end"][n].abs().max()), (n, d)
    assert all(t["clip_coef"] == 1.0 and t["skipped_updates"] == 0 and math.isfinite(t["grad_norm"]) for t in b["tele"])


def test_clipping_runs_inside_the_captured_step():
    e, g = _clipped("eager"), _clipped("graph")
    assert g["tr"].graph is not None
    for i, (x, y) in enumerate(zip(e["losses"], g["losses"])):
        if y is not None:
            assert abs(x - y) <= 2e-3 * abs(x) + 1e-4, (i, e["losses"], g["losses"])
    for r in (e, g):
        for t in r["tele"]:
            if t is not None:
                assert t["clip_coef"] < 1.0 and math.isfinite(t["grad_norm"]) and t["skipped_updates"] == 0, r["tele"]
    # Adam normalises every element's step to ~lr: at half the rate the captioner moves half as far, the detector as far
    full = _clipped("eager", transformer_lr=1e-6)
    cap = _moved(e["start"], e["end"], True) / _moved(full["start"], full["end"], True)
    det = _moved(e["start"], e["end"], False) / _moved(full["start"], full["end"], False)
    assert 0.45 < cap < 0.55 and 0.9 < det < 1.1, (cap, det)


def test_split_optimizer_tail_matches_the_in_graph_optimizer():
    g, s = _clipped("graph"), _clipped("graph-split")
    assert s["tr"].graph is not None and not s["tr"]._graph_with_opt
    for i, (x, y) in enumerate(zip(g["losses"], s["losses"])):
        if x is not None:
            assert abs(x - y) <= 2e-3 * abs(x) + 1e-4, (i, g["losses"], s["losses"])
    assert all(t["clip_coef"] < 1.0 for t in s["tele"] if t is not None)


def test_rate_change_needs_no_recapture_but_bn_momentum_does():
    from spacap3d_amd.engine import Trainer
    data = _data()
    new_lr, new_tlr = 4e-6, 2.5e-7          # far from the old rates: an update at the old ones would be off by 4x either way
    moved = {}
    for mode in ("graph", "eager"):
        model = _model()
        tr = Trainer(model, S.mean_size_arr().numpy(), lr=LR, transformer_lr=LR, max_grad_norm=0.5 * _first_norm())
        tr.step(data, next_data=data)
        if mode == "graph":
            assert tr.enable_graph(data, warmup=2), tr.graph_error
        else:
            for _ in range(2):
                tr.step(data, next_data=data)
        graph = tr.graph
        tr.set_hyper(lr=new_lr, transformer_lr=new_tlr)
        assert tr.graph is graph and tr._recapture is False
        before = _snapshot(model)
        tr.step(data, next_data=data)
        torch.cuda.synchronize()
        assert tr.graph is graph
        after = _snapshot(model)
        moved[mode] = (_moved(before, after, False), _moved(before, after, True))
        if mode == "graph":
            tr.set_hyper(bn_momentum=0.05)
            assert tr._recapture is True
            tr.step(data, next_data=data)
            assert tr._recapture is False and tr.graph is not None and tr.graph is not graph, tr.graph_error
    for k in (0, 1):
        assert 0.9 < moved["graph"][k] / moved["eager"][k] < 1.1, moved
    # the detector took the 4x rate, the captioner the quarter rate (per element Adam moves ~lr)
    n_det = sum(p.numel() for n, p in before.items() if "caption" not in n)
    assert moved["eager"][0] / n_det > 4 * moved["eager"][1] / sum(p.numel() for n, p in before.items() if "caption" in n)


def test_resume_from_an_optimizer_checkpoint():
    from spacap3d_amd.engine import Trainer
    data = _data()
    kw = dict(lr=LR, transformer_lr=5e-7, max_grad_norm=0.5 * _first_norm())
    model = _model()
    tr = Trainer(model, S.mean_size_arr().numpy(), **kw)
    with pytest.raises(RuntimeError, match="step\\(\\) or"):
        tr.optimizer_state_dict()
    for _ in range(3):
        tr.step(data)
    sd_opt = tr.optimizer_state_dict()
    sd_model = copy.deepcopy(model.state_dict())
    want = [float(tr.step(data)) for _ in range(2)]
    # the reference's own optimizer over the same model accepts the checkpoint as it is
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    twin = torch.optim.Adam([{"params": [p for n, p in named if "caption" not in n]},
                             {"params": [p for n, p in named if "caption" in n], "lr": 5e-7}], lr=LR, weight_decay=1e-5)
    twin.load_state_dict(sd_opt)
    assert len(twin.state_dict()["state"]) == len(tr.bucket.params) < len(named)
    assert all(float(e["step"]) == 3 for e in sd_opt["state"].values())
    assert [a["lr"] for a in sd_opt["param_groups"]] == [LR, 5e-7]
    for graph in (False, True):
        fresh = _model(seed=1)
        fresh.load_state_dict(sd_model)
        tr2 = Trainer(fresh, S.mean_size_arr().numpy(), lr=9e-3, transformer_lr=9e-3, max_grad_norm=kw["max_grad_norm"])
        tr2.load_optimizer_state_dict(sd_opt)        # before the first step: applied when the optimizer is built
        got = [float(tr2.step(data))]
        assert float(tr2.optimizer.step_t) == 4 and (tr2.lr, tr2.transformer_lr) == (LR, 5e-7)
        if graph:
            assert tr2.enable_graph(data, warmup=0), tr2.graph_error
            g = tr2.graph
            tr2.load_optimizer_state_dict(tr2.optimizer_state_dict())     # under an active graph: no re-capture
            assert tr2.graph is g and tr2._recapture is False
        got.append(float(tr2.step(data)))
        for i, (x, y) in enumerate(zip(want, got)):
            assert abs(x - y) <= 1e-5 * abs(x) + 1e-6, (graph, i, want, got)


def test_ungrouped_trainer_checkpoints_in_the_same_numbering():
    from spacap3d_amd.engine import Trainer
    data = _data()
    model = _model()
    tr = Trainer(model, S.mean_size_arr().numpy(), lr=LR)
    for _ in range(2):
        tr.step(data)
    sd = tr.optimizer_state_dict()
    grouped = _clipped("eager")["tr"].optimizer_state_dict()
    assert sorted(sd["state"]) == sorted(grouped["state"]) and [a["params"] for a in sd["param_groups"]] == [a["params"] for a in grouped["param_groups"]]
    assert [a["lr"] for a in sd["param_groups"]] == [LR, LR]
    tr.load_optimizer_state_dict(sd)
    assert float(tr.optimizer.step_t) == 2
    with pytest.raises(ValueError, match="different lr"):
        tr.load_optimizer_state_dict(grouped)          # two rates: needs a Trainer built with transformer_lr=
    with pytest.raises(ValueError, match="transformer_lr needs"):
        tr.set_hyper(transformer_lr=1e-7)
