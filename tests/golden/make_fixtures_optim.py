"""Generates tests/golden/optimizer_layout_ref.npz: how the REFERENCE's optimizer numbers its parameters and which of
them hold state, recorded by running the reference's own Python (imported in-process exactly as make_fixtures.py does;
only works where the reference tree exists).

The reference builds ``optim.Adam([{non-caption params}, {caption params, "lr": transformer_lr}], lr, weight_decay)``
(scripts/train.py:226-236) and checkpoints its ``state_dict()`` (lib/solver.py:216-225).  Recorded here, at the tiny
configuration and on the inputs of train_step_cfg1.npz, after two training steps with lr 1e-3 / transformer_lr 5e-4:

  names        the parameter names in the optimizer's index order (group 0, then group 1)
  boundary     how many of them are in group 0
  state_index  the sorted indices present in ``optimizer.state_dict()["state"]``
  step         the recorded ``step`` (one value: all entries agree)
  group_lr     each group's ``lr``

Names and numbers only: no weights, no moments.

Run:  python tests/golden/make_fixtures_optim.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_fixtures as MF  # noqa: E402  (import_reference, S, fill_)
from make_fixtures import S, fill_  # noqa: E402

LR, TRANSFORMER_LR, WD, STEPS = 1e-3, 5e-4, 1e-5, 2


def main():
    SpaCapNet, ref_loss, DCcls, tc, pu = MF.import_reference()
    DC = DCcls()
    old = np.load(os.path.join(HERE, "train_step_cfg1.npz"))
    P, V = 64, 40
    cfg = dict(N=2, h=8, d_model=128, d_ff=128)
    torch.manual_seed(0)
    model = SpaCapNet(num_class=DC.num_class, vocabulary=S.make_vocabulary(V), num_heading_bin=DC.num_heading_bin,
                      num_size_cluster=DC.num_size_cluster, mean_size_arr=DC.mean_size_arr, input_feature_dim=1,
                      num_proposal=P, transformer_dropout=0.0, src_pos_type="xyz", use_transformer_encoder=True,
                      early_guide=True, check_relation=True, **cfg)
    fill_(model, seed=1)
    model.train()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    pc = torch.from_numpy(old["point_clouds"])
    lab = {k[6:]: torch.from_numpy(old[k]) for k in old.files if k.startswith("label_")}

    # the optimizer, as scripts/train.py:226-236 builds it
    first = [(n, p) for n, p in model.named_parameters() if "caption" not in n and p.requires_grad]
    second = [(n, p) for n, p in model.named_parameters() if "caption" in n and p.requires_grad]
    optimizer = torch.optim.Adam([{"params": [p for _, p in first]},
                                  {"params": [p for _, p in second], "lr": TRANSFORMER_LR}], lr=LR, weight_decay=WD)
    for _ in range(STEPS):       # lib/solver.py:343-385: forward, loss, zero_grad, backward, step
        d = {"point_clouds": pc.clone()}
        d.update({k: v.clone() for k, v in lab.items()})
        d = model(d)
        d = ref_loss(d, "cpu", DC, detection=True, caption=True, use_relation=True)
        optimizer.zero_grad()
        d["loss"].backward()
        optimizer.step()
    sd = optimizer.state_dict()
    steps = {float(e["step"]) for e in sd["state"].values()}
    assert len(steps) == 1, steps
    assert [len(g["params"]) for g in sd["param_groups"]] == [len(first), len(second)]
    fx = {
        "names": np.array([n for n, _ in first + second]),
        "boundary": np.int64(len(first)),
        "state_index": np.array(sorted(sd["state"].keys()), dtype=np.int64),
        "step": np.int64(steps.pop()),
        "group_lr": np.array([g["lr"] for g in sd["param_groups"]], dtype=np.float64),
    }
    np.savez_compressed(os.path.join(HERE, "optimizer_layout_ref.npz"), **fx)
    print("optimizer_layout_ref.npz:", len(fx["names"]), "parameters,", int(fx["boundary"]), "in group 0,",
          len(fx["state_index"]), "with state, step", int(fx["step"]), "lr", fx["group_lr"])


if __name__ == "__main__":
    main()
