"""Lab: how many proposals per scene the relation head's backward finds selected in the benchmark's workload (cfg2: 8 scenes,
40 000 points, 256 proposals, seed 1000).  Eager steps; the selected backward is handed a workspace of this script's and its
per-scene counts {active rows, active columns} are read after each step (outside any timed region).
    python tools/lab/rel_sel_count.py [steps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from spacap3d_amd import synthetic as S  # noqa: E402
from spacap3d_amd._native import lib  # noqa: E402
from spacap3d_amd.engine import Trainer, synthetic_batch  # noqa: E402
from spacap3d_amd.spacapnet import build_default  # noqa: E402

DEV = torch.device("cuda:0")


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    torch.manual_seed(0)
    model = build_default().to(DEV).train()
    tr = Trainer(model, S.mean_size_arr().numpy())
    data = synthetic_batch(8, 40000, DEV, seed=1000)
    seen = {}
    fn = lib.spacap_relation_fused_bwd_sel_f32

    def wrapped(*a):
        B, K = a[7], a[8]
        ws = torch.empty(int(lib.spacap_relation_fused_sel_workspace_bytes(B, K)) // 4, dtype=torch.int32, device=DEV)
        seen["ws"], seen["B"] = ws, B
        return fn(*a[:14], ws.data_ptr(), a[15])
    lib.spacap_relation_fused_bwd_sel_f32 = wrapped
    for s in range(steps):
        tr.step(data, next_data=data)
        torch.cuda.synchronize()
        cnt = seen["ws"][:4 * seen["B"]].view(-1, 4).cpu()
        print(f"step {s:2d}: active rows per scene {cnt[:, 0].tolist()}  columns {cnt[:, 1].tolist()}  "
              f"tiles {int((cnt[:, 2] * cnt[:, 3]).sum())} of {seen['B'] * 32 * 32}", flush=True)


if __name__ == "__main__":
    main()
