"""Records tests/golden/enet_ref.npz from the reference's own ENet (lib/enet.py: create_enet, loaded by path; nothing of it
is copied).  The seeded weights of tests/enet_restated.py are loaded with strict=True -- which also pins the key names --, the
classifier is dropped, and the encoder runs in eval() on the CPU in float32 and, after .double(), in float64.

Per case (enet_restated.CASES): the float64 output and ``ref_err``, the maximum absolute difference of the reference's OWN
float32 run from its float64 run -- the yardstick of the tests.  Case a also records the float64 activations behind the
initial block, stage 1 and stage 2, with their own ref_err.  Weights and images are regenerated from seeds, not stored.

    python tests/golden/make_fixtures_enet.py [path of the reference checkout]
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import enet_restated as R  # noqa: E402

CHECKPOINTS = {"initial": 3, "stage1": 3 + R.STAGE_END["stage1"], "stage2": 3 + R.STAGE_END["stage2"],
               "stage3": 3 + R.STAGE_END["stage3"]}     # index of the last module of each part


def run(model, images):
    x, got = images, {}
    with torch.no_grad():
        for idx, mod in enumerate(model):
            x = mod(x)
            for name, at in CHECKPOINTS.items():
                if at == idx:
                    got[name] = x.numpy().copy()
    return got


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    spec = importlib.util.spec_from_file_location("reference_enet", os.path.join(ref, "lib", "enet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.set_num_threads(4)

    sd = R.random_state_dict(R.WEIGHT_SEED)
    assert R.weights_crc(sd) == R.WEIGHT_CRC, hex(R.weights_crc(sd))
    net = mod.create_enet(R.NUM_CLASSES)
    assert sorted(net.state_dict().keys()) == sorted(sd.keys()), "key names differ"
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    print(f"{len(sd)} keys loaded (strict)")
    enc32 = torch.nn.Sequential(*[net[i] for i in range(len(net) - 1)]).eval()
    out = {}
    for name, c in R.CASES.items():
        images = torch.from_numpy(R.random_images(c["seed"], c["B"], c["H"], c["W"]))
        got32 = run(enc32, images)
        enc32.double()
        got64 = run(enc32, images.double())
        enc32.float()
        for cp in CHECKPOINTS:
            a, b = got32[cp], got64[cp]
            assert a.dtype == np.float32 and b.dtype == np.float64
            err = float(np.abs(a.astype(np.float64) - b).max())
            assert not (b == 0).any(), (name, cp, "an exactly zero element")
            assert 0 < err < 1e-5 * np.abs(b).max(), (name, cp, err)
            print(f"case {name} {cp:8s} shape {b.shape} max |x| {np.abs(b).max():.3f} ref_err {err:.3e}")
            if cp == "stage3":
                out[f"{name}_out"], out[f"{name}_ref_err"] = b, np.float64(err)
            elif name == "a":
                out[f"a_{cp}"], out[f"a_{cp}_ref_err"] = b, np.float64(err)
        # the restatement and the folded evaluation against the same yardstick (printed; tests/test_enet_cpu.py asserts)
        want, err = out[f"{name}_out"], out[f"{name}_ref_err"]
        lit = np.abs(R.forward(sd, images.numpy(), np.float32).astype(np.float64) - want).max()
        fol = np.abs(R.forward_folded(R.fold(sd), images.numpy(), np.float32).astype(np.float64) - want).max()
        f64 = np.abs(R.forward(sd, images.numpy(), np.float64) - want).max()
        print(f"case {name}: restated f64 {f64:.2e}; f32 literal {lit / err:.2f} x ref_err, f32 folded {fol / err:.2f} x ref_err")
        assert f64 < 1e-12 and lit <= 4 * err and fol <= 4 * err
    path = os.path.join(HERE, "enet_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
