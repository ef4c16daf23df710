"""No-GPU checks of the ENet image encoder (spacap3d_amd/enet.py, csrc/enet.hip): the numpy restatement the GPU tests compare
with (tests/enet_restated.py) against what the reference's own network recorded (tests/golden/enet_ref.npz,
make_fixtures_enet.py), the folding and key mapping of ``ENetEncoder.from_state_dict``, the composed 5x5 weights of the
asymmetric bottleneck, and the C ABI's argument validation without a device.

The bound everywhere is 4 x ``ref_err``: the reference's own float32 run differs from its own float64 run by ref_err, and a
correct float32 evaluation in another summation order reorders those roundings but adds no new kind."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import enet_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spacap_enet_param_floats", "spacap_enet_bottleneck_param_floats", "spacap_enet_workspace_bytes",
         "spacap_enet_initial_f32", "spacap_enet_bottleneck_f32", "spacap_enet_encode_f32", "spacap_enet_encode_u8")


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


@pytest.fixture(scope="module")
def sd():
    sd = R.random_state_dict(R.WEIGHT_SEED)
    assert R.weights_crc(sd) == R.WEIGHT_CRC
    return sd


def test_generator_is_pinned(sd):
    assert len(sd) == 497 and len(R.LAYERS) == 22
    assert sum(1 for k in sd if k.endswith("num_batches_tracked")) == 67
    assert "4.0.0.0.weight" in sd and sd["4.0.0.0.weight"].shape == (16, 16, 2, 2) and sd["26.0.weight"].shape == (41, 128, 1, 1)
    img = R.random_images(11, 2, 44, 24)
    assert img.shape == (2, 3, 44, 24) and img.dtype == np.float32 and abs(float(img.std()) - 1) < 0.05


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_reproduces_the_reference(fixture, sd, name):
    c = R.CASES[name]
    images = R.random_images(c["seed"], c["B"], c["H"], c["W"])
    want, err = fixture[f"{name}_out"], float(fixture[f"{name}_ref_err"])
    assert want.shape == (c["B"], 128, c["H"] // 8, c["W"] // 8) and 0 < err < 1e-4 and not (want == 0).any()
    cp64 = R.forward(sd, images, np.float64, checkpoints=True)
    cp32 = R.forward(sd, images, np.float32, checkpoints=True)
    fol = R.forward_folded(R.fold(sd), images, np.float32, checkpoints=True)
    assert cp32["stage3"].dtype == np.float32 and fol["stage3"].dtype == np.float32
    assert np.abs(cp64["stage3"] - want).max() < 1e-11
    for got in (cp32, fol):
        d = float(np.abs(got["stage3"].astype(np.float64) - want).max())
        print(f"case {name}: {d / err:.2f} x ref_err")
        assert d <= 4 * err
    if name == "a":
        for cp in ("initial", "stage1", "stage2"):
            w, e = fixture[f"a_{cp}"], float(fixture[f"a_{cp}_ref_err"])
            assert np.abs(cp64[cp] - w).max() < 1e-11
            assert np.abs(cp32[cp].astype(np.float64) - w).max() <= 4 * e, cp
            assert np.abs(fol[cp].astype(np.float64) - w).max() <= 4 * e, cp
    # the dropout quirk is visible at this bound: without the (1 - p) the restatement is far outside
    assert np.abs(R.forward(sd, images, np.float64, drop=False) - want).max() > 1000 * err


def test_composed_5x5_equals_the_asymmetric_pair():
    rng = np.random.default_rng(5)
    w1, w2, b2 = rng.standard_normal((32, 32, 1, 5)), rng.standard_normal((32, 32, 5, 1)), rng.standard_normal(32)
    x = rng.standard_normal((2, 32, 7, 6))                      # smaller than the kernel's reach: borders everywhere
    two = R.conv2d(R.conv2d(x, w1, None, 1, (0, 2)), w2, b2, 1, (2, 0))
    one = R.conv2d(x, R.compose_asym(w1, w2), b2, 1, (2, 2))
    assert one.shape == two.shape == (2, 32, 7, 6)
    assert np.abs(one - two).max() < 1e-12 * np.abs(two).max()


def test_from_state_dict_key_handling(sd):
    from spacap3d_amd import enet
    packed, used = enet.fold_and_pack(sd)
    assert packed.dtype == np.float32 and packed.size == enet.lib.spacap_enet_param_floats() and np.isfinite(packed).all()
    want = {k for k in sd if not k.startswith("26.") and not k.endswith("num_batches_tracked")}
    assert used == want and len(want) == 429
    # torch tensors (a loaded checkpoint) and arrays give the same buffer; the counters and the classifier may be absent
    as_torch = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    assert np.array_equal(enet.fold_and_pack(as_torch)[0], packed)
    assert np.array_equal(enet.fold_and_pack({k: sd[k] for k in want})[0], packed)
    enc = enet.ENetEncoder.from_state_dict(as_torch, "cpu")
    assert enc.params.dtype == torch.float32 and enc.params.numel() == packed.size
    for key in ("0.0.bias", "12.0.0.4.weight", "25.2.weight", "9.0.0.1.running_var"):
        less = dict(sd)
        del less[key]
        with pytest.raises(KeyError, match=re.escape(key)):
            enet.fold_and_pack(less)
        bad = dict(sd)
        bad[key] = np.zeros(tuple(s + 1 for s in sd[key].shape), np.float32)
        with pytest.raises(ValueError, match=re.escape(key)):
            enet.fold_and_pack(bad)


def test_packed_buffer_is_the_restated_folding(sd):
    """the buffer's pieces, read back by the layout of include/spacap_hip.h, are fold() rounded to float32"""
    from spacap3d_amd import enet
    packed, _ = enet.fold_and_pack(sd)
    f = R.fold(sd)
    w0, b0, ps, pt, a0 = f["initial"]
    assert np.array_equal(packed[:16 * 27].reshape(16, 27)[:13], w0.transpose(0, 2, 3, 1).reshape(13, 27).astype(np.float32))
    assert np.array_equal(packed[432:445], b0.astype(np.float32)) and np.array_equal(packed[445:448], pt.astype(np.float32))
    assert np.array_equal(packed[461:464], ps.astype(np.float32)) and np.array_equal(packed[464:480], a0.astype(np.float32))
    off = 480
    for i, (kind, cin, cout, _, _) in enumerate(R.LAYERS):
        for j, piece in enumerate(f["layers"][i]):
            flat = (piece.transpose(0, 2, 3, 1) if piece.ndim == 4 else piece).reshape(-1).astype(np.float32)
            assert np.array_equal(packed[off:off + flat.size], flat), (i, j)
            off += flat.size
    assert off == packed.size


def test_cpu_tensors_are_refused(sd):
    from spacap3d_amd.enet import ENetEncoder
    enc = ENetEncoder.from_state_dict(sd, "cpu")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        enc(torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        enc.from_uint8(torch.zeros(1, 16, 16, 3, dtype=torch.uint8))
    assert len(ENetEncoder.SCANNET_MEAN) == 3 and len(ENetEncoder.SCANNET_STD) == 3


def test_header_signatures_and_symbols_agree():
    from spacap3d_amd import _native
    header = open(os.path.join(ROOT, "include", "spacap_hip.h")).read()
    for name in NAMES:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, name
        assert name in _native.SIGNATURES and hasattr(_native.lib, name)
        nargs = 0 if m.group(1).strip() == "void" else len(m.group(1).split(","))
        assert nargs == len(_native.SIGNATURES[name][1]), name


def test_argument_validation_needs_no_device():
    from spacap3d_amd._native import lib
    one = ctypes.c_void_p(16)       # never dereferenced: every check comes before the first device call
    n = lib.spacap_enet_param_floats()
    big = 1 << 40
    assert n == 480 + sum(lib.spacap_enet_bottleneck_param_floats({"reg": 0, "asym": 1, "down": 2}[k], ci, co)
                          for k, ci, co, _, _ in R.LAYERS)
    assert lib.spacap_enet_bottleneck_param_floats(0, 128, 128) == 32 * 128 + 32 * 288 + 128 * 32 + 4 * 32 + 2 * 128
    assert lib.spacap_enet_bottleneck_param_floats(0, 100, 100) == 0
    # the workspace: two activation buffers and the inner-width map
    assert lib.spacap_enet_workspace_bytes(2, 44, 24) == 2 * 4 * (2 * 22 * 12 * 16 + 11 * 6 * 16)
    assert lib.spacap_enet_workspace_bytes(1, 45, 24) == 0 and lib.spacap_enet_workspace_bytes(-1, 44, 24) == 0
    enc = lambda B, H, W, img=one, prm=one, np_=n, ws=one, nb=big, out=one: \
        lib.spacap_enet_encode_f32(img, B, H, W, prm, np_, ws, nb, out, None)
    u8 = lambda B, H, W, img=one, out=one: \
        lib.spacap_enet_encode_u8(img, B, H, W, 0.5, 0.5, 0.5, 0.25, 0.25, 0.25, one, n, one, big, out, None)
    for B, H, W in ((1, 45, 24), (1, 44, 23), (1, 6, 24), (1, 44, 6), (-1, 44, 24)):
        assert enc(B, H, W) == -1 and b"bad sizes" in lib.spacap_last_error(), (B, H, W)
        assert u8(B, H, W) == -1 and b"bad sizes" in lib.spacap_last_error(), (B, H, W)
        assert lib.spacap_enet_initial_f32(one, B, H, W, one, one, None) == -1 and b"bad sizes" in lib.spacap_last_error()
    for kw in (dict(img=None), dict(prm=None), dict(ws=None), dict(out=None)):
        assert enc(2, 44, 24, **kw) == -1 and b"null" in lib.spacap_last_error(), kw
    assert u8(2, 44, 24, img=None) == -1 and b"null" in lib.spacap_last_error()
    assert lib.spacap_enet_initial_f32(None, 2, 44, 24, one, one, None) == -1 and b"null" in lib.spacap_last_error()
    assert enc(2, 44, 24, np_=n - 1) == -1 and b"parameters" in lib.spacap_last_error()
    assert enc(2, 44, 24, nb=lib.spacap_enet_workspace_bytes(2, 44, 24) - 1) == -1 and b"workspace" in lib.spacap_last_error()
    assert enc(2, 44, 24, out=ctypes.c_void_p(8)) == -1 and b"aligned" in lib.spacap_last_error()
    # one bottleneck
    bn = lambda B, h, w, cin, cout, kind, dil, x=one, ws=one, nb=big, out=ctypes.c_void_p(32): \
        lib.spacap_enet_bottleneck_f32(x, B, h, w, cin, cout, kind, dil, one, ws, nb, out, None)
    assert bn(-1, 5, 3, 128, 128, 0, 1) == -1 and b"bad sizes" in lib.spacap_last_error()
    assert bn(1, 0, 3, 128, 128, 0, 1) == -1 and b"bad sizes" in lib.spacap_last_error()
    assert bn(1, 1, 3, 64, 128, 2, 1) == -1 and b"bad sizes" in lib.spacap_last_error()
    assert bn(1, 5, 3, 64, 64, 1, 1) == -1 and b"unsupported" in lib.spacap_last_error()
    assert bn(1, 5, 3, 128, 128, 3, 1) == -1 and b"unsupported" in lib.spacap_last_error()
    assert bn(1, 5, 3, 128, 128, 0, 0) == -1 and b"unsupported" in lib.spacap_last_error()
    assert bn(1, 5, 3, 128, 128, 0, 1, x=None) == -1 and b"null" in lib.spacap_last_error()
    assert bn(1, 5, 3, 128, 128, 0, 1, out=one) == -1 and b"in == out" in lib.spacap_last_error()
    assert bn(1, 5, 3, 128, 128, 0, 1, nb=15 * 32 * 4 - 1) == -1 and b"workspace" in lib.spacap_last_error()
    # nothing to do
    assert enc(0, 44, 24, img=None, prm=None, ws=None, nb=0, out=None) == 0
    assert u8(0, 44, 24, img=None, out=None) == 0
    assert lib.spacap_enet_initial_f32(None, 0, 44, 24, None, None, None) == 0
    assert bn(0, 5, 3, 128, 128, 0, 1, x=None, ws=None, nb=0, out=None) == 0
