"""The ENet image encoder on the device (spacap3d_amd/enet.py, csrc/enet.hip) against the reference's own network
(tests/golden/enet_ref.npz, recorded by make_fixtures_enet.py) and the float64 restatement (tests/enet_restated.py).

Bounds.  End to end and on the recorded intermediate activations: maximum absolute error <= 4 x ``ref_err``, the reference's
own float32 rounding against its own float64 run at that point (folding and another summation order reorder the roundings,
they add no new kind; the folded float32 restatement sits at 0.9 .. 1.1 x).  One layer alone: 1e-5 of the result's maximum
magnitude, the project's figure for fp32-MFMA products (tests/test_dense_rows_gpu.py)."""
import numpy as np
import pytest
import torch

import enet_restated as R
import multiview_restated as MV

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def sd():
    sd = R.random_state_dict(R.WEIGHT_SEED)
    assert R.weights_crc(sd) == R.WEIGHT_CRC
    return sd


@pytest.fixture(scope="module")
def enc(sd):
    from spacap3d_amd.enet import ENetEncoder
    return ENetEncoder.from_state_dict(sd, DEV)


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


def case_images(name):
    c = R.CASES[name]
    return torch.from_numpy(R.random_images(c["seed"], c["B"], c["H"], c["W"])).to(DEV)


def nchw(x, h, w):
    """pixel-major (B, h w, C) on the device -> float64 (B, C, h, w) on the host"""
    return x.view(x.shape[0], h, w, x.shape[2]).permute(0, 3, 1, 2).double().cpu().numpy()


def pixel_major(a):
    """float (B, C, h, w) array -> f32 (B, h w, C) on the device"""
    B, C, h, w = a.shape
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1)).reshape(B, h * w, C).astype(np.float32)).to(DEV)


@pytest.mark.parametrize("name", ["a", "b"])
def test_end_to_end_against_the_reference(enc, fixture, name):
    c = R.CASES[name]
    h, w = c["H"] // 8, c["W"] // 8
    images = case_images(name)
    out = enc(images)
    assert out.dtype == torch.float32 and tuple(out.shape) == (c["B"], h * w, 128) and out.is_contiguous()
    want, err = fixture[f"{name}_out"], float(fixture[f"{name}_ref_err"])
    got = float(np.abs(nchw(out, h, w) - want).max())
    print(f"case {name}: max error {got:.3e} = {got / err:.2f} x ref_err ({err:.3e})")
    assert got <= 4 * err
    planar = enc(images, layout="nchw")
    assert tuple(planar.shape) == (c["B"], 128, h, w)
    assert torch.equal(planar, out.view(c["B"], h, w, 128).permute(0, 3, 1, 2))
    # pixel-major: row p of image b is the 128-vector of pixel (p // w, p % w)
    assert np.abs(out[0, w + 1].double().cpu().numpy() - want[0, :, 1, 1]).max() <= 4 * err


def test_intermediate_activations_layer_by_layer(enc, fixture):
    c = R.CASES["a"]
    x = enc.initial(case_images("a"))
    h, w = c["H"] // 2, c["W"] // 2
    ends = {v: k for k, v in R.STAGE_END.items()}

    def check(name, x, h, w):
        want, err = (fixture[f"a_{name}"], float(fixture[f"a_{name}_ref_err"])) if name != "stage3" else \
            (fixture["a_out"], float(fixture["a_ref_err"]))
        got = float(np.abs(nchw(x, h, w) - want).max())
        print(f"{name}: {got:.3e} = {got / err:.2f} x ref_err")
        assert got <= 4 * err, name

    check("initial", x, h, w)
    for i, (kind, _, _, _, _) in enumerate(R.LAYERS):
        x = enc.bottleneck(i, x, h, w)
        if kind == "down":
            h, w = h // 2, w // 2
        if i + 1 in ends:
            check(ends[i + 1], x, h, w)
    assert torch.equal(x, enc(case_images("a")))        # the chained entry point is these launches


# (layer index in R.LAYERS, input map): every kind, every dilation, both inner widths; 18 x 19 = 342 pixels is a multiple of
# neither 16 nor 64 and holds dilation-16 taps on both axes, 5 x 3 is smaller than one MFMA tile and than every dilation above 2
ALONE = [(1, 18, 19), (1, 5, 3)] + [(i, h, w) for i in (6, 7, 8, 9, 11, 13) for h, w in ((18, 19), (5, 3))] \
    + [(0, 36, 38), (0, 11, 6), (5, 36, 38), (5, 11, 6)]


@pytest.mark.parametrize("i,h,w", ALONE, ids=[f"{R.LAYERS[i][0]}{R.LAYERS[i][2]}-d{R.LAYERS[i][3]}-{h}x{w}" for i, h, w in ALONE])
def test_every_bottleneck_kind_alone(enc, sd, i, h, w):
    kind, cin, cout, dil, p = R.LAYERS[i]
    x32 = np.random.default_rng(100 + i).standard_normal((2, cin, h, w)).astype(np.float32).astype(np.float64)
    want, branch = R.bottleneck(sd, i, x32, np.float64, parts=True)
    ho, wo = want.shape[2:]
    assert (ho, wo) == ((h // 2, w // 2) if kind == "down" else (h, w))
    got = nchw(enc.bottleneck(i, pixel_major(x32), h, w), ho, wo)
    bound = 1e-5 * np.abs(want).max()
    err = np.abs(got - want).max()
    print(f"{kind} {cin}->{cout} d{dil} {h}x{w}: {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    if kind == "down":      # channels from C_in on have no skip: PReLU of the conv branch alone
        alone = R.prelu(branch, sd[f"{4 + i}.2.weight"].astype(np.float64))
        assert np.abs(got[:, cin:] - alone[:, cin:]).max() <= bound
        assert np.abs(got[:, :cin] - alone[:, :cin]).max() > 1000 * bound      # (and the others do have one)
    # the reference's dropout factor is visible at this bound: the network without it is outside
    assert np.abs(got - R.bottleneck(sd, i, x32, np.float64, drop=False)).max() > bound


def test_initial_block_alone(enc, sd):
    images = R.random_images(7, 2, 44, 24)
    want = R.initial_block(sd, images, np.float64)
    got = nchw(enc.initial(torch.from_numpy(images).to(DEV)), 22, 12)
    err, bound = np.abs(got - want).max(), 1e-5 * np.abs(want).max()
    print(f"initial: {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_batch_independence(enc):
    a = case_images("a")
    three = torch.cat([a, torch.from_numpy(R.random_images(3, 1, 44, 24)).to(DEV)])
    together = enc(three)
    for b in range(3):
        assert torch.equal(enc(three[b:b + 1])[0], together[b]), b


def test_from_uint8_is_the_normalised_call(enc):
    u8 = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (2, 44, 24, 3), dtype=np.uint8)).to(DEV)
    mean = torch.tensor(enc.SCANNET_MEAN, dtype=torch.float32, device=DEV)
    std = torch.tensor(enc.SCANNET_STD, dtype=torch.float32, device=DEV)
    # tensor divisors: a division by a Python number may be turned into a multiplication by its reciprocal
    x = (u8.float() / torch.full((1,), 255.0, device=DEV) - mean) / std
    host = (u8.cpu().float().numpy() / np.float32(255.0) - np.asarray(enc.SCANNET_MEAN, np.float32)) \
        / np.asarray(enc.SCANNET_STD, np.float32)
    assert np.array_equal(x.cpu().numpy(), host)         # the stated order in IEEE f32, as numpy has it
    want = enc(x.permute(0, 3, 1, 2))
    got = enc.from_uint8(u8, enc.SCANNET_MEAN, enc.SCANNET_STD)
    assert torch.equal(got, want) and float(got.abs().max()) > 0
    assert torch.equal(enc.from_uint8(u8), want)


def test_graph_capture_replays_the_eager_result(enc):
    images = case_images("a")
    eager = enc(images).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = enc(images)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_encoder_output_feeds_the_projection_as_it_is(enc):
    from spacap3d_amd.multiview import MultiviewProjector
    rng = np.random.default_rng(21)
    points = MV.room_points(rng, 2000)
    poses = MV.room_poses(rng, 3)
    depths = MV.zbuffer(points, poses, MV.INTRINSIC, MV.CAM["image_dims"])
    images = torch.from_numpy(R.random_images(31, 3, 256, 328)).to(DEV)
    feats = enc(images)
    assert tuple(feats.shape) == (3, 32 * 41, 128) and feats.is_contiguous()
    proj = MultiviewProjector(**MV.CAM)
    args = [torch.from_numpy(v).to(DEV) for v in (points, depths, poses)]
    rows = proj.project_features(*args, feats, channels_last=True)
    planar = enc(images, layout="nchw")
    assert tuple(planar.shape) == (3, 128, 32, 41)
    again = proj.project_features(*args, planar)
    assert tuple(rows.shape) == (2000, 128) and torch.equal(rows, again)
    assert int((rows != 0).any(1).sum()) > 200           # the frames do cover points


def test_no_library_kernel(enc):
    from torch.profiler import ProfilerActivity, profile
    images = case_images("b")
    enc(images)
    torch.cuda.synchronize()
    names = set()
    for attempt in range(5):    # (the tracer sometimes returns an incomplete event list)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            enc(images)
            torch.cuda.synchronize()
        got = [e.key for e in prof.key_averages() if e.device_type is not None and "cuda" in str(e.device_type).lower()]
        bad = [n for n in got if n.startswith("Cijk_") or "naive_conv" in n or "miopen" in n.lower() or "hipblaslt" in n.lower()
               or "rocblas" in n.lower()]
        assert not bad, bad
        names |= set(got)
        if all(any(k in n for n in names) for k in ("enet_initial_kernel", "enet_reduce_kernel", "enet_main_kernel")):
            break
    for k in ("enet_initial_kernel", "enet_reduce_kernel", "enet_main_kernel"):
        assert any(k in n for n in names), (k, sorted(names))
