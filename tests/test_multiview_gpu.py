"""Multiview projection on the device (spacap3d_amd/multiview.py, csrc/multiview.hip) against the results the reference's
own ProjectionHelper recorded (tests/golden/multiview_ref.npz) and, on small shapes, against the numpy restatement
(tests/multiview_restated.py).

The kernel's f32 arithmetic and the reference's differ in the last bit and the decisions are discontinuous, so the map is
compared on every (frame, point) pair outside the float64 guard band and aggregated rows bit for bit on every point that has
no in-band pair in any frame; every test that uses the band asserts the cap (0.2 % of the pairs, 3 % of the hits) for its own
inputs."""
import numpy as np
import pytest
import torch

import multiview_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H = R.CAM["image_dims"]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def proj():
    from spacap3d_amd.multiview import MultiviewProjector
    return MultiviewProjector(**R.CAM)


@pytest.fixture(scope="module", params=["a", "b"])
def case(request):
    c = R.load_case(request.param)
    c["dev"] = {k: _dev(c[k]) for k in ("points", "depths", "poses", "feats", "labels")}
    return c


def _check_against(proj, c, pmap_ref, band, feats_ref, labels_ref):
    """map outside the band, aggregated rows of band-free points; returns the device map"""
    d = c["dev"]
    hits = int((pmap_ref >= 0).sum())
    assert R.band_within_cap(band, hits), (int(band.sum()), band.size, hits)
    pmap = proj.projection_map(d["points"], d["depths"], d["poses"]).cpu().numpy()
    assert pmap.dtype == np.int32 and pmap.shape == pmap_ref.shape
    assert np.array_equal(pmap[~band], pmap_ref[~band])
    clean = ~band.any(0)
    for mode, want in feats_ref.items():
        got = proj.project_features(d["points"], d["depths"], d["poses"], d["feats"], mode=mode).cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got[clean], want[clean]), mode
    for mode, want in labels_ref.items():
        got = proj.project_labels(d["points"], d["depths"], d["poses"], d["labels"], mode=mode).cpu().numpy()
        assert got.dtype == np.int64 and np.array_equal(got[clean], want[clean]), mode
    return pmap


def test_fixture_matches_the_reference(proj, case):
    c = case
    _check_against(proj, c, c["map"], c["band"], {"max": c["feat_max"], "first": c["feat_first"]},
                   {"vote": c["label_vote"], "first": c["label_first"]})


def _small_case(N, F, C, seed):
    """a room of 130 points of which the first N are used, F cameras; with F = 70: frame 5 has a -inf pose, frame 9 looks away
    from outside; with C = 128 a quirk pair is planted"""
    rng = np.random.default_rng(seed)
    points = R.room_points(rng, 130)[:N]
    poses = R.room_poses(rng, F)
    if N == 1:       # look (nearly) at the one point from 2 m away
        poses[0] = R.look_at(points[0] + np.array([1.2, 1.4, 0.8], np.float32), points[0] + np.array([0.1, 0.05, 0.08], np.float32))
    if F > 9:
        poses[5] = -np.inf
        poses[9] = R.look_at([30.0, 30.0, 1.5], [40.0, 40.0, 1.5])
    depths = R.zbuffer(points, poses, R.CAM["intrinsic"], R.CAM["image_dims"])
    pmap = R.projection_map(points, depths, poses, **R.CAM)
    band = R.band(points, depths, poses, **R.CAM)
    feats = R.random_features(seed + 1, F, C, H, W).reshape(F, C, -1)
    labels = R.random_labels(seed + 2, F, H, W)
    clean = ~band.any(0)
    quirk = None
    if C >= 2 and F > 9:
        # a band-free point with exactly three covering frames: the first two get (-1, 0, ...) and (0, -1, 0, ...), their
        # maximum is all-zero, and the third frame's vector then REPLACES it (its negative entries survive)
        for n in np.nonzero(clean)[0]:
            fr = [f for f in range(F) if pmap[f, n] >= 0 and np.any(feats[f][:, pmap[f, n]] != 0)]
            if len(fr) == 3 and (feats[fr[2]][2:, pmap[fr[2], n]] < 0).any():
                for i, f in enumerate(fr[:2]):
                    feats[f][:, pmap[f, n]] = 0
                    feats[f][i, pmap[f, n]] = -1
                quirk = int(n)
                break
    feats = feats.reshape(F, C, H, W)
    c = dict(points=points, depths=depths, poses=poses, feats=feats, labels=labels, map=pmap, band=band, quirk=quirk)
    c["dev"] = {k: _dev(c[k]) for k in ("points", "depths", "poses", "feats", "labels")}
    return c


@pytest.mark.parametrize("N,F", [(1, 1), (63, 1), (65, 1), (130, 1), (130, 70)])
@pytest.mark.parametrize("C", [1, 128])
def test_small_cases_match_the_restatement(proj, N, F, C):
    c = _small_case(N, F, C, seed=100 + N + F)
    pmap, band = c["map"], c["band"]
    if N == 1:
        assert pmap[0, 0] >= 0 and not band.any()
    fr = {m: R.aggregate_features(pmap, c["feats"], m) for m in ("max", "first")}
    lr = {m: R.aggregate_labels(pmap, c["labels"], m) for m in ("vote", "first")}
    got = _check_against(proj, c, pmap, band, fr, lr)
    if F == 70:      # more frames than one LDS chunk holds
        flat, lab = c["feats"].reshape(F, C, -1), c["labels"].reshape(F, -1)
        assert (got[5] < 0).all() and (got[9] < 0).all() and (pmap >= 0).sum() > 200
        assert (pmap >= 0).any(1).sum() > 16
        zero_hits = sum(int(np.all(flat[f][:, pmap[f, pmap[f] >= 0]] == 0, axis=0).sum()) for f in range(F))
        assert zero_hits > 0                                            # all-zero vectors at hit pixels
        assert not np.array_equal(fr["max"], fr["first"]) and not np.array_equal(lr["vote"], lr["first"])
        ties = 0
        for n in range(N):
            seen = [int(lab[f, pmap[f, n]]) for f in range(F) if pmap[f, n] >= 0]
            cnt = sorted((seen.count(s) for s in set(seen) if s), reverse=True)
            ties += len(cnt) >= 2 and cnt[0] == cnt[1]
        assert ties > 0
        if C == 128:
            q = c["quirk"]
            assert q is not None
            pooled = np.stack([flat[f][:, pmap[f, q]] for f in range(F) if pmap[f, q] >= 0]).max(0)
            assert not np.array_equal(fr["max"][q], pooled)             # the all-zero-after-max quirk shows in the reference value


def test_points_behind_the_camera_map_nothing(proj):
    pose = R.look_at([3.0, 2.5, 1.2], [3.0, 0.0, 1.2])                  # looks along -y
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(2, 4, 64), rng.uniform(3.0, 5.0, 64), rng.uniform(0.5, 2, 64)], 1).astype(np.float32)   # y > 2.5
    depth = np.full((1, H, W), 1.5, np.float32)
    got = proj.projection_map(_dev(pts), _dev(depth), _dev(pose[None]))
    assert (got < 0).all()
    front = pts * np.array([1, -1, 1], np.float32) + np.array([0, 5.0, 0], np.float32)     # mirrored: in front
    depth = R.zbuffer(front, pose[None], R.CAM["intrinsic"], R.CAM["image_dims"])
    assert (proj.projection_map(_dev(front), _dev(depth), _dev(pose[None])) >= 0).any()


def test_chunked_frames_and_two_runs_are_bit_identical(proj, case):
    d = case["dev"]
    p, dep, pos, ft, lb = d["points"], d["depths"], d["poses"], d["feats"], d["labels"]
    for mode in ("max", "first"):
        whole = proj.project_features(p, dep, pos, ft, mode=mode)
        again = proj.project_features(p, dep, pos, ft, mode=mode)
        part = proj.project_features(p, dep[:3], pos[:3], ft[:3], mode=mode)
        out = proj.project_features(p, dep[3:], pos[3:], ft[3:], mode=mode, out=part)
        assert out is part and torch.equal(whole, again) and torch.equal(whole, part), mode
        cl = proj.project_features(p, dep, pos, ft.permute(0, 2, 3, 1).contiguous(), mode=mode, channels_last=True)
        assert torch.equal(whole, cl)
    whole = proj.project_labels(p, dep, pos, lb, mode="vote")
    state = proj.vote_state(p.shape[0], p.device)
    proj.project_labels(p, dep[:3], pos[:3], lb[:3], mode="vote", out=state)
    part = proj.project_labels(p, dep[3:], pos[3:], lb[3:], mode="vote", out=state)
    assert torch.equal(whole, part) and torch.equal(whole, proj.project_labels(p, dep, pos, lb, mode="vote"))
    assert torch.equal(whole, proj.project_labels(p, dep[:0], pos[:0], lb[:0], mode="vote", out=state))   # no frames: the state
    whole = proj.project_labels(p, dep, pos, lb, mode="first")
    part = proj.project_labels(p, dep[:3], pos[:3], lb[:3], mode="first")
    assert torch.equal(whole, proj.project_labels(p, dep[3:], pos[3:], lb[3:], mode="first", out=part))
    m1, m2 = proj.projection_map(p, dep, pos), proj.projection_map(p, dep, pos)
    assert torch.equal(m1, m2) and torch.equal(m1[3:], proj.projection_map(p, dep[3:], pos[3:]))


def test_compute_projection_drop_in(proj, case):
    c, d = case, case["dev"]
    N = c["map"].shape[1]
    f = next(f for f in range(len(c["map"])) if not c["band"][f].any() and (c["map"][f] >= 0).sum() > 20)
    idx = np.nonzero(c["map"][f] >= 0)[0]
    i3, i2 = proj.compute_projection(d["points"], d["depths"][f], d["poses"][f])
    assert i3.dtype == torch.int64 and i3.shape == (N + 1,) and i2.shape == (N + 1,)
    want3, want2 = np.zeros(N + 1, np.int64), np.zeros(N + 1, np.int64)
    want3[0] = want2[0] = len(idx)
    want3[1:1 + len(idx)], want2[1:1 + len(idx)] = idx, c["map"][f, idx]
    assert np.array_equal(i3.cpu().numpy(), want3) and np.array_equal(i2.cpu().numpy(), want2)
    assert proj.compute_projection(d["points"], d["depths"][3], d["poses"][3]) is None      # the frame that sees nothing


def test_dataset_keeps_device_rows():
    """add_scene(multiview=<device tensor>) gives the batch that the same rows give as a host array"""
    from spacap3d_amd.dataset import DeviceSceneDataset
    rng = np.random.default_rng(11)
    n = 300
    vert = rng.uniform(-1, 1, (n, 9)).astype(np.float32)
    ins = rng.integers(0, 3, n)
    sem = np.where(ins > 0, 5, 1)
    bbox = np.array([[0.1, 0.2, 0.3, 0.5, 0.6, 0.7, 5, 1], [-0.2, 0.1, 0.0, 0.4, 0.4, 0.4, 5, 2]])
    rows = rng.normal(0, 1, (n, 128)).astype(np.float32)
    batches = []
    for mv in (rows, _dev(rows)):
        ds = DeviceSceneDataset(DEV, np.ones((18, 3)), {5: 2}, num_points=128, use_multiview=True, use_normal=True, augment=False,
                                max_instances=8)
        ds.add_scene("s", vert, ins, sem, bbox, multiview=mv)
        ds.add_item("s", 1)
        draws = ds.draw([0], torch.Generator(device=DEV).manual_seed(3))
        batches.append(ds.batch([0], draws=draws))
        if isinstance(mv, torch.Tensor):
            assert ds._scenes[0]["multiview"].data_ptr() == mv.data_ptr()       # kept as it is
    a, b = batches
    assert a.keys() == b.keys() and a["point_clouds"].shape == (1, 128, 3 + 3 + 128 + 1)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float(a["point_clouds"][..., 6:134].abs().sum()) > 0
    with pytest.raises(ValueError):
        ds.add_scene("t", vert, ins, sem, bbox, multiview=_dev(rows[:10]))
