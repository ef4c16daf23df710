"""Generates tests/golden/multiview_ref.npz by RUNNING THE REFERENCE'S OWN ``ProjectionHelper`` (lib/projection.py) on the
CPU: the module is loaded by path, ``torch.Tensor.cuda`` is made the identity and the helper is built with ``cuda=False``;
``compute_projection`` and ``project`` are called as they are.  Nothing of the reference is copied.

The aggregation loops of scripts/project_multiview_features.py:190-222 and scripts/project_multiview_labels.py:303-356 sit
under ``__main__`` and cannot be called: ``reference_features`` / ``reference_labels`` below restate those few lines in this
file's own words, on the reference's ``project`` outputs (frames that map nothing are skipped, as the scripts'
``projections`` list does).

Cases (keys prefixed ``<case>/``): ``a`` N = 2 000, F = 10, C = 128; ``b`` N = 3 000, F = 12, C = 32.  Synthetic rooms of
tests/multiview_restated.py: points on the walls and floor of a 6 x 5 x 2.5 m box with 1 cm noise, cameras inside looking
around, depth maps z-buffered from the points themselves.  One frame looks at the room from far outside and one has an empty
depth map (both map nothing); 10 % of the pixels of every feature map are all-zero; one pair of frames is constructed so
that a maximum turns a point's accumulator all-zero (the reference then treats it as unfilled); the label maps come in
4 x 4 patches of 4 labels, so votes tie.  The features and labels are NOT stored: ``random_features(seed, ...)`` /
``random_labels(seed, ...)`` of tests/multiview_restated.py regenerate them, the few overwritten vectors are stored as
(frame, pixel, channel, value) rows, and a checksum guards the generator.

Recorded: the map of every frame (from indices_3d / indices_2d), the "max" and "first" features (int8 eighths), the "vote"
and "first" labels, and the float64 guard band per (frame, point) pair.  The generator asserts that the band is within the
issue's cap and that the float64 evaluation agrees with the reference on every pair outside it.

Run:  python tests/golden/make_fixtures_multiview.py
"""
import importlib.util
import os
import sys
from collections import Counter

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference"

import multiview_restated as R  # noqa: E402


def reference_helper():
    import torch
    torch.Tensor.cuda = lambda self, *a, **k: self
    spec = importlib.util.spec_from_file_location("ref_projection", os.path.join(REF, "lib", "projection.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    c = R.CAM
    return mod.ProjectionHelper(c["intrinsic"], c["depth_min"], c["depth_max"], c["image_dims"], c["accuracy"], cuda=False)


def reference_maps(helper, points, depths, poses):
    """per frame the reference's (indices_3d, indices_2d) or None, and the same as an (F, N) map"""
    import torch
    F, N = len(depths), len(points)
    pairs, pmap = [], np.full((F, N), -1, np.int32)
    for f in range(F):
        r = helper.compute_projection(torch.Tensor(points), torch.Tensor(depths[f]), torch.Tensor(poses[f]))
        pairs.append(r)
        if r is not None:
            n = int(r[0][0])
            pmap[f, r[0][1:1 + n].numpy()] = r[1][1:1 + n].numpy()
    return pairs, pmap


def reference_features(helper, pairs, feats, N, maxpool):
    """point features over the frames that map something, in order"""
    import torch
    C = feats.shape[1]
    acc = torch.zeros(N, C)
    first = True
    for f, r in enumerate(pairs):
        if r is None:
            continue
        proj = helper.project(torch.Tensor(feats[f]), r[0], r[1], N).transpose(1, 0)
        if maxpool:
            covered = (proj == 0).sum(1) != C
            unfilled = (acc == 0).sum(1) == C
            take, pool = unfilled & covered, ~unfilled & covered
            acc[take] = proj[take]
            acc[pool] = torch.max(acc[pool], proj[pool])
        elif first:
            acc = proj.clone()
        else:
            unfilled = (acc == 0).sum(1) == C
            acc[unfilled] = proj[unfilled]
        first = False
    return acc.numpy()


def reference_labels(helper, pairs, labels, N, maxpool):
    import torch
    used = [(f, r) for f, r in enumerate(pairs) if r is not None]
    if maxpool:
        table = torch.zeros(N, len(used)).long()
        for i, (f, r) in enumerate(used):
            proj = helper.project(torch.Tensor(labels[f].astype(np.float32)).unsqueeze(0), r[0], r[1], N).transpose(1, 0)
            covered = proj[:, 0] != 0
            table[covered, i] = proj[covered, 0].long()
        out = []
        for row in table.numpy().tolist():
            ranked = sorted(Counter(row).items(), key=lambda kv: kv[1], reverse=True)   # stable: ties keep first-seen order
            ranked = [k for k, _ in ranked if k != 0]
            out.append(ranked[0] if ranked else 0)
        return np.array(out, np.int64)
    acc = None
    for f, r in used:
        proj = helper.project(torch.Tensor(labels[f].astype(np.float32)).unsqueeze(0), r[0], r[1], N).transpose(1, 0)
        if acc is None:
            acc = proj.clone()
        else:
            acc[acc == 0] = proj[acc == 0]
    return (acc if acc is not None else torch.zeros(N, 1))[:, 0].long().numpy()


def make_case(helper, name, seed, N, F, C):
    c = R.CAM
    W, H = c["image_dims"]
    rng = np.random.default_rng(seed)
    points = R.room_points(rng, N)
    poses = R.room_poses(rng, F)
    poses[3] = R.look_at([30.0, 30.0, 1.5], [40.0, 40.0, 1.5])      # far outside, looking away: maps nothing
    depths = R.zbuffer(points, poses, c["intrinsic"], c["image_dims"])
    depths[6] = 0                                                    # an empty depth map: maps nothing
    pairs, pmap = reference_maps(helper, points, depths, poses)
    assert pairs[3] is None and pairs[6] is None
    hits = int((pmap >= 0).sum())

    band = R.band(points, depths, poses, **c)
    assert R.band_within_cap(band, hits), (int(band.sum()), band.size, hits)
    mine = R.projection_map(points, depths, poses, **c)
    assert np.array_equal(mine[~band], pmap[~band]), "the restatement disagrees with the reference outside the band"
    clean = ~band.any(0)

    feats = R.random_features(seed + 1, F, C, H, W)
    labels = R.random_labels(seed + 2, F, H, W)
    # the quirk: a band-free point whose first two covering frames get (-1, 0, ...) and (0, -1, 0, ...): their maximum is
    # all-zero, so the third covering frame's vector replaces it instead of being pooled
    flat = feats.reshape(F, C, -1)
    patch = []
    quirk = -1
    for n in np.nonzero(clean)[0]:
        fr = [f for f in range(F) if pmap[f, n] >= 0 and np.any(flat[f][:, pmap[f, n]] != 0)]
        if len(fr) >= 3 and (C >= 2):
            for i, f in enumerate(fr[:2]):
                vec = np.zeros(C, np.float32)
                vec[i] = -1
                flat[f][:, pmap[f, n]] = vec
                patch += [(f, int(pmap[f, n]), ch, float(vec[ch])) for ch in range(C)]
            quirk = int(n)
            break
    assert quirk >= 0
    feats = flat.reshape(F, C, H, W)

    fmax = reference_features(helper, pairs, feats, N, True)
    ffirst = reference_features(helper, pairs, feats, N, False)
    lvote = reference_labels(helper, pairs, labels, N, True)
    lfirst = reference_labels(helper, pairs, labels, N, False)
    pooled = np.stack([flat[f][:, pmap[f, quirk]] for f in range(F) if pmap[f, quirk] >= 0]).max(0)
    assert not np.array_equal(fmax[quirk], pooled), "the quirk point does not show the quirk"
    # some vote really ties: the two most frequent labels of a point have equal counts
    ties = 0
    lab_flat = labels.reshape(F, -1)
    for n in range(N):
        seen = [int(lab_flat[f, pmap[f, n]]) for f in range(F) if pmap[f, n] >= 0]
        cnt = sorted(Counter(s for s in seen if s).values(), reverse=True)
        ties += len(cnt) >= 2 and cnt[0] == cnt[1]
    zero_hits = sum(int(np.all(flat[f][:, pmap[f, pmap[f] >= 0]] == 0, axis=0).sum()) for f in range(F))
    assert ties > 0 and zero_hits > 0
    for a in (fmax, ffirst):
        assert np.array_equal(np.rint(a * 8) / 8, a) and np.abs(a * 8).max() < 128
    print(f"{name}: N={N} F={F} C={C}: hits {hits} ({100 * hits / pmap.size:.2f} %), band {int(band.sum())} "
          f"({100 * band.sum() / band.size:.3f} % of pairs, {100 * band.sum() / hits:.2f} % of hits), band-free points "
          f"{int(clean.sum())}, vote ties {ties}, all-zero hits {zero_hits}, quirk point {quirk}")
    return {f"{name}/points": points, f"{name}/depths": depths, f"{name}/poses": poses, f"{name}/map": pmap.astype(np.int16),
            f"{name}/band": np.packbits(band), f"{name}/seed": np.array([seed + 1, seed + 2, C]),
            f"{name}/patch": np.array(patch, np.float32).reshape(-1, 4), f"{name}/quirk": np.array(quirk),
            f"{name}/checksum": np.array([float(feats.astype(np.float64).sum()), float(labels.sum())]),
            f"{name}/feat_max": np.rint(fmax * 8).astype(np.int8), f"{name}/feat_first": np.rint(ffirst * 8).astype(np.int8),
            f"{name}/label_vote": lvote.astype(np.int8), f"{name}/label_first": lfirst.astype(np.int8)}


def main():
    helper = reference_helper()
    out = {}
    out.update(make_case(helper, "a", 7100, 2000, 10, 128))
    out.update(make_case(helper, "b", 7200, 3000, 12, 32))
    path = os.path.join(HERE, "multiview_ref.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < 1_000_000


if __name__ == "__main__":
    main()
