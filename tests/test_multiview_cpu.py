"""No-GPU checks of the multiview projection (spacap3d_amd/multiview.py, csrc/multiview.hip): the numpy restatement the GPU
tests compare with (tests/multiview_restated.py) against the results the reference's own ProjectionHelper recorded
(tests/golden/multiview_ref.npz, make_fixtures_multiview.py), the C ABI's argument validation without a device, and the
CPU-tensor errors.

The restatement's f32 arithmetic and the reference's differ in the last bit (BLAS mm, f32 LU inverse), and the decisions are
discontinuous: the map is compared on every (frame, point) pair outside the float64 guard band, aggregated rows on every
point without an in-band pair in any frame; the band itself must stay within the cap (0.2 % of the pairs, 3 % of the
hits)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import multiview_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["a", "b"])
def case(request):
    return R.load_case(request.param)


def test_restatement_reproduces_the_reference(case):
    c = case
    band = R.band(c["points"], c["depths"], c["poses"], **R.CAM)
    assert np.array_equal(band, c["band"])
    hits = int((c["map"] >= 0).sum())
    assert hits > 0.05 * band.size and R.band_within_cap(band, hits), (int(band.sum()), band.size, hits)
    pmap = R.projection_map(c["points"], c["depths"], c["poses"], **R.CAM)
    assert np.array_equal(pmap[~band], c["map"][~band])
    assert not (pmap[3] >= 0).any() and not (pmap[6] >= 0).any()            # the two frames that see nothing
    clean = ~band.any(0)
    assert clean.sum() > 0.95 * clean.size and clean[int(c["quirk"])]
    for mode in ("max", "first"):
        assert np.array_equal(R.aggregate_features(pmap, c["feats"], mode)[clean], c[f"feat_{mode}"][clean]), mode
    for mode in ("vote", "first"):
        assert np.array_equal(R.aggregate_labels(pmap, c["labels"], mode)[clean], c[f"label_{mode}"][clean]), mode
    assert not np.array_equal(c["feat_max"], c["feat_first"]) and not np.array_equal(c["label_vote"], c["label_first"])


def test_frustum_corners_match_the_restatement():
    from spacap3d_amd import multiview
    got = multiview.frustum_corners(R.INTRINSIC, 0.1, 4.0, [41, 32])
    assert got.dtype == np.float32 and np.array_equal(got, R.camera_corners(R.INTRINSIC, 0.1, 4.0, [41, 32]))


def test_header_signatures_and_symbols_agree():
    from spacap3d_amd import _native
    header = open(os.path.join(ROOT, "include", "spacap_hip.h")).read()
    for name in ("spacap_multiview_workspace_bytes", "spacap_multiview_map_f32", "spacap_multiview_features_f32",
                 "spacap_multiview_vote_i32"):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, name
        assert name in _native.SIGNATURES and hasattr(_native.lib, name)
        assert len(m.group(1).split(",")) == len(_native.SIGNATURES[name][1]), name
    assert _native.lib.spacap_abi_version() == 5


def test_argument_validation_needs_no_device():
    from spacap3d_amd._native import lib
    cam = (37.0, 38.5, 20.0, 15.5, 0.1, 4.0, 0.05)
    one = ctypes.c_void_p(16)       # never dereferenced: every check comes before the first device call
    assert lib.spacap_multiview_workspace_bytes(300) >= 300 * 37 * 4 and lib.spacap_multiview_workspace_bytes(0) == 0
    # bad sizes
    assert lib.spacap_multiview_map_f32(one, -1, one, one, 2, 32, 41, *cam, one, one, 1 << 20, one, None) == -1
    assert b"bad sizes" in lib.spacap_last_error()
    assert lib.spacap_multiview_map_f32(one, 10, one, one, 2, 200, 200, *cam, one, one, 1 << 20, one, None) == -1
    assert b"H * W" in lib.spacap_last_error()
    assert lib.spacap_multiview_features_f32(one, 10, one, one, 2, 32, 41, *cam, one, one, 257, 0, one, 1 << 20, one, None) == -1
    assert b"C=257" in lib.spacap_last_error()
    assert lib.spacap_multiview_features_f32(one, 10, one, one, 2, 32, 41, *cam, one, one, 128, 2, one, 1 << 20, one, None) == -1
    assert b"mode=2" in lib.spacap_last_error()
    # null pointers
    assert lib.spacap_multiview_map_f32(None, 10, one, one, 2, 32, 41, *cam, one, one, 1 << 20, one, None) == -1
    assert b"null" in lib.spacap_last_error()
    assert lib.spacap_multiview_map_f32(one, 10, one, one, 2, 32, 41, *cam, one, one, 1 << 20, None, None) == -1
    assert b"null" in lib.spacap_last_error()
    assert lib.spacap_multiview_features_f32(one, 10, one, one, 2, 32, 41, *cam, one, None, 128, 0, one, 1 << 20, one, None) == -1
    assert b"null" in lib.spacap_last_error()
    assert lib.spacap_multiview_vote_i32(one, 10, one, one, 2, 32, 41, *cam, one, one, one, 1 << 20, None, one, None) == -1
    assert b"null" in lib.spacap_last_error()
    # a workspace that is too small
    assert lib.spacap_multiview_vote_i32(one, 10, one, one, 2, 32, 41, *cam, one, one, one, 8, one, one, None) == -1
    assert b"workspace" in lib.spacap_last_error()
    # nothing to do
    assert lib.spacap_multiview_map_f32(None, 0, None, None, 2, 32, 41, *cam, None, None, 0, None, None) == 0
    assert lib.spacap_multiview_features_f32(None, 10, None, None, 0, 32, 41, *cam, None, None, 128, 0, None, 0, None, None) == 0
    assert lib.spacap_multiview_vote_i32(None, 10, None, None, 0, 32, 41, *cam, None, None, None, 0, None, None, None) == 0


def test_cpu_tensors_are_refused():
    from spacap3d_amd.multiview import MultiviewProjector
    proj = MultiviewProjector(**R.CAM)
    pts, dep, pose = torch.rand(5, 3), torch.ones(2, 32, 41), torch.eye(4).repeat(2, 1, 1)
    for call in (lambda: proj.projection_map(pts, dep, pose),
                 lambda: proj.project_features(pts, dep, pose, torch.rand(2, 8, 32, 41)),
                 lambda: proj.project_labels(pts, dep, pose, torch.ones(2, 32, 41, dtype=torch.int64)),
                 lambda: proj.project_labels(pts, dep, pose, torch.ones(2, 32, 41, dtype=torch.int64), mode="first"),
                 lambda: proj.compute_projection(pts, dep[0], pose[0])):
        with pytest.raises(RuntimeError, match="CPU not supported"):
            call()
    with pytest.raises(ValueError, match="image_dims"):
        MultiviewProjector(R.INTRINSIC, 0.1, 4.0, [400, 400], 0.05)
