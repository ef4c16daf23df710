"""Multiview image features projected onto scene points on the device (csrc/multiview.hip): the
``(N, 128)`` rows that ``DeviceSceneDataset(use_multiview=True)`` takes, which the reference produces with
``scripts/project_multiview_features.py`` (labels: ``scripts/project_multiview_labels.py``) on top of ``lib/projection.py``
-- per frame a few dozen torch ops over all vertices, three host reads and a ``torch.inverse``.  Here one launch walks all
frames of a call, and there is no host synchronisation.

* ``MultiviewProjector.projection_map``   -- (F, N) int32: the pixel of every point in every frame, or -1;
* ``MultiviewProjector.project_features`` -- (N, C) f32 rows, ``mode="max"`` (the reference's ``--maxpool``, the mode behind
  ``enet_feats_maxpool.hdf5``) or ``"first"``;
* ``MultiviewProjector.project_labels``   -- (N,) int64 labels, ``mode="vote"`` (``--maxpool`` of the label script) or ``"first"``;
* ``MultiviewProjector.compute_projection`` -- the drop-in for ``ProjectionHelper.compute_projection`` (one frame, reads the
  count on the host as the reference does).

The 2D network that makes the feature maps is ``spacap3d_amd/enet.py``; its pixel-major output goes in as it is
(``channels_last=True``), and any other ``(F, C, H, W)`` maps do too.  The frames of a scene may come in several calls
(``out=``): 300 frames of (128, 32, 41) f32 are 200 MB, and the result does not depend on the split.

Vertex set: the reference projects onto the scene's UNALIGNED vertices (``<scene>_vert.npy``, the frame poses live in that
coordinate system); their row order is that of ``<scene>_aligned_vert.npy``, so the rows go to ``add_scene(multiview=)`` as
they are.

CPU tensors raise ``RuntimeError("... CPU not supported")``: there is no host fallback.
"""
import ctypes

import numpy as np
import torch

from ._eval_util import gpu
from ._native import check, lib

MAX_PIXELS = 6656      # H * W of one depth map (csrc/multiview.hip: MV_DEPTH_FLOATS)
MAX_CHANNELS = 256
NUM_LABELS = 64        # labels 0..63; 0 = none
_MODES = {"max": 0, "first": 1}


def frustum_corners(intrinsic, depth_min, depth_max, image_dims):
    """The eight camera-space frustum corners (8, 3) f32 of lib/projection.py:17-46: computed in double, rounded to f32."""
    fx, fy, cx, cy = (float(intrinsic[0][0]), float(intrinsic[1][1]), float(intrinsic[0][2]), float(intrinsic[1][2]))
    W, H = int(image_dims[0]), int(image_dims[1])
    rows = []
    for d in (float(depth_min), float(depth_max)):
        for ux, uy in ((0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1)):
            rows.append([d * ((ux - cx) / fx), d * ((uy - cy) / fy), d])
    return np.asarray(rows, dtype=np.float64).astype(np.float32)


class MultiviewProjector:
    """``ProjectionHelper``'s constructor arguments (lib/projection.py:6): ``intrinsic`` (at least 2 x 3: fx, fy, cx, cy),
    the depth range in metres, ``image_dims = [W, H]`` and the depth ``accuracy``.  The reference's scripts use
    fx = 37.01983, fy = 38.52470, cx = 20, cy = 15.5, 0.1 .. 4.0, [41, 32], 0.05."""

    def __init__(self, intrinsic, depth_min, depth_max, image_dims, accuracy):
        self.intrinsic = [[float(v) for v in row] for row in intrinsic]
        self.depth_min, self.depth_max, self.accuracy = float(depth_min), float(depth_max), float(accuracy)
        self.image_dims = [int(image_dims[0]), int(image_dims[1])]
        W, H = self.image_dims
        if W < 1 or H < 1 or W * H > MAX_PIXELS:
            raise ValueError(f"multiview: image_dims={self.image_dims}: 1 <= W * H <= {MAX_PIXELS}")
        self._corners = np.ascontiguousarray(frustum_corners(self.intrinsic, depth_min, depth_max, self.image_dims))
        self._cam = (self.intrinsic[0][0], self.intrinsic[1][1], self.intrinsic[0][2], self.intrinsic[1][2],
                     self.depth_min, self.depth_max, self.accuracy)

    # ---- arguments ---------------------------------------------------------------------------------------------
    def _frames(self, points, depths, poses):
        W, H = self.image_dims
        points = gpu("multiview", points, "points")
        dev = points.device
        depths = gpu("multiview", depths, "depths")
        poses = gpu("multiview", poses, "poses")
        if points.dim() != 2 or points.shape[1] != 3:
            raise RuntimeError(f"multiview: points must be (N, 3), got {tuple(points.shape)}")
        if depths.dim() == 2:
            depths, poses = depths[None], poses[None]
        F = depths.shape[0]
        if tuple(depths.shape) != (F, H, W) or tuple(poses.shape) != (F, 4, 4):
            raise RuntimeError(f"multiview: depths must be (F, {H}, {W}) and poses (F, 4, 4), got {tuple(depths.shape)}, "
                               f"{tuple(poses.shape)}")
        if depths.device != dev or poses.device != dev:
            raise RuntimeError(f"multiview: depths and poses must be on {dev}")
        return points.float().contiguous(), depths.float().contiguous(), poses.float().contiguous(), F

    def _call(self, fn, name, points, depths, poses, F, middle, tail):
        dev = points.device
        W, H = self.image_dims
        with torch.cuda.device(dev):
            nb = int(lib.spacap_multiview_workspace_bytes(F))
            ws = torch.empty(max(nb, 4) // 4, dtype=torch.float32, device=dev)
            check(fn(points.data_ptr(), points.shape[0], depths.data_ptr(), poses.data_ptr(), F, H, W, *self._cam,
                     self._corners.ctypes.data_as(ctypes.c_void_p), *middle, ws.data_ptr(), nb, *tail,
                     torch.cuda.current_stream(dev).cuda_stream), name)

    # ---- the map -----------------------------------------------------------------------------------------------
    def projection_map(self, points, depths, poses):
        """``points`` (N, 3), ``depths`` (F, H, W) in metres, ``poses`` (F, 4, 4) camera_to_world, all on the device ->
        (F, N) int32: the pixel ``v * W + u`` of point n in frame f, or -1."""
        points, depths, poses, F = self._frames(points, depths, poses)
        N = points.shape[0]
        with torch.cuda.device(points.device):
            out = torch.empty(F, N, dtype=torch.int32, device=points.device)
        if F and N:
            self._call(lib.spacap_multiview_map_f32, "spacap_multiview_map_f32", points, depths, poses, F, (),
                       (out.data_ptr(),))
        return out

    # ---- features ----------------------------------------------------------------------------------------------
    def project_features(self, points, depths, poses, feats, mode="max", out=None, channels_last=False):
        """``feats``: (F, C, H, W) as the reference's per-frame ``.npy`` files stack, or (F, H, W, C) / (F, H W, C) with
        ``channels_last=True`` (no transposing copy then; the second is ``ENetEncoder``'s output as it is); C <= 256.
        Returns the (N, C) f32 rows on the device.  ``mode``:
        ``"max"`` -- per point, over the frames that cover it (the point maps and the pixel's vector is not all-zero) in
        ascending order: an all-zero row takes the vector, any other row the element-wise maximum (a row that a maximum turns
        all-zero counts as unfilled again, as in the reference); ``"first"`` -- the first covering frame's vector.
        ``out``: the result of an earlier call on the same points, continued with these frames (it is updated in place and
        returned): a scene's frames in any number of chunks give bit-identical rows.  No host synchronisation."""
        if mode not in _MODES:
            raise ValueError(f"multiview: mode={mode!r}, expected 'max' or 'first'")
        points, depths, poses, F = self._frames(points, depths, poses)
        dev, N = points.device, points.shape[0]
        W, H = self.image_dims
        feats = gpu("multiview", feats, "feats")
        if channels_last and feats.dim() == 3 and feats.shape[0] == F and feats.shape[1] == H * W:
            feats = feats.view(F, H, W, feats.shape[2]) if feats.is_contiguous() else feats.reshape(F, H, W, feats.shape[2])
        elif feats.dim() == 3 and F == 1:
            feats = feats[None]
        want = "(F, H, W, C)" if channels_last else "(F, C, H, W)"
        if feats.dim() != 4 or feats.device != dev or \
                (tuple(feats.shape[:3]) if channels_last else (feats.shape[0],) + tuple(feats.shape[2:])) != (F, H, W):
            raise RuntimeError(f"multiview: feats must be {want} with F={F}, H={H}, W={W} on {dev}, got {tuple(feats.shape)}")
        C = feats.shape[3] if channels_last else feats.shape[1]
        if not 1 <= C <= MAX_CHANNELS:
            raise RuntimeError(f"multiview: C={C} channels, supported 1..{MAX_CHANNELS}")
        feats = feats.float()
        # pixel-major: a hit reads one contiguous C-float row (one pass over the input, not the hot part)
        feats = feats.contiguous() if channels_last else feats.permute(0, 2, 3, 1).contiguous()
        if out is None:
            with torch.cuda.device(dev):
                out = torch.zeros(N, C, dtype=torch.float32, device=dev)
        else:
            out = gpu("multiview", out, "out")
            if tuple(out.shape) != (N, C) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
                raise RuntimeError(f"multiview: out must be a contiguous float32 tensor of shape {(N, C)} on {dev}")
        if F and N:
            self._call(lib.spacap_multiview_features_f32, "spacap_multiview_features_f32", points, depths, poses, F,
                       (feats.data_ptr(), C, _MODES[mode]), (out.data_ptr(),))
        return out

    # ---- labels ------------------------------------------------------------------------------------------------
    def vote_state(self, num_points, device):
        """The (N, 64) int32 counts ``project_labels(mode="vote", out=)`` carries from call to call, zeroed."""
        with torch.cuda.device(device):
            return torch.zeros(int(num_points), NUM_LABELS, dtype=torch.int32, device=device)

    def project_labels(self, points, depths, poses, labels, mode="vote", out=None):
        """``labels``: (F, H, W) integer label maps, 0 = none, 1..63.  Returns (N,) int64 on the device.  ``mode``:
        ``"vote"`` -- the most frequent non-zero label over the frames that cover the point, a tie goes to the label seen
        first, 0 when there is none (scripts/project_multiview_labels.py --maxpool); ``out``: the ``vote_state`` tensor of the
        scene, updated in place (the returned labels are the result over all frames so far).  ``"first"`` -- the first
        covering frame's label; ``out``: the (N,) int64 result of an earlier call, updated in place."""
        if mode not in ("vote", "first"):
            raise ValueError(f"multiview: mode={mode!r}, expected 'vote' or 'first'")
        W, H = self.image_dims
        pts, dep, pos, F = self._frames(points, depths, poses)
        dev, N = pts.device, pts.shape[0]
        labels = gpu("multiview", labels, "labels")
        if labels.dim() == 2 and F == 1:
            labels = labels[None]
        if tuple(labels.shape) != (F, H, W) or labels.device != dev:
            raise RuntimeError(f"multiview: labels must be (F, H, W) with F={F}, H={H}, W={W} on {dev}, got {tuple(labels.shape)}")
        if mode == "first":
            if out is not None and (gpu("multiview", out, "out").dtype != torch.int64 or tuple(out.shape) != (N,)):
                raise RuntimeError(f"multiview: out must be an int64 tensor of shape {(N,)}")
            acc = None if out is None else out.float().unsqueeze(1).contiguous()
            acc = self.project_features(pts, dep, pos, labels.float().unsqueeze(3), "first", acc, channels_last=True)
            res = acc[:, 0].long()
            return res if out is None else out.copy_(res)
        if out is None:
            out = self.vote_state(N, dev)
        else:
            out = gpu("multiview", out, "out")
            if tuple(out.shape) != (N, NUM_LABELS) or out.dtype != torch.int32 or out.device != dev or not out.is_contiguous():
                raise RuntimeError(f"multiview: out must be the contiguous int32 vote_state of shape {(N, NUM_LABELS)} on {dev}")
        if F and N:
            with torch.cuda.device(dev):
                voted = torch.empty(N, dtype=torch.int32, device=dev)
            lab = labels.to(torch.int32).contiguous()
            self._call(lib.spacap_multiview_vote_i32, "spacap_multiview_vote_i32", pts, dep, pos, F, (lab.data_ptr(),),
                       (out.data_ptr(), voted.data_ptr()))
            return voted.long()
        if N == 0:
            return torch.zeros(0, dtype=torch.int64, device=dev)
        best, arg = out[:, 1:].max(1)                  # no new frames: the labels the state holds
        return torch.where(best > 0, arg + 1, torch.zeros_like(arg))

    # ---- drop-in -----------------------------------------------------------------------------------------------
    def compute_projection(self, points, depth, camera_to_world):
        """``ProjectionHelper.compute_projection`` (lib/projection.py:189-260) for one frame: ``(indices_3d, indices_2d)``,
        int64 of length N + 1 -- the count, then the mapped points in ascending order / their pixels, zeros behind -- or
        ``None`` when nothing maps.  Reads the count on the host, as the reference does."""
        pix = self.projection_map(points, depth, camera_to_world)[0]
        idx = torch.nonzero(pix >= 0)[:, 0]
        n = idx.numel()
        if n == 0:
            return None
        i3 = torch.zeros(pix.numel() + 1, dtype=torch.int64, device=pix.device)
        i2 = torch.zeros_like(i3)
        i3[0] = i2[0] = n
        i3[1:1 + n] = idx
        i2[1:1 + n] = pix[idx].long()
        return i3, i2
