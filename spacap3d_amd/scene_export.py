"""ScanNet scene preparation on the device (csrc/scene_export.hip): decoded mesh arrays in, the
per-scene arrays ``DeviceSceneDataset.add_scene`` takes out -- what the reference produces offline with
``data/scannet/load_scannet_data.py::export`` (normals from ``scannet_utils.compute_normal``) and
``data/scannet/generate_spatiality_label.py``.  The results are the reference's own, bit for bit; ``save`` writes them
under the reference's nine file names.  Parsing the PLY / JSON / TSV files stays with the caller.

* ``segment_tables``    -- host: ``aggregation.json``'s ``segGroups`` + the label map -> per-segment instance / label tables;
* ``vertex_normals``    -- (N, 3) f32 on the device;
* ``export_scene``      -- ``vert``, ``aligned_vert``, ``sem_label``, ``ins_label``, ``bbox``, ``aligned_bbox``, ``x``, ``y``, ``z``;
* ``spatial_relations`` -- (3, M, M) relation classes of an (M, 8) box array;
* ``save``              -- the nine ``.npy`` files, with the reference's dtypes.

Arrays may be numpy arrays (uploaded to ``device``) or tensors on a GPU; CPU tensors raise
``RuntimeError("... CPU not supported")``: there is no host fallback.  Either way positions, colours and boxes of any real
dtype are converted to float32 / float32 / float64 (a float64 position is rounded, as the reference's float32 PLY reader
would have stored it), while faces, segment ids and the tables must have an integer dtype: a floating-point index array is
refused, not truncated.  ``axis_align`` may be a list, an array or a tensor anywhere: its 16 numbers go to the kernel by value.  Labels and relation classes are int32 on the device
(uint32 in the files).

Write order of the labels (load_scannet_data.py:17-32, 84-102).  Semantic labels are written label by label in the order
the labels first appear in ``segGroups``, within a label group by group, segment by segment; instance ids group by group;
in both the later write wins.  The reference's ``label_to_segs[label] = segs`` aliases the first object's segment list and
``.extend`` then grows it by the segments of the later objects of that label, so the first object also writes ITS id onto
their segments -- but every one of those later objects comes after it in the instance loop and overwrites all of its own
segments, so the outcome equals the plain order, which is what ``segment_tables`` implements.  A box's label is the label
id of its object's first segment after all label writes.

Limits: 1 <= N < 2^24 vertices, F >= 0 faces, 1 <= M <= 1024 instances (``DeviceSceneDataset``'s ``max_instances``
default).  Positions must be finite.  Indices are validated here, before the first launch: face corners in [0, N), segment
ids inside the tables, ``objectId``s unique and < M, no group without segments.
"""
import ctypes

import numpy as np
import torch

from ._native import check, lib

MAX_VERTICES = 1 << 24
MAX_INSTANCES = 1024
FILES = (("vert", np.float32), ("aligned_vert", np.float32), ("sem_label", np.uint32), ("ins_label", np.uint32),
         ("bbox", np.float64), ("aligned_bbox", np.float64), ("x", np.uint32), ("y", np.uint32), ("z", np.uint32))


def segment_tables(seg_groups, label_map, seg_indices):
    """``seg_groups``: the ``segGroups`` entries of ``<scene>.aggregation.json`` (dicts with ``objectId``, ``label``,
    ``segments``), or None for a scene without aggregation; ``label_map``: raw_category -> nyu40id; ``seg_indices``: the
    ``segIndices`` array of ``<scene>_vh_clean_2.0.010000.segs.json``.  Returns int32 arrays ``(seg_ins, seg_sem,
    box_label)``: instance id (objectId + 1, 0 = none) and label id per segment id, label id per object.  A listed segment
    that no vertex carries is skipped."""
    seg = np.asarray(seg_indices).reshape(-1).astype(np.int64)
    if seg.size and int(seg.min()) < 0:
        raise ValueError("scene_export: negative segment id in seg_indices")
    S = int(seg.max()) + 1 if seg.size else 1
    seg_ins, seg_sem = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
    if seg_groups is None:
        return seg_ins, seg_sem, np.zeros(1, dtype=np.int32)
    present = np.zeros(S, dtype=bool)
    present[seg] = True
    M = len(seg_groups)
    if not 1 <= M <= MAX_INSTANCES:
        raise ValueError(f"scene_export: {M} objects, supported 1..{MAX_INSTANCES}")
    ids = [int(g["objectId"]) for g in seg_groups]
    if len(set(ids)) != M or min(ids) < 0 or max(ids) >= M:
        raise ValueError(f"scene_export: objectIds must be unique and in [0, {M})")
    by_label = {}
    for g in seg_groups:
        segs = [int(s) for s in g["segments"]]
        if not segs:
            raise ValueError(f"scene_export: object {g['objectId']} has an empty segment list")
        if min(segs) < 0:
            raise ValueError(f"scene_export: object {g['objectId']} lists a negative segment id")
        by_label.setdefault(g["label"], []).append(segs)
    for label, groups in by_label.items():            # dicts keep the order of first appearance
        label_id = int(label_map[label])
        for segs in groups:
            for s in segs:
                if s < S and present[s]:
                    seg_sem[s] = label_id
    box_label = np.zeros(M, dtype=np.int32)
    for g in seg_groups:
        for s in g["segments"]:
            if s < S and present[s]:
                seg_ins[s] = int(g["objectId"]) + 1
    for g in seg_groups:
        first = next((int(s) for s in g["segments"] if s < S and present[s]), None)
        if first is not None:
            box_label[int(g["objectId"])] = seg_sem[first]
    return seg_ins, seg_sem, box_label


def _device_of(device, *arrays):
    for a in arrays:
        if isinstance(a, torch.Tensor) and not a.is_cuda:
            raise RuntimeError("scene_export: CPU not supported")
    for a in arrays:
        if isinstance(a, torch.Tensor):
            return a.device
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("scene_export: CPU not supported")
    return dev


_NP = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32}


def _checked(name, a, dtype, dev, tail, hi=None):
    """``a`` -- a numpy array or a tensor on ``dev`` -- with its shape ``(n,) + tail`` checked and, with ``hi``, every entry in
    [0, hi): on the host for a host array, by one reduction for a device tensor (read before anything is launched).  Host
    arrays stay on the host until ``_put``: nothing touches the device before every argument has passed.  Index arrays
    (``dtype`` int32) must have an integer dtype, array and tensor alike; numbers of any real dtype are converted to
    ``dtype``."""
    if dtype == torch.int32:
        integer = (not a.is_floating_point() and not a.is_complex() and a.dtype != torch.bool) \
            if isinstance(a, torch.Tensor) else np.asarray(a).dtype.kind in "iu"
        if not integer:
            raise ValueError(f"scene_export: {name} must have an integer dtype, got {a.dtype if hasattr(a, 'dtype') else type(a)}")
    if isinstance(a, torch.Tensor):
        if a.device != dev:
            raise RuntimeError(f"scene_export: {name} must be on {dev}")
        bad = hi is not None and a.numel() and bool(((a < 0) | (a >= hi)).any())
    else:
        a = np.asarray(a)
        bad = hi is not None and a.size and (int(a.min()) < 0 or int(a.max()) >= hi)
        a = np.ascontiguousarray(a, dtype=_NP[dtype])
    if a.ndim != 1 + len(tail) or tuple(a.shape[1:]) != tuple(tail):
        raise ValueError(f"scene_export: {name} must be {('n',) + tuple(tail)}, got {tuple(a.shape)}")
    if bad:
        raise ValueError(f"scene_export: {name}: a value outside [0, {hi})")
    return a


def _put(a, dtype, dev):
    return a.to(dtype).contiguous() if isinstance(a, torch.Tensor) else torch.as_tensor(a).to(dev)


def _mesh(xyz, faces, dev):
    xyz = _checked("xyz", xyz, torch.float32, dev, (3,))
    N = xyz.shape[0]
    if not 1 <= N < MAX_VERTICES:
        raise ValueError(f"scene_export: N={N} vertices, supported 1..{MAX_VERTICES - 1}")
    if faces is None or (not isinstance(faces, torch.Tensor) and np.size(faces) == 0):
        faces = np.zeros((0, 3), dtype=np.int32)
    faces = _checked("faces", faces, torch.int32, dev, (3,), hi=N)
    return xyz, faces, N


def vertex_normals(xyz, faces, device="cuda:0"):
    """``xyz`` (N, 3) f32, ``faces`` (F, 3) integer -> the reference's vertex normals (N, 3) f32 on the device."""
    dev = _device_of(device, xyz, faces)
    xyz, faces, N = _mesh(xyz, faces, dev)
    xyz, faces = _put(xyz, torch.float32, dev), _put(faces, torch.int32, dev)
    with torch.cuda.device(dev):
        nb = int(lib.spacap_scene_export_workspace_bytes(N, 0))
        ws = torch.empty(nb // 4, dtype=torch.int32, device=dev)
        out = torch.empty(N, 3, dtype=torch.float32, device=dev)
        check(lib.spacap_scene_normals_f32(xyz.data_ptr(), N, faces.data_ptr(), faces.shape[0], ws.data_ptr(), nb,
                                           out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
              "spacap_scene_normals_f32")
    return out


def spatial_relations(bbox, device="cuda:0"):
    """``bbox`` (M, 8) f64 [centre, size, ...] -> (3, M, M) int32 on the device: the x, y and z relation classes
    (0 = forward / up, 1 = same, 2 = behind / below)."""
    dev = _device_of(device, bbox)
    bbox = _checked("bbox", bbox, torch.float64, dev, (8,))
    M = bbox.shape[0]
    if not 1 <= M <= MAX_INSTANCES:
        raise ValueError(f"scene_export: M={M} boxes, supported 1..{MAX_INSTANCES}")
    bbox = _put(bbox, torch.float64, dev)
    with torch.cuda.device(dev):
        rel = torch.empty(3, M, M, dtype=torch.int32, device=dev)
        check(lib.spacap_scene_relations_f64(bbox.data_ptr(), M, rel.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
              "spacap_scene_relations_f64")
    return rel


def export_scene(xyz, rgb, faces, seg_indices, tables, axis_align=None, device="cuda:0"):
    """``xyz`` (N, 3) f32, ``rgb`` (N, 3) in 0..255, ``faces`` (F, 3), ``seg_indices`` (N,), ``tables`` =
    ``segment_tables(...)``, ``axis_align``: the scene's 4 x 4 ``axisAlignment`` (16 numbers, row-major; list, array or tensor) or
    None.
    Returns device tensors: ``vert`` / ``aligned_vert`` (N, 9) f32, ``sem_label`` / ``ins_label`` (N,) int32, ``bbox`` /
    ``aligned_bbox`` (M, 8) f64, ``x`` / ``y`` / ``z`` (M, M) int32.  Five launches; nothing is read back after the index
    checks."""
    dev = _device_of(device, xyz, rgb, faces, seg_indices, *tables)
    xyz, faces, N = _mesh(xyz, faces, dev)
    rgb = _checked("rgb", rgb, torch.float32, dev, (3,))
    seg_ins, seg_sem, box_label = tables
    S, M = int(seg_ins.shape[0]), int(box_label.shape[0])
    if S < 1 or int(seg_sem.shape[0]) != S or not 1 <= M <= MAX_INSTANCES:
        raise ValueError(f"scene_export: tables of {S} / {int(seg_sem.shape[0])} segments and {M} objects (1..{MAX_INSTANCES})")
    seg = _checked("seg_indices", seg_indices, torch.int32, dev, (), hi=S)
    if rgb.shape[0] != N or seg.shape[0] != N:
        raise ValueError(f"scene_export: rgb and seg_indices must have N={N} rows")
    seg_ins = _checked("seg_ins", seg_ins, torch.int32, dev, (), hi=M + 1)
    seg_sem = _checked("seg_sem", seg_sem, torch.int32, dev, ())
    box_label = _checked("box_label", box_label, torch.int32, dev, ())
    align = None
    if axis_align is not None:
        if isinstance(axis_align, torch.Tensor):          # 16 numbers: they travel to the kernel as an argument
            axis_align = axis_align.detach().cpu().numpy()
        align = np.ascontiguousarray(np.asarray(axis_align, dtype=np.float64).reshape(-1))
        if align.size != 16:
            raise ValueError("scene_export: axis_align must hold 16 numbers")
    xyz, rgb = _put(xyz, torch.float32, dev), _put(rgb, torch.float32, dev)
    faces, seg, seg_ins, seg_sem, box_label = (_put(t, torch.int32, dev) for t in (faces, seg, seg_ins, seg_sem, box_label))
    with torch.cuda.device(dev):
        nb = int(lib.spacap_scene_export_workspace_bytes(N, M))
        ws = torch.empty(nb // 4, dtype=torch.int32, device=dev)
        f32, i32, f64 = (dict(dtype=d, device=dev) for d in (torch.float32, torch.int32, torch.float64))
        vert, aligned = torch.empty(N, 9, **f32), torch.empty(N, 9, **f32)
        ins, sem = torch.empty(N, **i32), torch.empty(N, **i32)
        bbox, abox = torch.empty(M, 8, **f64), torch.empty(M, 8, **f64)
        rel = torch.empty(3, M, M, **i32)
        check(lib.spacap_scene_export_f32(
            xyz.data_ptr(), rgb.data_ptr(), N, faces.data_ptr(), faces.shape[0], seg.data_ptr(), seg_ins.data_ptr(),
            seg_sem.data_ptr(), S, box_label.data_ptr(), M, None if align is None else align.ctypes.data_as(ctypes.c_void_p),
            ws.data_ptr(), nb, vert.data_ptr(), aligned.data_ptr(), ins.data_ptr(), sem.data_ptr(), bbox.data_ptr(),
            abox.data_ptr(), rel.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "spacap_scene_export_f32")
    return {"vert": vert, "aligned_vert": aligned, "sem_label": sem, "ins_label": ins, "bbox": bbox, "aligned_bbox": abox,
            "x": rel[0], "y": rel[1], "z": rel[2]}


def save(result, prefix):
    """Writes ``export_scene``'s result (tensors or numpy arrays) as ``<prefix>_vert.npy``, ``_aligned_vert.npy``,
    ``_sem_label.npy``, ``_ins_label.npy``, ``_bbox.npy``, ``_aligned_bbox.npy``, ``_x.npy``, ``_y.npy``, ``_z.npy`` with the
    reference's dtypes: float32 vertices, uint32 labels and relations, float64 boxes."""
    for key, dtype in FILES:
        v = result[key]
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        np.save(f"{prefix}_{key}.npy", np.ascontiguousarray(v.astype(dtype)))
