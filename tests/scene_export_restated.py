"""Numpy restatement of the scene export (spacap3d_amd/scene_export.py, csrc/scene_export.hip):
what the reference's ``load_scannet_data.export`` / ``scannet_utils.compute_normal`` / ``generate_spatiality_label`` compute,
written down per vertex and per pair instead of through numpy's fancy indexing.  tests/test_scene_export_cpu.py holds it
against the reference's recorded results (tests/golden/scene_export_ref.npz, make_fixtures_scene_export.py); the GPU
tests compare the kernels with the same recordings."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "scene_export_ref.npz")
CASES = ("a", "b", "c")
RELATION_CASES = ("grid1", "grid2", "grid39", "grid128", "grid200", "free64")
OUTPUTS = ("vert", "aligned_vert", "sem_label", "ins_label", "bbox", "aligned_bbox", "x", "y", "z")
F32 = np.float32


def load_fixture():
    return np.load(FIXTURE)


def load_case(name, fx=None):
    """Inputs and recorded results of case ``name``: xyz, rgb, faces, seg_indices, groups (list of dicts or None),
    label_map (dict), axis_align ((4, 4) f64 or None), and the nine outputs."""
    fx = fx if fx is not None else load_fixture()
    c = {k: fx[f"{name}/{k}"] for k in ("xyz", "rgb", "faces", "seg_indices") + OUTPUTS}
    groups = json.loads(str(fx[f"{name}/groups"]))
    c["groups"] = groups
    c["label_map"] = dict(zip(fx["label_names"].tolist(), fx["label_ids"].tolist()))
    c["axis_align"] = fx[f"{name}/axis_align"] if f"{name}/axis_align" in fx.files else None
    return c


# ---- normals ------------------------------------------------------------------------------------------------------
def _unit(n):
    """n / (|n| + 1e-8) in float32, the sum of squares added left to right."""
    n = np.asarray(n, dtype=F32)
    length = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
    return n / (length + F32(1e-8))[..., None]


def face_normals(xyz, faces):
    v0, v1, v2 = (xyz[faces[:, c]].astype(F32) for c in range(3))
    a, b = v1 - v0, v2 - v0
    n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                  a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    return _unit(n)


def last_faces(faces, N):
    last = np.full((3, N), -1, dtype=np.int64)
    for f in range(faces.shape[0]):
        for c in range(3):
            last[c, faces[f, c]] = f
    return last


def vertex_normals(xyz, faces, accumulate_all=False):
    """Per vertex ((0 + n[f_0]) + n[f_1]) + n[f_2] with f_c the LAST face that holds the vertex in corner c, normalised.
    ``accumulate_all``: what a true scatter-add would give instead (the generator shows that the two differ)."""
    N = xyz.shape[0]
    out = np.zeros((N, 3), dtype=F32)
    if faces.shape[0]:
        fn = face_normals(xyz, faces)
        if accumulate_all:
            for c in range(3):
                np.add.at(out, faces[:, c], fn)
        else:
            last = last_faces(faces, N)
            for v in range(N):
                for c in range(3):
                    if last[c, v] >= 0:
                        out[v] = out[v] + fn[last[c, v]]
    return _unit(out)


# ---- alignment ------------------------------------------------------------------------------------------------------
def aligned_xyz64(xyz, A):
    """[x, y, z, 1] . A^T in float64, plain left to right."""
    p = xyz.astype(np.float64)
    return np.stack([((p[:, 0] * A[r, 0] + p[:, 1] * A[r, 1]) + p[:, 2] * A[r, 2]) + 1.0 * A[r, 3] for r in range(3)], 1)


def band(xyz, A):
    """(N, 3) bool: coordinates whose float32 rounding is not the same over the plain float64 value and the extended-
    precision value +- 4 float64 ulps -- where a BLAS that fuses or reorders the products could round differently."""
    plain = aligned_xyz64(xyz, A)
    L = np.longdouble
    p, a = xyz.astype(L), A.astype(L)
    ext = np.stack([p[:, 0] * a[r, 0] + p[:, 1] * a[r, 1] + p[:, 2] * a[r, 2] + a[r, 3] for r in range(3)], 1)
    ulp = np.spacing(np.abs(plain)).astype(L)
    lo, hi = (ext - 4 * ulp).astype(F32), (ext + 4 * ulp).astype(F32)
    return (lo != hi) | (plain.astype(F32) != lo)


# ---- labels ---------------------------------------------------------------------------------------------------------
def labels(seg_indices, groups, label_map):
    """(sem, ins, box_label): uint32 per-vertex label and instance ids, and the label id of every object's box."""
    N = seg_indices.shape[0]
    sem, ins = np.zeros(N, dtype=np.uint32), np.zeros(N, dtype=np.uint32)
    if groups is None:
        return sem, ins, np.zeros(1, dtype=np.uint32)
    order = []
    for g in groups:
        if g["label"] not in order:
            order.append(g["label"])
    for label in order:
        for g in groups:
            if g["label"] == label:
                for s in g["segments"]:
                    sem[seg_indices == s] = label_map[label]
    for g in groups:
        for s in g["segments"]:
            ins[seg_indices == s] = g["objectId"] + 1
    box_label = np.zeros(len(groups), dtype=np.uint32)
    for g in groups:
        box_label[g["objectId"]] = sem[np.nonzero(seg_indices == g["segments"][0])[0][0]]
    return sem, ins, box_label


# ---- boxes ----------------------------------------------------------------------------------------------------------
def boxes(xyz, ins, box_label):
    M = box_label.shape[0]
    out = np.zeros((M, 8), dtype=np.float64)
    for m in range(M):
        pts = xyz[ins == m + 1].astype(F32)
        if len(pts) == 0:
            continue
        lo, hi = pts.min(0), pts.max(0)
        out[m, 0:3] = (lo + hi) / F32(2)
        out[m, 3:6] = hi - lo
        out[m, 6], out[m, 7] = box_label[m], m
    return out


# ---- relations ------------------------------------------------------------------------------------------------------
def relations(bbox):
    """(3, M, M) uint32 from the closed forms, pair by pair in float64."""
    M = bbox.shape[0]
    out = np.zeros((3, M, M), dtype=np.uint32)
    for d in range(2):
        c, s = bbox[:, d], bbox[:, d + 3]
        mn, mx = c - s * 0.5, c + s * 0.5
        first, second, eps = mn + s * 0.3, mn + s * 0.7, s * 0.1

        def zero(i, j):
            return abs(mx[i] - mx[j]) <= eps[j] and abs(mn[i] - mn[j]) <= eps[j]

        def fwd0(i, j):
            return (mx[i] > mx[j] and mn[i] >= mn[j]) or (mx[i] <= mx[j] and mx[i] > second[j] and mn[i] > first[j])

        def back(i, j):
            return mx[i] < second[j] and mn[i] > mn[j] and mn[i] < first[j]

        def f1(i, j):
            return fwd0(i, j) or back(j, i)

        for i in range(M):
            for j in range(M):
                out[d, i, j] = 1 if (zero(i, j) or zero(j, i)) else 2 if f1(j, i) else 0 if f1(i, j) else 1
    zm, sz = bbox[:, 2] - bbox[:, 5] * 0.5, bbox[:, 5]
    for i in range(M):
        for j in range(M):
            out[2, i, j] = 2 if zm[j] - zm[i] >= 0.3 * sz[i] else 0 if zm[i] - zm[j] >= 0.3 * sz[j] else 1
    return out


# ---- the whole export -----------------------------------------------------------------------------------------------
def export(c):
    """The nine arrays of a case from its inputs alone."""
    xyz, rgb, faces = c["xyz"].astype(F32), c["rgb"].astype(F32), c["faces"]
    vert = np.concatenate([xyz, rgb, vertex_normals(xyz, faces)], 1).astype(F32)
    aligned = vert.copy()
    if c["axis_align"] is not None:
        aligned[:, 0:3] = aligned_xyz64(xyz, np.asarray(c["axis_align"], dtype=np.float64).reshape(4, 4)).astype(F32)
    sem, ins, box_label = labels(c["seg_indices"], c["groups"], c["label_map"])
    bbox, abox = boxes(vert[:, 0:3], ins, box_label), boxes(aligned[:, 0:3], ins, box_label)
    rel = relations(abox)
    return {"vert": vert, "aligned_vert": aligned, "sem_label": sem, "ins_label": ins, "bbox": bbox, "aligned_bbox": abox,
            "x": rel[0], "y": rel[1], "z": rel[2]}
