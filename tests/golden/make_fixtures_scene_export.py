"""Generates tests/golden/scene_export_ref.npz by RUNNING THE REFERENCE'S OWN FUNCTIONS, unchanged, in this container:
``data/scannet/load_scannet_data.py::export`` (with ``scannet_utils.compute_normal`` behind it) and
``data/scannet/generate_spatiality_label.py::get_z_relation_per_scene`` / ``get_xy_relation_per_scene`` (save_npy=True).

The three modules are loaded by path.  ``plyfile`` and ``seaborn`` are not installed here and are stubbed: ``PlyData.read``
returns the synthetic vertex and face records (structured arrays, as plyfile would give them).  The mesh, aggregation,
segmentation, label-map and meta files the functions open are written to a temporary working directory, which is also
where the relation functions find ``./scannet_data/<scene>_aligned_bbox.npy`` and leave their ``_x / _y / _z.npy``; the
alignment matrix is written with ``repr`` so that it round-trips.  Nothing of the reference is copied; the fixture holds
only the synthetic inputs and the recorded results.

The generator asserts what the tests rely on: no aligned coordinate lies in the float32 guard band
(tests/scene_export_restated.band), and every quirk occurs where the cases claim it -- a vertex whose accumulate-all
normal differs from the last-face-wins one, an overwritten segment, an all-zero box row, every relation class on every
axis.

Run:  python tests/golden/make_fixtures_scene_export.py            (writes the fixture)
      python tests/golden/make_fixtures_scene_export.py --time     (also times the reference on a full-size synthetic scene)
"""
import importlib.util
import json
import math
import os
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import scene_export_restated as R  # noqa: E402

REF = "/root/reference/data/scannet"
LABELS = {"wall": 1, "floor": 2, "cabinet": 3, "bed": 4, "chair": 5, "sofa": 6, "table": 7, "door": 8, "window": 9,
          "ceiling": 22, "desk": 14, "toilet": 33, "lamp": 35, "box": 39}          # "ceiling" -> 22 is outside NYU40IDS
_MESH = {}


def load_reference():
    ply = types.ModuleType("plyfile")

    class _Element:
        def __init__(self, data):
            self.data, self.count = data, len(data)

    class PlyData:
        @staticmethod
        def read(f):
            return {"vertex": _Element(_MESH["vertex"]), "face": _Element(_MESH["face"])}

    ply.PlyData, ply.PlyElement = PlyData, object
    sys.modules["plyfile"] = ply
    sys.modules["seaborn"] = types.ModuleType("seaborn")
    os.environ.setdefault("MPLBACKEND", "Agg")
    mods = {}
    for name in ("scannet_utils", "load_scannet_data", "generate_spatiality_label"):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods


def run_export(mods, tmp, name, xyz, rgb, faces, seg_indices, groups, axis_align):
    """The reference's export on synthetic arrays, through the files it opens."""
    vertex = np.zeros(len(xyz), dtype=[("x", "f4"), ("y", "f4"), ("z", "f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                                       ("alpha", "u1")])
    for k, col in zip(("x", "y", "z"), xyz.T):
        vertex[k] = col
    for k, col in zip(("red", "green", "blue"), rgb.T):
        vertex[k] = col
    face = np.zeros(len(faces), dtype=[("vertex_indices", "i4", (3,))])
    face["vertex_indices"] = faces
    _MESH["vertex"], _MESH["face"] = vertex, face
    base = os.path.join(tmp, name)
    open(base + ".ply", "wb").close()
    json.dump({"segIndices": seg_indices.tolist()}, open(base + ".segs.json", "w"))
    agg = base + ".aggregation.json"
    if groups is not None:
        json.dump({"segGroups": groups}, open(agg, "w"))
    with open(base + ".txt", "w") as f:
        if axis_align is not None:
            f.write("axisAlignment = " + " ".join(repr(float(v)) for v in axis_align.reshape(-1)) + "\n")
        f.write("numDepthFrames = 0\n")
    tsv = os.path.join(tmp, "labels.tsv")
    with open(tsv, "w") as f:
        f.write("id\traw_category\tnyu40id\n")
        for i, (k, v) in enumerate(LABELS.items()):
            f.write(f"{i}\t{k}\t{v}\n")
    t0 = time.perf_counter()
    out = mods["load_scannet_data"].export(base + ".ply", agg, base + ".segs.json", base + ".txt", tsv)
    return out, time.perf_counter() - t0


def run_relations(mods, tmp, name, aligned_bbox):
    """The reference's three relation functions on ./scannet_data/<name>_aligned_bbox.npy."""
    os.makedirs(os.path.join(tmp, "scannet_data"), exist_ok=True)
    np.save(os.path.join(tmp, "scannet_data", name + "_aligned_bbox.npy"), aligned_bbox)
    g = mods["generate_spatiality_label"]
    t0 = time.perf_counter()
    g.get_z_relation_per_scene(scene_id=name, visualize=False, savefig=False, dryrun=False, verbose=False, save_npy=True)
    g.get_xy_relation_per_scene(dim=0, scene_id=name, visualize=False, savefig=False, dryrun=False, verbose=False, save_npy=True)
    g.get_xy_relation_per_scene(dim=1, scene_id=name, visualize=False, savefig=False, dryrun=False, verbose=False, save_npy=True)
    dt = time.perf_counter() - t0
    return [np.load(os.path.join(tmp, "scannet_data", f"{name}_{a}.npy")) for a in "xyz"], dt


def rot_z(t, tx, ty, tz):
    c, s = math.cos(t), math.sin(t)
    return np.array([[c, -s, 0, tx], [s, c, 0, ty], [0, 0, 1, tz], [0, 0, 0, 1]], dtype=np.float64)


def case_a(rng):
    """A 50 x 40 jittered height field with raised boxes, two faces per cell; 8 x 8 vertex blocks as segments."""
    W, H = 50, 40
    gx, gy = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    z = rng.uniform(0, 0.02, (W, H))
    for _ in range(9):
        x0, y0 = rng.integers(0, W - 8), rng.integers(0, H - 8)
        z[x0:x0 + rng.integers(3, 8), y0:y0 + rng.integers(3, 8)] += rng.uniform(0.3, 1.4)
    for bx, by in ((0, 2), (1, 4), (2, 4), (4, 1)):                     # whole segments raised: objects above others
        z[8 * bx:8 * bx + 8, 8 * by:8 * by + 8] += rng.uniform(0.4, 1.2)
    xyz = np.stack([gx * 0.1 + rng.uniform(-0.03, 0.03, (W, H)), gy * 0.1 + rng.uniform(-0.03, 0.03, (W, H)), z], -1).reshape(-1, 3)
    seg = ((gx // 8) * 5 + gy // 8).reshape(-1)                         # 7 x 5 = 35 segments
    iso = rng.uniform(0, 3, (7, 3))                                      # isolated vertices: segment 35
    xyz = np.concatenate([xyz, iso]).astype(np.float32)
    seg = np.concatenate([seg, np.full(7, 35)]).astype(np.int32)
    idx = (gx * H + gy)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    faces = np.concatenate([faces, faces[rng.integers(0, len(faces), 12)]])                    # repeated faces
    deg = rng.integers(0, W * H, (6, 2))
    faces = np.concatenate([faces, np.stack([deg[:, 0], deg[:, 1], deg[:, 1]], 1)])            # two equal corners
    faces = faces[rng.permutation(len(faces))].astype(np.int32)
    names = ["chair", "chair", "table", "wall", "chair", "floor", "ceiling", "cabinet", "bed", "chair", "sofa", "table", "door",
             "window", "desk", "toilet", "lamp", "box", "chair", "cabinet", "table", "wall", "sofa", "door", "box"]
    ids = rng.permutation(len(names))
    groups = []
    for k, nm in enumerate(names):
        segs = [k] + ([25 + k] if k < 8 else [])                        # segments 0..32; 33 is shared below, 34 in no group
        groups.append({"objectId": int(ids[k]), "label": nm, "segments": segs})
    groups[3]["segments"].append(33)                                     # "wall" ...
    groups[17]["segments"].insert(0, 33)                                 # ... then "box": the later object wins the instance
    groups[20]["segments"].append(35)                                    # the isolated vertices belong to a table
    rgb = rng.integers(0, 256, (len(xyz), 3)).astype(np.uint8)
    return xyz, rgb, faces, seg, groups, rot_z(0.3, 1.25, -0.75, 0.1)


def case_b(rng):
    """Random points and random triples: corners are reused heavily, so "the last face wins" decides almost every vertex."""
    N, F = 1537, 6000
    xyz = rng.uniform(-2, 2, (N, 3)).astype(np.float32)
    faces = rng.integers(0, N, (F, 3)).astype(np.int32)
    seg = rng.integers(0, 70, N).astype(np.int32)
    names = list(LABELS)
    groups = [{"objectId": k, "label": names[int(rng.integers(0, len(names)))], "segments": [k] + ([40 + k] if k < 25 else [])}
              for k in range(40)]
    groups[5]["segments"] = [30, 31]                                     # both listed again by objects 30 and 31: a zero row
    rgb = rng.integers(0, 256, (N, 3)).astype(np.uint8)
    return xyz, rgb, faces, seg, groups, None


def case_c(rng):
    N = 300
    xyz = rng.uniform(-1, 3, (N, 3)).astype(np.float32)
    faces = rng.integers(0, N, (450, 3)).astype(np.int32)
    rgb = rng.integers(0, 256, (N, 3)).astype(np.uint8)
    A = rot_z(-1.1, 0.3, 2.0, -0.4)
    return xyz, rgb, faces, rng.integers(0, 9, N).astype(np.int32), None, A


def relation_boxes(rng, M, grid):
    b = np.zeros((M, 8))
    if grid:
        b[:, 0:3] = rng.integers(0, 13, (M, 3)) * 0.25
        b[:, 3:6] = rng.integers(0, 7, (M, 3)) * 0.25                   # zero sizes included
    else:
        b[:, 0:3] = rng.uniform(-3, 3, (M, 3))
        b[:, 3:6] = rng.uniform(0.05, 2.5, (M, 3))
    b[:, 6], b[:, 7] = rng.integers(1, 40, M), np.arange(M)
    return b


def main():
    mods = load_reference()
    tmp = tempfile.mkdtemp(prefix="spacap_scene_export_")
    os.chdir(tmp)
    out = {"label_names": np.array(list(LABELS)), "label_ids": np.array(list(LABELS.values()), dtype=np.int32)}
    rng = np.random.default_rng(20240611)
    for name, make in (("a", case_a), ("b", case_b), ("c", case_c)):
        xyz, rgb, faces, seg, groups, A = make(rng)
        (vert, aligned, sem, ins, bbox, abox), _ = run_export(mods, tmp, name, xyz, rgb, faces, seg, groups, A)
        rel, _ = run_relations(mods, tmp, name, abox)
        assert vert.dtype == np.float32 and sem.dtype == np.uint32 and bbox.dtype == np.float64 and rel[0].dtype == np.uint32
        if A is not None:
            assert not R.band(xyz, A).any(), f"case {name}: an aligned coordinate lies in the guard band; change the seed"
            out[f"{name}/axis_align"] = A
        # the quirks
        every = R.vertex_normals(xyz, faces, accumulate_all=True)
        assert (every.view(np.int32) != vert[:, 6:9].view(np.int32)).any(1).sum() > {"a": 0.2, "b": 0.9, "c": 0.3}[name] * len(xyz), name
        if name == "a":
            assert (vert[:, 6:9] == 0).all(1).sum() >= 7                            # isolated vertices
            assert (ins[seg == 33] == groups[17]["objectId"] + 1).all() and (sem[seg == 33] == LABELS["box"]).all()
            assert (ins[seg == 34] == 0).all() and (sem[seg == 34] == 0).all() and (sem == 22).any()
            assert bbox.shape == (25, 8) and (bbox[:, 3:6] > 0).all()
        if name == "b":
            assert not bbox[5].any() and not abox[5].any() and (np.abs(bbox).sum(1) == 0).sum() == 1
            assert np.array_equal(vert, aligned)
        if name == "c":
            assert bbox.shape == (1, 8) and not bbox.any() and not ins.any()
        if name != "c":
            assert all(set(np.unique(r).tolist()) == {0, 1, 2} for r in rel), name
        out.update({f"{name}/xyz": xyz, f"{name}/rgb": rgb, f"{name}/faces": faces, f"{name}/seg_indices": seg,
                    f"{name}/groups": np.array(json.dumps(groups)), f"{name}/vert": vert, f"{name}/aligned_vert": aligned,
                    f"{name}/sem_label": sem, f"{name}/ins_label": ins, f"{name}/bbox": bbox, f"{name}/aligned_bbox": abox,
                    f"{name}/x": rel[0], f"{name}/y": rel[1], f"{name}/z": rel[2]})
    for name in R.RELATION_CASES:
        grid = name.startswith("grid")
        b = relation_boxes(rng, int(name[4:]), grid)
        rel, _ = run_relations(mods, tmp, name, b)
        if b.shape[0] >= 39:
            assert all(set(np.unique(r).tolist()) == {0, 1, 2} for r in rel), name
        out[f"{name}/bbox"] = b
        out[f"{name}/rel"] = np.stack(rel)
    path = os.path.join(HERE, "scene_export_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000

    if "--time" in sys.argv:
        # a full-size synthetic scene: N = 150 000 vertices, F = 300 000 faces, M = 60 objects
        N, F, M = 150_000, 300_000, 60
        xyz = rng.uniform(0, 8, (N, 3)).astype(np.float32)
        faces = rng.integers(0, N, (F, 3)).astype(np.int32)
        seg = (np.arange(N) // 250).astype(np.int32)
        groups = [{"objectId": k, "label": list(LABELS)[k % len(LABELS)], "segments": list(range(10 * k, 10 * k + 10))} for k in range(M)]
        rgb = rng.integers(0, 256, (N, 3)).astype(np.uint8)
        (_, _, _, _, _, abox), t_export = run_export(mods, tmp, "big", xyz, rgb, faces, seg, groups, rot_z(0.3, 1, 2, 0))
        _, t_rel = run_relations(mods, tmp, "big", abox)
        print(f"reference on this CPU, N={N} F={F} M={M}: export {t_export:.2f} s + relations {t_rel * 1e3:.1f} ms")


if __name__ == "__main__":
    main()
