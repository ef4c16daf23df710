"""No-GPU checks of the scene export (spacap3d_amd/scene_export.py, csrc/scene_export.hip): the numpy
restatement (tests/scene_export_restated.py) against every array the reference's own functions recorded
(tests/golden/scene_export_ref.npz, make_fixtures_scene_export.py) bit for bit, the empty alignment guard band, the host-side
segment tables, ``save``, the C ABI's argument validation without a device, and the index checks that come before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import scene_export_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("spacap_scene_export_workspace_bytes", "spacap_scene_normals_f32", "spacap_scene_relations_f64",
           "spacap_scene_export_f32")


def same_bits(got, want):
    """Equal shape, dtype and bytes (-0.0 and 0.0 differ)."""
    return got.shape == want.shape and got.dtype == want.dtype and \
        np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes()


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


@pytest.fixture(scope="module", params=R.CASES)
def case(request, fixture):
    return R.load_case(request.param, fixture)


def test_restatement_reproduces_every_recorded_array(case):
    got = R.export(case)
    for k in R.OUTPUTS:
        assert same_bits(got[k], case[k]), k
    assert case["vert"].dtype == np.float32 and case["sem_label"].dtype == np.uint32 and case["ins_label"].dtype == np.uint32
    assert case["bbox"].dtype == np.float64 and case["x"].dtype == np.uint32


def test_alignment_guard_band_is_empty(case):
    if case["axis_align"] is None:
        assert same_bits(case["vert"], case["aligned_vert"])
    else:
        assert not R.band(case["xyz"], case["axis_align"]).any()


@pytest.mark.parametrize("name", R.RELATION_CASES)
def test_relation_closed_forms_reproduce_the_reference(fixture, name):
    want = fixture[f"{name}/rel"]
    assert want.dtype == np.uint32 and same_bits(R.relations(fixture[f"{name}/bbox"]), want)


def test_segment_tables_give_the_recorded_labels(case):
    from spacap3d_amd.scene_export import segment_tables
    seg_ins, seg_sem, box_label = segment_tables(case["groups"], case["label_map"], case["seg_indices"])
    assert seg_ins.dtype == seg_sem.dtype == box_label.dtype == np.int32
    assert np.array_equal(seg_ins[case["seg_indices"]], case["ins_label"])
    assert np.array_equal(seg_sem[case["seg_indices"]], case["sem_label"])
    rows = case["bbox"][:, 3:6].any(1)                       # an object without a vertex keeps label 0 in its zero row
    assert box_label.shape[0] == case["bbox"].shape[0]
    assert np.array_equal(box_label[rows], case["bbox"][rows, 6]) and np.array_equal(np.nonzero(rows)[0], case["bbox"][rows, 7])


def test_save_writes_the_reference_file_names_and_dtypes(tmp_path, fixture):
    from spacap3d_amd.scene_export import save
    c = R.load_case("a", fixture)
    result = {k: (c[k].astype(np.int32) if c[k].dtype == np.uint32 else c[k]) for k in R.OUTPUTS}   # labels as the device holds them
    save(result, str(tmp_path / "scene0000_00"))
    assert sorted(os.listdir(tmp_path)) == sorted(f"scene0000_00_{k}.npy" for k in R.OUTPUTS)
    for k in R.OUTPUTS:
        assert same_bits(np.load(tmp_path / f"scene0000_00_{k}.npy"), c[k]), k


def test_header_signatures_and_symbols_agree():
    from spacap3d_amd import _native
    header = open(os.path.join(ROOT, "include", "spacap_hip.h")).read()
    for name in SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, name
        assert name in _native.SIGNATURES and hasattr(_native.lib, name)
        assert len(m.group(1).split(",")) == len(_native.SIGNATURES[name][1]), name
    assert _native.lib.spacap_abi_version() == 5


def test_argument_validation_needs_no_device():
    from spacap3d_amd._native import lib
    one = ctypes.c_void_p(16)       # never dereferenced: every check comes before the first device call
    big = 1 << 30
    assert lib.spacap_scene_export_workspace_bytes(1000, 0) >= 3 * 1000 * 4
    assert lib.spacap_scene_export_workspace_bytes(1000, 60) >= 3 * 1000 * 4 + 60 * 12 * 4
    assert lib.spacap_scene_export_workspace_bytes(0, 0) == 0
    export_ok = dict(xyz=one, rgb=one, N=100, faces=one, F=10, seg=one, seg_ins=one, seg_sem=one, S=5, box_label=one, M=3,
                     align=None, ws=one, nb=big, vert=one, aligned=one, ins=one, sem=one, bbox=one, abox=one, rel=one)

    def export(**kw):
        return lib.spacap_scene_export_f32(*{**export_ok, **kw}.values(), None)

    # bad sizes
    assert lib.spacap_scene_normals_f32(one, -1, one, 4, one, big, one, None) == -1
    assert b"bad sizes" in lib.spacap_last_error()
    assert lib.spacap_scene_normals_f32(one, 1 << 24, one, 4, one, big, one, None) == -1
    assert b"bad sizes" in lib.spacap_last_error()
    assert lib.spacap_scene_normals_f32(one, 10, one, -4, one, big, one, None) == -1
    assert b"bad sizes" in lib.spacap_last_error()
    assert lib.spacap_scene_relations_f64(one, 1025, one, None) == -1
    assert b"M=1025" in lib.spacap_last_error()
    assert lib.spacap_scene_relations_f64(one, -1, one, None) == -1
    assert export(M=1025) == -1 and b"M=1025" in lib.spacap_last_error()
    assert export(M=0) == -1 and b"bad sizes" in lib.spacap_last_error()
    assert export(S=0) == -1 and b"bad sizes" in lib.spacap_last_error()
    assert export(N=1 << 24) == -1 and b"bad sizes" in lib.spacap_last_error()
    # null pointers
    assert lib.spacap_scene_normals_f32(None, 10, one, 4, one, big, one, None) == -1
    assert b"null" in lib.spacap_last_error()
    assert lib.spacap_scene_normals_f32(one, 10, None, 4, one, big, one, None) == -1
    assert lib.spacap_scene_normals_f32(one, 10, one, 4, one, big, None, None) == -1
    assert lib.spacap_scene_relations_f64(None, 4, one, None) == -1 and b"null" in lib.spacap_last_error()
    assert lib.spacap_scene_relations_f64(one, 4, None, None) == -1
    for k in ("xyz", "rgb", "faces", "seg", "seg_ins", "seg_sem", "box_label", "ws", "vert", "aligned", "ins", "sem", "bbox",
              "abox", "rel"):
        assert export(**{k: None}) == -1 and b"null" in lib.spacap_last_error(), k
    # a workspace that is too small
    assert lib.spacap_scene_normals_f32(one, 10, one, 4, one, 3 * 10 * 4 - 1, one, None) == -1
    assert b"workspace" in lib.spacap_last_error()
    assert export(nb=3 * 100 * 4) == -1 and b"workspace" in lib.spacap_last_error()
    # nothing to do
    assert lib.spacap_scene_normals_f32(None, 0, None, 0, None, 0, None, None) == 0
    assert lib.spacap_scene_relations_f64(None, 0, None, None) == 0
    assert export(N=0, xyz=None, vert=None) == 0


def test_index_validation_comes_before_any_launch(fixture):
    from spacap3d_amd import scene_export as E
    c = R.load_case("a", fixture)
    N = c["xyz"].shape[0]
    tables = E.segment_tables(c["groups"], c["label_map"], c["seg_indices"])
    for bad in (N, -1):
        faces = c["faces"].copy()
        faces[17, 1] = bad
        with pytest.raises(ValueError, match="faces"):
            E.vertex_normals(c["xyz"], faces)
        with pytest.raises(ValueError, match="faces"):
            E.export_scene(c["xyz"], c["rgb"], faces, c["seg_indices"], tables, c["axis_align"])
    with pytest.raises(ValueError, match="faces must have an integer dtype"):     # refused, not truncated
        E.vertex_normals(c["xyz"], c["faces"].astype(np.float32))
    with pytest.raises(ValueError, match="seg_ins must have an integer dtype"):
        E.export_scene(c["xyz"], c["rgb"], c["faces"], c["seg_indices"], (tables[0].astype(np.float64), tables[1], tables[2]))
    seg = c["seg_indices"].copy()
    seg[5] = tables[0].shape[0]
    with pytest.raises(ValueError, match="seg_indices"):
        E.export_scene(c["xyz"], c["rgb"], c["faces"], seg, tables, c["axis_align"])
    with pytest.raises(ValueError, match="seg_ins"):
        E.export_scene(c["xyz"], c["rgb"], c["faces"], c["seg_indices"], (tables[0] + 26, tables[1], tables[2]))
    groups = [dict(g) for g in c["groups"]]
    groups[4]["objectId"] = groups[9]["objectId"]
    with pytest.raises(ValueError, match="unique"):
        E.segment_tables(groups, c["label_map"], c["seg_indices"])
    groups = [dict(g) for g in c["groups"]]
    groups[2]["objectId"] = len(groups)
    with pytest.raises(ValueError, match="unique"):
        E.segment_tables(groups, c["label_map"], c["seg_indices"])
    groups = [dict(g) for g in c["groups"]]
    groups[7]["segments"] = []
    with pytest.raises(ValueError, match="empty segment list"):
        E.segment_tables(groups, c["label_map"], c["seg_indices"])
    with pytest.raises(ValueError, match="supported"):
        E.spatial_relations(np.zeros((1025, 8)))
    with pytest.raises(ValueError, match="supported"):
        E.segment_tables([{"objectId": k, "label": "chair", "segments": [0]} for k in range(1025)], c["label_map"], c["seg_indices"])


def test_cpu_tensors_are_refused(fixture):
    from spacap3d_amd import scene_export as E
    c = R.load_case("c", fixture)
    tables = E.segment_tables(None, c["label_map"], c["seg_indices"])
    xyz, rgb, faces, seg = (torch.as_tensor(np.ascontiguousarray(c[k])) for k in ("xyz", "rgb", "faces", "seg_indices"))
    for call in (lambda: E.vertex_normals(xyz, faces),
                 lambda: E.vertex_normals(c["xyz"], faces),
                 lambda: E.export_scene(xyz, rgb, faces, seg, tables),
                 lambda: E.export_scene(c["xyz"], c["rgb"], c["faces"], seg, tables),
                 lambda: E.spatial_relations(torch.zeros(4, 8, dtype=torch.float64)),
                 lambda: E.vertex_normals(c["xyz"], c["faces"], device="cpu")):
        with pytest.raises(RuntimeError, match="CPU not supported"):
            call()
