"""GPU leg of the scene export (spacap3d_amd/scene_export.py, csrc/scene_export.hip): the kernels
against the arrays the reference's own functions recorded (tests/golden/scene_export_ref.npz), bit for bit -- float values
are compared through their integer views, so -0.0 and 0.0 differ -- and ``DeviceSceneDataset.add_scene`` fed with the
device tensors against the same dataset fed with the recorded host arrays."""
import numpy as np
import pytest
import torch

import scene_export_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_VIEW = {np.dtype(np.float32): np.int32, np.dtype(np.float64): np.int64}


def assert_bits(name, got, want):
    """``got`` (device tensor) holds the recorded array ``want``: same shape and bits; int32 on the device is uint32 on disk."""
    got = got.cpu().numpy()
    if want.dtype == np.uint32:
        assert got.dtype == np.int32, (name, got.dtype)
        got = got.astype(np.uint32)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, got.dtype, want.shape, want.dtype)
    view = _VIEW.get(want.dtype, want.dtype)
    bad = np.ascontiguousarray(got).view(view) != np.ascontiguousarray(want).view(view)
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist())


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


@pytest.fixture(scope="module", params=R.CASES)
def case(request, fixture):
    return R.load_case(request.param, fixture)


def _export(c, on_device=False):
    from spacap3d_amd import scene_export as E
    tables = E.segment_tables(c["groups"], c["label_map"], c["seg_indices"])
    args = [c["xyz"], c["rgb"], c["faces"], c["seg_indices"]]
    if on_device:      # the index checks then run as reductions on the device
        args = [torch.as_tensor(np.ascontiguousarray(a)).to(DEV) for a in args]
        tables = tuple(torch.as_tensor(t).to(DEV) for t in tables)
    return E.export_scene(*args, tables, axis_align=c["axis_align"], device=DEV)


def test_export_scene_equals_the_reference(case):
    for on_device in (False, True):
        out = _export(case, on_device)
        assert sorted(out) == sorted(R.OUTPUTS)
        for k in R.OUTPUTS:
            assert_bits(k, out[k], case[k])


def _sorted_by_instance(c):
    """Case ``c`` with its vertices grouped by the recorded instance id and the faces renamed: the order a real mesh has,
    whole waves of one instance.  Every instance's vertices come in file order, as many whole 64-vertex waves of them as it
    has first (so those waves start on a wave boundary), then what is left of every instance, unannotated vertices first.
    The per-vertex results are the recorded ones in the new order, the boxes and relations the recorded ones as they are
    (min and max do not depend on order)."""
    whole, left = [], []
    for m in np.unique(c["ins_label"]):
        mine = np.nonzero(c["ins_label"] == m)[0]
        k = mine.size // 64 * 64 if m > 0 else 0
        whole.append(mine[:k])
        left.append(mine[k:])
    order = np.concatenate(whole + left)
    new_index = np.empty_like(order)
    new_index[order] = np.arange(order.size)
    s = dict(c)
    for k in ("xyz", "rgb", "seg_indices", "vert", "aligned_vert", "sem_label", "ins_label"):
        s[k] = np.ascontiguousarray(c[k][order])
    s["faces"] = new_index[c["faces"]].astype(np.int32)
    return s


def _slots_decided_by_a_wave_reduction(c):
    """Of the 12 extrema a box is made of (raw / aligned, min / max, x / y / z): those for which some instance's extremum is
    held by exactly one vertex, and that vertex sits in a full 64-vertex wave of that one instance, in another lane than 0 --
    the lane that issues the atomics.  Such a box entry reaches the table only through the cross-lane reduction."""
    ins = c["ins_label"].astype(np.int64)
    full = ins[:ins.size // 64 * 64].reshape(-1, 64)
    uniform = np.nonzero((full == full[:, :1]).all(1) & (full[:, 0] > 0))[0]
    slots = set()
    for w, pts in enumerate((c["vert"][:, 0:3], c["aligned_vert"][:, 0:3])):
        for m in np.unique(ins[ins > 0]):
            mine = np.nonzero(ins == m)[0]
            for d in range(3):
                for hi in (0, 1):
                    best = pts[mine, d].max() if hi else pts[mine, d].min()
                    holders = mine[pts[mine, d] == best]
                    if holders.size == 1 and holders[0] // 64 in uniform and holders[0] % 64 != 0:
                        slots.add((w, hi, d))
    return uniform.size, slots


def test_vertices_in_instance_order_take_the_wave_reduction(fixture):
    """Waves whose vertices all belong to one instance reduce their extrema across lanes before the atomics: the path almost
    every wave of a real mesh takes, and none of the recorded cases as they are."""
    a = _sorted_by_instance(R.load_case("a", fixture))
    n_uniform, slots = _slots_decided_by_a_wave_reduction(a)
    assert n_uniform >= 20 and len(slots) == 12, (n_uniform, sorted(slots))
    for c in (a, _sorted_by_instance(R.load_case("b", fixture))):
        for on_device in (False, True):
            out = _export(c, on_device)
            for k in R.OUTPUTS:
                assert_bits(k, out[k], c[k])


def test_long_instance_runs_equal_the_restatement():
    """500 consecutive vertices per instance, so most waves are uniform (and every box takes its extrema from them), held to
    the numpy restatement, which tests/test_scene_export_cpu.py holds to the reference's recordings."""
    rng = np.random.default_rng(11)
    N, F, M = 4000 + 37, 6000, 8
    c = {"xyz": rng.uniform(-3, 5, (N, 3)).astype(np.float32), "rgb": rng.integers(0, 256, (N, 3)).astype(np.uint8),
         "faces": rng.integers(0, N, (F, 3)).astype(np.int32), "seg_indices": (np.arange(N) // 250).astype(np.int32),
         "groups": [{"objectId": (3 * k + 1) % M, "label": ("chair", "table", "wall")[k % 3], "segments": [2 * k, 2 * k + 1]}
                    for k in range(M)],
         "label_map": {"chair": 5, "table": 7, "wall": 1},
         "axis_align": np.array([[np.cos(0.7), -np.sin(0.7), 0, 0.5], [np.sin(0.7), np.cos(0.7), 0, -1.25], [0, 0, 1, 0.1],
                                 [0, 0, 0, 1]])}
    assert not R.band(c["xyz"], c["axis_align"]).any()
    want = R.export(c)
    n_uniform, slots = _slots_decided_by_a_wave_reduction({**c, **want})
    assert n_uniform >= 6 * M and len(slots) == 12, (n_uniform, sorted(slots))
    out = _export(c, on_device=True)
    for k in R.OUTPUTS:
        assert_bits(k, out[k], want[k])


def test_tensor_arguments_are_taken_strictly(fixture):
    from spacap3d_amd import scene_export as E
    c = R.load_case("a", fixture)
    tables = E.segment_tables(c["groups"], c["label_map"], c["seg_indices"])
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    out = E.export_scene(up(c["xyz"]), up(c["rgb"]), up(c["faces"]), up(c["seg_indices"]), tables,
                         axis_align=up(c["axis_align"]))                    # the matrix as a device tensor
    for k in R.OUTPUTS:
        assert_bits(k, out[k], c[k])
    with pytest.raises(ValueError, match="faces must have an integer dtype"):
        E.vertex_normals(up(c["xyz"]), up(c["faces"]).float())
    with pytest.raises(ValueError, match="seg_indices must have an integer dtype"):
        E.export_scene(up(c["xyz"]), up(c["rgb"]), up(c["faces"]), up(c["seg_indices"]).double(), tables)


def test_vertex_normals_alone(case):
    from spacap3d_amd.scene_export import vertex_normals
    assert_bits("normals", vertex_normals(case["xyz"], case["faces"], device=DEV), case["vert"][:, 6:9])
    no_faces = vertex_normals(case["xyz"], np.zeros((0, 3), np.int32), device=DEV)
    assert_bits("no faces", no_faces, np.zeros_like(case["xyz"]))


@pytest.mark.parametrize("name", R.RELATION_CASES + R.CASES)
def test_spatial_relations_alone(fixture, name):
    from spacap3d_amd.scene_export import spatial_relations
    if name in R.CASES:
        bbox, want = fixture[f"{name}/aligned_bbox"], np.stack([fixture[f"{name}/{a}"] for a in "xyz"])
    else:
        bbox, want = fixture[f"{name}/bbox"], fixture[f"{name}/rel"]
    assert_bits(name, spatial_relations(bbox, device=DEV), want)
    assert_bits(name, spatial_relations(torch.as_tensor(bbox).to(DEV)), want)


def test_a_second_call_into_the_same_buffers_gives_the_same_bytes(fixture):
    """The workspace arrives full of junk and is not touched between the calls: the kernels initialise it themselves."""
    from spacap3d_amd import scene_export as E
    from spacap3d_amd._native import check, lib
    c = R.load_case("a", fixture)
    tables = E.segment_tables(c["groups"], c["label_map"], c["seg_indices"])
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(DEV)   # noqa: E731
    xyz, rgb, faces, seg = up(c["xyz"], np.float32), up(c["rgb"], np.float32), up(c["faces"], np.int32), up(c["seg_indices"], np.int32)
    seg_ins, seg_sem, box_label = (up(t, np.int32) for t in tables)
    N, F, S, M = xyz.shape[0], faces.shape[0], seg_ins.shape[0], box_label.shape[0]
    align = np.ascontiguousarray(c["axis_align"], dtype=np.float64)
    nb = int(lib.spacap_scene_export_workspace_bytes(N, M))
    ws = torch.full((nb,), 0x5A, dtype=torch.uint8, device=DEV)
    f32, i32, f64 = (dict(dtype=d, device=DEV) for d in (torch.float32, torch.int32, torch.float64))
    outs = {"vert": torch.zeros(N, 9, **f32), "aligned_vert": torch.zeros(N, 9, **f32), "ins_label": torch.zeros(N, **i32),
            "sem_label": torch.zeros(N, **i32), "bbox": torch.zeros(M, 8, **f64), "aligned_bbox": torch.zeros(M, 8, **f64),
            "rel": torch.zeros(3, M, M, **i32)}
    normals = torch.zeros(N, 3, **f32)
    snapshots = []
    for _ in range(2):
        check(lib.spacap_scene_export_f32(
            xyz.data_ptr(), rgb.data_ptr(), N, faces.data_ptr(), F, seg.data_ptr(), seg_ins.data_ptr(), seg_sem.data_ptr(), S,
            box_label.data_ptr(), M, align.ctypes.data, ws.data_ptr(), nb, outs["vert"].data_ptr(),
            outs["aligned_vert"].data_ptr(), outs["ins_label"].data_ptr(), outs["sem_label"].data_ptr(), outs["bbox"].data_ptr(),
            outs["aligned_bbox"].data_ptr(), outs["rel"].data_ptr(), torch.cuda.current_stream().cuda_stream),
            "spacap_scene_export_f32")
        check(lib.spacap_scene_normals_f32(xyz.data_ptr(), N, faces.data_ptr(), F, ws.data_ptr(), nb, normals.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), "spacap_scene_normals_f32")
        snapshots.append({k: v.clone() for k, v in outs.items()})
        snapshots[-1]["normals"] = normals.clone()
    for k in snapshots[0]:
        assert torch.equal(snapshots[0][k].view(torch.uint8), snapshots[1][k].view(torch.uint8)), k
    for k in ("vert", "aligned_vert", "ins_label", "sem_label", "bbox", "aligned_bbox"):
        assert_bits(k, snapshots[1][k], c[k])
    assert_bits("rel", snapshots[1]["rel"], np.stack([c[a] for a in "xyz"]))
    assert_bits("normals", snapshots[1]["normals"], c["vert"][:, 6:9])


@pytest.mark.parametrize("color_renorm", ["once", "per_access"])
def test_dataset_takes_the_device_tensors_as_it_takes_the_host_arrays(fixture, color_renorm):
    from spacap3d_amd.dataset import DeviceSceneDataset
    from tests.test_scene_pipeline import load_fixture
    fx, _ = load_fixture()
    c = R.load_case("a", fixture)
    out = _export(c)

    def dataset(arrays):
        ds = DeviceSceneDataset(DEV, fx["mean_size_arr"], dict(zip(fx["nyu40id2class_keys"].tolist(), fx["nyu40id2class_vals"].tolist())),
                                dict(zip(fx["raw2label_names"].tolist(), fx["raw2label_vals"].tolist())), num_points=1024,
                                max_instances=64, use_height=True, use_normal=True, use_color=True, use_relation=True,
                                color_renorm=color_renorm)
        ds.add_scene("scene", *(arrays[k] for k in ("aligned_vert", "ins_label", "sem_label", "aligned_bbox", "x", "y", "z")))
        for obj in (3, 11):
            ds.add_item("scene", obj, "chair")
        return ds

    host, device = dataset(c), dataset(out)
    hs, dv = host._scenes[0], device._scenes[0]
    assert sorted(hs) == sorted(dv) and ("color0" in hs) == (color_renorm == "per_access")
    for k in hs:
        if isinstance(hs[k], torch.Tensor):
            assert hs[k].dtype == dv[k].dtype and hs[k].shape == dv[k].shape and dv[k].is_contiguous(), k
            assert torch.equal(hs[k].view(torch.uint8), dv[k].view(torch.uint8)), k
        elif isinstance(hs[k], np.ndarray):
            assert hs[k].dtype == dv[k].dtype and hs[k].tobytes() == dv[k].tobytes(), k
        else:
            assert hs[k] == dv[k], k
    draws = host.draw([0, 1], torch.Generator(device=DEV).manual_seed(5))
    want, got = host.batch([0, 1], draws=draws), device.batch([0, 1], draws=draws)
    assert sorted(want) == sorted(got)
    for k in want:
        assert want[k].dtype == got[k].dtype and want[k].shape == got[k].shape, k
        assert torch.equal(want[k].contiguous().view(torch.uint8), got[k].contiguous().view(torch.uint8)), k
    with pytest.raises(ValueError, match="max_instances"):
        DeviceSceneDataset(DEV, fx["mean_size_arr"], {}, max_instances=8).add_scene(
            "scene", out["aligned_vert"], out["ins_label"], out["sem_label"], out["aligned_bbox"])
