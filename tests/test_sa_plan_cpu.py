"""Which launches a set-abstraction module's shared MLP makes for a shape (spacap3d_amd/sa_mlp.py: plan): pure host logic over
the module's switches and the library's ``*_supported`` predicates, so it needs the built library but no GPU."""
import pytest

SA1 = (64, 64, 128, 64, 8 * 2048 * 64)          # (C1, C2, C3, S, R) at cfg2: 8 scenes, 2 048 groups of 64
DEFAULT = ("moments", "candidates", "z2", "one_pass")

# (C1, C2, C3, S, R, has_pm, need_xyz), switches -> (first, tail, l3_wgrad, l2_l1)
PINS = [
    ((*SA1, False, False), {}, DEFAULT),
    ((*SA1, False, False), {"L1_MOMENTS": False}, ("stats", "candidates", "z2", "one_pass")),
    ((*SA1, False, False), {"FUSE_L2_WGRAD": False}, ("moments", "candidates", "z2", "l1in")),
    ((*SA1, False, False), {"RECOMPUTE_Z1": False}, ("stored", "candidates", "z2", "l1_sums")),
    ((*SA1, False, False), {"RECOMPUTE_Z1": False, "L1_MOMENTS": False, "FUSE_L2_WGRAD": False}, ("stored", "candidates", "z2", "l1_sums")),
    ((*SA1, True, False), {}, ("stored", "candidates", "z2", "generic")),       # 7 / 132 feature channels (cfg3 / cfg4): point-major
    ((*SA1, False, True), {}, ("stored", "candidates", "z2", "generic")),       # SA1-shaped, but a coordinate gradient is wanted
    ((128, 128, 256, 32, 8 * 1024 * 32, True, False), {}, ("stored", "candidates", "z2", "generic")),     # SA2
    ((128, 128, 256, 16, 8 * 512 * 16, True, False), {}, ("stored", "candidates", "dense", "generic")),   # SA3: S = 16 has no z2 kernel
    ((128, 128, 256, 16, 8 * 256 * 16, True, False), {}, ("stored", "candidates", "dense", "generic")),   # SA4
    ((128, 128, 128, 16, 8 * 256 * 16, True, True), {}, ("stored", "candidates", "dense", "generic")),    # vote aggregation
    ((64, 64, 128, 64, 131072, False, False), {}, DEFAULT),                                               # the row threshold of "z2"
    ((64, 64, 128, 64, 131071, False, False), {}, ("moments", "candidates", "dense", "one_pass")),
    ((64, 64, 128, 64, 131072, False, False), {"POOL_WGRAD": False}, ("moments", "candidates", "dense", "one_pass")),
    ((64, 64, 128, 64, 64, False, False), {"POOL_WGRAD_MIN_ROWS": 0}, DEFAULT),                           # (as the float64 gates set it)
    ((64, 64, 128, 48, 8 * 2048 * 48, False, False), {}, ("moments", "plain", "dense", "one_pass")),      # S without a candidate kernel
    ((64, 64, 128, 8, 8 * 2048 * 8, False, False), {}, ("moments", "plain", "dense", "one_pass")),
    ((128, 128, 256, 48, 8 * 1024 * 48, True, False), {}, ("stored", "plain", "dense", "generic")),
]


@pytest.mark.parametrize("shape,switches,want", PINS)
def test_plan_names_the_launches_of_a_shape(shape, switches, want, monkeypatch):
    from spacap3d_amd import sa_mlp
    for name, value in switches.items():
        assert hasattr(sa_mlp, name)
        monkeypatch.setattr(sa_mlp, name, value)
    got = sa_mlp.plan(*shape)
    assert isinstance(got, sa_mlp.Plan) and tuple(got) == want
    assert got._fields == ("first", "tail", "l3_wgrad", "l2_l1")


def test_every_value_of_every_field_is_pinned():
    seen = [{want[k] for _, _, want in PINS} for k in range(4)]
    assert seen == [{"moments", "stats", "stored"}, {"candidates", "plain"}, {"z2", "dense"},
                    {"one_pass", "l1in", "l1_sums", "generic"}]


def test_the_switches_are_read_in_plan_only():
    """Each of the five switches is assigned once at module level and read in exactly one function, ``plan``: a node's backward
    follows the record its forward made and re-derives nothing."""
    import ast
    import inspect
    from spacap3d_amd import sa_mlp
    switches = {"RECOMPUTE_Z1", "L1_MOMENTS", "POOL_WGRAD", "POOL_WGRAD_MIN_ROWS", "FUSE_L2_WGRAD"}
    tree = ast.parse(inspect.getsource(sa_mlp))
    readers = {}
    for fn in ast.walk(tree):
        if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
            for node in ast.walk(fn):
                if isinstance(node, ast.Name) and node.id in switches:
                    readers.setdefault(node.id, set()).add(fn.name)
    assert readers == {name: {"plan"} for name in switches}
