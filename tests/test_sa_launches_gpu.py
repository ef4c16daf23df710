"""Which C entry points one forward and one backward of a set-abstraction module launch, per plan (spacap3d_amd/sa_mlp.py:
plan): a recording proxy on ``sa_mlp.lib`` -- the substitution bench.py's InStepTimer makes -- against a table recorded from the
host path as it was before ``plan`` existed.  A condition that moves a module onto another kernel fails here even while every
float64 gate (tests/test_sa_mlp_gpu.py, which remains the numeric check) stays green.  Names are given without the ``spacap_sa_``
prefix and the ``_f32`` suffix; host queries (``*_supported``, ``*_slabs``, ...) are not launches and not recorded."""
import pytest
import torch

from spacap3d_amd import backend
from spacap3d_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SA1, SA2, VOTE = [64, 64, 128], [128, 128, 256], [128, 128, 128]
REBUILT = ["l1_moments", "l1_moments_finalize", "mid_fwd_l1in", "bn_finalize"]
STORED = ["l1_fwd", "bn_finalize", "mid_fwd", "bn_finalize"]
CANDIDATES = ["mid_fwd_pool", "bn_finalize", "pool_finalize"]
PLAIN = ["mid_fwd", "bn_finalize", "pool_fwd"]
L3_DENSE = ["pool_bwd", "bwd_finalize", "wgrad", "dgrad", "bwd_finalize"]
L3_Z2 = ["pool_bwd", "bwd_finalize", "wgrad_pool", "l3bwd_dw", "dgrad", "bwd_finalize"]
ONE_PASS = ["dgrad_wgrad_l1in", "bwd_finalize", "l1_dw"]
GENERIC = ["wgrad", "dgrad", "bwd_finalize", "l1_bwd"]
TALL = ["spacap_dense_wgrad_tall", "dw1_assemble"]       # feature columns of dW1: 7 channels
SLABS = ["spacap_linear_wgrad", "dw1_assemble"]          # ... a multiple of 128 channels

# name, (Np, N, S, Cf, mlp widths, feature gradient, coordinate gradient, prebuilt rows index), switches,
#   plan, forward launches, backward launches.  B = 2; N = 33: R = 66 S is no multiple of a 256-row tile
CASES = [
    ("sa1", (300, 33, 64, 1, SA1, False, False, False), {},
     ("moments", "candidates", "dense", "one_pass"), REBUILT + CANDIDATES, L3_DENSE + ONE_PASS),
    ("sa1_z2", (300, 33, 64, 1, SA1, False, False, False), {"POOL_WGRAD_MIN_ROWS": 0},
     ("moments", "candidates", "z2", "one_pass"), REBUILT + CANDIDATES, L3_Z2 + ONE_PASS),
    ("sa1_no_feature", (300, 33, 64, 0, SA1, False, False, False), {},
     ("moments", "candidates", "dense", "one_pass"), REBUILT + CANDIDATES, L3_DENSE + ONE_PASS),
    ("sa1_summed_stats", (300, 33, 64, 1, SA1, False, False, False), {"L1_MOMENTS": False},
     ("stats", "candidates", "dense", "one_pass"), ["l1_stats", "bn_finalize", "mid_fwd_l1in", "bn_finalize"] + CANDIDATES,
     L3_DENSE + ONE_PASS),
    ("sa1_two_kernels", (300, 33, 64, 1, SA1, False, False, False), {"FUSE_L2_WGRAD": False},
     ("moments", "candidates", "dense", "l1in"), REBUILT + CANDIDATES, L3_DENSE + ["wgrad_l1in", "dgrad_l1in", "bwd_finalize", "l1_dw"]),
    ("sa1_stored", (300, 33, 64, 1, SA1, False, False, False), {"RECOMPUTE_Z1": False},
     ("stored", "candidates", "dense", "l1_sums"), STORED + CANDIDATES, L3_DENSE + ["wgrad", "dgrad_l1", "bwd_finalize", "l1_dw"]),
    ("sa1_7_channels", (300, 33, 64, 7, SA1, False, False, False), {},
     ("stored", "candidates", "dense", "generic"), STORED + CANDIDATES, L3_DENSE + GENERIC + ["rows_scatter"] + TALL),
    ("sa1_coordinate_gradient", (300, 33, 64, 1, SA1, False, True, False), {},
     ("stored", "candidates", "dense", "generic"), STORED + CANDIDATES, L3_DENSE + GENERIC + ["rows_index", "drel_sums"]),
    ("sa2", (300, 33, 32, 128, SA2, True, False, False), {"POOL_WGRAD_MIN_ROWS": 0},
     ("stored", "candidates", "z2", "generic"), STORED + CANDIDATES, L3_Z2 + GENERIC + ["rows_scatter"] + SLABS),
    ("sa2_rows_index", (300, 33, 32, 128, SA2, True, False, True), {},
     ("stored", "candidates", "dense", "generic"), STORED + CANDIDATES, L3_DENSE + GENERIC + ["rows_gather"] + SLABS),
    ("sa3", (300, 33, 16, 256, SA2, True, False, False), {"POOL_WGRAD_MIN_ROWS": 0},
     ("stored", "candidates", "dense", "generic"), STORED + CANDIDATES, L3_DENSE + GENERIC + ["rows_scatter"] + SLABS),
    ("vote_aggregation", (300, 33, 16, 128, VOTE, True, True, False), {},
     ("stored", "candidates", "dense", "generic"), STORED + CANDIDATES, L3_DENSE + GENERIC + ["rows_scatter"] + SLABS + ["drel_sums"]),
    ("sa1_48_samples", (300, 33, 48, 1, SA1, False, False, False), {"POOL_WGRAD_MIN_ROWS": 0},
     ("moments", "plain", "dense", "one_pass"), REBUILT + PLAIN, L3_DENSE + ONE_PASS),
    ("sa2_48_samples", (300, 33, 48, 128, SA2, True, False, False), {},
     ("stored", "plain", "dense", "generic"), STORED + PLAIN, L3_DENSE + GENERIC + ["rows_scatter"] + SLABS),
    # the row threshold of the pooled layer's weight gradient from z2, at its real size: R = 131 072 and 130 944 (z3: 64 MB)
    ("threshold_at", (4096, 1024, 64, 1, SA1, False, False, False), {},
     ("moments", "candidates", "z2", "one_pass"), REBUILT + CANDIDATES, L3_Z2 + ONE_PASS),
    ("threshold_below", (4096, 1023, 64, 1, SA1, False, False, False), {},
     ("moments", "candidates", "dense", "one_pass"), REBUILT + CANDIDATES, L3_DENSE + ONE_PASS),
]
EVAL_LAUNCHES = ["l1_fwd", "mid_fwd", "mid_fwd", "pool_fwd"]


class _Recorder:
    """Stands in for ``sa_mlp.lib``: every ``*_f32`` entry point called through it is noted by name, then runs."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.endswith("_f32"):
            return f

        def call(*a):
            self.names.append(name[:-4].replace("spacap_sa_", ""))
            return f(*a)
        return call

    def take(self):
        names, self.names = self.names, []
        return names


def _module(shape):
    from spacap3d_amd.pointnet2_modules import PointnetSAModuleVotes
    Np, N, Sn, Cf, widths, feat_grad, xyz_grad, rows = shape
    torch.manual_seed(Np + N + Sn + Cf)
    sa = PointnetSAModuleVotes(npoint=N, radius=0.4, nsample=Sn, mlp=[Cf] + widths, use_xyz=True, normalize_xyz=True).to(DEV)
    xyz = S.scene_batch(2, Np, use_height=False, seed=11).to(DEV).requires_grad_(xyz_grad)
    feats = torch.randn(2, Cf, Np, device=DEV).relu_().requires_grad_(feat_grad) if Cf else None
    return sa, xyz, feats


def record(shape, switches=None):
    """(plan or None, forward launches, backward launches) of one training forward + backward of a module of this shape, after
    the checks that the output and every parameter gradient are finite and non-zero.  Uses nothing but the proxied attribute
    ``sa_mlp.lib``, so that the table above can be recorded from any revision of the host path."""
    from spacap3d_amd import pointnet2_utils as PU, sa_mlp
    sa_mlp._selftest(torch.device(DEV))      # (its own launches: once per process, before anything is recorded)
    sa, xyz, feats = _module(shape)
    sa.train()
    rows_idx = None
    if shape[7]:
        with torch.no_grad():
            inds = PU.furthest_point_sample(xyz, shape[1])
            new_xyz = torch.gather(xyz, 1, inds.long().unsqueeze(-1).expand(-1, -1, 3))
            idx = PU.ball_query(0.4, shape[2], xyz, new_xyz)
            rows_idx = sa_mlp.rows_index(idx, shape[0])
    keep = {k: getattr(sa_mlp, k) for k in (switches or {})}
    rec, lib = _Recorder(sa_mlp.lib), sa_mlp.lib
    try:
        for k, v in (switches or {}).items():
            setattr(sa_mlp, k, v)
        sa_mlp.lib = rec
        if rows_idx is not None:
            _, out, _ = sa(xyz, feats, inds=inds, idx=idx, rows_idx=rows_idx)
        else:
            _, out, _ = sa(xyz, feats)
        fwd = rec.take()
        node = out.grad_fn
        while node is not None and "_SAMLP" not in type(node).__name__:
            node = node.next_functions[0][0]
        torch.manual_seed(1)
        (out * torch.randn_like(out)).sum().backward()
        bwd = rec.take()
    finally:
        sa_mlp.lib = lib
        for k, v in keep.items():
            setattr(sa_mlp, k, v)
    tensors = [("out", out.detach())] + [(n + ".grad", p.grad) for n, p in sa.named_parameters()]
    for what, t in tensors:
        assert t is not None and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0, what
    return getattr(node, "plan", None), fwd, bwd


@pytest.mark.parametrize("name,shape,switches,plan,fwd,bwd", CASES, ids=[c[0] for c in CASES])
def test_launches_of_one_forward_and_backward(name, shape, switches, plan, fwd, bwd):
    got_plan, got_fwd, got_bwd = record(shape, switches)
    assert tuple(got_plan) == plan
    assert got_fwd == fwd
    assert got_bwd == bwd


def test_launches_of_the_inference_forward():
    from spacap3d_amd import sa_mlp
    for shape in ((300, 33, 64, 1, SA1, False, False, False), (300, 33, 32, 128, SA2, False, False, False)):
        sa, xyz, feats = _module(shape)
        sa.eval()
        rec, lib = _Recorder(sa_mlp.lib), sa_mlp.lib
        try:
            sa_mlp.lib = rec
            with torch.no_grad():
                _, out, _ = sa(xyz, feats)
        finally:
            sa_mlp.lib = lib
        assert rec.take() == EVAL_LAUNCHES
        assert out.shape == (2, shape[4][-1], 33) and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
    assert backend.ops().sa_mlp_eval is sa_mlp.sa_mlp_eval
