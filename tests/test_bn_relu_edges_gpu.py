"""The kernels of csrc/bn_relu.hip and csrc/group_max.hip at every edge of their dispatch, against the float64 restatement of
tests/bn_relu_restated.py: ``fused_bn.bn_relu_train`` and ``bn_relu_eval``, ``ext.group_max`` and ``group_max_grad`` called on the
inputs of its tables, and the C ABI itself where the Python layer cannot reach (the pooled backward at an S no forward serves,
the refusals).

Arg-max and exact zeros are compared with ``torch.equal``; values and gradients are held to the bars recorded in
bn_relu_restated.py -- 16 times what float32 done right uses, capped at tests/test_ops_gpu.py's own -- and the inputs are
conditioned so that no element sits where float32 rounding could turn a comparison (tests/test_bn_relu_restated_cpu.py asserts
it for every case).  Every case that qualifies for the single launch runs under both settings of
``spacap_bn_set_single_launch``, each held to float64.  A NaN or a +Inf in one channel must come out as the composition the
kernels replace returns it: NaN outputs, statistics and running buffers for that channel, the bars for every other channel.
Each comparison prints its figures before it asserts (``BN-EDGES gpu ...``, pytest -s)."""
import numpy as np
import pytest
import torch

import bn_relu_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_name = lambda c: c.name
_NAN = float("nan")


@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spacap3d_amd import _native
    return _native


def _dev(a):
    return torch.tensor(np.asarray(a)).to(DEV)


def _cpu(t):
    return t.detach().cpu().numpy()


def _module(case, x):
    C = case.shape[1]
    bn = (torch.nn.BatchNorm2d if len(case.shape) == 4 else torch.nn.BatchNorm1d)(
        C, eps=R.EPS, momentum=case.momentum, track_running_stats=case.track).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(_dev(x.gamma)), bn.bias.copy_(_dev(x.beta))
        if case.track:
            bn.running_mean.copy_(_dev(x.running_mean)), bn.running_var.copy_(_dev(x.running_var))
    return bn


def _hold(tag, case, got, want, zeros=()):
    """got / want: {quantity: array}.  Prints the figures, then asserts the bars, the non-finite pattern and the exact zeros."""
    bar = R.bars(case)
    key = lambda q: "y" if q == "eval" else q
    fig = {q: R.figure(got[q], want[q]) for q in want}
    nonfinite = {q: R.same_nonfinite(got[q], want[q]) for q in want}
    zero = {q: R.same_zeros(got[q], want[q]) for q in zeros}
    print(f"BN-EDGES gpu {tag} {case.name} " + " ".join(f"{q}={v:.2e}/{bar[key(q)]:.1e}" for q, v in fig.items())
          + f" non-finite as the reference={nonfinite} zeros as the reference={zero}")
    for q in want:
        assert got[q].dtype == np.float32 and got[q].shape == want[q].shape, q
        assert fig[q] < bar[key(q)], (q, fig[q], bar[key(q)])
        assert nonfinite[q], q
    assert all(zero.values()), zero


def _train(native, case, single_launch):
    from spacap3d_amd.fused_bn import bn_relu_train
    x, want = R.inputs(case), R.reference(case)
    bn = _module(case, x)
    z = _dev(x.z).requires_grad_(True)
    assert native.lib.spacap_bn_set_single_launch(1 if single_launch else 0) == 0
    try:
        out = bn_relu_train(z, bn, pool_S=case.S)
        saved = [t.clone() for t in out.grad_fn.saved_tensors]       # z, stats (C, 2), gamma, beta [, arg]
        if case.kind == "expanded":
            out.sum().backward()                                     # the upstream gradient arrives as an expanded scalar
        else:
            (out * _dev(x.up)).sum().backward()
        torch.cuda.synchronize()
    finally:
        native.lib.spacap_bn_set_single_launch(1)
    stats = _cpu(saved[1])
    got = {"pooled" if case.S else "y": _cpu(out), "dz": _cpu(z.grad), "dgamma": _cpu(bn.weight.grad), "dbeta": _cpu(bn.bias.grad),
           "stats_mean": stats[:, 0], "stats_istd": stats[:, 1]}
    ref = {"pooled" if case.S else "y": want.fwd.pooled if case.S else want.fwd.y, "dz": want.bwd.dz, "dgamma": want.bwd.dgamma,
           "dbeta": want.bwd.dbeta, "stats_mean": want.fwd.mean, "stats_istd": want.fwd.istd}
    if case.track:
        got.update(running_mean=_cpu(bn.running_mean), running_var=_cpu(bn.running_var))
        ref.update(running_mean=want.running_mean, running_var=want.running_var)
        assert int(bn.num_batches_tracked) == 1
    else:
        assert bn.running_mean is None
    form = "single launch" if R.bn_small(*case.shape[:2], int(np.prod(case.shape[2:])), single_launch) and not case.S else "three passes"
    if case.S:
        arg = saved[4]
        same = torch.equal(arg.cpu(), torch.tensor(want.fwd.arg))
        print(f"BN-EDGES gpu train {case.name} arg-max equal={same}")
        assert arg.dtype == torch.uint8 and same
    _hold(f"train ({form})", case, got, ref, zeros=("pooled" if case.S else "y", "dz"))
    if case.momentum is None and case.track:    # momentum None leaves the buffers as they were, to the bit
        assert np.array_equal(got["running_mean"], x.running_mean) and np.array_equal(got["running_var"], x.running_var)
    if case.kind in ("nan", "inf"):
        c = R.POISON_CHANNEL
        assert np.isnan(got["pooled" if case.S else "y"][:, c]).all() and np.isnan(got["dz"][:, c]).all()
        assert np.isnan(got["stats_istd"][c]) and np.isnan(got["running_var"][c]) and not np.isfinite(got["running_mean"][c])


_DENSE = [(c, s) for c in R.DENSE_CASES for s in ((True, False) if R.bn_small(*c.shape) else (True,))]


@pytest.mark.parametrize("case,single_launch", _DENSE, ids=lambda v: v.name if isinstance(v, R.Case) else ("default" if v else "single-launch-off"))
def test_dense_bn_relu_against_float64(native, case, single_launch):
    _train(native, case, single_launch)


@pytest.mark.parametrize("case", R.POOLED_CASES, ids=_name)
def test_pooled_bn_relu_max_against_float64(native, case):
    _train(native, case, True)


@pytest.mark.parametrize("case", R.DENSE_CASES, ids=_name)
def test_eval_form_against_float64(native, case):
    """bn_relu_eval on the batch's own statistics (float32): bn_relu_apply_kernel alone, at every dense shape of the table"""
    from spacap3d_amd.fused_bn import bn_relu_eval
    x = R.inputs(case)
    rm, rv = R.eval_buffers(case)
    bn = _module(case._replace(track=True), x).eval()
    with torch.no_grad():
        bn.running_mean.copy_(_dev(rm)), bn.running_var.copy_(_dev(rv))
        out = bn_relu_eval(_dev(x.z), bn)
    assert out is not None
    _hold("eval", case, {"eval": _cpu(out)}, {"eval": R.eval_forward(x.z, x.gamma, x.beta, rm, rv)}, zeros=("eval",))


# ---- the pooled backward at an S the forward does not serve: the C ABI itself --------------------------------------------------
@pytest.mark.parametrize("case", R.CABI_CASES, ids=_name)
def test_pooled_backward_of_the_c_abi_against_float64(native, case):
    """spacap_bn_relu_max_bwd_f32 takes any S up to 256: the scalar branch of bn_bwd_dz_kernel<true> (S % 4 != 0, with L % 4 == 0
    and without), its vector branch at S = 20, and S = 256 with a maximum at sample 255.  The statistics come from
    spacap_bn_stats_f32, the arg-max from the restatement; every output starts as NaN and must be written."""
    lib, check = native.lib, native.check
    x, want = R.inputs(case), R.reference(case)
    B, C, P, S = case.shape
    st = torch.cuda.current_stream().cuda_stream
    z, gamma, beta, dP, arg = _dev(x.z), _dev(x.gamma), _dev(x.beta), _dev(x.up), _dev(want.fwd.arg)
    ws = torch.empty(int(lib.spacap_bn_workspace_bytes(C)), dtype=torch.uint8, device=DEV)
    full = lambda *s: torch.full(s, _NAN, dtype=torch.float32, device=DEV)
    stats, dz, dgamma, dbeta = full(C, 2), full(*case.shape), full(C), full(C)
    check(lib.spacap_bn_stats_f32(z.data_ptr(), B, C, P * S, R.EPS, 0.0, None, None, stats.data_ptr(), ws.data_ptr(), st), "stats")
    check(lib.spacap_bn_relu_max_bwd_f32(z.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dP.data_ptr(), arg.data_ptr(),
                                         B, C, P, S, dz.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), st), "max_bwd")
    torch.cuda.synchronize()
    left = {k: int(torch.isnan(v).sum()) for k, v in (("stats", stats), ("dz", dz), ("dgamma", dgamma), ("dbeta", dbeta))}
    print(f"BN-EDGES gpu c-abi {case.name} NaN left: {left}")
    assert all(v == 0 for v in left.values()), left
    s = _cpu(stats)
    _hold("c-abi pooled backward", case, {"dz": _cpu(dz), "dgamma": _cpu(dgamma), "dbeta": _cpu(dbeta), "stats_mean": s[:, 0], "stats_istd": s[:, 1]},
          {"dz": want.bwd.dz, "dgamma": want.bwd.dgamma, "dbeta": want.bwd.dbeta, "stats_mean": want.fwd.mean, "stats_istd": want.fwd.istd})
    if case.kind == "top-index":
        assert int(arg[0, 1, 0]) == 255


# ---- refusals: by return code, before any launch ---------------------------------------------------------------------------------
_ENTRIES = ("stats", "train", "apply", "max", "bwd", "max_bwd")


def _calls(lib, B, C, L, P, S, only=_ENTRIES, null=None):
    """the named entry points of csrc/bn_relu.hip on buffers of the full size the arguments describe (a refusal that were missing
    would still stay inside them), every buffer pre-filled with 7; ``null`` names the one argument passed as a null pointer.
    Returns the return codes, the library's error text of each, and whether every buffer still holds its fill."""
    st = torch.cuda.current_stream().cuda_stream
    f = lambda *s: torch.full(s, 7.0, dtype=torch.float32, device=DEV)
    t = {"z": f(B, C, L), "gamma": f(C), "beta": f(C), "stats": f(C, 2), "out": f(B, C, L), "up": f(B, C, L), "dP": f(B, C, P), "dz": f(B, C, L),
         "dgamma": f(C), "dbeta": f(C), "pooled": f(B, C, P), "arg": torch.full((B, C, P), 7, dtype=torch.uint8, device=DEV),
         "ws": torch.full((int(lib.spacap_bn_workspace_bytes(C)),), 7, dtype=torch.uint8, device=DEV)}
    p = {k: (None if k == null else v.data_ptr()) for k, v in t.items()}
    entry = {
        "stats": lambda: lib.spacap_bn_stats_f32(p["z"], B, C, L, R.EPS, 0.1, None, None, p["stats"], p["ws"], st),
        "train": lambda: lib.spacap_bn_relu_train_f32(p["z"], B, C, L, R.EPS, 0.1, None, None, p["gamma"], p["beta"], p["stats"], p["out"],
                                                      p["ws"], st),
        "apply": lambda: lib.spacap_bn_relu_apply_f32(p["z"], p["stats"], p["gamma"], p["beta"], B, C, L, p["out"], st),
        "max": lambda: lib.spacap_bn_relu_max_f32(p["z"], p["stats"], p["gamma"], p["beta"], B, C, P, S, p["pooled"], p["arg"], st),
        "bwd": lambda: lib.spacap_bn_relu_bwd_f32(p["z"], p["stats"], p["gamma"], p["beta"], p["up"], B, C, L, p["dz"], p["dgamma"], p["dbeta"],
                                                  p["ws"], st),
        "max_bwd": lambda: lib.spacap_bn_relu_max_bwd_f32(p["z"], p["stats"], p["gamma"], p["beta"], p["dP"], p["arg"], B, C, P, S, p["dz"],
                                                          p["dgamma"], p["dbeta"], p["ws"], st),
    }
    rc, text = {}, {}
    for k in only:
        rc[k] = entry[k]()
        text[k] = lib.spacap_last_error().decode()
    torch.cuda.synchronize()
    return rc, text, all(bool((v == 7).all()) for v in t.values())


def test_out_of_range_sizes_and_null_pointers_are_refused_before_any_launch(native):
    """B C = 65536 is one past the blockIdx.y extent of the kernels that take a (b, c) row per workgroup: train, apply, bwd and
    max_bwd refuse it (the statistics and the pooled forward index their rows otherwise and are not asked).  C = 65536 is refused
    by the statistics, S = 48 by the pooled forward, a null z by all six, and the group max refuses S = 0, S = 257 and null
    pointers.  Only calls that must be refused are made; nothing is launched: every buffer keeps its fill."""
    lib = native.lib
    rc, text, untouched = _calls(lib, 2, 32768, 4, 1, 4, only=("train", "apply", "bwd", "max_bwd"))
    print(f"BN-EDGES gpu refusals B*C=65536: {rc} untouched={untouched} {text}")
    assert all(v == -1 for v in rc.values()) and untouched and all("bad sizes" in v for v in text.values())
    rc, text, untouched = _calls(lib, 1, 65536, 4, 1, 4, only=("stats",))
    print(f"BN-EDGES gpu refusals C=65536: {rc} untouched={untouched} {text}")
    assert rc["stats"] == -1 and untouched and "C out of range" in text["stats"]
    rc, text, untouched = _calls(lib, 2, 3, 5 * 48, 5, 48, only=("max",))
    print(f"BN-EDGES gpu refusals S=48: {rc} untouched={untouched} {text}")
    assert rc["max"] == -1 and untouched and "S=48 unsupported" in text["max"]
    rc, text, untouched = _calls(lib, 2, 3, 64, 4, 16, null="z")
    print(f"BN-EDGES gpu refusals null z: {rc} untouched={untouched}")
    assert all(v == -1 for v in rc.values()) and untouched and all("null pointer" in v for v in text.values())
    with pytest.raises(RuntimeError, match="null pointer"):
        native.check(rc["train"], "spacap_bn_relu_train_f32")
    assert lib.spacap_group_max_f32(None, 4, 16, None, None, None) == -1 and lib.spacap_group_max_grad_f32(None, None, 4, 16, None, None) == -1
    assert lib.spacap_group_max_f32(None, 4, 257, None, None, None) == -1 and lib.spacap_group_max_f32(None, 4, 0, None, None, None) == -1


# ---- group max -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GM_CASES, ids=_name)
def test_group_max_against_the_restatement(hip_ext, case):
    """the templated kernels at S = 16 .. 128 with row counts that do not fill a wave's step, the generic one at S = 1, 7 and 256
    and for an input that starts one float past a 16-byte boundary; ties at the top of every third row, one NaN"""
    x = R.gm_inputs(case)
    S = case.shape[3]
    val, arg = R.group_max(x.x)
    buf = torch.empty(x.x.size + 4, dtype=torch.float32, device=DEV)
    view = buf[case.offset:case.offset + x.x.size].view(case.shape)
    view.copy_(_dev(x.x))
    assert view.is_contiguous() and (view.data_ptr() % 16 == 0) == (case.offset == 0)
    out, a = hip_ext.group_max(view)
    gi = hip_ext.group_max_grad(_dev(x.go), a, S)
    same = (torch.equal(a.cpu(), torch.tensor(arg)), torch.equal(out.cpu().nan_to_num(123.0), torch.tensor(val).nan_to_num(123.0)),
            torch.equal(gi.cpu(), torch.tensor(R.group_max_grad(x.go, arg, S))))
    print(f"BN-EDGES gpu group_max {case.name} rows={x.x.size // S} arg / values / gradient equal={same}")
    assert a.dtype == torch.uint8 and all(same), same
