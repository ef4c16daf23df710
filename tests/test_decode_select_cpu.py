"""No-GPU checks of decoding over the kept proposals only (spacap3d_amd/decode_select.py): the numpy
restatement (tests/decode_select_restated.py) against an independent brute force and its invariants, header and binding agree
on the new symbols, the C entry points reject bad arguments without touching a device, and the Python layer refuses CPU
tensors and bad arguments."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import decode_select_restated as R

HERE = os.path.dirname(os.path.abspath(__file__))
SYMBOLS = {"spacap_decode_select_i32": 7, "spacap_decode_gather_f32": 7, "spacap_decode_scatter_i64": 8,
           "spacap_decode_scatter_f32": 7, "spacap_decode_scatter_i32": 7}


@pytest.mark.parametrize("density", R.DENSITIES)
@pytest.mark.parametrize("n", R.SIZES)
def test_restatement_against_brute_force_and_invariants(n, density):
    mask = R.mask_case(n, density)
    set_ = np.flatnonzero(mask)                        # the independent statement: the set flags in flat order
    count = int(set_.shape[0])
    assert count == {0.0: 0, 1.0: n}.get(density, count)
    for capacity in R.capacities(n, count):
        rows, slot, cnt = R.select_case(n, density, capacity)
        held = min(count, capacity)
        assert rows.dtype == slot.dtype == cnt.dtype == np.int32 and rows.shape == (capacity,) and slot.shape == (n,)
        assert list(cnt) == [count, held]
        assert np.array_equal(rows[:held], set_[:held]) and (rows[held:] == -1).all()
        want_slot = np.full(n, -1, np.int64)
        want_slot[set_[:held]] = np.arange(held)
        assert np.array_equal(slot, want_slot)
        # invariants
        assert (np.diff(rows[:held]) > 0).all()                                   # strictly increasing up to count[1]
        assert np.array_equal(slot[rows[:held]], np.arange(held))                 # slot[rows[i]] == i
        none = np.flatnonzero(slot == -1)
        overflowed = set_[held:]
        assert np.isin(none, np.concatenate([np.flatnonzero(mask == 0), overflowed])).all()
        assert (slot[overflowed] == -1).all() and (slot[mask == 0] == -1).all()


def test_gather_and_scatter_restated_against_numpy_indexing():
    rng = np.random.default_rng(3)
    n, d = 37, 8
    obj, mem = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
    rows, slot, cnt = R.select(rng.random(n) < 0.4, 20)
    held = int(cnt[1])
    assert 0 < held < 20
    for memory in (None, mem):
        got = R.gather(obj, memory, rows)
        want = obj[rows[:held]] if memory is None else obj[rows[:held]] + mem[rows[:held]]
        assert got[:held].tobytes() == want.tobytes() and got[held:].tobytes() == np.zeros((20 - held, d), np.float32).tobytes()
    ys = rng.integers(0, 100, (20, 6)).astype(np.int64)
    out = R.scatter_words(ys, slot, 3, 7)
    dec = slot >= 0
    assert np.array_equal(out[dec], ys[slot[dec]]) and (out[~dec] == np.array([7, 0, 0, 7, 0, 0])).all()
    vals = rng.integers(0, 100, (20, 2)).astype(np.int32)
    out = R.scatter_values(vals, slot, 1)
    assert out.dtype == np.int32 and np.array_equal(out[dec], vals[slot[dec]]) and (out[~dec] == 1).all()
    out = R.scatter_values(vals.astype(np.float32), slot, 0.0)
    assert out.dtype == np.float32 and (out[~dec] == 0.0).all()


def test_symbols_are_declared_and_exported():
    from spacap3d_amd import _native, decode_select
    header = open(os.path.join(os.path.dirname(HERE), "include", "spacap_hip.h")).read()
    for name, nargs in SYMBOLS.items():
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _native.SIGNATURES and hasattr(_native.lib, name)
        decl = re.search(r"\bint %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_native.SIGNATURES[name][1]) == nargs, name     # as many arguments on both sides
    assert decode_select.MAX_FLAGS == R.SIZES[-1]
    makefile = open(os.path.join(os.path.dirname(HERE), "spacap3d_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bdecode_select\.hip\b", makefile, flags=re.M)
    assert "decode_select" not in re.search(r"^CONTRACT_FAST\s*:=(.*)$", makefile, flags=re.M).group(1)


def test_entry_points_reject_bad_arguments_without_a_device():
    from spacap3d_amd._native import lib
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 15) & ~15           # a 16-byte aligned host address: never dereferenced by a refusal
    err = lib.spacap_last_error

    sel = lambda n=64, cap=8, mask=a, rows=a, slot=a, count=a: lib.spacap_decode_select_i32(mask, n, cap, rows, slot, count, None)  # noqa: E731
    for bad in (dict(n=-1), dict(n=65537), dict(cap=0), dict(cap=65), dict(cap=-1)):
        assert sel(**bad) == -1 and b"bad sizes" in err(), bad
    for bad in (dict(mask=None), dict(rows=None), dict(slot=None), dict(count=None)):
        assert sel(**bad) == -1 and b"null" in err(), bad
    assert sel(n=0, cap=0, mask=None, rows=None, slot=None, count=None) == 0

    gat = lambda cap=8, d=128, obj=a, mem=a, rows=a, out=a: lib.spacap_decode_gather_f32(obj, mem, rows, cap, d, out, None)  # noqa: E731
    for bad in (dict(cap=-1), dict(d=0), dict(d=2), dict(d=126), dict(d=-4)):
        assert gat(**bad) == -1 and b"bad sizes" in err(), bad
    for bad in (dict(obj=None), dict(rows=None), dict(out=None)):
        assert gat(**bad) == -1 and b"null" in err(), bad
    for bad in (dict(obj=a + 4), dict(mem=a + 8), dict(out=a + 12)):
        assert gat(**bad) == -1 and b"16-byte aligned" in err(), bad
    assert gat(cap=0, obj=None, mem=None, rows=None, out=None) == 0

    words = lambda n=8, inner=32, L=32, ys=a, slot=a, out=a: lib.spacap_decode_scatter_i64(ys, slot, n, inner, L, 3, out, None)  # noqa: E731
    for bad in (dict(n=-1), dict(inner=0), dict(L=0), dict(inner=33), dict(inner=32, L=5), dict(inner=96, L=64)):
        assert words(**bad) == -1 and b"bad sizes" in err(), bad
    for bad in (dict(ys=None), dict(slot=None), dict(out=None)):
        assert words(**bad) == -1 and b"null" in err(), bad
    assert words(n=0, ys=None, slot=None, out=None) == 0

    for fn, fill in ((lib.spacap_decode_scatter_f32, 0.0), (lib.spacap_decode_scatter_i32, 1)):
        vals = lambda n=8, inner=3, v=a, slot=a, out=a: fn(v, slot, n, inner, fill, out, None)  # noqa: E731
        for bad in (dict(n=-1), dict(inner=0), dict(inner=-3)):
            assert vals(**bad) == -1 and b"bad sizes" in err(), bad
        for bad in (dict(v=None), dict(slot=None), dict(out=None)):
            assert vals(**bad) == -1 and b"null" in err(), bad
        assert vals(n=0, v=None, slot=None, out=None) == 0


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    from spacap3d_amd import decode_select as ds
    from spacap3d_amd.engine import Evaluator
    from spacap3d_amd.spacapnet import build_default
    mask = torch.zeros(2, 8, dtype=torch.bool)
    i32 = torch.zeros(4, dtype=torch.int32)
    for call in (lambda: ds.select(mask, 4), lambda: ds.gather(torch.zeros(16, 128), None, i32),
                 lambda: ds.scatter_words(torch.zeros(4, 31, dtype=torch.long), i32, 3),
                 lambda: ds.scatter_values(torch.zeros(4), i32, 0.0)):
        with pytest.raises(RuntimeError, match=r"decode_select: .*: CPU not supported"):
            call()

    cap = build_default(vocab_size=40, num_proposal=8, N=1, d_ff=128).caption.eval()
    ep = {"aggregated_vote_features": torch.zeros(2, 8, 128)}
    with pytest.raises(ValueError, match=r"decode_mask must be a \(B, K\) = \(2, 8\) tensor"):
        cap.forward_eval(dict(ep), decode_mask=torch.zeros(2, 7, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"decode_mask must be a \(B, K\)"):
        cap.forward_eval(dict(ep), decode_mask=torch.zeros(16, dtype=torch.bool))
    with pytest.raises(ValueError, match="decode_mask must be bool or uint8"):
        cap.forward_eval(dict(ep), decode_mask=torch.zeros(2, 8))
    for bad in (0, -1, 17, 2.0, True):
        with pytest.raises(ValueError, match=r"decode_capacity .* must be None or an int in 1\.\.B K = 16"):
            cap.forward_eval(dict(ep), decode_mask=mask, decode_capacity=bad)
        with pytest.raises(ValueError, match="decode_capacity"):                           # ... read from the dict as well
            cap.forward_eval(dict(ep, decode_mask=mask, decode_capacity=bad))
    with pytest.raises(ValueError, match="decode_mask packs the rows of the cached decoders"):
        cap.forward_eval(dict(ep), use_cache=False, decode_mask=mask)
    with pytest.raises(RuntimeError, match="decode_mask: CPU not supported"):
        cap.forward_eval(dict(ep), decode_mask=mask, decode_capacity=16)

    with pytest.raises(ValueError, match="decode='kept' needs postprocess"):
        Evaluator(None, decode="kept")
    with pytest.raises(ValueError, match="decode 'some' must be 'all' or 'kept'"):
        Evaluator(None, postprocess={}, decode="some")
    with pytest.raises(ValueError, match="decode_capacity"):
        Evaluator(None, postprocess={}, decode="kept", decode_capacity=0)
    assert Evaluator(None).decode == "all" and Evaluator(None, postprocess={}, decode="kept", decode_capacity=5).decode_capacity == 5
