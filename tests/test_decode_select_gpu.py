"""Decoding over the kept proposals only on the MI355X (csrc/decode_select.hip, spacap3d_amd/decode_select.py,
transformer_captioner.forward_eval with a ``decode_mask``, engine.Evaluator(decode="kept")) against the
numpy restatement (tests/decode_select_restated.py), the unchanged decoders called directly on the packed rows, and the
unmasked forward.  Everything is compared exactly except (d6), which keeps the criteria of the existing fused-against-generic
tests.  The restatement itself, the C ABI's refusals and the Python layer's: tests/test_decode_select_cpu.py."""
import numpy as np
import pytest
import torch

import decode_select_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0x7F


@pytest.fixture(autouse=True, scope="module")
def _needs_a_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _poison(shape, dtype):
    """A device tensor whose every byte is 0x7f."""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(POISON)
    return t


def _raw():
    from spacap3d_amd._native import check, lib
    return lib, check, torch.cuda.current_stream().cuda_stream


def _select_raw(mask, capacity):
    """spacap_decode_select_i32 on poisoned outputs."""
    lib, check, st = _raw()
    n = mask.numel()
    rows, slot, count = _poison((capacity,), torch.int32), _poison((n,), torch.int32), _poison((2,), torch.int32)
    check(lib.spacap_decode_select_i32(mask.data_ptr(), n, capacity, rows.data_ptr(), slot.data_ptr(), count.data_ptr(), st),
          "spacap_decode_select_i32")
    return rows, slot, count


# ---- a. select ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SIZES)
def test_select_against_the_restatement(n):
    """Every density and capacity of the restatement's list at this n: exact, on poisoned outputs (every element is written),
    with mask bytes other than 0 and 1, and a second call gives the same bits; the Python wrapper gives the same."""
    from spacap3d_amd import decode_select as ds
    for density in R.DENSITIES:
        host = R.mask_case(n, density)
        assert density in (0.0, 1.0) or n < 64 or (host > 1).any()
        mask = torch.from_numpy(host.copy()).to(DEV)
        for capacity in R.capacities(n, int(np.count_nonzero(host))):
            want = R.select_case(n, density, capacity)
            got = _select_raw(mask, capacity)
            again = _select_raw(mask, capacity)
            for g, a, w in zip(got, again, want):
                assert np.array_equal(g.cpu().numpy(), w), (density, capacity)
                assert torch.equal(g, a)
    rows, slot, count = ds.select(mask.view(-1, 1) if n % 2 else mask.view(2, -1), capacity)
    for g, w in zip((rows, slot, count), want):
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w)
    wrapped = ds.select(mask != 0, capacity)                 # a bool mask
    assert all(torch.equal(a, b) for a, b in zip(wrapped, (rows, slot, count)))


def test_select_captured_replays_on_a_new_mask():
    from spacap3d_amd import decode_select as ds
    n, capacity = 2049, 700
    first, second = R.mask_case(n, 0.5), R.mask_case(n, 0.1)
    static = torch.from_numpy(first.copy()).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ds.select(static, capacity)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ds.select(static, capacity)
    for host in (first, second):
        static.copy_(torch.from_numpy(host.copy()))
        g.replay()
        torch.cuda.synchronize()
        eager = ds.select(torch.from_numpy(host.copy()).to(DEV), capacity)
        for o, e, w in zip(out, eager, R.select(host, capacity)):
            assert torch.equal(o, e) and np.array_equal(o.cpu().numpy(), w)
    assert int(out[2][0]) < capacity < int(np.count_nonzero(first))      # one mask overflowed, the other left padding rows


# ---- b. gather ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_memory", (False, True))
@pytest.mark.parametrize("capacity", (1, 15, 16, 17, 300))
def test_gather_is_the_torch_sum_and_padding_is_zero(capacity, with_memory):
    lib, check, st = _raw()
    from spacap3d_amd import decode_select as ds
    g = torch.Generator().manual_seed(capacity)
    n, d = 320, 128
    obj, mem = torch.randn(n, d, generator=g).to(DEV), torch.randn(n, d, generator=g).to(DEV)
    obj[5], mem[5] = -0.0, -0.0
    rows = torch.randperm(n, generator=g)[:capacity].sort().values.to(torch.int32)
    rows[0] = 5
    pad = torch.arange(capacity) % 4 == 3 if capacity > 1 else torch.zeros(1, dtype=torch.bool)
    if capacity == 17:
        pad[:] = False
        pad[-1] = True                                          # the one row past a block of 16 is padding
    rows[pad] = -1
    rows = rows.to(DEV)
    out = _poison((capacity, d), torch.float32)
    check(lib.spacap_decode_gather_f32(obj.data_ptr(), mem.data_ptr() if with_memory else None, rows.data_ptr(), capacity, d,
                                       out.data_ptr(), st), "spacap_decode_gather_f32")
    live = (rows >= 0).nonzero().view(-1)
    src = rows[live].long()
    want = obj[src] + mem[src] if with_memory else obj[src]
    assert torch.equal(out[live].view(torch.int32), want.view(torch.int32))                      # bit-equal
    assert bool((out[(rows < 0)].view(torch.int32) == 0).all())                                  # exactly +0.0
    assert np.array_equal(out.cpu().numpy().view(np.int32),
                          R.gather(obj.cpu().numpy(), mem.cpu().numpy() if with_memory else None, rows.cpu().numpy()).view(np.int32))
    assert torch.equal(ds.gather(obj, mem if with_memory else None, rows).view(torch.int32), out.view(torch.int32))


# ---- c. scatter --------------------------------------------------------------------------------------------------------------------
def _slots(kind, n, capacity, g):
    if kind == "none":
        return torch.full((n,), -1, dtype=torch.int32)
    if kind == "all":
        return (torch.randperm(n, generator=g) % capacity).to(torch.int32)
    s = torch.full((n,), -1, dtype=torch.int32)
    at = torch.randperm(n, generator=g)[:capacity]
    s[at] = torch.randperm(capacity, generator=g).to(torch.int32)
    return s


@pytest.mark.parametrize("kind", ("mixed", "none", "all"))
@pytest.mark.parametrize("inner,L", ((32, 32), (96, 32), (3, 1)))
def test_scatter_against_the_restatement(inner, L, kind):
    """The three entry points on poisoned outputs, exactly; word ids 0 and 2^40 + 7; a slot vector that is all -1 and one with
    none at -1."""
    lib, check, st = _raw()
    from spacap3d_amd import decode_select as ds
    g = torch.Generator().manual_seed(inner + L)
    n, capacity, big = 301, 77, 2 ** 40 + 7
    slot = _slots(kind, n, capacity, g)
    ys = torch.randint(0, 3, (capacity, inner), generator=g) * big // 2        # 0, big // 2 and ...
    ys[::2, 0] = big                                                            # ... 2^40 + 7 itself
    ys[1, :] = 0
    d_slot, d_ys = slot.to(DEV), ys.to(DEV)
    for eos in (3, big):
        out = _poison((n, inner), torch.int64)
        check(lib.spacap_decode_scatter_i64(d_ys.data_ptr(), d_slot.data_ptr(), n, inner, L, eos, out.data_ptr(), st),
              "spacap_decode_scatter_i64")
        assert np.array_equal(out.cpu().numpy(), R.scatter_words(ys.numpy(), slot.numpy(), L, eos))
    W = inner // L
    assert torch.equal(ds.scatter_words(d_ys.view(capacity, W, L) if W > 1 else d_ys, d_slot, big).view(n, inner), out)
    for dtype, fill, fn in ((torch.float32, 0.0, lib.spacap_decode_scatter_f32), (torch.float32, -2.5, lib.spacap_decode_scatter_f32),
                            (torch.int32, 1, lib.spacap_decode_scatter_i32), (torch.int32, -9, lib.spacap_decode_scatter_i32)):
        vals = (torch.randn(capacity, inner, generator=g) * 100).to(dtype)
        d_vals = vals.to(DEV)
        out = _poison((n, inner), dtype)
        check(fn(d_vals.data_ptr(), d_slot.data_ptr(), n, inner, fill, out.data_ptr(), st), "spacap_decode_scatter")
        want = R.scatter_values(vals.numpy(), slot.numpy(), fill)
        assert out.cpu().numpy().tobytes() == want.tobytes()
        assert torch.equal(ds.scatter_values(d_vals, d_slot, fill), out)


# ---- d. the decoders ---------------------------------------------------------------------------------------------------------------
from test_beam_search_gpu import SCORE_TOL as BEAM_TOL  # noqa: E402
from test_sampling_gpu import SAMPLE_SEED, SEED  # noqa: E402

ALL_KEYS = ("lang_cap", "lang_cap_score", "lang_cap_beams", "lang_cap_beam_scores", "lang_cap_beam_lengths", "lang_cap_samples",
            "lang_cap_sample_scores", "lang_cap_sample_lengths", "lang_cap_decoded", "lang_cap_rows")


class _Scene:
    pass


@pytest.fixture(scope="module")
def scene():
    """The model and scenes of tests/test_sampling_gpu.py (two scenes, 32 proposals each, eval mode), one forward, the
    indicator rows the unmasked forward_eval hands its decoder, and two random masks with their restated selections (shared,
    not modified)."""
    from spacap3d_amd import caption_decode as cd
    from spacap3d_amd.engine import synthetic_batch
    from spacap3d_amd.spacapnet import build_default
    s = _Scene()
    torch.manual_seed(SEED)
    s.model = build_default(vocab_size=120, num_proposal=32, N=2, d_ff=256).to(DEV).eval()
    s.cap = s.model.caption
    data = synthetic_batch(2, 4096, DEV, seed=1, vocab=120)
    seen = {}
    plain = cd.greedy_decode

    def spy(dec, generator, embed, pe, indicator, sos, n_words):
        seen["indicator"] = indicator.clone()
        return plain(dec, generator, embed, pe, indicator, sos, n_words)

    cd.greedy_decode = spy
    try:
        with torch.no_grad():
            s.d = s.model(dict(data), is_eval=True)
    finally:
        cd.greedy_decode = plain
    s.indicator = seen["indicator"]                             # (B K, 128): obj + memory, as torch adds them
    s.B, s.K, s.L = s.d["lang_cap"].shape
    s.n = s.B * s.K
    s.sos, s.eos = s.cap.word_to_idx["sos"], s.cap.word_to_idx["eos"]
    rng = np.random.default_rng(5)
    s.masks = [rng.random((s.B, s.K)) < p for p in (0.5, 0.3)]
    s.counts = [int(m.sum()) for m in s.masks]
    s.dmasks = [torch.from_numpy(m).to(DEV) for m in s.masks]
    s.mask, s.dmask, s.count = s.masks[0], s.dmasks[0], s.counts[0]
    return s


def _masked(s, mask, capacity, **kw):
    with torch.no_grad():
        out = s.cap.forward_eval(dict(s.d), decode_mask=mask, decode_capacity=capacity, **kw)
    return {k: out[k] for k in ALL_KEYS if k in out}


def _empty(s, reps=1):
    e = torch.zeros(reps * s.L, dtype=torch.long, device=DEV)
    e[::s.L] = s.eos
    return e


def test_the_masks_leave_something_in_and_something_out(scene):
    s = scene
    assert s.n == 64 and all(0 < c < 128 and 0 < c < s.n for c in s.counts) and s.counts[0] != s.counts[1]
    assert s.indicator.shape == (s.n, 128)


def test_a_zero_indicator_row_decodes_to_finite_values(scene):
    """What makes the padding rows harmless: LayerNorm puts eps on the std, so a zero row normalises to zero."""
    from spacap3d_amd import caption_decode as cd
    s = scene
    m = s.cap.model
    zero = torch.zeros(3, 128, device=DEV)
    args = (m.decoder, m.generator, m.tgt_embed[0], m.tgt_embed[1].pe, zero, s.sos)
    words = cd.greedy_decode(*args, s.L)
    assert bool(((words >= 0) & (words < 120)).all())
    ys, score, length = cd.sample_decode(*args, s.eos, s.L, 2, 1.0, 0, SAMPLE_SEED)
    assert bool(torch.isfinite(score).all()) and bool(((ys >= 0) & (ys < 120)).all()) and bool(((length >= 1) & (length <= s.L)).all())
    _, best, _, scores, _ = cd.beam_decode(*args, s.eos, s.L, 3, return_all=True)
    assert bool(torch.isfinite(best).all()) and bool(torch.isfinite(scores).all())


def test_d1_greedy_rows_equal_the_unmasked_forward(scene):
    s = scene
    out = _masked(s, s.dmask, s.count)
    assert set(out) == {"lang_cap", "lang_cap_decoded", "lang_cap_rows"}
    cap = out["lang_cap"]
    assert cap.shape == (s.B, s.K, s.L) and cap.dtype == torch.long
    assert torch.equal(out["lang_cap_decoded"], s.dmask) and out["lang_cap_decoded"].dtype == torch.bool
    assert out["lang_cap_rows"].dtype == torch.int32 and out["lang_cap_rows"].tolist() == [s.count, s.count]
    assert torch.equal(cap[s.dmask], s.d["lang_cap"][s.dmask])                       # bit for bit where decoded
    assert bool((cap[~s.dmask] == _empty(s)).all())                                  # the empty caption elsewhere
    slot = s.cap.last_decode_slot
    assert np.array_equal(slot.cpu().numpy(), R.select(s.mask, s.count)[1])
    assert not bool((s.d["lang_cap"][~s.dmask] == _empty(s)).all(-1).all())          # (the unmasked run writes captions there)
    uint8 = _masked(s, s.dmask.to(torch.uint8) * 7, s.count)                         # a uint8 mask with bytes other than 1
    assert all(torch.equal(uint8[k], out[k]) for k in out)


def _direct(s, rows, mode):
    """beam_decode / sample_decode called directly on indicator[rows]."""
    from spacap3d_amd import caption_decode as cd
    m = s.cap.model
    ind = s.indicator[torch.from_numpy(rows).long().to(DEV)]
    args = (m.decoder, m.generator, m.tgt_embed[0], m.tgt_embed[1].pe, ind, s.sos, s.eos, s.L)
    if mode == "beam":
        ys, best, beams, scores, lengths = cd.beam_decode(*args, 3, 0.0, return_all=True)
        return {"lang_cap": ys, "lang_cap_score": best, "lang_cap_beams": beams, "lang_cap_beam_scores": scores,
                "lang_cap_beam_lengths": lengths}
    ys, score, length = cd.sample_decode(*args, 3, 1.0, mode.get("top_k", 0), SAMPLE_SEED, mode.get("top_p"))
    return {"lang_cap": ys[:, 0], "lang_cap_score": score[:, 0], "lang_cap_samples": ys, "lang_cap_sample_scores": score,
            "lang_cap_sample_lengths": length}


def _scattered(s, direct, slot):
    """The direct results put back by the restatement: words with the empty caption, scores with 0.0, lengths with 1."""
    want = {}
    for k, t in direct.items():
        h = t.reshape(t.shape[0], -1).cpu().numpy()
        if h.dtype == np.int64:
            got = R.scatter_words(h, slot, s.L, s.eos)
        else:
            got = R.scatter_values(h, slot, 0.0 if h.dtype == np.float32 else 1)
        want[k] = got.reshape((s.B, s.K) + tuple(t.shape[1:]))
    return want


@pytest.mark.parametrize("mode", ("beam", "sample", "top_k", "top_p"))
def test_d2_beam_and_samples_equal_the_decoders_on_the_packed_rows(scene, mode):
    """W = 3 / S = 3 at a fixed seed (unrestricted, top_k = 4, top_p = 0.8): every output is the direct call's on
    indicator[rows], scattered by the restatement, bit for bit.  (Not the unmasked run's: its log-sum-exp merges another
    number of vocabulary slices and its noise is keyed by other rows.)"""
    s = scene
    rows, slot, _ = R.select(s.mask, s.count)
    kw = {"sample": {}, "top_k": {"top_k": 4}, "top_p": {"top_p": 0.8}}.get(mode)
    try:
        if mode == "beam":
            s.cap.beam_return_all = True
            out = _masked(s, s.dmask, s.count, beam_size=3)
            assert torch.equal(s.cap.last_beam_trace["slot"], s.cap.last_decode_slot)
            assert s.cap.last_beam_trace["word"].shape == (s.L, s.count, 3)           # the packed-row layout
            want = _scattered(s, _direct(s, rows, "beam"), slot)
        else:
            out = _masked(s, s.dmask, s.count, num_samples=3, temperature=1.0, sample_seed=SAMPLE_SEED, **kw)
            want = _scattered(s, _direct(s, rows, kw), slot)
    finally:
        s.cap.__dict__.pop("beam_return_all", None)
        s.cap.__dict__.pop("last_beam_trace", None)
    assert set(out) == set(want) | {"lang_cap_decoded", "lang_cap_rows"} and len(want) == 5
    for k, w in want.items():
        got = out[k].cpu().numpy()
        assert got.dtype == w.dtype and got.shape == w.shape and got.tobytes() == w.tobytes(), k
    lengths = out["lang_cap_beam_lengths" if mode == "beam" else "lang_cap_sample_lengths"]
    assert bool((lengths[~s.dmask] == 1).all()) and bool((out["lang_cap_score"][~s.dmask] == 0.0).all())
    assert np.array_equal(s.cap.last_decode_slot.cpu().numpy(), slot)


def test_d3_capacity_below_and_above_the_count(scene):
    s = scene
    exact = _masked(s, s.dmask, s.count)
    below = s.count // 2
    out = _masked(s, s.dmask, below)
    rows, slot, count = R.select(s.mask, below)
    assert out["lang_cap_rows"].tolist() == [s.count, below] == list(count)
    first = torch.from_numpy(slot >= 0).to(DEV).view(s.B, s.K)                       # the first `below` flags in flat order
    assert int(first.sum()) == below and torch.equal(out["lang_cap_decoded"], first)
    assert np.array_equal(np.flatnonzero(slot >= 0), np.flatnonzero(s.mask.reshape(-1))[:below])
    assert torch.equal(out["lang_cap"][first], exact["lang_cap"][first]) and bool((out["lang_cap"][~first] == _empty(s)).all())
    for above in (s.count + 1, s.n):                                                 # padding rows change nothing
        out = _masked(s, s.dmask, above)
        assert out["lang_cap_rows"].tolist() == [s.count, s.count]
        assert torch.equal(out["lang_cap"], exact["lang_cap"]) and torch.equal(out["lang_cap_decoded"], s.dmask)
    try:
        s.cap.beam_return_all = True
        outs = [_masked(s, s.dmask, s.n, num_samples=2, sample_seed=SAMPLE_SEED), _masked(s, s.dmask, s.n, beam_size=3)]
    finally:
        s.cap.__dict__.pop("beam_return_all", None)
        s.cap.__dict__.pop("last_beam_trace", None)
    for out in outs:
        for k, t in out.items():
            assert bool(torch.isfinite(t.double()).all()), k
            if t.dtype == torch.long:
                assert bool(((t >= 0) & (t < 120)).all()), k


def test_d4_exact_mode(scene, monkeypatch):
    from spacap3d_amd import caption_decode as cd
    s = scene
    calls = []
    plain = cd.greedy_decode

    def counted(*a, **k):
        calls.append(a[4].shape[0])
        return plain(*a, **k)

    monkeypatch.setattr(cd, "greedy_decode", counted)
    fixed = _masked(s, s.dmask, s.count)
    exact = _masked(s, s.dmask, None)
    assert calls == [s.count, s.count]
    assert set(exact) == set(fixed) and all(torch.equal(exact[k], fixed[k]) for k in fixed)
    none = _masked(s, torch.zeros_like(s.dmask), None)
    assert calls == [s.count, s.count], "an all-false mask must not call the decoder"
    assert bool((none["lang_cap"] == _empty(s)).all()) and none["lang_cap"].shape == (s.B, s.K, s.L)
    assert not bool(none["lang_cap_decoded"].any()) and none["lang_cap_rows"].tolist() == [0, 0]
    try:
        s.cap.beam_return_all = True
        nb = _masked(s, torch.zeros_like(s.dmask), None, beam_size=3)
        ns = _masked(s, torch.zeros_like(s.dmask), None, num_samples=2)
    finally:
        s.cap.__dict__.pop("beam_return_all", None)
    assert bool((nb["lang_cap_beams"].reshape(s.n, -1) == _empty(s, 3)).all()) and bool((nb["lang_cap_beam_lengths"] == 1).all())
    assert bool((ns["lang_cap_samples"].reshape(s.n, -1) == _empty(s, 2)).all()) and bool((ns["lang_cap_sample_scores"] == 0).all())
    assert nb["lang_cap_beam_scores"].shape == (s.B, s.K, 3) and ns["lang_cap_sample_lengths"].dtype == torch.int32
    every = _masked(s, torch.ones_like(s.dmask), None)
    assert calls == [s.count, s.count, s.n]
    assert torch.equal(every["lang_cap"], s.d["lang_cap"]) and bool(every["lang_cap_decoded"].all())


def test_d5_captured_forward_eval_replays_on_a_second_mask(scene):
    s = scene
    capacity = max(s.counts) + 3
    static = s.dmasks[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _masked(s, static, capacity)                           # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _masked(s, static, capacity)
    for m, c in zip(s.dmasks, s.counts):
        static.copy_(m)
        g.replay()
        torch.cuda.synchronize()
        eager = _masked(s, m, capacity)
        assert out["lang_cap_rows"].tolist() == [c, c]
        assert set(out) == set(eager) and all(torch.equal(out[k], eager[k]) for k in eager)


def test_d6_generic_paths_under_a_mask(scene):
    """beam_generic / sample_generic under the mask against the fused paths, by the criteria of
    tests/test_beam_search_gpu.py and tests/test_sampling_gpu.py without a mask: rows are identical, or the first differing
    step is a near-tie by the generic path's recorded gap; at most 5 % of the rows differ."""
    s = scene
    cap = s.cap
    lmax = []
    hook = cap.model.generator.proj.register_forward_hook(lambda m, a, o: lmax.append(o.detach().abs().max()))
    try:
        fused_b = _masked(s, s.dmask, s.count, beam_size=3)
        tz = {k: v.cpu() for k, v in cap.last_beam_trace.items()}
        fused_s = _masked(s, s.dmask, s.count, num_samples=3, temperature=1.0, sample_seed=SAMPLE_SEED)
        assert "gap" not in tz and cap.last_sample_trace is None, "forward_eval did not take the fused decoders"
        cap.beam_generic = cap.sample_generic = True
        gen_b = _masked(s, s.dmask, s.count, beam_size=3)
        tg = {k: v.cpu() for k, v in cap.last_beam_trace.items()}
        del lmax[:]
        gen_s = _masked(s, s.dmask, s.count, num_samples=3, temperature=1.0, sample_seed=SAMPLE_SEED)
        gap_s = cap.last_sample_trace["gap"].cpu()
        assert torch.equal(cap.last_sample_trace["slot"], cap.last_decode_slot) and torch.equal(tg["slot"], tz["slot"])
    finally:
        hook.remove()
        for k in ("beam_generic", "sample_generic", "last_beam_trace", "last_sample_trace"):
            cap.__dict__.pop(k, None)
    assert tg["gap"].shape == (s.L, s.count) and gap_s.shape == (s.L, 3 * s.count)              # the packed-row layout
    for a, b in ((fused_b, gen_b), (fused_s, gen_s)):
        assert set(a) == set(b)
        assert torch.equal(a["lang_cap_decoded"], b["lang_cap_decoded"]) and torch.equal(a["lang_cap_rows"], b["lang_cap_rows"])
        assert torch.equal(a["lang_cap"][~s.dmask], b["lang_cap"][~s.dmask])
    # beam search: per packed row the (parent, word) traces
    differs = ((tz["parent"].long() != tg["parent"].long()) | (tz["word"].long() != tg["word"].long())).any(-1)   # (n_words, rows)
    diff = [(r, int(torch.nonzero(differs[:, r])[0])) for r in range(s.count) if bool(differs[:, r].any())]
    print(f"beam, fused vs generic: {len(diff)} of {s.count} rows differ; gaps {[float(tg['gap'][t, r]) for r, t in diff]}")
    for r, t in diff:
        assert float(tg["gap"][t, r]) < BEAM_TOL, (r, t)
    assert len(diff) <= 0.05 * s.count
    if not diff:
        assert torch.equal(fused_b["lang_cap"], gen_b["lang_cap"])
        assert float((fused_b["lang_cap_score"] - gen_b["lang_cap_score"]).abs().max()) <= BEAM_TOL
    # samples: per packed row and sample the words
    pick = lambda o: o["lang_cap_samples"][s.dmask].reshape(-1, s.L).cpu().numpy()  # noqa: E731  (rows in packed order)
    a, b = pick(fused_s), pick(gen_s)
    tol = 1e-4 * float(torch.stack(lmax).max()) / 1.0 + 1e-5
    diff = [(int(r), int(np.flatnonzero(a[r] != b[r])[0])) for r in np.flatnonzero((a != b).any(1))]
    print(f"samples, fused vs generic: {len(diff)} of {a.shape[0]} rows differ; gaps {[float(gap_s[t, r]) for r, t in diff]} "
          f"(open below {tol:.3g})")
    for r, t in diff:
        assert float(gap_s[t, r]) < tol, (r, t)
    assert len(diff) <= 0.05 * a.shape[0]
    if not diff:
        assert torch.equal(fused_s["lang_cap_sample_lengths"], gen_s["lang_cap_sample_lengths"])
        assert float((fused_s["lang_cap_sample_scores"] - gen_s["lang_cap_sample_scores"]).abs().max()) <= 1e-3


# ---- e. Evaluator ------------------------------------------------------------------------------------------------------------------
class _Labelled(torch.nn.Module):
    """tests/test_caption_eval_gpu.py's _LabelledForward with the ``after_proposal`` hook passed on: proposal k is assigned
    ground-truth box k, its own box for even k (IoU 1), that box moved 100 m away for odd k (IoU 0)."""

    def __init__(self, model, M):
        super().__init__()
        self.model, self.M, self.caption = model, M, model.caption

    def forward(self, d, is_eval=True, after_proposal=None):
        out = self.model(d, is_eval=is_eval, after_proposal=after_proposal)
        B, K = out["bbox_mask"].shape
        gt = torch.zeros(B, self.M, 8, 3, device=out["bbox_corner"].device)
        gt[:, :K] = out["bbox_corner"].float()
        gt[:, 1:K:2] += 100.0
        out["gt_box_corner_label"] = gt
        out["object_assignment"] = torch.arange(K, device=gt.device).expand(B, K).contiguous()
        return out


def test_e_evaluator_kept_equals_all(monkeypatch):
    """Evaluator(decode="kept") against decode="all" on a synthetic batch: every pred_* and post_* tensor bit-equal, the
    caption metrics' candidates equal, post-processing run once, and the decoder run on the kept rows only."""
    import caption_eval_restated as CR
    from spacap3d_amd import caption_decode as cd
    from spacap3d_amd import postprocess
    from spacap3d_amd.caption_eval import CaptionCorpus, CaptionEval
    from spacap3d_amd.engine import Evaluator, synthetic_batch
    from spacap3d_amd.spacapnet import build_default
    from test_caption_eval_cpu import FIX, corpus_of
    from test_postprocess_gpu import POST_DICT
    torch.manual_seed(0)
    K = 64
    model = build_default(vocab_size=200, num_proposal=K, N=2, d_ff=256).to(DEV).eval()
    with torch.no_grad():                                # an objectness head that says "object" (tests/test_caption_eval_gpu.py):
        head = model.proposal.proposal[-1]               # the NMS alone decides pred_mask
        head.bias[0] -= 4.0
        head.bias[1] += 4.0
    # The untrained boxes do not overlap, so the NMS keeps all 128 at any nms_iou; they hold 7 .. 185 points, median 27
    # (measured on the MI355X): with min_points = 30 the empty-box rule keeps about half of them.
    post = dict(POST_DICT, dataset_config=None, min_points=30)
    batch = synthetic_batch(2, 4096, DEV, seed=1, vocab=200)
    M = batch["sem_cls_label"].shape[1]
    ids = (3 * torch.arange(M, device=DEV)) % 10
    batch["scene_object_ids"] = torch.stack([ids, (ids + 1) % 10])
    batch["dataset_idx"] = torch.tensor([[0], [1]], device=DEV)
    sos, eos = model.caption.word_to_idx["sos"], model.caption.word_to_idx["eos"]

    def evaluator(**kw):
        corpus, w2i = corpus_of("select")
        ce = CaptionEval(CaptionCorpus(corpus, w2i, key_of=FIX["select/key_table"]), CR.SOS, CR.EOS)
        return Evaluator(_Labelled(model, M), postprocess=post, predictions=(sos, eos), caption_eval=ce, **kw), ce

    rows, posts = [], []
    plain_greedy, plain_post = cd.greedy_decode, postprocess.detection_postprocess
    monkeypatch.setattr(cd, "greedy_decode", lambda *a, **k: (rows.append(a[4].shape[0]), plain_greedy(*a, **k))[1])
    monkeypatch.setattr(postprocess, "detection_postprocess", lambda *a, **k: (posts.append(1), plain_post(*a, **k))[1])
    ev_all, ce_all = evaluator(decode="all")
    full = ev_all(dict(batch))
    ev_kept, ce_kept = evaluator(decode="kept")
    kept = ev_kept(dict(batch))
    ev_cap, ce_cap = evaluator(decode="kept", decode_capacity=2 * K)
    capped = ev_cap(dict(batch))
    torch.cuda.synchronize()
    count = int(full["post_pred_mask"].sum())
    print(f"pred_mask keeps {count} of {2 * K} proposals; decoder rows per call {rows}")
    assert 0 < count < 2 * K
    assert rows == [2 * K, count, 2 * K] and posts == [1, 1, 1]                      # kept rows only; post-processing once
    names = [k for k in full if k.startswith(("pred_", "post_"))]
    assert len([k for k in names if k.startswith("pred_")]) == 7 and len([k for k in names if k.startswith("post_")]) >= 6
    for other, ce in ((kept, ce_kept), (capped, ce_cap)):
        for k in names:
            assert other[k].dtype == full[k].dtype and torch.equal(other[k], full[k]), k
        assert torch.equal(other["lang_cap_decoded"], full["post_pred_mask"])
        assert other["lang_cap_rows"].tolist() == [count, count]
        assert torch.equal(other["lang_cap"][full["post_pred_mask"]], full["lang_cap"][full["post_pred_mask"]])
        assert torch.equal(ce.cand_tok, ce_all.cand_tok) and torch.equal(ce.cand_len, ce_all.cand_len)
        assert torch.equal(ce.stamp, ce_all.stamp)
        idx2word = {i: str(i) for i in range(4096)}
        assert ce.candidates(idx2word) == ce_all.candidates(idx2word)
    assert int((ce_all.stamp > 0).sum()) >= 2                                        # the run wrote candidates
    assert "lang_cap_decoded" not in full and "decode_mask" not in full
