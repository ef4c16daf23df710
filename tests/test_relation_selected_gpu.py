"""The relation head's backward over the selected proposal pairs (csrc/relation_fused.hip: rel_sel_scan_kernel,
rel_sel_compact_kernel, rel_fused_bwd_sel_kernel; C entry spacap_relation_fused_bwd_sel_f32).

The relation loss (reference lib/loss_helper.py:240-289) weights pair (i, j) by "both proposals are positive and assigned",
so dpred is zero outside (selected i) x (selected j).  The backward finds the active query rows and key columns from dpred
itself, compacts them into ascending lists padded to a multiple of 8, and runs the dense kernel's tile loop over the lists.

  1. sparse gradients against float64 autograd of the reference composition, the gate of
     test_attention_gpu.py::test_relation_head_one_kernel_each_way (max |got - ref| / max |ref| < 5e-5, nothing excluded);
  2. everything active: bit for bit the dense entry;  3. exact zeros and full coverage of the outputs from NaN-filled
  buffers;  4. the lists in the workspace (layout: include/spacap_hip.h) against a numpy restatement;  5. a captured graph
  replayed on another selection;  6. determinism;  7. few active 8-blocks: the dense kernel's tiles walked in place, bit for bit
  the dense entry.
Shapes stay below 100 000 pairs.  K = 8 holds at most 8 proposals: the selections of 9 and 17 take min(n, K) there.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, D, C, NO = 8, 16, 128, 9
SHAPES = [(1, 8), (2, 24), (3, 40), (2, 64)]
SELECTIONS = ["none", "one", "ends", "n3", "n9", "n17", "all", "ragged", "rows_ne_cols", "single"]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spacap3d_amd._native import lib
    return lib


def _pick(g, K, n):
    m = torch.zeros(K, dtype=torch.bool)
    m[torch.randperm(K, generator=g)[:min(n, K)]] = True
    return m


def selection(name, B, K, seed):
    """(rowmask, colmask) bool [B, K]; 'single' is one element of w (see weights())."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.zeros(B, K, dtype=torch.bool)
    if name == "none":
        pass
    elif name in ("one", "single"):
        for b in range(B):
            rows[b] = _pick(g, K, 1)
    elif name == "ends":
        rows[:, 0] = rows[:, K - 1] = True
    elif name in ("n3", "n9", "n17"):
        for b in range(B):
            rows[b] = _pick(g, K, int(name[1:]))
    elif name == "all":
        rows[:] = True
    elif name == "ragged":   # different counts per scene, one of them empty (a single scene keeps its five)
        for b, n in enumerate([5, 0, 11][:B]):
            rows[b] = _pick(g, K, n)
    elif name == "rows_ne_cols":
        rows[:, [1, 5]] = True
        cols = torch.zeros(B, K, dtype=torch.bool)
        cols[:, [0, 7] + ([8] if K > 8 else [])] = True
        return rows, cols
    return rows, rows.clone()


def weights(name, B, K, seed):
    """dpred of the test's loss sum(pred * w): randn on (selected rows) x (selected columns), exact zeros elsewhere."""
    g = torch.Generator().manual_seed(seed + 7)
    rows, cols = selection(name, B, K, seed)
    w = torch.randn(B, K, K, NO, generator=g) * rows[:, :, None, None] * cols[:, None, :, None]
    if name == "single":   # one non-zero element: output 4 of the last scene's one selected pair
        keep = torch.zeros(NO)
        keep[4] = 1.0
        w = w * keep
        w[:B - 1] = 0
        rows, cols = (w != 0).any(-1).any(2), (w != 0).any(-1).any(1)
    return w, rows, cols


def problem(B, K):
    """P, V and the three Linears as test_relation_head_one_kernel_each_way builds them."""
    torch.manual_seed(B * 1000 + K)
    g = torch.Generator().manual_seed(B * 1000 + K)
    P = torch.softmax(torch.randn(B, H, K, K, generator=g), -1)
    V = torch.randn(B, H, K, D, generator=g)
    lins = [torch.nn.Linear(128, 128), torch.nn.Linear(128, 128), torch.nn.Linear(128, 9)]
    return P, V, lins


@pytest.mark.parametrize("name", SELECTIONS)
@pytest.mark.parametrize("B,K", SHAPES)
def test_sparse_gradients_against_float64(lib, B, K, name):
    from spacap3d_amd.relation import relation_head
    P, V, lins = problem(B, K)
    w, _, _ = weights(name, B, K, seed=B * 100 + K)
    refs = [torch.nn.Linear(l.in_features, l.out_features).double() for l in lins]
    for l, r in zip(lins, refs):
        r.load_state_dict({k: v.double() for k, v in l.state_dict().items()})
    Pr, Vr = P.double().requires_grad_(True), V.double().requires_grad_(True)
    feat = (Pr.unsqueeze(-1) * Vr.unsqueeze(2)).permute(0, 2, 3, 1, 4).reshape(B, K, K, H * D)
    want = refs[2](torch.relu(refs[1](torch.relu(refs[0](feat)))))
    (want * w.double()).sum().backward()
    lins = [l.to(DEV) for l in lins]
    Pg, Vg = P.to(DEV).requires_grad_(True), V.to(DEV).requires_grad_(True)
    got = relation_head(Pg, Vg, *lins)
    assert got is not None
    (got * w.to(DEV)).sum().backward()
    pairs = [(Pg.grad, Pr.grad), (Vg.grad, Vr.grad)]
    for l, r in zip(lins, refs):
        pairs += [(l.weight.grad, r.weight.grad), (l.bias.grad, r.bias.grad)]
    names = ["dP", "dV", "dW1", "db1", "dW2", "db2", "dW3", "db3"]
    errs = {n: float(((a.double().cpu() - b).abs() / (float(b.abs().max()) + 1e-12)).max()) for n, (a, b) in zip(names, pairs)}
    print(B, K, name, errs)
    for n, e in errs.items():
        assert e < 5e-5, (n, e)


class Abi:
    """The head's forward once at (B, K); then either backward entry on a given dpred, through the C ABI."""

    def __init__(self, lib, B, K):
        self.lib, self.B, self.K = lib, B, K
        g = torch.Generator().manual_seed(B * 1000 + K + 1)
        r = lambda *s: torch.randn(*s, generator=g).to(DEV)
        self.P, self.U = torch.softmax(r(B, H, K, K), -1).contiguous(), r(B, K, H, C) * 0.3
        self.b1, self.W2, self.b2, self.W3, self.b3 = r(C) * 0.1, r(C, C) * 0.1, r(C) * 0.1, r(NO, C) * 0.1, r(NO)
        self.hid2 = torch.empty(B, K, K, C, device=DEV)
        pred = torch.empty(B, K, K, NO, device=DEV)
        self.nparts = int(lib.spacap_relation_fused_nparts(B, K))
        self.zslots = int(lib.spacap_relation_fused_sel_zsplit(B, K, self.nparts))
        assert self.zslots >= max(3, int(lib.spacap_relation_fused_zsplit(B, K, self.nparts)))
        self.ws_bytes = int(lib.spacap_relation_fused_sel_workspace_bytes(B, K))
        self.call(lib.spacap_relation_fused_fwd_f32, self.P, self.U, self.b1, self.W2, self.b2, self.W3, self.b3, B, K, self.hid2, pred)

    def call(self, fn, *args):
        from spacap3d_amd._native import check
        check(fn(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], torch.cuda.current_stream().cuda_stream), "call")

    def buffers(self, fill=None):
        B, K = self.B, self.K
        out = [torch.empty(B, H, K, K, device=DEV), torch.empty(self.zslots, B, K, H, C, device=DEV),
               torch.empty(self.nparts, int(self.lib.spacap_relation_fused_part_floats()), device=DEV),
               torch.empty(self.ws_bytes // 4, dtype=torch.float32, device=DEV)]
        if fill is not None:
            for t in out:
                t.fill_(fill)
        return out

    def dense(self, dpred):
        dP, dU, part, _ = self.buffers()
        self.call(self.lib.spacap_relation_fused_bwd_f32, dpred, self.hid2, self.P, self.U, self.b1, self.W2, self.W3, self.B, self.K,
                  self.nparts, self.zslots, dP, dU, part)
        return dP, dU, part

    def selected(self, dpred, bufs=None):
        dP, dU, part, ws = bufs if bufs is not None else self.buffers()
        self.call(self.lib.spacap_relation_fused_bwd_sel_f32, dpred, self.hid2, self.P, self.U, self.b1, self.W2, self.W3, self.B, self.K,
                  self.nparts, self.zslots, dP, dU, part, ws)
        return dP, dU, part, ws


@pytest.fixture(scope="module")
def abi(lib):
    cache = {}

    def get(B, K):
        if (B, K) not in cache:
            cache[(B, K)] = Abi(lib, B, K)
        return cache[(B, K)]
    return get


@pytest.mark.parametrize("B,K", [(2, 64), (1, 8)])
def test_all_active_is_the_dense_entry_bit_for_bit(abi, B, K):
    a = abi(B, K)
    dpred = torch.randn(B, K, K, NO, generator=torch.Generator().manual_seed(5)).to(DEV)
    assert bool((dpred != 0).all())
    dP0, dU0, part0 = a.dense(dpred)
    dP1, dU1, part1, ws = a.selected(dpred)
    cnt = ws.view(torch.int32)[:4 * B].view(B, 4).cpu()
    assert cnt.tolist() == [[K, K, K // 8, K // 8]] * B
    assert torch.equal(dP0, dP1)
    assert torch.equal(dU0.sum(0), dU1.sum(0))
    assert torch.equal(part0.sum(0), part1.sum(0))


@pytest.mark.parametrize("B,K,name", [(2, 64, "ends"), (2, 64, "one"), (2, 64, "single"), (2, 24, "one"), (3, 40, "single")])
def test_few_active_blocks_walk_the_dense_tiles_bit_for_bit(abi, B, K, name):
    """While the dense kernel's tiles that hold an active pair are at most 1/16 of all tiles (or no more than the tiles over the
    lists), the selected entry visits exactly those tiles with the dense kernel's partition: the same bits, not only the same
    values -- a training run keeps the trajectory it had with the dense entry."""
    a = abi(B, K)
    w, rows, cols = weights(name, B, K, seed=B * 100 + K)
    blocks = lambda m: m.view(B, K // 8, 8).any(-1).sum(1)
    tiles_in_place = int((blocks(rows) * blocks(cols)).sum())
    tiles_lists = int((((rows.sum(1) + 7) // 8) * ((cols.sum(1) + 7) // 8)).sum())
    assert tiles_in_place <= tiles_lists or tiles_in_place * 16 <= B * (K // 8) ** 2   # the case is one of the in-place walk
    dP0, dU0, part0 = a.dense(w.to(DEV))
    dP1, dU1, part1, _ = a.selected(w.to(DEV))
    assert torch.equal(dP0, dP1)
    assert torch.equal(dU0.sum(0), dU1.sum(0))
    assert torch.equal(part0.sum(0), part1.sum(0))


def want_list(mask):
    """numpy restatement: active indices ascending, padded to a multiple of 8 with the first inactive ones, ascending."""
    act, ina = np.flatnonzero(mask), np.flatnonzero(~mask)
    n8 = (len(act) + 7) // 8 * 8
    return np.concatenate([act, ina[:n8 - len(act)]])


@pytest.mark.parametrize("name", SELECTIONS)
@pytest.mark.parametrize("B,K", SHAPES)
def test_lists_zeros_and_coverage_from_nan_filled_buffers(abi, B, K, name):
    a = abi(B, K)
    w, rows, cols = weights(name, B, K, seed=B * 100 + K)
    dP, dU, part, ws = a.selected(w.to(DEV), a.buffers(fill=float("nan")))
    # 4. the lists
    wi = ws.view(torch.int32).cpu().numpy()
    cnt, qi, kj = wi[:4 * B].reshape(B, 4), wi[4 * B:4 * B + B * K].reshape(B, K), wi[4 * B + B * K:4 * B + 2 * B * K].reshape(B, K)
    for b in range(B):
        wq, wk = want_list(rows[b].numpy()), want_list(cols[b].numpy())
        assert cnt[b].tolist() == [int(rows[b].sum()), int(cols[b].sum()), len(wq) // 8, len(wk) // 8]
        assert qi[b, :len(wq)].tolist() == wq.tolist() and kj[b, :len(wk)].tolist() == wk.tolist()
    # 3. every byte of the outputs written; exact zeros off the active grid
    dUs = dU.sum(0)
    assert bool(torch.isfinite(dP).all()) and bool(torch.isfinite(dU).all()) and bool(torch.isfinite(part).all())
    live = (rows[:, None, :, None] & cols[:, None, None, :]).expand(B, H, K, K).to(DEV)
    assert bool((dP[~live] == 0).all())
    assert bool((dUs[~cols.to(DEV)] == 0).all())
    if name != "none":
        assert float(dP.abs().max()) > 0 and float(dUs.abs().max()) > 0
    # 6. determinism
    again = a.selected(w.to(DEV))
    assert torch.equal(dP, again[0]) and torch.equal(dU, again[1]) and torch.equal(part, again[2])


@pytest.mark.parametrize("value", [0.0, -0.0])
def test_zero_gradient_gives_exact_zeros(abi, value):
    a = abi(2, 24)
    dP, dU, part, ws = a.selected(torch.full((2, 24, 24, NO), value, device=DEV), a.buffers(fill=float("nan")))
    assert ws.view(torch.int32)[:8].tolist() == [0] * 8
    for t in (dP, dU, part):
        assert bool((t == 0).all())


def test_nan_gradient_is_active_and_propagates(abi):
    a = abi(2, 24)
    dpred = torch.zeros(2, 24, 24, NO, device=DEV)
    dpred[1, 3, 17, 2] = float("nan")
    dP, dU, part, ws = a.selected(dpred)
    assert ws.view(torch.int32)[:8].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert bool(torch.isnan(dP[1, :, 3, 17]).all()) and bool(torch.isnan(part.sum(0)).any())
    assert bool(torch.isfinite(dP[0]).all())


def test_replayed_graph_follows_the_selection_of_the_replay(abi):
    B, K = 2, 24
    a = abi(B, K)
    wA = weights("n9", B, K, seed=11)[0].to(DEV)
    rows = torch.zeros(B, K, dtype=torch.bool)
    rows[1, [2, 3, 20]] = True   # other counts, scene 0 empty
    wB = (torch.randn(B, K, K, NO, generator=torch.Generator().manual_seed(12)) * rows[:, :, None, None] * rows[:, None, :, None]).to(DEV)
    dpred = wA.clone()
    bufs = a.buffers()
    a.selected(dpred, bufs)   # (first call outside the capture: it sets the kernel's LDS attribute)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a.selected(dpred, bufs)
    graph.replay()
    wantA = a.selected(wA)
    for got, want in zip(bufs[:3], wantA[:3]):
        assert torch.equal(got, want)
    dpred.copy_(wB)
    graph.replay()
    wantB = a.selected(wB)
    torch.cuda.synchronize()
    for got, want in zip(bufs[:3], wantB[:3]):
        assert torch.equal(got, want)
    assert not torch.equal(wantA[0], wantB[0])
