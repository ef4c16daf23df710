"""``relation.relation_pred`` once per form of its ladder (spacap3d_amd/relation.py: tier), at the smallest shapes that reach each
form, against float64 autograd of the reference composition (models/transformer_captioner.py:319-326, 392-397): the bars of
test_attention_gpu.py::test_relation_head_one_kernel_each_way -- 3e-5 absolute on the prediction, 5e-5 of the largest reference
entry on every gradient."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# form -> the autograd node that produces its prediction
NODE = {"fused": "RelationHeadBackward", "wide": "RelationWideBackward", "l1+tail": "RelationTailBackward",
        "feature+tail": "RelationTailBackward", "l1+tall": "_TallLinearBackward", "feature+tall": "_TallLinearBackward"}


def _problem(H, K, NO, seed):
    B, D = 1, 128 // H
    torch.manual_seed(seed)     # (the Linear initialisers draw from the global generator)
    g = torch.Generator().manual_seed(seed)
    P = torch.softmax(torch.randn(B, H, K, K, generator=g), -1)
    V = torch.randn(B, H, K, D, generator=g)
    w = torch.randn(B, K, K, NO, generator=g)
    lins = [torch.nn.Linear(128, 128), torch.nn.Linear(128, 128), torch.nn.Linear(128, NO)]
    refs = [torch.nn.Linear(l.in_features, l.out_features).double() for l in lins]
    for l, r in zip(lins, refs):
        r.load_state_dict({k: v.double() for k, v in l.state_dict().items()})
    Pr, Vr = P.double().requires_grad_(True), V.double().requires_grad_(True)
    feat = (Pr.unsqueeze(-1) * Vr.unsqueeze(2)).permute(0, 2, 3, 1, 4).reshape(B, K, K, H * D)
    want = refs[2](torch.relu(refs[1](torch.relu(refs[0](feat)))))
    return P, V, w, [l.to(DEV) for l in lins], refs, Pr, Vr, want


@pytest.mark.parametrize("H,K,NO,form", [(8, 8, 9, "fused"), (8, 7, 9, "wide"), (4, 16, 9, "l1+tail"), (8, 16, 5, "l1+tall"),
                                         (2, 16, 9, "feature+tail")])
def test_relation_pred_values_and_gradients_per_form(H, K, NO, form):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spacap3d_amd.relation import relation_pred, tier
    P, V, w, lins, refs, Pr, Vr, want = _problem(H, K, NO, seed=100 * H + K)
    assert tier(H, K, 128 // H, 128, NO, True, True) == form
    (want * w.double()).sum().backward()
    Pg, Vg = P.to(DEV).requires_grad_(True), V.to(DEV).requires_grad_(True)
    got = relation_pred(Pg, Vg, *lins)
    assert got.shape == want.shape and type(got.grad_fn).__name__ == NODE[form]
    err = float((got.detach().double().cpu() - want.detach()).abs().max())
    print(f"{form}: prediction error {err:.3g}")
    assert err < 3e-5
    (got * w.to(DEV)).sum().backward()
    pairs = [(Pg.grad, Pr.grad), (Vg.grad, Vr.grad)]
    for l, r in zip(lins, refs):
        pairs += [(l.weight.grad, r.weight.grad), (l.bias.grad, r.bias.grad)]
    for n, (a, b) in enumerate(pairs):
        d = float((a.double().cpu() - b).abs().max()) / (float(b.abs().max()) + 1e-12)
        print(f"{form}: gradient {n} error {d:.3g}")
        assert d < 5e-5, (n, d)


@pytest.mark.parametrize("H,K,form", [(8, 8, "fused"), (4, 16, "l1+tall"), (2, 16, "feature+tall")])
def test_relation_pred_without_gradient_recording(H, K, form):
    """The forms of the inference forward: no tail node (it exists for its backward)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spacap3d_amd.relation import relation_pred, tier
    P, V, _, lins, _, _, _, want = _problem(H, K, 9, seed=100 * H + K + 1)
    assert tier(H, K, 128 // H, 128, 9, True, False) == form
    with torch.no_grad():
        got = relation_pred(P.to(DEV), V.to(DEV), *lins)
    assert float((got.double().cpu() - want.detach()).abs().max()) < 3e-5
