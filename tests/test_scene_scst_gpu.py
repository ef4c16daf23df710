"""Self-critical training over every matched object of a scene on the MI355X: the selection kernel
(csrc/scst_select.hip) and the row-indexed decoder input (csrc/caption_prep.hip) against their restatement
(tests/scene_scst_restated.py) bit for bit, the matched training forward end to end against float64 autograd on the CPU oracle
backend (the fixture follows tests/test_self_critical_gpu.py's), two eager ``Trainer`` steps and the refusal of a batch without
its labels.  The largest figures are printed."""
import numpy as np
import pytest
import torch

import losses_restated as LR
import scene_scst_restated as SS
import self_critical_restated as SC
from caption_eval_restated import decode as decode_caption
from test_self_critical_gpu import CIDER_TOL, GRAD_TENSORS, _cpu_copy, _grad_leaves, _no_dropout, _run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W2I = {"pad_": 0, "unk": 1, "sos": 2, "eos": 3, "a": 4}


@pytest.fixture(autouse=True, scope="module")
def _needs_a_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _up(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _ids(case):
    return "-".join(str(v) for v in case)


# ---- (a) the selection kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SS.SELECT_CASES, ids=_ids)
def test_selection_kernel_equals_the_restatement(case):
    from spacap3d_amd.caption_eval import CaptionCorpus
    from spacap3d_amd.self_critical import SelfCritical
    B, K, G, M = case
    x, ref = SS.select_inputs(case), SS.select_reference(case)
    cc = CaptionCorpus({"k%d" % i: ["sos a eos"] for i in range(SS.SELECT_NKEYS)}, W2I, key_of=np.array(x.key_table))
    sc = SelfCritical(cc, 2, 3, proposals="matched", max_proposals=M, near_threshold=SS.SELECT_NEAR)
    out = (torch.full((B, M), -7, dtype=torch.int64, device=DEV), torch.full((B, M), -7, dtype=torch.int64, device=DEV),
           torch.full((B, M), -7, dtype=torch.int32, device=DEV), torch.full((B, M), -7, dtype=torch.int32, device=DEV),
           torch.full((B, M), float("nan"), device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV))
    got = sc.select(_up(x.xyz), _up(x.center), _up(x.label_mask), _up(x.object_ids), _up(x.dataset_idx), out=out)
    print(f"{case}: filled slots per scene {ref.n_sel.tolist()}")
    for name, g, w in zip(ref._fields, got, ref):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=name)


def test_selection_refuses_more_slots_than_objects():
    from spacap3d_amd._native import lib
    z = torch.zeros(64, device=DEV)
    zi = torch.zeros(64, dtype=torch.int64, device=DEV)
    for K, G, M in ((0, 4, 2), (4, 257, 2), (4, 4, 5), (4, 4, 0)):
        assert lib.spacap_scst_select_f32(z.data_ptr(), z.data_ptr(), z.data_ptr(), zi.data_ptr(), zi.data_ptr(), zi.data_ptr(), 1, K, G, M,
                                          1, 1, 1, 0.09, zi.data_ptr(), zi.data_ptr(), zi.data_ptr(), zi.data_ptr(), z.data_ptr(),
                                          zi.data_ptr(), None) != 0


# ---- (b) the row-indexed decoder input -------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", (0.0, 0.3))
@pytest.mark.parametrize("case", SS.PREP_CASES, ids=_ids)
def test_row_indexed_input_both_ways(case, p):
    from spacap3d_amd._native import check, lib
    from spacap3d_amd.attention import rng_state
    from spacap3d_amd.transformer_captioner import PositionalEncoding
    B, K, M, S, D, T, V = case
    R, L, seed = B * M * S, T - 1, 20261021
    x = SS.prep_inputs(case)
    pe = PositionalEncoding(D, 0.0).pe[0].to(DEV).contiguous()
    src, mem, prop, tok, emb, g = (_up(a) for a in (x.src, x.memory, x.prop.reshape(-1), x.tok, x.emb, x.g))
    st, sdev = torch.cuda.current_stream().cuda_stream, rng_state(torch.device(DEV)).data_ptr()
    nan = float("nan")

    def forward():
        x0, mask = torch.full((R, L, D), nan, device=DEV), torch.full((R, L, L), 9, dtype=torch.uint8, device=DEV)
        check(lib.spacap_caption_prep_rows_fwd_f32(src.data_ptr(), mem.data_ptr(), prop.data_ptr(), tok.data_ptr(), emb.data_ptr(),
                                                   pe.data_ptr(), B, K, M, S, D, T, V, p, seed, sdev, x0.data_ptr(), mask.data_ptr(), st),
              "spacap_caption_prep_rows_fwd_f32")
        return x0, mask

    def backward():
        d_rows, d_emb = torch.full((B, K, D), nan, device=DEV), torch.full((V, D), nan, device=DEV)
        check(lib.spacap_caption_prep_rows_bwd_f32(g.data_ptr(), tok.data_ptr(), prop.data_ptr(), B, K, M, S, D, T, V, p, seed, sdev,
                                                   d_rows.data_ptr(), d_emb.data_ptr(), st), "spacap_caption_prep_rows_bwd_f32")
        return d_rows, d_emb

    x0, mask = forward()
    if p == 0.0:
        want = SS.prep_rows_fwd(x.src, x.memory, x.prop, x.tok, x.emb, pe.cpu().numpy(), M, S)
        np.testing.assert_array_equal(x0.cpu().numpy(), want[0])
        np.testing.assert_array_equal(mask.cpu().numpy(), want[1])
    # the existing kernel on copied rows whose referred centre is the chosen proposal's own position
    grp = torch.arange(R, device=DEV) // S
    scene, k = grp // M, prop[grp]
    some = k >= 0
    xyz = _up(x.xyz)
    xyz_r, ref_r = xyz[scene].contiguous(), xyz[scene, k.clamp(min=0)].contiguous()
    src_r, mem_r = src[scene].contiguous(), mem[scene].contiguous()
    x0e, maske = torch.empty(R, L, D, device=DEV), torch.empty(R, L, L, dtype=torch.uint8, device=DEV)
    idx, dist, pred = torch.empty(R, dtype=torch.int64, device=DEV), torch.empty(R, device=DEV), torch.empty(1, device=DEV)
    good, ticket = torch.empty(R, dtype=torch.bool, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)
    check(lib.spacap_caption_prep_fwd_f32(xyz_r.data_ptr(), ref_r.data_ptr(), src_r.data_ptr(), mem_r.data_ptr(), tok.data_ptr(),
                                          emb.data_ptr(), pe.data_ptr(), R, K, D, T, V, p, seed, sdev, x0e.data_ptr(), maske.data_ptr(),
                                          idx.data_ptr(), dist.data_ptr(), good.data_ptr(), pred.data_ptr(), ticket.data_ptr(), st),
          "spacap_caption_prep_fwd_f32")
    assert torch.equal(idx[some], k[some])
    assert torch.equal(x0[some], x0e[some]) and torch.equal(x0[:, 1:], x0e[:, 1:]) and torch.equal(mask, maske)
    assert not x0[~some][:, 0].any()
    if p > 0.0 and L > 1:
        share = float((x0[:, 1:] == 0).float().mean())
        assert abs(share - p) < 0.1, share

    d_rows, d_emb = backward()
    d_emb_e = torch.full((V, D), nan, device=DEV)
    check(lib.spacap_caption_prep_bwd_f32(g.data_ptr(), tok.data_ptr(), idx.data_ptr(), R, K, D, T, V, p, seed, sdev, None,
                                          d_emb_e.data_ptr(), st), "spacap_caption_prep_bwd_f32")
    assert torch.equal(d_emb, d_emb_e)
    want, n = SS.prep_rows_bwd(x.g, x.prop, B, K, M, S)
    got = d_rows.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    g0 = x.g[:, 0].astype(np.float64)
    d64, sabs = np.zeros((B, K, D)), np.zeros((B, K, D))
    for r in range(R):
        b_, k_ = r // S // M, int(x.prop.reshape(-1)[r // S])
        if k_ >= 0:
            d64[b_, k_] += g0[r]
            sabs[b_, k_] += np.abs(g0[r])
    excess = np.abs(got - d64) - np.maximum(n - 1, 0)[..., None] * 2.0 ** -24 * sabs
    print(f"{case} p={p}: up to {n.max()} rows per element, largest |d_rows - float64| = {np.abs(got - d64).max():.3e}")
    assert (excess <= 0).all() and (got[n == 0] == 0).all()
    again = backward()
    assert torch.equal(again[0], d_rows) and torch.equal(again[1], d_emb) and torch.equal(forward()[0], x0)


def test_row_indexed_op_through_autograd():
    """``caption_prep_rows`` as the captioner calls it: the gradients of src and memory are the kernel's d_rows, the embedding's
    its d_emb."""
    from spacap3d_amd.backend import HipBackend
    from spacap3d_amd.transformer_captioner import Embeddings, PositionalEncoding
    case = SS.PREP_CASES[2]
    B, K, M, S, D, T, V = case
    x = SS.prep_inputs(case)
    torch.manual_seed(0)
    emb, pos = Embeddings(D, V).to(DEV), PositionalEncoding(D, 0.0).to(DEV)
    src, mem = _up(x.src).requires_grad_(True), _up(x.memory).requires_grad_(True)
    x0, mask = HipBackend().caption_prep_rows(src, mem, _up(x.prop), _up(x.tok), emb, pos, S)
    (x0 * _up(x.g)).sum().backward()
    want, _ = SS.prep_rows_bwd(x.g, x.prop, B, K, M, S)
    np.testing.assert_array_equal(src.grad.cpu().numpy(), want)
    assert torch.equal(src.grad, mem.grad) and emb.lut.weight.grad is not None and mask.dtype == torch.uint8
    with pytest.raises(RuntimeError, match="caption_prep_rows"):
        HipBackend().caption_prep_rows(src, mem, _up(x.prop)[:, :-1], _up(x.tok), emb, pos, S)


# ---- (c) the matched training forward, end to end --------------------------------------------------------------------------
# M = 4 is the least that leaves every scene three filled slots and one scene an empty one
SEED, SAMPLE_SEED, CORPUS_SEED, S_SAMPLES, M_SLOTS, NEAR, N_WORDS = 0, 20261020, 20261021, 3, 4, 0.3, 31
KEYED_SLOTS = ((0, 1, 2, 3, 4), (1, 3, 5))         # the object slots with a key row, per scene: more than M, fewer than M
ID_OFFSET = 3                                      # scene_object_ids[b, j] = j + 3


@pytest.fixture(scope="module")
def matched():
    from oracle.attention_ref import OracleBackend
    from spacap3d_amd import backend, caption_decode
    from spacap3d_amd import synthetic as SY
    from spacap3d_amd.caption_eval import CaptionCorpus
    from spacap3d_amd.engine import synthetic_batch
    from spacap3d_amd.loss_helper import compute_cap_loss
    from spacap3d_amd.self_critical import SelfCritical
    from spacap3d_amd.spacapnet import build_default
    torch.manual_seed(SEED)
    model = build_default(vocab_size=120, num_proposal=32, N=2, d_ff=256).to(DEV).eval()
    data = synthetic_batch(2, 4096, DEV, seed=1, vocab=120)
    with torch.no_grad():
        d = model(dict(data), is_eval=True)
    anchored = SY.anchor_boxes_on_proposals(data, d["aggregated_vote_xyz"])
    cap = _no_dropout(model.caption).train()
    B, K, D = d["aggregated_vote_features"].shape
    G = data["center_label"].shape[1]
    ep = {k: v.detach() for k, v in d.items() if torch.is_tensor(v) and not k.startswith("lang_cap")}
    ep["center_label"], ep["ref_center_label"] = anchored["center_label"], anchored["ref_center_label"]
    ep["dataset_idx"] = torch.arange(B, device=DEV).view(B, 1)
    ep["scene_object_ids"] = (torch.arange(G, device=DEV) + ID_OFFSET).repeat(B, 1)
    ep["object_id"] = torch.tensor([KEYED_SLOTS[b][0] + ID_OFFSET for b in range(B)], device=DEV)      # (the referred mode's)
    table = np.full((B, G + ID_OFFSET), -1, np.int32)
    keys = [(b, j) for b in range(B) for j in KEYED_SLOTS[b]]
    for row, (b, j) in enumerate(keys):
        table[b, j + ID_OFFSET] = row
    sos, eos = cap.word_to_idx["sos"], cap.word_to_idx["eos"]
    idx2word = {i: w for w, i in cap.word_to_idx.items()}
    res = {"cap": cap, "ep": ep, "table": table, "B": B, "K": K}

    # the restated selection on the CPU copy of the inputs
    xyz = ep["aggregated_vote_xyz"].cpu().numpy()
    sel = SS.select(xyz, ep["center_label"].cpu().numpy(), ep["box_label_mask"].cpu().numpy(), ep["scene_object_ids"].cpu().numpy(),
                    np.arange(B), table, len(keys), NEAR, M_SLOTS)
    res["sel"] = sel
    assert len({tuple(p) for p in xyz.reshape(-1, 3)}) == B * K                       # the proposals are distinct points

    res["ce_before"] = _run(cap, ep)
    te, dec, gen = cap.model.tgt_embed, cap.model.decoder, cap.model.generator
    with torch.no_grad():
        src = ep["aggregated_vote_features"]
        memory = cap.model.encode(src, cap._src_pos(ep), ep["bbox_mask"].unsqueeze(1))
        both = src + memory
        # references: captions of each keyed object's nearest proposal at another seed, plus its greedy caption
        near_k = [SS.nearest(xyz[b], ep["center_label"][b, j].cpu().numpy())[0] for b, j in keys]
        ind = torch.stack([both[b, k] for (b, _), k in zip(keys, near_k)])
        other = caption_decode.sample_decode(dec, gen, te[0], te[1].pe, ind, sos, eos, N_WORDS, S_SAMPLES, 1.0, 0, CORPUS_SEED)[0]
        greedy = caption_decode.greedy_decode(dec, gen, te[0], te[1].pe, ind, sos, N_WORDS)
        prop = _up(sel.prop)
        ind_sel = both[torch.arange(B, device=DEV)[:, None], prop.clamp(min=0)].masked_fill((prop < 0).unsqueeze(-1), 0.0).reshape(B * M_SLOTS, D)
        res["direct"] = caption_decode.sample_decode(dec, gen, te[0], te[1].pe, ind_sel, sos, eos, N_WORDS, S_SAMPLES, 1.0, 0, SAMPLE_SEED)
        res["greedy"] = caption_decode.greedy_decode(dec, gen, te[0], te[1].pe, ind_sel, sos, N_WORDS).cpu().numpy()
    other, greedy = other.cpu().numpy(), greedy.cpu().numpy()
    refs = [[decode_caption(w, sos, eos) for w in other[i]] + [decode_caption(greedy[i], sos, eos)] for i in range(len(keys))]
    corpus = {"k%d" % i: [" ".join(idx2word[t] for t in r) for r in refs[i]] for i in range(len(keys))}
    res["refs"] = refs
    cc = CaptionCorpus(corpus, cap.word_to_idx, key_of=table)
    mk = lambda mode: SelfCritical(cc, sos, eos, num_samples=S_SAMPLES, seed=SAMPLE_SEED, proposals=mode, max_proposals=M_SLOTS,
                                   near_threshold=NEAR)
    try:
        cap.self_critical = mk("referred")
        res["referred_before"] = _run(cap, ep)
        cap.self_critical = mk("matched")
        res["scst"] = _run(cap, ep)
        res["scst_again"] = _run(cap, ep)[0]["_cap_loss"][0].detach().clone()
        cap.self_critical = mk("referred")
        res["referred_after"] = _run(cap, ep)
    finally:
        del cap.self_critical
    res["ce_after"] = _run(cap, ep)
    res["mk"] = mk

    # the restated rewards over the B M groups, and the float64 oracle over the rows of the filled groups
    out = res["scst"][0]
    samples = out["scst_samples"].cpu().numpy().reshape(B * M_SLOTS * S_SAMPLES, N_WORDS)
    rc = SC.Corpus(refs)
    didx, oid = np.repeat(np.arange(B), M_SLOTS), sel.obj.reshape(-1)
    rw = SC.rewards(rc, samples, S_SAMPLES, didx, oid, table, sos, eos)
    base = SC.rewards(rc, res["greedy"], 1, didx, oid, table, sos, eos).cider
    count = sel.prop.reshape(-1) >= 0
    res["rw"], res["base"], res["count"], res["samples"] = rw, base, count, samples
    cap64 = _no_dropout(_cpu_copy(cap).double()).train()
    cap64.check_relation = False
    ep64 = {k: (ep[k].cpu().double() if ep[k].is_floating_point() else ep[k].cpu())
            for k in ("aggregated_vote_features", "aggregated_vote_xyz", "bbox_mask", "ref_center_label", "lang_label", "lang_ids")}

    def run64(rows_scene, ep_rows, loss_of):
        for p in cap64.parameters():
            p.grad = None
        feat = ep64["aggregated_vote_features"].clone().requires_grad_(True)
        e = {k: v[rows_scene] for k, v in dict(ep64, aggregated_vote_features=feat).items()}
        e.update(ep_rows)
        with backend.use_backend(OracleBackend()):
            o = cap64.forward_train(e)
            value = loss_of(o)
            value.backward()
        g = {k: p.grad.clone() for k, p in _grad_leaves(cap64).items()}
        g["aggregated_vote_features"] = feat.grad.clone()
        return o, value.detach(), g

    res["ce64"] = run64(torch.arange(B), {}, lambda o: compute_cap_loss(o)[0])
    # Every scene keeps its M S rows in the float64 run, the empty groups' among them (pointed at proposal 0, advantage 0: they
    # contribute nothing): the position embedding of the encoder holds a BatchNorm1d in training mode, whose statistics over
    # unevenly repeated scenes are not those of the B scenes the device encodes once.
    live = np.repeat(count, S_SAMPLES)
    res["live"] = live
    grp = np.arange(B * M_SLOTS * S_SAMPLES) // S_SAMPLES
    rows_scene = torch.from_numpy(grp // M_SLOTS)
    ref_xyz = torch.from_numpy(xyz[grp // M_SLOTS, np.maximum(sel.prop.reshape(-1)[grp], 0)]).double()
    A64, _ = SC.advantage(rw.cider, base, count, S_SAMPLES)
    A = torch.from_numpy(A64.astype(np.float32).astype(np.float64))
    length = torch.from_numpy(rw.length.astype(np.int64))
    words = torch.from_numpy(samples)
    den = float(LR._den(float(rw.length[live].sum())))
    tok = torch.cat([torch.ones(len(grp), 1, dtype=torch.long), torch.from_numpy(rw.tf_tok[:, :-1])], 1)

    def scst_loss64(o):
        lp = o["lang_cap"].gather(2, words.unsqueeze(-1)).squeeze(-1)
        live = (torch.arange(N_WORDS)[None, :] < length[:, None]).double()
        return -(A * (lp * live).sum(1)).sum() / den

    res["scst64"] = run64(rows_scene, {"lang_label": tok, "lang_ids": tok[:, 1:], "ref_center_label": ref_xyz}, scst_loss64)
    assert torch.equal(res["scst64"][0]["match_idx"][torch.from_numpy(live)], torch.from_numpy(sel.prop.reshape(-1)[grp][live]))
    return res


def test_matched_forward_selection_samples_and_rewards(matched):
    out, sel, rw, base, count = matched["scst"][0], matched["sel"], matched["rw"], matched["base"], matched["count"]
    B, M, S = matched["B"], M_SLOTS, S_SAMPLES
    # what M was chosen for, in the restatement
    adv = out["scst_advantage"].cpu().numpy()
    assert (sel.n_sel >= 3).all() and (sel.n_sel < M).any()
    print(f"filled slots {sel.n_sel.tolist()}, share of rows with |A| > 1e-3: {(np.abs(adv) > 1e-3).mean():.2f}")
    assert (np.abs(adv) > 1e-3).mean() >= 0.5
    assert "lang_cap" not in out and "_cap_vec" not in out
    for k, shape in (("scst_proposal", (B, M)), ("scst_object_id", (B, M)), ("scst_count", (B, M)), ("scst_baseline", (B, M)),
                     ("scst_samples", (B, M, S, N_WORDS)), ("scst_reward", (B, M, S)), ("scst_advantage", (B, M, S)),
                     ("scst_logp", (B, M, S)), ("scst_sample_scores", (B, M, S))):
        assert tuple(out[k].shape) == shape, k
    np.testing.assert_array_equal(out["scst_proposal"].cpu().numpy(), sel.prop)
    np.testing.assert_array_equal(out["scst_object_id"].cpu().numpy(), sel.obj)
    np.testing.assert_array_equal(out["scst_count"].cpu().numpy(), sel.prop >= 0)
    ys, score, _ = matched["direct"]
    assert torch.equal(out["scst_samples"].reshape(ys.shape), ys) and torch.equal(out["scst_sample_scores"].reshape(score.shape), score)
    e_r = float(np.abs(out["scst_reward"].cpu().numpy().reshape(-1) - rw.cider).max())
    e_b = float(np.abs(out["scst_baseline"].cpu().numpy().reshape(-1) - base).max())
    print(f"largest |scst_reward - restated CIDEr| = {e_r:.3e}, baseline {e_b:.3e}; rewards up to {rw.cider.max():.3f}")
    assert e_r <= CIDER_TOL and e_b <= CIDER_TOL
    np.testing.assert_array_equal(rw.key.reshape(B, M, S)[:, :, 0] >= 0, sel.prop >= 0)      # a key row exactly where the slot counts
    np.testing.assert_array_equal(out["scst_key"].cpu().numpy(), sel.key)
    A64, _ = SC.advantage(rw.cider, base, count, S)
    assert np.abs(adv.reshape(-1) - A64).max() <= 2.0 ** -24 * np.abs(A64).max() + CIDER_TOL
    assert (adv.reshape(B * M, S)[~count] == 0).all()
    # the referred object's match keeps its meaning
    assert torch.equal(out["match_idx"], matched["ce_before"][0]["match_idx"])


def test_matched_forward_loss_and_gradients(matched):
    out, grads = matched["scst"]
    rw, base, live = matched["rw"], matched["base"], matched["live"]
    o64, v64, g64 = matched["scst64"]
    ref = SC.loss(o64["lang_cap"].detach().numpy(), matched["samples"], rw.length, rw.cider, base, matched["count"], S_SAMPLES)
    loss = float(out["_cap_loss"][0].detach())
    assert abs(float(v64) - ref.loss) <= LR.F64_BAR * max(1.0, ref.labs)
    e = abs(loss - ref.loss) / (LR.CAP_LOSS_REL * max(1.0, ref.labs))
    print(f"loss {loss:.7g} vs float64 {ref.loss:.7g} (scale {ref.labs:.3g}): excess {e:.3g}")
    row_dev = np.abs(out["scst_logp"].detach().cpu().numpy().reshape(-1).astype(np.float64) - ref.rowlogp)[live]
    print(f"largest |scst_logp - float64 row sum| over the filled groups: {row_dev.max():.3e} (sums down to {ref.rowlogp.min():.1f})")
    assert e <= 1
    assert torch.equal(matched["scst_again"], out["_cap_loss"][0].detach())
    ce_g, ce64_g = matched["ce_before"][1], matched["ce64"][2]
    bad = []
    for k in GRAD_TENSORS:
        f_ce = LR.figure(ce_g[k].cpu().numpy(), ce64_g[k].numpy())
        f_sc = LR.figure(grads[k].cpu().numpy(), g64[k].numpy())
        print(f"{k}: cross-entropy path {f_ce:.3e}, matched self-critical path {f_sc:.3e} (allowed {4 * f_ce:.3e}); "
              f"largest reference entry {float(g64[k].abs().max()):.3e}")
        if not f_sc <= 4 * f_ce:
            bad.append(k)
    dev = (grads["aggregated_vote_features"].cpu().double() - g64["aggregated_vote_features"]).abs().amax(-1)
    print(f"aggregated_vote_features: largest deviation per scene {dev.amax(1).tolist()}, at proposals {dev.argmax(1).tolist()}; "
          f"selected {matched['sel'].prop.tolist()}")
    assert not bad, bad


def test_defaults_are_untouched_by_a_matched_run(matched):
    (o0, g0), (o1, g1) = matched["referred_before"], matched["referred_after"]
    assert torch.equal(o0["_cap_loss"][0], o1["_cap_loss"][0]) and torch.equal(o0["scst_samples"], o1["scst_samples"])
    assert tuple(o0["scst_reward"].shape) == (matched["B"], S_SAMPLES) and "scst_proposal" not in o0
    for k in GRAD_TENSORS:
        assert torch.equal(g0[k], g1[k]), k
    (o0, g0), (o1, g1) = matched["ce_before"], matched["ce_after"]
    assert matched["cap"].self_critical is None
    for k in ("lang_cap", "_cap_vec", "match_idx", "good_bbox_masks", "pred_ious"):
        assert torch.equal(o0[k], o1[k]), k
    assert torch.equal(o0["_cap_loss"][0], o1["_cap_loss"][0]) and torch.equal(o0["_cap_loss"][1], o1["_cap_loss"][1])
    for k in GRAD_TENSORS:
        assert torch.equal(g0[k], g1[k]), k
    assert not any(k.startswith("scst_") for k in o1)


def test_a_batch_without_its_labels_is_refused(matched):
    cap, ep = matched["cap"], matched["ep"]
    cap.self_critical = matched["mk"]("matched")
    try:
        for k in ("scene_object_ids", "center_label", "box_label_mask", "dataset_idx"):
            with pytest.raises(KeyError, match=k):
                cap.forward_train({n: v for n, v in ep.items() if n != k})
        cap.forward_train({n: v for n, v in ep.items() if n != "object_id"})          # not read in this mode
    finally:
        del cap.self_critical


# ---- (d) Trainer -----------------------------------------------------------------------------------------------------------
def test_trainer_steps_eagerly_in_matched_mode():
    from spacap3d_amd import synthetic as SY
    from spacap3d_amd.caption_eval import CaptionCorpus
    from spacap3d_amd.engine import Trainer, synthetic_batch
    from spacap3d_amd.self_critical import SelfCritical
    from spacap3d_amd.spacapnet import build_default
    torch.manual_seed(0)
    model = build_default(vocab_size=120, num_proposal=32, N=2, d_ff=256).to(DEV).train()
    data = synthetic_batch(2, 4096, DEV, seed=0, vocab=120)
    with torch.no_grad():
        probe = model(dict(data))
    data = SY.anchor_boxes_on_proposals(data, probe["aggregated_vote_xyz"])
    B, G = data["box_label_mask"].shape
    data["dataset_idx"] = torch.arange(B, device=DEV)
    data["scene_object_ids"] = (torch.arange(G, device=DEV) + ID_OFFSET).repeat(B, 1)
    cap = model.caption
    idx2word = {i: w for w, i in cap.word_to_idx.items()}
    rng = np.random.default_rng(3)
    nkeys = 2 * B
    corpus = {"k%d" % i: ["sos " + " ".join(idx2word[int(t)] for t in rng.integers(4, 120, 12)) + " eos" for _ in range(2)] for i in range(nkeys)}
    table = np.full((B, G + ID_OFFSET), -1, np.int32)
    for i in range(nkeys):
        table[i % B, ID_OFFSET + 2 * (i // B)] = i
    cap.self_critical = SelfCritical(CaptionCorpus(corpus, cap.word_to_idx, key_of=table), cap.word_to_idx["sos"], cap.word_to_idx["eos"],
                                     num_samples=3, seed=11, proposals="matched", max_proposals=3)
    tr = Trainer(model, SY.mean_size_arr().numpy())
    w_cap, w_det = cap.model.generator.proj.weight, model.proposal.proposal[-1].weight
    before = (w_cap.detach().clone(), w_det.detach().clone())
    losses = []
    for _ in range(2):
        tr.step(data)
        losses.append({k: float(v) for k, v in tr.last_losses.items()})
    print(f"two eager matched self-critical steps: {losses}")
    assert tr.graph is None
    assert all(np.isfinite(v) for h in losses for v in h.values())
    assert not torch.equal(before[0], w_cap) and not torch.equal(before[1], w_det)
