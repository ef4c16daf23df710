"""Cross-entropy caption training over every matched object of a scene on the MI355X: the target kernel
(csrc/dense_xe.hip) against its restatement (tests/dense_xe_restated.py) bit for bit through the C ABI and under graph replay,
the dense training forward end to end against float64 autograd on the CPU oracle backend (the construction and the margins of
tests/test_scene_scst_gpu.py's ``run64``), its reduction to the plain training forward, dropout under fixed seeds, the refusals
and two eager ``Trainer`` steps.  The largest figures are printed."""
import copy

import numpy as np
import pytest
import torch

import dense_xe_restated as DX
import losses_restated as LR
import scene_scst_restated as SS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True, scope="module")
def _needs_a_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _up(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _ids(case):
    return "-".join(str(v) for v in case)


@pytest.fixture(scope="module")
def hand():
    from spacap3d_amd.caption_eval import CaptionCorpus
    corpus, w2i = DX.hand_corpus()
    return CaptionCorpus(corpus, w2i, key_of=np.arange(len(corpus), dtype=np.int32).reshape(1, -1))


def _restated(cc, key, r, seed, word, unk=DX.UNK, sos=DX.SOS, eos=DX.EOS):
    return DX.targets(key, cc.ref_tok, cc.ref_off, cc.ref_len, cc.key_ref_off, cc.n_vocab, unk, sos, eos, r, DX.T_IDS, seed, word)


def _assert_targets(got, want, what):
    for name, g, w in zip(DX.Targets._fields, got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


# ---- (a) the target kernel through the C ABI -------------------------------------------------------------------------------
@pytest.mark.parametrize("word", DX.DEVICE_WORDS, ids=lambda w: f"dev{w}")
@pytest.mark.parametrize("case", DX.TARGET_CASES, ids=_ids)
def test_target_kernel_equals_the_restatement(hand, case, word):
    """All five outputs, poisoned before the call, over keys with 0, 1, 2, 3, 7 and 9 references, -1, a scene without a key, a
    key in two scenes and one behind the table; the device word absent, 0 and 2^33 + 5."""
    from spacap3d_amd._native import check, lib
    B, M, r = case
    T, R = DX.T_IDS, B * M * r
    c = hand.on(torch.device(DEV))
    key = _up(DX.key_array(case))
    dev_word = None if word is None else torch.tensor([word], dtype=torch.int64, device=DEV)
    tok = torch.full((R, T + 1), -7, dtype=torch.int64, device=DEV)
    ids = torch.full((R, T), -7, dtype=torch.int64, device=DEV)
    ref = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    good = torch.full((R,), 7, dtype=torch.uint8, device=DEV)
    length = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    check(lib.spacap_dense_xe_targets_i64(key.data_ptr(), B, M, c["ref_tok"].data_ptr(), c["ref_tok"].numel(), c["ref_off"].data_ptr(),
                                          c["ref_len"].data_ptr(), c["ref_len"].numel(), c["key_ref_off"].data_ptr(), hand.nkeys,
                                          hand.n_vocab, DX.UNK, DX.SOS, DX.EOS, r, T, DX.HOST_SEED,
                                          None if dev_word is None else dev_word.data_ptr(), ids.data_ptr(), tok.data_ptr(),
                                          ref.data_ptr(), good.data_ptr(), length.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), "spacap_dense_xe_targets_i64")
    want = _restated(hand, DX.key_array(case), r, DX.HOST_SEED, word)
    _assert_targets((tok, ids, ref, good, length), want, f"{case} device word {word}")
    assert R == 1 or ((want.good == 1).any() and (want.good == 0).any())


def test_targets_method_equals_the_c_abi_and_refuses_bad_arguments(hand):
    from spacap3d_amd.dense_xe import DenseCaptionXE
    case = (2, 16, 3)
    dx = DenseCaptionXE(hand, DX.SOS, DX.EOS, DX.UNK, max_proposals=16, refs_per_object=3, seed=DX.HOST_SEED)
    key = _up(DX.key_array(case))
    _assert_targets(dx.targets(key), _restated(hand, DX.key_array(case), 3, DX.HOST_SEED, None), "targets()")
    with pytest.raises(RuntimeError, match="int32"):
        dx.targets(key.long())
    with pytest.raises(RuntimeError, match="out must"):
        dx.targets(key, out=tuple(torch.empty(1, device=DEV) for _ in range(5)))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        dx.targets(key.cpu())


# ---- (b) under graph replay ------------------------------------------------------------------------------------------------
def test_a_captured_launch_replays_and_draws_anew_after_advance_rng(hand):
    """The ``targets`` launch alone in a graph on one stream.  An integer seed: two replays are equal.  seed=None: equal without
    ``advance_rng``, different after it (nine groups with 2 .. 9 references: all of them keep their first reference with
    probability 3e-6), every replay the restatement's rows at the host word of the capture and the device word read back."""
    from spacap3d_amd import attention
    from spacap3d_amd.dense_xe import DenseCaptionXE
    case = (2, 16, 3)
    B, M, r = case
    R, T = B * M * r, DX.T_IDS
    key_h = DX.key_array(case)
    key = _up(key_h)
    word = attention.rng_state(torch.device(DEV))       # (exists before the capture: its first use allocates and zeroes it)
    word_saved = word.clone()
    assert sum(DX.REFS_PER_KEY[k] >= 2 for k in key_h.reshape(-1) if k >= 0) == 9

    def capture(dx):
        out = (torch.zeros(R, T + 1, dtype=torch.int64, device=DEV), torch.zeros(R, T, dtype=torch.int64, device=DEV),
               torch.zeros(R, dtype=torch.int32, device=DEV), torch.zeros(R, dtype=torch.uint8, device=DEV),
               torch.zeros(R, dtype=torch.int32, device=DEV))
        dx.targets(key, out=out)                         # (uploads the corpus outside the capture)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            dx.targets(key, out=out)
        return g, out, attention._CALL_COUNTER[0]

    def replay(g, out):
        for t in out:
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        return tuple(t.clone() for t in out)

    g, out, _ = capture(DenseCaptionXE(hand, DX.SOS, DX.EOS, DX.UNK, max_proposals=M, refs_per_object=r, seed=77))
    first, second = replay(g, out), replay(g, out)
    attention.advance_rng(torch.device(DEV))
    third = replay(g, out)
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(first, second, third))
    _assert_targets(first, _restated(hand, key_h, r, 77, None), "an integer seed")

    g, out, host = capture(DenseCaptionXE(hand, DX.SOS, DX.EOS, DX.UNK, max_proposals=M, refs_per_object=r, seed=None))
    w0 = int(word.item())
    first, second = replay(g, out), replay(g, out)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    _assert_targets(first, _restated(hand, key_h, r, host, w0), "seed=None")
    attention.advance_rng(torch.device(DEV))
    w1 = int(word.item())
    third = replay(g, out)
    assert w1 == w0 + 1 and not torch.equal(first[2], third[2])
    _assert_targets(third, _restated(hand, key_h, r, host, w1), "seed=None after advance_rng")
    word.copy_(word_saved)


# ---- (c) the training forward ----------------------------------------------------------------------------------------------
B_, K_, M_, R_, G_, VOCAB, NEAR = 2, 19, 3, 2, 8, 37, 0.3
SEED, XE_SEED, ID_OFFSET = 0, 20261021, 3
# key rows per (scene, object slot): scene 0 holds four qualifying objects (one more than M), the two nearest on ONE proposal;
# scene 1 two -- one with a single sentence (its second row is empty), one with none at all -- and an empty slot
KEYED = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (0, 3): 3, (1, 0): 4, (1, 1): 5}
N_REFS = (3, 2, 7, 9, 1, 0)
GRAD_SKIP = ("src_attn", "sublayer.1.", "self_attn.linears.1.bias")


def _grad_leaves(cap):
    """The embedding, every decoder parameter the early guide uses and the generator's two.  Left out, by reasoning and not by
    result: the cross-attention modules and their sublayer norms (never called with the early guide: no gradient at all) and
    the key projections' bias, whose gradient is identically zero in exact arithmetic (a constant added to every key of a row
    moves no softmax), so that its figure would compare one rounding residue with another."""
    leaves = {"embedding": cap.model.tgt_embed[0].lut.weight, "generator.proj.weight": cap.model.generator.proj.weight,
              "generator.proj.bias": cap.model.generator.proj.bias}
    for n, p in cap.model.decoder.named_parameters():
        if not any(s in n for s in GRAD_SKIP):
            leaves["decoder." + n] = p
    return leaves


def _run(cap, ep_base):
    """One forward_train + backward of the captioner on a fresh leaf of the proposal features: (output dict, gradients)."""
    for p in cap.parameters():
        p.grad = None
    feat = ep_base["aggregated_vote_features"].detach().clone().requires_grad_(True)
    out = cap.forward_train(dict(ep_base, aggregated_vote_features=feat))
    out["_cap_loss"][0].backward()
    grads = {k: p.grad.detach().clone() for k, p in _grad_leaves(cap).items()}
    grads["aggregated_vote_features"] = feat.grad.detach().clone()
    return out, grads


def _cpu_copy(cap):
    for m in cap.modules():
        if hasattr(m, "attn") and hasattr(m, "keep_value"):
            m.attn, m.value = None, None
    return copy.deepcopy(cap).cpu()


def _captioner(dropout=0.0):
    from spacap3d_amd import synthetic as SY
    from spacap3d_amd.transformer_captioner import TransformerDecoderModel
    torch.manual_seed(SEED)
    cap = TransformerDecoderModel(SY.make_vocabulary(VOCAB), N=2, h=8, d_model=128, d_ff=256, transformer_dropout=dropout,
                                  src_pos_type="xyz", use_transformer_encoder=True, early_guide=True)
    for m in cap.modules():                 # (the attention modules keep their own default of 0.1 whatever transformer_dropout says)
        if isinstance(m, torch.nn.Dropout):
            m.p = dropout
    return cap.to(DEV).train()


def _sentences(rng, idx2word, n, lengths=None):
    out = []
    for j in range(n):
        nw = int(lengths[j]) if lengths is not None else int(rng.integers(3, 36))
        words = [idx2word[str(int(t))] for t in rng.integers(4, VOCAB, nw)]
        if j % 2:
            words[int(rng.integers(0, nw))] = f"outside{j}"
        out.append("sos " + " ".join(words) + " eos")
    return out


def _scene_inputs():
    """Proposals at distinct lattice points, features, and the labelled objects of KEYED placed beside their proposals."""
    rng = np.random.default_rng(31)
    k = np.arange(K_)
    xyz = np.stack([k % 5, (k // 5) % 5, np.zeros(K_)], 1).astype(np.float32)[None].repeat(B_, 0)
    xyz = xyz + rng.uniform(-0.05, 0.05, xyz.shape).astype(np.float32)
    center = np.full((B_, G_, 3), 50.0, np.float32)
    mask = np.zeros((B_, G_), np.float32)
    # (scene, slot) -> (proposal, offset along x): distances 0.02 < 0.05 < 0.1 < 0.2 in scene 0, the nearest two on proposal 7
    place = {(0, 0): (7, 0.02), (0, 1): (7, -0.05), (0, 2): (12, 0.1), (0, 3): (3, 0.2), (1, 0): (5, 0.03), (1, 1): (16, 0.06),
             (1, 2): (9, 0.01), (0, 4): (1, 0.29)}          # (1, 2) and (0, 4) have no key row; (0, 5) lies too far away
    for (b, j), (p, dx) in place.items():
        center[b, j] = xyz[b, p] + np.array([dx, 0, 0], np.float32)
        mask[b, j] = 1
    center[0, 5], mask[0, 5] = xyz[0, 2] + np.array([0.4, 0, 0], np.float32), 1
    table = np.full((B_, G_ + ID_OFFSET), -1, np.int32)
    for (b, j), row in KEYED.items():
        table[b, j + ID_OFFSET] = row
    table[0, 5 + ID_OFFSET] = 2                              # a key row, but no proposal within the threshold
    feat = rng.normal(0, 1, (B_, K_, 128)).astype(np.float32)
    return xyz, center, mask, table, feat


@pytest.fixture(scope="module")
def trained():
    """Everything the checks of (c) and (e) share, computed once: the plain forward before the attribute was ever set, the dense
    forward (twice), the plain forward afterwards, and the float64 oracles on the CPU oracle backend."""
    from oracle.attention_ref import OracleBackend
    from spacap3d_amd import backend
    from spacap3d_amd.caption_eval import CaptionCorpus
    from spacap3d_amd.dense_xe import DenseCaptionXE
    from spacap3d_amd.loss_helper import compute_cap_loss
    cap = _captioner()
    w2i = cap.word_to_idx
    sos, eos, unk = w2i["sos"], w2i["eos"], w2i["unk"]
    rng = np.random.default_rng(32)
    corpus = {"k%d" % i: _sentences(rng, cap.vocabulary["idx2word"], n) for i, n in enumerate(N_REFS)}
    xyz, center, mask, table, feat = _scene_inputs()
    cc = CaptionCorpus(corpus, w2i, key_of=table)
    gt = DX.sentence_row(corpus["k0"][0], w2i)                              # the plain path's caption: any sentence will do
    lang_ids = np.stack([gt, DX.sentence_row(corpus["k3"][4], w2i)])
    ep = {"aggregated_vote_features": _up(feat), "aggregated_vote_xyz": _up(xyz), "bbox_mask": torch.ones(B_, K_, dtype=torch.long, device=DEV),
          "center_label": _up(center), "box_label_mask": _up(mask), "ref_center_label": _up(center[:, 0]),
          "scene_object_ids": (torch.arange(G_, device=DEV) + ID_OFFSET).repeat(B_, 1), "dataset_idx": torch.arange(B_, device=DEV),
          "lang_ids": _up(lang_ids), "lang_label": _up(np.concatenate([np.ones((B_, 1), np.int64), lang_ids], 1))}
    res = {"cap": cap, "ep": ep, "cc": cc, "corpus": corpus, "table": table, "xyz": xyz, "words": (sos, eos, unk)}
    mk = lambda seed=XE_SEED, **kw: DenseCaptionXE(cc, sos, eos, unk, **dict(dict(max_proposals=M_, near_threshold=NEAR,
                                                                                  refs_per_object=R_, seed=seed), **kw))
    res["mk"] = mk
    res["sel"] = sel = SS.select(xyz, center, mask, ep["scene_object_ids"].cpu().numpy(), np.arange(B_), table, cc.nkeys, NEAR, M_)
    res["tg"] = tg = _restated(cc, sel.key, R_, XE_SEED, None, unk, sos, eos)
    res["plain_before"] = _run(cap, ep)
    assert cap.dense_xe is None
    try:
        cap.dense_xe = mk()
        res["dense"] = _run(cap, ep)
        res["dense_again"] = _run(cap, ep)[0]["_cap_loss"][0].detach().clone()
        # a scene with no qualifying object: scene 1's labels switched off
        off = dict(ep, box_label_mask=_up(mask * np.array([[1.0], [0.0]], np.float32)))
        res["scene_off"] = _run(cap, off)
    finally:
        del cap.dense_xe
    res["plain_after"] = _run(cap, ep)

    # float64 on the CPU oracle backend: the plain rows, then the B M r dense rows with the scenes repeated evenly (the position
    # embedding of the encoder holds a BatchNorm1d in training mode: evenly repeated scenes keep the statistics of the B scenes)
    cap64 = _cpu_copy(cap).double().train()
    ep64 = {k: (ep[k].cpu().double() if ep[k].is_floating_point() else ep[k].cpu())
            for k in ("aggregated_vote_features", "aggregated_vote_xyz", "bbox_mask", "ref_center_label", "lang_label", "lang_ids")}

    def run64(rows_scene, ep_rows, loss_of, extra=None):
        for p in cap64.parameters():
            p.grad = None
        feat64 = ep64["aggregated_vote_features"].clone().requires_grad_(True)
        e = {k: v[rows_scene] for k, v in dict(ep64, aggregated_vote_features=feat64).items()}
        e.update(ep_rows)
        with backend.use_backend(OracleBackend()):
            o = cap64.forward_train(e)
            value, acc = loss_of(o)
            more = extra(o, feat64) if extra is not None else None
            value.backward()
        g = {k: p.grad.clone() for k, p in _grad_leaves(cap64).items()}
        g["aggregated_vote_features"] = feat64.grad.clone()
        return o, (value.detach(), acc.detach()), g, more

    res["run64"] = run64
    res["plain64"] = run64(torch.arange(B_), {}, compute_cap_loss)
    grp = np.arange(B_ * M_ * R_) // R_
    prop = sel.prop.reshape(-1)[grp]
    good = torch.from_numpy(tg.good.astype(bool))

    def dense_loss(o):
        o["good_bbox_masks"] = good                         # the plain formula with the rows in the place of the scenes
        return compute_cap_loss(o)

    def per_group(o, feat64):
        """d(sum of a group's cross-entropies / the loss's denominator) / d features, for the groups of scene 0"""
        lp, tgt = o["lang_cap"], o["lang_ids"][:, 1:o["lang_cap"].shape[1] + 1]
        ce = -(lp.gather(2, tgt.unsqueeze(-1)).squeeze(-1) * (tgt != 0)).sum(1) * good
        den = good.sum() * lp.shape[1] + 1e-6
        return [torch.autograd.grad(ce[m * R_:(m + 1) * R_].sum() / den, feat64, retain_graph=True)[0] for m in range(M_)]

    rows = {"lang_label": torch.from_numpy(tg.tok), "lang_ids": torch.from_numpy(tg.ids),
            "ref_center_label": torch.from_numpy(xyz[grp // M_, np.maximum(prop, 0)]).double()}
    res["dense64"] = run64(torch.from_numpy(grp // M_), rows, dense_loss, per_group)
    live = tg.good.astype(bool)
    assert torch.equal(res["dense64"][0]["match_idx"][torch.from_numpy(live)], torch.from_numpy(prop[live]))
    return res


def test_dense_forward_selection_references_and_outputs(trained):
    out, sel, tg, cc = trained["dense"][0], trained["sel"], trained["tg"], trained["cc"]
    B, M, r, T = B_, M_, R_, DX.T_IDS
    # what the inputs are built to contain, in the restatements
    assert sel.n_sel.tolist() == [3, 2] and sel.prop[0, 0] == sel.prop[0, 1] == 7 and sel.slot_of[0].tolist() == [0, 1, 2]
    assert sel.key[1].tolist() == [4, 5, -1]
    np.testing.assert_array_equal(tg.good.reshape(B, M, r), np.array([[[1, 1]] * 3, [[1, 0], [0, 0], [0, 0]]], np.uint8))
    assert (tg.ids >= VOCAB).sum() == 0 and (tg.ids == trained["words"][2]).any() and (cc.ref_len > T).any()
    assert "lang_cap" not in out and "_cap_vec" not in out
    for k, shape, dtype in (("dense_proposal", (B, M), torch.int64), ("dense_object_id", (B, M), torch.int64),
                            ("dense_key", (B, M), torch.int32), ("dense_ref", (B, M, r), torch.int32),
                            ("dense_count", (B, M, r), torch.bool), ("dense_length", (B, M, r), torch.int32),
                            ("dense_lang_ids", (B, M, r, T), torch.int64)):
        assert tuple(out[k].shape) == shape and out[k].dtype == dtype, k
    np.testing.assert_array_equal(out["dense_proposal"].cpu().numpy(), sel.prop)
    np.testing.assert_array_equal(out["dense_object_id"].cpu().numpy(), sel.obj)
    np.testing.assert_array_equal(out["dense_key"].cpu().numpy(), sel.key)
    np.testing.assert_array_equal(out["dense_ref"].cpu().numpy().reshape(-1), tg.ref)
    np.testing.assert_array_equal(out["dense_count"].cpu().numpy().reshape(-1), tg.good.astype(bool))
    np.testing.assert_array_equal(out["dense_length"].cpu().numpy().reshape(-1), tg.length)
    np.testing.assert_array_equal(out["dense_lang_ids"].cpu().numpy().reshape(-1, T), tg.ids)
    # the sentences are the corpus's, as the reference's dataset would lay them out
    sents = [s for v in trained["corpus"].values() for s in v]
    for row in np.flatnonzero(tg.good):
        np.testing.assert_array_equal(tg.ids[row], DX.sentence_row(sents[tg.ref[row]], trained["cap"].word_to_idx))
    # the referred object's match keeps its meaning
    plain = trained["plain_before"][0]
    assert torch.equal(out["match_idx"], plain["match_idx"]) and torch.equal(out["good_bbox_masks"], plain["good_bbox_masks"])
    assert torch.equal(out["pred_ious"], plain["pred_ious"])
    # the decoder input of these rows is the restated one (dropout 0)
    from spacap3d_amd.caption_prep import caption_prep_rows
    cap, ep = trained["cap"], trained["ep"]
    te = cap.model.tgt_embed
    with torch.no_grad():
        src = ep["aggregated_vote_features"]
        memory = cap.model.encode(src, cap._src_pos(ep), ep["bbox_mask"].unsqueeze(1))
        x0, m8 = caption_prep_rows(src, memory, _up(sel.prop), _up(tg.tok), te[0], te[1], r)
    want_x0, want_m = SS.prep_rows_fwd(src.cpu().numpy(), memory.cpu().numpy(), sel.prop, tg.tok, te[0].lut.weight.detach().cpu().numpy(),
                                       te[1].pe[0].cpu().numpy(), M, r)
    np.testing.assert_array_equal(x0.cpu().numpy(), want_x0)
    np.testing.assert_array_equal(m8.cpu().numpy(), want_m)


def test_dense_forward_loss_accuracy_and_gradients(trained):
    (out, grads), (o64, (v64, a64), g64, _) = trained["dense"], trained["dense64"]
    loss, acc = float(out["_cap_loss"][0].detach()), float(out["_cap_loss"][1].detach())
    e = abs(loss - float(v64)) / (LR.CAP_LOSS_REL * max(1.0, abs(float(v64))))
    print(f"dense loss {loss:.7g} vs float64 {float(v64):.7g}: excess {e:.3g}; accuracy {acc:.7g} vs {float(a64):.7g}")
    p_loss, p64 = float(trained["plain_before"][0]["_cap_loss"][0].detach()), float(trained["plain64"][1][0])
    print(f"plain loss {p_loss:.7g} vs float64 {p64:.7g}: excess {abs(p_loss - p64) / (LR.CAP_LOSS_REL * max(1.0, abs(p64))):.3g}")
    assert e <= 1 and abs(acc - float(a64)) <= LR.CAP_ACC_ABS
    assert torch.equal(trained["dense_again"], out["_cap_loss"][0].detach())
    ce_g, ce64_g = trained["plain_before"][1], trained["plain64"][2]
    assert set(grads) == set(g64) and len(grads) >= 20
    bad = []
    for k in grads:
        f_ce = LR.figure(ce_g[k].cpu().numpy(), ce64_g[k].numpy())
        f_dx = LR.figure(grads[k].cpu().numpy(), g64[k].numpy())
        print(f"{k}: plain path {f_ce:.3e}, dense path {f_dx:.3e} (allowed {4 * f_ce:.3e}); largest reference entry "
              f"{float(g64[k].abs().max()):.3e}")
        if not f_dx <= 4 * f_ce:
            bad.append(k)
    assert not bad, bad


def test_a_shared_proposal_receives_the_sum_and_an_empty_scene_nothing(trained):
    (out, grads), (_, _, g64, groups) = trained["dense"], trained["dense64"]
    sel = trained["sel"]
    p = int(sel.prop[0, 0])
    got = grads["aggregated_vote_features"][0, p].cpu().double()
    # float64, per group of scene 0: the two objects on this proposal reach it through its own indicator row, the third group
    # only through the encoder (its proposal's memory row attends to every token of the scene)
    a, b, c = (g[0, p] for g in groups)
    scale = float(g64["aggregated_vote_features"].abs().max())
    f_ce = LR.figure(trained["plain_before"][1]["aggregated_vote_features"].cpu().numpy(), trained["plain64"][2]["aggregated_vote_features"].numpy())
    e_sum, e_a, e_b = (float((got - t).abs().max()) / scale for t in (a + b + c, a + c, b + c))
    print(f"proposal {p} of scene 0, matched by two objects: deviation from the sum of both {e_sum:.3e}, with one of them left out "
          f"{e_a:.3e} / {e_b:.3e} (of the largest entry; allowed {4 * f_ce:.3e}); the third group's share {float(c.abs().max()) / scale:.3e}")
    assert float(a.abs().max()) > 0 and float(b.abs().max()) > 0
    assert e_sum <= 4 * f_ce and e_a > 100 * e_sum and e_b > 100 * e_sum
    # proposals nobody selected receive exact zeros through the indicator; scene 1 with its labels off: zeros, a finite loss
    off_out, off_g = trained["scene_off"]
    assert (off_out["dense_proposal"][1] == -1).all() and not bool(off_out["dense_count"][1].any())
    assert bool(off_out["dense_count"][0].all())
    assert np.isfinite(float(off_out["_cap_loss"][0].detach())) and float(off_out["_cap_loss"][0].detach()) > 0
    assert float(off_g["aggregated_vote_features"][1].abs().max()) == 0.0
    assert float(off_g["aggregated_vote_features"][0].abs().max()) > 0.0


# ---- (d) reduction to the plain path ---------------------------------------------------------------------------------------
def test_one_object_one_reference_is_the_plain_forward(trained):
    """One annotated object per scene, the referred one, with one reference equal to lang_ids; M = 1, r = 1: the dense rows are
    the plain forward's rows, and both losses and accuracies lie within the margin of ONE float64 value."""
    from spacap3d_amd.caption_eval import CaptionCorpus
    from spacap3d_amd.dense_xe import DenseCaptionXE
    from spacap3d_amd.loss_helper import compute_cap_loss
    cap, ep, corpus = trained["cap"], trained["ep"], trained["corpus"]
    sos, eos, unk = trained["words"]
    mask = np.zeros((B_, G_), np.float32)
    mask[:, 0] = 1
    one = {"a": [corpus["k2"][1]], "b": [corpus["k3"][5]]}          # both hold a word outside the vocabulary
    table = np.full((B_, G_ + ID_OFFSET), -1, np.int32)
    table[0, ID_OFFSET], table[1, ID_OFFSET] = 0, 1
    ids = np.stack([DX.sentence_row(one["a"][0], cap.word_to_idx), DX.sentence_row(one["b"][0], cap.word_to_idx)])
    e = dict(ep, box_label_mask=_up(mask), lang_ids=_up(ids), lang_label=_up(np.concatenate([np.ones((B_, 1), np.int64), ids], 1)))
    plain, _ = _run(cap, e)
    try:
        cap.dense_xe = DenseCaptionXE(CaptionCorpus(one, cap.word_to_idx, key_of=table), sos, eos, unk, max_proposals=1,
                                      near_threshold=NEAR, refs_per_object=1, seed=3)
        dense, _ = _run(cap, e)
    finally:
        del cap.dense_xe
    assert torch.equal(dense["dense_lang_ids"].view(B_, -1), e["lang_ids"]) and bool(dense["dense_count"].all())
    assert torch.equal(dense["dense_proposal"].view(-1).long(), plain["match_idx"].view(-1).long())
    rows = {"lang_ids": torch.from_numpy(ids), "lang_label": torch.from_numpy(np.concatenate([np.ones((B_, 1), np.int64), ids], 1))}
    _, (v64, a64), _, _ = trained["run64"](torch.arange(B_), rows, compute_cap_loss)
    bar = LR.CAP_LOSS_REL * max(1.0, abs(float(v64)))
    lp, ld = float(plain["_cap_loss"][0]), float(dense["_cap_loss"][0])
    ap, ad = float(plain["_cap_loss"][1]), float(dense["_cap_loss"][1])
    print(f"plain {lp:.9g}, dense {ld:.9g}, float64 {float(v64):.9g} (allowed {bar:.3g}); dense - plain = {ld - lp:.3e}; "
          f"accuracy {ap:.7g} / {ad:.7g} / {float(a64):.7g}")
    assert abs(lp - float(v64)) <= bar and abs(ld - float(v64)) <= bar
    assert abs(ap - float(a64)) <= LR.CAP_ACC_ABS and abs(ad - float(a64)) <= LR.CAP_ACC_ABS


# ---- (e) dropout, and the defaults afterwards ------------------------------------------------------------------------------
def test_dropout_repeats_under_fixed_seeds_and_another_seed_differs(trained):
    """Dropout 0.1: the masks come from the library's host call counter and device step word, the sentences from the mode's
    seed.  From one state of all three, two calls give one loss; another sentence seed gives another."""
    from spacap3d_amd import attention
    cap = _captioner(dropout=0.1)
    ep, mk, sel, cc = trained["ep"], trained["mk"], trained["sel"], trained["cc"]
    sos, eos, unk = trained["words"]
    assert (_restated(cc, sel.key, R_, 11, None, unk, sos, eos).ref != trained["tg"].ref).any()      # other sentences, in the restatement
    saved, word = attention._CALL_COUNTER[0], attention.rng_state(torch.device(DEV)).clone()

    def once(seed):
        attention._CALL_COUNTER[0] = 20261021 << 20
        attention.rng_state(torch.device(DEV)).zero_()
        cap.dense_xe = mk(seed)
        with torch.no_grad():
            return cap.forward_train(dict(ep))["_cap_loss"][0].clone()
    try:
        a, b, c = once(11), once(11), once(XE_SEED)
        cap.dense_xe = None
        attention._CALL_COUNTER[0] = 20261021 << 20
        with torch.no_grad():
            plain = cap.forward_train(dict(ep))
    finally:
        attention._CALL_COUNTER[0] = saved
        attention.rng_state(torch.device(DEV)).copy_(word)
    print(f"dropout 0.1: seed 11 {float(a):.7g} and {float(b):.7g}, seed {XE_SEED} {float(c):.7g}")
    assert torch.equal(a, b) and not torch.equal(a, c) and np.isfinite(float(c))
    assert "dense_proposal" not in plain and "lang_cap" in plain
    dry = _captioner(dropout=0.0)
    dry.load_state_dict(cap.state_dict())                 # the attribute is not in the state dict
    assert dry.dense_xe is None and not any("dense" in k for k in cap.state_dict())


def test_defaults_are_untouched_by_a_dense_run(trained):
    (o0, g0), (o1, g1) = trained["plain_before"], trained["plain_after"]
    assert trained["cap"].dense_xe is None
    for k in ("lang_cap", "_cap_vec", "match_idx", "good_bbox_masks", "pred_ious"):
        assert torch.equal(o0[k], o1[k]), k
    assert torch.equal(o0["_cap_loss"][0], o1["_cap_loss"][0]) and torch.equal(o0["_cap_loss"][1], o1["_cap_loss"][1])
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    assert not any(k.startswith("dense_") for k in o1)
    cap = trained["cap"]
    cap.dense_xe = trained["mk"]()
    try:
        cap.eval()
        with torch.no_grad():
            o2 = cap.forward_train(dict(trained["ep"]))       # read in training mode only
        assert "dense_proposal" not in o2
    finally:
        cap.train()
        del cap.dense_xe


# ---- (f) refusals and the Trainer ------------------------------------------------------------------------------------------
def test_refusals(trained):
    from oracle.attention_ref import OracleBackend
    from spacap3d_amd import backend
    from spacap3d_amd.self_critical import SelfCritical
    cap, ep, cc = trained["cap"], trained["ep"], trained["cc"]
    sos, eos, _ = trained["words"]
    cap.dense_xe = trained["mk"]()
    try:
        for k in ("center_label", "box_label_mask", "scene_object_ids", "dataset_idx", "ref_center_label"):
            with pytest.raises(KeyError, match=k):
                cap.forward_train({n: v for n, v in ep.items() if n != k})
        cap.forward_train({n: v for n, v in ep.items() if n not in ("lang_ids", "lang_label", "object_id")})      # not read in this mode
        cap.self_critical = SelfCritical(cc, sos, eos, num_samples=2)
        try:
            with pytest.raises(ValueError, match="dense_xe and self_critical"):
                cap.forward_train(dict(ep))
        finally:
            del cap.self_critical
        with backend.use_backend(OracleBackend()):
            with pytest.raises(RuntimeError, match="dense_xe.*not supported"):
                cap.forward_train(dict(ep))
        cap.early_guide = False
        try:
            with pytest.raises(RuntimeError, match="dense_xe.*not supported"):
                cap.forward_train(dict(ep))
        finally:
            cap.early_guide = True
        enc, cap.model.encoder = cap.model.encoder, None
        try:
            with pytest.raises(RuntimeError, match="dense_xe.*not supported"):
                cap.forward_train(dict(ep))
        finally:
            cap.model.encoder = enc
    finally:
        del cap.dense_xe


def test_trainer_steps_eagerly_in_dense_mode():
    from spacap3d_amd import synthetic as SY
    from spacap3d_amd.caption_eval import CaptionCorpus
    from spacap3d_amd.dense_xe import DenseCaptionXE
    from spacap3d_amd.engine import Trainer, synthetic_batch
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
    nkeys = 4 * B
    corpus = {"k%d" % i: ["sos " + " ".join(idx2word[int(t)] for t in rng.integers(4, 120, 12)) + " eos" for _ in range(3)] for i in range(nkeys)}
    table = np.full((B, G + ID_OFFSET), -1, np.int32)
    for i in range(nkeys):
        table[i % B, ID_OFFSET + 2 * (i // B)] = i
    w2i = cap.word_to_idx
    cap.dense_xe = DenseCaptionXE(CaptionCorpus(corpus, w2i, key_of=table), w2i["sos"], w2i["eos"], w2i["unk"], max_proposals=3,
                                  refs_per_object=2, seed=None)
    tr = Trainer(model, SY.mean_size_arr().numpy())
    w_cap, w_det = cap.model.generator.proj.weight, model.proposal.proposal[-1].weight
    before = (w_cap.detach().clone(), w_det.detach().clone())
    losses = []
    for _ in range(2):
        tr.step(data)
        losses.append({k: float(v) for k, v in tr.last_losses.items()})
    print(f"two eager dense cross-entropy steps: {losses}")
    assert tr.graph is None
    assert all(np.isfinite(v) for h in losses for v in h.values())
    assert not torch.equal(before[0], w_cap) and not torch.equal(before[1], w_det)
    assert tr.enable_graph(data) is False and "dense_xe" in tr.graph_error and tr.graph is None
