"""Self-critical caption training on the MI355X: the reward kernel (csrc/caption_reward.hip) against the
reference's recorded CIDEr (tests/golden/caption_eval_ref.npz), the loss kernels (csrc/scst_loss.hip) at their dispatch edges
against the float64 restatement (tests/self_critical_restated.py), the training forward end to end against float64 autograd of
the restated loss on the CPU oracle backend, two eager ``Trainer`` steps, and the refusals.  The largest figures are printed."""
import copy

import numpy as np
import pytest
import torch

import caption_eval_restated as R
import losses_restated as LR
import sampling_restated as SR
import self_critical_restated as SC
from test_caption_eval_cpu import FIX, SCORE_CASES, corpus_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CIDER_TOL = 1e-9           # tests/test_caption_eval_gpu.py: the same sums in wave order


@pytest.fixture(autouse=True, scope="module")
def _needs_a_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _up(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the shared case arrays are read-only)


# ---- (a) the reward kernel -------------------------------------------------------------------------------------------------
def _poisoned(rows, L):
    return (torch.full((rows,), float("nan"), dtype=torch.float64, device=DEV), torch.full((rows,), -7, dtype=torch.int32, device=DEV),
            torch.full((rows,), -7, dtype=torch.int32, device=DEV), torch.full((rows, L + 2), -7, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("case", SCORE_CASES)
def test_reward_kernel_against_the_recorded_cider(case):
    """Rows built back from the fixture's candidates (every key 0 to 3 times, the placeholder [sos, eos], with `edge` the 64-token
    candidate), some pointed outside the key table or at a -1 entry: CIDEr within 1e-9 of the recorded cider_scores[key], 0 and
    key -1 without a key row, tf_tok and length exactly, outputs poisoned before the call; a captured call replays with new
    inputs."""
    from spacap3d_amd.caption_eval import CaptionCorpus
    from spacap3d_amd.self_critical import SelfCritical
    tokens, didx, oid, table, want_key, perm = SC.fixture_rows(FIX, case, extra=True)
    corpus, w2i = corpus_of(case)
    sc = SelfCritical(CaptionCorpus(corpus, w2i, key_of=table), R.SOS, R.EOS)
    want = SC.rewards(SC.Corpus(R.refs_of(FIX, case)), tokens, 1, didx, oid, table, R.SOS, R.EOS)
    rows, L = tokens.shape
    out = _poisoned(rows, L)
    got = sc.rewards(_up(tokens), _up(didx), _up(oid), 1, out=out)
    cider, key, length, tf = (t.cpu().numpy() for t in got)
    np.testing.assert_array_equal(key, want_key)
    np.testing.assert_array_equal(length, want.length)
    np.testing.assert_array_equal(tf, want.tf_tok)
    keyed = want_key >= 0
    share = 1.0 - keyed.mean()
    uses = np.bincount(perm, minlength=len(FIX[f"{case}/cand_len"]))
    print(f"{case}: {rows} rows, {share:.3f} without a key row, keys used {uses.min()} to {uses.max()} times")
    assert 0 < share < 0.25 and uses.min() == 0 and uses.max() == 3
    assert (cider[~keyed] == 0).all()
    err = np.abs(cider[keyed] - FIX[f"{case}/cider_scores"][want_key[keyed]])
    print(f"{case}: largest |reward - recorded CIDEr| = {err.max():.3e}; against the restatement {np.abs(cider - want.cider).max():.3e}")
    assert err.max() <= CIDER_TOL
    assert length[-1] == 1 and list(tf[-1, :3]) == [R.SOS, R.EOS, 0]                    # the placeholder
    if case == "edge":
        assert (length == SC.L_WORDS).any()                                               # 62 words, no eos

    # two rows per scene, captured; the replay sees other tokens and other scenes
    n = (rows // 4) * 2
    st_tok, st_idx, st_oid = _up(tokens[:n]), _up(didx[0:n:2]), _up(oid[0:n:2])
    st_out = _poisoned(n, L)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sc.rewards(st_tok, st_idx, st_oid, 2, out=st_out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sc.rewards(st_tok, st_idx, st_oid, 2, out=st_out)
    st_tok.copy_(_up(tokens[n:2 * n]))
    st_idx.copy_(_up(didx[n:2 * n:2]))
    st_oid.copy_(_up(oid[n:2 * n:2]))
    for t, v in zip(st_out, _poisoned(n, L)):
        t.copy_(v)
    g.replay()
    torch.cuda.synchronize()
    want2 = SC.rewards(SC.Corpus(R.refs_of(FIX, case)), tokens[n:2 * n], 2, didx[n:2 * n:2], oid[n:2 * n:2], table, R.SOS, R.EOS)
    np.testing.assert_array_equal(st_out[1].cpu().numpy(), want2.key)
    np.testing.assert_array_equal(st_out[3].cpu().numpy(), want2.tf_tok)
    assert np.abs(st_out[0].cpu().numpy() - want2.cider).max() <= CIDER_TOL and (want2.cider > 0).any()


def test_reward_equals_the_scorer_bit_for_bit():
    """The same caption as its key's candidate through spacap_caption_score_f64: the same bits (one definition of the sums)."""
    from spacap3d_amd.caption_eval import CaptionCorpus, CaptionEval
    from spacap3d_amd.self_critical import SelfCritical
    case = "random"
    tokens, didx, oid, table, want_key, perm = SC.fixture_rows(FIX, case)
    corpus, w2i = corpus_of(case)
    cc = CaptionCorpus(corpus, w2i, key_of=table)
    cider = SelfCritical(cc, R.SOS, R.EOS).rewards(_up(tokens), _up(didx), _up(oid))[0]
    ce = CaptionEval(cc, R.SOS, R.EOS)
    ce.set_candidates(_up(FIX[f"{case}/cand_tok"]), _up(FIX[f"{case}/cand_len"]))
    assert torch.equal(cider, ce.scores()["cider"][_up(perm)])


# ---- (b) the loss kernels --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.LOSS_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_loss_kernels_at_their_dispatch_edges(case):
    from spacap3d_amd._native import check, lib
    x, ref = SC.loss_inputs(case), SC.loss_reference(case)
    Rn, S, W, V = case.R, case.S, case.W, case.V
    st = torch.cuda.current_stream().cuda_stream
    logits, words, length, reward = _up(x.logits), _up(x.words), _up(x.length), _up(x.reward)
    base = _up(x.baseline) if x.baseline is not None else None
    count = _up(x.count.astype(np.uint8))
    nan = float("nan")
    pair, hit = torch.full((Rn, W, 2), nan, device=DEV), torch.full((Rn, W), 9, dtype=torch.uint8, device=DEV)
    adv, rowlogp, out = torch.full((Rn,), nan, device=DEV), torch.full((Rn,), nan, device=DEV), torch.full((8,), nan, device=DEV)
    dlogits = torch.full((Rn, W, V), nan, device=DEV)
    gl = torch.tensor([SC.LOSS_UPSTREAM], device=DEV)
    check(lib.spacap_scst_loss_fwd_f32(logits.data_ptr(), words.data_ptr(), length.data_ptr(), reward.data_ptr(),
                                       base.data_ptr() if base is not None else None, count.data_ptr(), Rn, S, W, V, pair.data_ptr(),
                                       hit.data_ptr(), adv.data_ptr(), rowlogp.data_ptr(), out.data_ptr(), st), "spacap_scst_loss_fwd_f32")
    check(lib.spacap_scst_loss_bwd_f32(logits.data_ptr(), words.data_ptr(), length.data_ptr(), pair.data_ptr(), adv.data_ptr(),
                                       out.data_ptr(), gl.data_ptr(), Rn, W, V, dlogits.data_ptr(), st), "spacap_scst_loss_bwd_f32")
    torch.cuda.synchronize()
    o, a, rl, d = out.cpu().numpy().astype(np.float64), adv.cpu().numpy(), rowlogp.cpu().numpy(), dlogits.cpu().numpy()
    e_loss = abs(o[0] - ref.loss) / (LR.CAP_LOSS_REL * max(1.0, ref.labs))
    e_acc = abs(o[1] - ref.acc) / LR.CAP_ACC_ABS
    e_adv = float((np.abs(a.astype(np.float64) - ref.adv) / np.maximum(2.0 ** -24 * np.abs(ref.adv), 1e-300)).max())
    bar = LR.CAP_GRAD_REL * max(float(np.abs(ref.dlogits).max()), 1e-6) + LR.CAP_GRAD_ABS
    e_grad = float(np.abs(d - ref.dlogits).max()) / bar
    e_row = float(np.abs(rl - ref.rowlogp).max()) / (W * LR.CAP_LOGP_ABS)
    print(f"excess (at most 1): loss {e_loss:.3g}  acc {e_acc:.3g}  adv {e_adv:.3g}  dlogits {e_grad:.3g}  rowlogp {e_row:.3g}"
          f"   loss {o[0]:.6g} vs {ref.loss:.6g} (scale {ref.labs:.3g})")
    assert np.isfinite(o).all() and np.isfinite(d).all() and np.isfinite(a).all() and np.isfinite(rl).all()
    assert e_loss <= 1 and e_acc <= 1 and e_adv <= 1 and e_grad <= 1 and e_row <= 1
    live = (np.arange(W)[None, :] < x.length[:, None]) & np.repeat(x.count, S)[:, None]
    assert (d[~live] == 0).all()                                     # exact zeros behind length and on scenes that do not count
    z = slice(SC.ZERO_SCENE * S, (SC.ZERO_SCENE + 1) * S)
    assert (a[z] == 0).all() and (d[z] == 0).all()                   # advantage exactly 0
    assert abs(o[2] - ref.inv_den) <= 1e-6 * ref.inv_den and o[3] == ref.n_scenes
    assert abs(o[4] - ref.mean_reward) <= 1e-6 * max(1.0, abs(ref.mean_reward))
    assert abs(o[5] - ref.mean_baseline) <= 1e-6 * max(1.0, abs(ref.mean_baseline)) and o[6] == 0 and o[7] == 0
    if case.count == "none":
        assert o[0] == 0 and not d.any()
    # a second call gives the same bits (fixed-order sums)
    out2 = torch.full((8,), nan, device=DEV)
    check(lib.spacap_scst_loss_fwd_f32(logits.data_ptr(), words.data_ptr(), length.data_ptr(), reward.data_ptr(),
                                       base.data_ptr() if base is not None else None, count.data_ptr(), Rn, S, W, V, pair.data_ptr(),
                                       hit.data_ptr(), adv.data_ptr(), rowlogp.data_ptr(), out2.data_ptr(), st), "spacap_scst_loss_fwd_f32")
    assert torch.equal(out, out2)


# ---- (c) the training forward, end to end ----------------------------------------------------------------------------------
SEED = 0                       # weight seed of the model (tests/test_sampling_gpu.py's)
SAMPLE_SEED = 20261020         # the seed of the samples under test
CORPUS_SEED = 20261021         # another seed: the captions that become the references
S_SAMPLES = 3
GRAD_TENSORS = ("generator.proj.weight", "embedding", "last decoder layer w_2", "aggregated_vote_features")


def _no_dropout(module):
    for m in module.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return module


def _cpu_copy(cap):
    """A deep copy of the captioner on the CPU (the attention modules' kept maps are autograd tensors: dropped first)."""
    for m in cap.modules():
        if hasattr(m, "attn") and hasattr(m, "keep_value"):
            m.attn, m.value = None, None
    return copy.deepcopy(cap).cpu()


def _grad_leaves(cap):
    return {"generator.proj.weight": cap.model.generator.proj.weight, "embedding": cap.model.tgt_embed[0].lut.weight,
            "last decoder layer w_2": cap.model.decoder.layers[-1].feed_forward.w_2.weight}


def _run(cap, ep_base, key="_cap_loss"):
    """One forward_train + backward of the captioner on a fresh leaf of the proposal features: (output dict, gradients)."""
    for p in cap.parameters():
        p.grad = None
    feat = ep_base["aggregated_vote_features"].detach().clone().requires_grad_(True)
    out = cap.forward_train(dict(ep_base, aggregated_vote_features=feat))
    out[key][0].backward()
    grads = {k: p.grad.detach().clone() for k, p in _grad_leaves(cap).items()}
    grads["aggregated_vote_features"] = feat.grad.detach().clone()
    return out, grads


def _sentences(words, idx2word, sos, eos):
    return " ".join(idx2word[int(t)] for t in R.decode(words, sos, eos))


@pytest.fixture(scope="module")
def trained():
    """The model and scenes of tests/test_sampling_gpu.py in train() mode with dropout 0, the corpus (captions of the matched
    proposals drawn with CORPUS_SEED plus their greedy captions), and everything the checks of (c) share, computed once: the
    cross-entropy forward before the attribute was ever set, the self-critical forward, the cross-entropy forward afterwards,
    and the float64 oracles on the CPU oracle backend."""
    from oracle.attention_ref import OracleBackend
    from spacap3d_amd import backend, caption_decode
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
    cap = _no_dropout(model.caption).train()
    B = d["aggregated_vote_features"].shape[0]
    ep = {k: v.detach() for k, v in d.items() if torch.is_tensor(v) and not k.startswith("lang_cap")}
    ep["dataset_idx"] = torch.arange(B, device=DEV).view(B, 1)
    ep["object_id"] = torch.arange(B, device=DEV) + 3
    sos, eos = cap.word_to_idx["sos"], cap.word_to_idx["eos"]
    idx2word = {i: w for w, i in cap.word_to_idx.items()}
    n_words = 31
    res = {"cap": cap, "ep": ep, "sos": sos, "eos": eos}

    res["ce_before"] = _run(cap, ep)                                   # the parent's path, before the attribute exists

    # the matched proposals' indicator rows, as forward_train forms them, for the direct decodes
    with torch.no_grad():
        src = ep["aggregated_vote_features"]
        memory = cap.model.encode(src, cap._src_pos(ep), ep["bbox_mask"].unsqueeze(1))
        idx = res["ce_before"][0]["match_idx"]
        sel = idx.view(B, 1, 1).expand(B, 1, src.shape[-1])
        ind = (src.gather(1, sel) + memory.gather(1, sel)).squeeze(1)
        te, dec, gen = cap.model.tgt_embed, cap.model.decoder, cap.model.generator
        other = caption_decode.sample_decode(dec, gen, te[0], te[1].pe, ind, sos, eos, n_words, S_SAMPLES, 1.0, 0, CORPUS_SEED)[0]
        greedy = caption_decode.greedy_decode(dec, gen, te[0], te[1].pe, ind, sos, n_words)
        res["direct"] = caption_decode.sample_decode(dec, gen, te[0], te[1].pe, ind, sos, eos, n_words, S_SAMPLES, 1.0, 0, SAMPLE_SEED)
    other, greedy = other.cpu().numpy(), greedy.cpu().numpy()
    refs = [[R.decode(w, sos, eos) for w in other[b]] + [R.decode(greedy[b], sos, eos)] for b in range(B)]
    corpus = {"k%d" % b: [" ".join(idx2word[t] for t in r) for r in refs[b]] for b in range(B)}
    table = np.full((B, B + 3), -1, np.int32)
    for b in range(B):
        table[b, b + 3] = b
    res["refs"], res["table"], res["greedy"] = refs, table, greedy
    sc = SelfCritical(CaptionCorpus(corpus, cap.word_to_idx, key_of=table), sos, eos, num_samples=S_SAMPLES, seed=SAMPLE_SEED)
    cap.self_critical = sc
    try:
        res["scst"] = _run(cap, ep)
        res["scst_again"] = _run(cap, ep)[0]["_cap_loss"][0].detach().clone()
    finally:
        del cap.self_critical
    res["ce_after"] = _run(cap, ep)

    # float64 oracles: the same module on the CPU oracle backend in double precision, train() mode, dropout 0
    out = res["scst"][0]
    samples = out["scst_samples"].cpu().numpy().reshape(B * S_SAMPLES, n_words)
    rc = SC.Corpus(refs)
    rw = SC.rewards(rc, samples, S_SAMPLES, np.arange(B), np.arange(B) + 3, table, sos, eos)
    base = SC.rewards(rc, greedy, 1, np.arange(B), np.arange(B) + 3, table, sos, eos).cider
    res["restated_rewards"], res["restated_base"] = rw, base
    cap64 = _no_dropout(_cpu_copy(cap).double()).train()
    cap64.check_relation = False
    ep64 = {k: (ep[k].cpu().double() if ep[k].is_floating_point() else ep[k].cpu())      # what forward_train reads, per scene
            for k in ("aggregated_vote_features", "aggregated_vote_xyz", "bbox_mask", "ref_center_label", "lang_label", "lang_ids")}

    def run64(ep_rows, loss_of, rep):
        for p in cap64.parameters():
            p.grad = None
        feat = ep64["aggregated_vote_features"].clone().requires_grad_(True)
        e = {k: (v.repeat_interleave(rep, 0) if rep > 1 else v) for k, v in dict(ep64, aggregated_vote_features=feat).items()}
        e.update(ep_rows)
        with backend.use_backend(OracleBackend()):
            o = cap64.forward_train(e)
            value = loss_of(o)
            value.backward()
        g = {k: p.grad.clone() for k, p in _grad_leaves(cap64).items()}
        g["aggregated_vote_features"] = feat.grad.clone()
        return o, value.detach(), g

    res["ce64"] = run64({}, lambda o: compute_cap_loss(o)[0], 1)
    count = np.ones(B, bool)
    A64, _ = SC.advantage(rw.cider, base, count, S_SAMPLES)
    A = torch.from_numpy(A64.astype(np.float32).astype(np.float64))
    length = torch.from_numpy(rw.length.astype(np.int64))
    words = torch.from_numpy(samples)
    den = float(LR._den(float(rw.length.sum())))
    tok = torch.cat([torch.ones(B * S_SAMPLES, 1, dtype=torch.long), torch.from_numpy(rw.tf_tok[:, :-1])], 1)

    def scst_loss64(o):
        lp = o["lang_cap"].gather(2, words.unsqueeze(-1)).squeeze(-1)                 # (B S, n_words) log-probabilities
        live = (torch.arange(n_words)[None, :] < length[:, None]).double()
        return -(A * (lp * live).sum(1)).sum() / den

    res["scst64"] = run64({"lang_label": tok, "lang_ids": tok[:, 1:]}, scst_loss64, S_SAMPLES)
    res["logp64"] = res["scst64"][0]["lang_cap"].detach().numpy()
    # the issue's oracle for the teacher-forced sums: sampling_restated.teacher_forced_logits, at every proposal (the matched
    # proposal's rows carry the samples, the others a row of sos)
    K = ep["aggregated_vote_features"].shape[1]
    allrows = torch.full((B, K, S_SAMPLES, n_words), sos, dtype=torch.long)
    mi = idx.cpu()
    for b in range(B):
        allrows[b, mi[b]] = words.view(B, S_SAMPLES, n_words)[b]
    with backend.use_backend(OracleBackend()), torch.no_grad():
        tf = SR.teacher_forced_logits(cap64, ep64, allrows.view(-1, n_words)).view(B, K, S_SAMPLES, n_words, -1)
    res["tf_logits64"] = torch.stack([tf[b, mi[b]] for b in range(B)]).reshape(B * S_SAMPLES, n_words, -1).numpy()
    return res


def test_training_forward_samples_rewards_and_logp(trained):
    out = trained["scst"][0]
    rw, base = trained["restated_rewards"], trained["restated_base"]
    B, S = out["scst_reward"].shape
    assert "lang_cap" not in out and "_cap_vec" not in out
    assert out["scst_samples"].shape == (B, S, 31) and out["scst_reward"].dtype == torch.float64 and out["scst_baseline"].shape == (B,)
    assert out["scst_advantage"].shape == (B, S) and out["scst_logp"].shape == (B, S) and out["scst_sample_scores"].shape == (B, S)
    assert bool(out["scst_count"].all()) and bool(out["good_bbox_masks"].all())       # every scene counts
    adv = out["scst_advantage"].cpu().numpy()
    print(f"rewards {out['scst_reward'].cpu().numpy().round(4).tolist()}, baseline {out['scst_baseline'].cpu().numpy().round(4).tolist()}, "
          f"share of rows with |A| > 1e-3: {(np.abs(adv) > 1e-3).mean():.2f}")
    assert (np.abs(adv) > 1e-3).mean() >= 0.5
    # the samples are sample_decode's for the matched proposals at that seed
    ys, score, _ = trained["direct"]
    assert torch.equal(out["scst_samples"], ys) and torch.equal(out["scst_sample_scores"], score)
    e_r = float(np.abs(out["scst_reward"].cpu().numpy().reshape(-1) - rw.cider).max())
    e_b = float(np.abs(out["scst_baseline"].cpu().numpy() - base).max())
    print(f"largest |scst_reward - restated CIDEr| = {e_r:.3e}, baseline {e_b:.3e}")
    assert e_r <= CIDER_TOL and e_b <= CIDER_TOL
    A64, _ = SC.advantage(rw.cider, base, np.ones(B, bool), S)
    assert np.abs(adv.reshape(-1) - A64).max() <= 2.0 ** -24 * np.abs(A64).max() + CIDER_TOL
    # the alignment: one logit row per decoded word -- the float64 training forward on tf_tok gives teacher_forced_logits' rows
    lp64 = trained["logp64"]
    t64 = trained["tf_logits64"]
    t64 = t64 - (t64.max(-1, keepdims=True) + np.log(np.exp(t64 - t64.max(-1, keepdims=True)).sum(-1, keepdims=True)))
    live = np.arange(31)[None, :] < rw.length[:, None]
    assert np.abs((lp64 - t64)[live]).max() <= 1e-9
    words = out["scst_samples"].cpu().numpy().reshape(B * S, 31)
    sum64 = (np.take_along_axis(t64, words[..., None], -1)[..., 0] * live).sum(1)
    logp = out["scst_logp"].cpu().numpy().reshape(-1).astype(np.float64)
    fig = float(np.abs(logp - sum64).max())
    gap = float(np.abs(logp - out["scst_sample_scores"].cpu().numpy().reshape(-1)).max())
    from test_sampling_gpu import SCORE_TOL
    bound = SCORE_TOL + 4 * fig
    print(f"teacher-forced training path: largest |scst_logp - float64 sum| = {fig:.3e} (sums down to {sum64.min():.1f}); "
          f"largest |scst_logp - scst_sample_scores| = {gap:.3e} (bound {bound:.3e})")
    assert bound < 1e-3 and gap <= bound


def test_training_forward_loss_and_gradients(trained):
    out, grads = trained["scst"]
    rw, base = trained["restated_rewards"], trained["restated_base"]
    B, S = out["scst_reward"].shape
    words = out["scst_samples"].cpu().numpy().reshape(B * S, 31)
    ref = SC.loss(trained["logp64"], words, rw.length, rw.cider, base, np.ones(B, bool), S)
    loss = float(out["_cap_loss"][0])
    o64, v64, g64 = trained["scst64"]
    assert abs(float(v64) - ref.loss) <= LR.F64_BAR * max(1.0, ref.labs)               # torch float64 and numpy float64 agree
    e = abs(loss - ref.loss) / (LR.CAP_LOSS_REL * max(1.0, ref.labs))
    print(f"loss {loss:.7g} vs float64 {ref.loss:.7g} (scale {ref.labs:.3g}): excess {e:.3g}; acc {float(out['_cap_loss'][1]):.4f} vs {ref.acc:.4f}")
    assert e <= 1
    assert torch.equal(trained["scst_again"], out["_cap_loss"][0].detach())            # the same bits at the same seed
    # gradients: four times the deviation of the existing cross-entropy path from ITS float64 oracle, per tensor
    ce_g, ce64_g = trained["ce_before"][1], trained["ce64"][2]
    ce_loss, ce64_loss = float(trained["ce_before"][0]["_cap_loss"][0]), float(trained["ce64"][1])
    print(f"cross-entropy path: loss {ce_loss:.7g} vs float64 {ce64_loss:.7g}")
    assert abs(ce_loss - ce64_loss) <= LR.CAP_LOSS_REL * max(1.0, abs(ce64_loss))
    bad = []
    for k in GRAD_TENSORS:
        f_ce = LR.figure(ce_g[k].cpu().numpy(), ce64_g[k].numpy())
        f_sc = LR.figure(grads[k].cpu().numpy(), g64[k].numpy())
        print(f"{k}: cross-entropy path {f_ce:.3e}, self-critical path {f_sc:.3e} (allowed {4 * f_ce:.3e}); "
              f"largest reference entry {float(g64[k].abs().max()):.3e}")
        if not f_sc <= 4 * f_ce:
            bad.append(k)
    assert not bad, bad


def test_without_the_attribute_forward_train_is_bit_equal(trained):
    (o0, g0), (o1, g1) = trained["ce_before"], trained["ce_after"]
    assert trained["cap"].self_critical is None
    for k in ("lang_cap", "_cap_vec", "match_idx", "good_bbox_masks", "pred_ious"):
        assert torch.equal(o0[k], o1[k]), k
    assert torch.equal(o0["_cap_loss"][0], o1["_cap_loss"][0]) and torch.equal(o0["_cap_loss"][1], o1["_cap_loss"][1])
    for k in GRAD_TENSORS:
        assert torch.equal(g0[k], g1[k]), k
    assert not any(k.startswith("scst_") for k in o1)


# ---- (d) Trainer -----------------------------------------------------------------------------------------------------------
def _small_trainer(self_critical):
    from spacap3d_amd import synthetic as S
    from spacap3d_amd.engine import Trainer, synthetic_batch
    from spacap3d_amd.spacapnet import build_default
    torch.manual_seed(0)
    model = build_default(vocab_size=120, num_proposal=32, N=2, d_ff=256).to(DEV).train()
    data = synthetic_batch(2, 4096, DEV, seed=0, vocab=120)
    if self_critical is not None:
        B = data["point_clouds"].shape[0]
        data["dataset_idx"] = torch.arange(B, device=DEV)
        data["object_id"] = torch.arange(B, device=DEV) + 3
        model.caption.self_critical = self_critical(model.caption, B)
    return model, Trainer(model, S.mean_size_arr().numpy()), data


def _corpus_for(cap, B):
    """Two references per scene out of the vocabulary's own words (the rewards of an untrained model's samples against them are
    small but the step only has to run)."""
    from spacap3d_amd.caption_eval import CaptionCorpus
    from spacap3d_amd.self_critical import SelfCritical
    idx2word = {i: w for w, i in cap.word_to_idx.items()}
    rng = np.random.default_rng(3)
    corpus = {"k%d" % b: ["sos " + " ".join(idx2word[int(t)] for t in rng.integers(4, 120, 12)) + " eos" for _ in range(2)] for b in range(B)}
    table = np.full((B, B + 3), -1, np.int32)
    for b in range(B):
        table[b, b + 3] = b
    return SelfCritical(CaptionCorpus(corpus, cap.word_to_idx, key_of=table), cap.word_to_idx["sos"], cap.word_to_idx["eos"],
                        num_samples=3, seed=11)


def test_trainer_steps_eagerly_with_self_critical():
    model, tr, data = _small_trainer(_corpus_for)
    w_cap = model.caption.model.generator.proj.weight
    w_det = model.proposal.proposal[-1].weight
    before = (w_cap.detach().clone(), w_det.detach().clone())
    losses = []
    for _ in range(2):                                   # (the deferred weight-gradient check of _core runs in both)
        tr.step(data)
        losses.append({k: float(v) for k, v in tr.last_losses.items()})
    print(f"two eager self-critical steps: {losses}")
    assert tr.graph is None and tr._eager_checks == 0
    assert all(np.isfinite(v) for h in losses for v in h.values())
    assert not torch.equal(before[0], w_cap) and not torch.equal(before[1], w_det)


def test_default_trainer_is_untouched_by_a_self_critical_run():
    """Two steps of the default model without the attribute: the same two losses, to the bit, whether or not a self-critical
    Trainer ran in the process before."""
    from spacap3d_amd import attention

    def two_steps():
        # the dropout masks come from a host call counter and a device step counter that live with the process: both from a
        # fixed state, so that two runs draw the same masks
        attention._CALL_COUNTER[0] = 1 << 20
        attention.rng_state(torch.device(DEV)).zero_()
        model, tr, data = _small_trainer(None)
        return [tr.step(data).clone() for _ in range(2)]
    first = two_steps()
    model, tr, data = _small_trainer(_corpus_for)
    tr.step(data)
    second = two_steps()
    torch.cuda.synchronize()
    print(f"default losses: {[float(v) for v in first]} and after a self-critical step {[float(v) for v in second]}")
    assert all(torch.equal(a, b) for a, b in zip(first, second))


# ---- (e) refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(trained):
    from spacap3d_amd.caption_eval import CaptionCorpus
    from spacap3d_amd.self_critical import SelfCritical
    cap, ep = trained["cap"], trained["ep"]
    cc = CaptionCorpus({"k0": ["sos a eos"]}, cap.word_to_idx, key_of=np.zeros((1, 1), np.int32))
    with pytest.raises(ValueError, match="num_samples 1 < 2"):
        SelfCritical(cc, trained["sos"], trained["eos"], baseline="samples", num_samples=1)
    cap.self_critical = SelfCritical(cc, trained["sos"], trained["eos"], num_samples=2)
    try:
        with pytest.raises(KeyError, match="object_id"):
            cap.forward_train({k: v for k, v in ep.items() if k != "object_id"})
        with pytest.raises(KeyError, match="dataset_idx"):
            cap.forward_train({k: v for k, v in ep.items() if k != "dataset_idx"})
        with pytest.raises(RuntimeError, match="self_critical.*not supported"):
            _cpu_copy(cap).forward_train({k: v.cpu() for k, v in ep.items()})
        cap.eval()                                       # eval mode does not read the attribute
        with torch.no_grad():
            assert "scst_reward" not in cap.forward_train(dict(ep))
    finally:
        cap.train()
        del cap.self_critical
