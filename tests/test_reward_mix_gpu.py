"""Mixed rewards and the mixed caption loss of self-critical training on the MI355X: the reward kernel
(csrc/caption_reward.hip) against what the reference's own ``BleuScorer`` and ``Rouge`` recorded (tests/golden/
caption_reward_ref.npz) and, bit for bit, against the two kernels it shares its arithmetic with; the loss kernels
(csrc/scst_loss.hip) at their dispatch edges against the float64 restatement (tests/reward_mix_restated.py) and bit for bit
against ``spacap_scst_loss_*``; the training forward in both proposal modes against float64 autograd of the restated loss on the
CPU oracle backend; two eager ``Trainer`` steps per mode; and the refusals.  The largest figures are printed."""
import os

import numpy as np
import pytest
import torch

import caption_eval_restated as R
import losses_restated as LR
import reward_mix_restated as RM
import self_critical_restated as SC
from test_caption_eval_cpu import FIX, corpus_of
from test_self_critical_gpu import GRAD_TENSORS, _cpu_copy, _grad_leaves, _no_dropout, _run, _small_trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
REC = np.load(os.path.join(HERE, "golden", "caption_reward_ref.npz"))
REWARD_TOL = 1e-9          # the bound the project holds rewards to (tests/test_self_critical_gpu.py: CIDER_TOL)
WEIGHTS = (1.0, 2.0, 1.0)
REWARD = {"cider": 1, "bleu4": 2, "rouge": 1}
XE_WEIGHT = 0.5


@pytest.fixture(autouse=True, scope="module")
def _needs_a_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _up(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the shared case arrays are read-only)


# ---- (a) the reward kernel -------------------------------------------------------------------------------------------------
def _poisoned(rows, L):
    nan = float("nan")
    return (torch.full((rows,), nan, dtype=torch.float64, device=DEV), torch.full((rows,), -7, dtype=torch.int32, device=DEV),
            torch.full((rows,), -7, dtype=torch.int32, device=DEV), torch.full((rows, L + 2), -7, dtype=torch.int64, device=DEV),
            torch.full((3, rows), nan, dtype=torch.float64, device=DEV), torch.full((rows, 10), -7, dtype=torch.int32, device=DEV))


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _sc(case, table, **kw):
    from spacap3d_amd.caption_eval import CaptionCorpus
    from spacap3d_amd.self_critical import SelfCritical
    corpus, w2i = corpus_of(case)
    cc = CaptionCorpus(corpus, w2i, key_of=table)
    return cc, SelfCritical(cc, R.SOS, R.EOS, **kw)


@pytest.mark.parametrize("name", RM.ROW_SET_NAMES)
def test_reward_kernel_against_the_recorded_scores(name):
    from spacap3d_amd.caption_eval import CaptionEval
    tokens, didx, oid, table, want_key, case = RM.row_set(FIX, name)
    rows, L = tokens.shape
    cc, plain = _sc(case, table)
    _, mix = _sc(case, table, reward=REWARD)
    d_tok, d_idx, d_oid = _up(tokens), _up(didx), _up(oid)
    old = plain.rewards(d_tok, d_idx, d_oid, 1, out=_poisoned(rows, L)[:4])
    got = mix.rewards(d_tok, d_idx, d_oid, 1, out=_poisoned(rows, L), terms=True)
    reward, key, length, tf, scores, comp = got
    assert scores.shape == (rows, 3) and comp.shape == (rows, 10)
    # integers first
    np.testing.assert_array_equal(key.cpu().numpy(), REC[f"{name}/key"])
    np.testing.assert_array_equal(key.cpu().numpy(), want_key)
    np.testing.assert_array_equal(comp.cpu().numpy(), REC[f"{name}/bleu_comp"])
    for a, b in zip(old[1:], got[1:4]):
        assert torch.equal(a, b)                                                      # key, length, tf_tok: section 7j's
    # CIDEr bit for bit at any weights; weights (1, 0, 0) give the old entry's reward bits
    assert _bits(scores[:, 0]) == _bits(old[0])
    one = _sc(case, table, reward={"cider": 1.0})[1].rewards(d_tok, d_idx, d_oid, 1, out=_poisoned(rows, L), terms=True)
    assert _bits(one[0]) == _bits(old[0]) and _bits(one[4][:, 0]) == _bits(old[0])
    assert all(torch.equal(a, b) for a, b in zip(old[1:], one[1:4]))
    z = one[4][:, 1:].cpu().numpy()
    assert not z.any() and not np.signbit(z).any() and not one[5].any()               # a zero weight: +0.0, components zero
    other = _sc(case, table, reward={"cider": 0.25, "rouge": 3.0})[1].rewards(d_tok, d_idx, d_oid, 1, out=_poisoned(rows, L), terms=True)
    assert _bits(other[4][:, 0]) == _bits(old[0]) and _bits(other[4][:, 2]) == _bits(scores[:, 2])
    z = other[4][:, 1].cpu().numpy()
    assert not z.any() and not np.signbit(z).any()
    only_b = _sc(case, table, reward="bleu4")[1].rewards(d_tok, d_idx, d_oid, 1, out=_poisoned(rows, L), terms=True)
    assert _bits(only_b[4][:, 1]) == _bits(scores[:, 1]) and torch.equal(only_b[5], comp) and _bits(only_b[0]) == _bits(scores[:, 1])
    assert not only_b[4][:, 0].any() and not only_b[4][:, 2].any()
    # the recorded scores
    s = scores.cpu().numpy()
    keyed = want_key >= 0
    e_b = float(np.abs(s[:, 1] - REC[f"{name}/bleu4"]).max())
    e_r = float(np.abs(s[:, 2] - REC[f"{name}/rouge"]).max())
    print(f"{name}: {rows} rows, {int((~keyed).sum())} without a key row; largest |BLEU-4 - recorded| = {e_b:.3e}, |ROUGE - recorded| = {e_r:.3e}")
    assert e_b <= REWARD_TOL
    assert s[:, 2].tobytes() == REC[f"{name}/rouge"].tobytes()                         # IEEE divisions in the reference's order
    # the reward is the float64 combination of the three returned terms, bit for bit
    assert reward.cpu().numpy().tobytes() == RM.combine(s, WEIGHTS).tobytes()
    # rows without a key row: all zeros
    lost = ~keyed
    assert not s[lost].any() and not reward.cpu().numpy()[lost].any() and not comp.cpu().numpy()[lost].any()
    # the same caption planted as its key's candidate through spacap_caption_score_f64: the same bits (one definition).  A key
    # takes one candidate: round j plants the j-th row of every key.
    ce = CaptionEval(cc, R.SOS, R.EOS)
    nkeys = cc.nkeys
    seen = np.zeros(nkeys, np.int64)
    rnd = np.full(rows, -1)
    for r in np.flatnonzero(keyed):
        rnd[r] = seen[want_key[r]]
        seen[want_key[r]] += 1
    for j in range(int(rnd.max()) + 1):
        tok, ln = R.new_table(nkeys, R.SOS, R.EOS)
        mine = np.flatnonzero(rnd == j)
        for r in mine:
            cap = R.decode(tokens[r], R.SOS, R.EOS)
            tok[want_key[r]] = 0
            tok[want_key[r], :len(cap)] = cap
            ln[want_key[r]] = len(cap)
        ce.set_candidates(_up(tok), _up(ln))
        sc_ = ce.scores()
        k = _up(want_key[mine].astype(np.int64))
        m = _up(mine)
        assert _bits(sc_["rouge"][k]) == _bits(scores[m, 2]), j
        assert _bits(sc_["cider"][k]) == _bits(scores[m, 0]), j
        assert torch.equal(sc_["bleu"][k], comp[m]), j
    # a second call gives the same bits
    again = mix.rewards(d_tok, d_idx, d_oid, 1, out=_poisoned(rows, L), terms=True)
    assert all(_bits(a) == _bits(b) for a, b in zip(got, again))


def test_reward_kernel_replays_on_new_inputs():
    """Two rows per scene, captured; the replay sees other tokens and other scenes."""
    tokens, didx, oid, table, want_key, case = RM.row_set(FIX, "random_extra")
    rows, L = tokens.shape
    _, mix = _sc(case, table, reward=REWARD)
    n = (rows // 4) * 2
    st_tok, st_idx, st_oid = _up(tokens[:n]), _up(didx[0:n:2]), _up(oid[0:n:2])
    st_out = _poisoned(n, L)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mix.rewards(st_tok, st_idx, st_oid, 2, out=st_out, terms=True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mix.rewards(st_tok, st_idx, st_oid, 2, out=st_out, terms=True)
    st_tok.copy_(_up(tokens[n:2 * n]))
    st_idx.copy_(_up(didx[n:2 * n:2]))
    st_oid.copy_(_up(oid[n:2 * n:2]))
    for t, v in zip(st_out, _poisoned(n, L)):
        t.copy_(v)
    g.replay()
    torch.cuda.synchronize()
    want = RM.rewards(SC.Corpus(R.refs_of(FIX, case)), tokens[n:2 * n], 2, didx[n:2 * n:2], oid[n:2 * n:2], table, R.SOS, R.EOS, WEIGHTS)
    np.testing.assert_array_equal(st_out[1].cpu().numpy(), want.key)
    np.testing.assert_array_equal(st_out[3].cpu().numpy(), want.tf_tok)
    np.testing.assert_array_equal(st_out[5].cpu().numpy(), want.bleu_comp)
    got = st_out[4].t().cpu().numpy()
    assert np.abs(got - want.scores).max() <= REWARD_TOL and got[:, 2].tobytes() == want.scores[:, 2].tobytes()
    assert st_out[0].cpu().numpy().tobytes() == RM.combine(got, WEIGHTS).tobytes()
    assert (want.scores > 0).any(0).all() and (want.key < 0).any()


# ---- (b) the loss kernels --------------------------------------------------------------------------------------------------
def _call_mixed(x, case, poison=float("nan"), W0=None):
    """The pair of launches on a case's inputs with poisoned outputs: (out, adv, rowlogp, pair, hit, dlogits) on the device."""
    from spacap3d_amd._native import check, lib
    B0, Rn, S, W, V = case.B0, case.R, case.S, case.W, case.V
    N, W0 = B0 + Rn, W if W0 is None else W0
    st = torch.cuda.current_stream().cuda_stream
    logits, words, length, reward = _up(x.logits), _up(x.words), _up(x.length), _up(x.reward)
    ids = _up(x.lang_ids) if B0 else None
    good = _up(x.good.astype(np.uint8)) if B0 else None
    base = _up(x.baseline) if x.baseline is not None else None
    count = _up(x.count.astype(np.uint8))
    pair, hit = torch.full((N, W, 2), poison, device=DEV), torch.full((N, W), 9, dtype=torch.uint8, device=DEV)
    adv, rowlogp, out = torch.full((Rn,), poison, device=DEV), torch.full((Rn,), poison, device=DEV), torch.full((12,), poison, device=DEV)
    dlogits = torch.full((N, W, V), poison, device=DEV)
    gl = torch.tensor([RM.LOSS_UPSTREAM], device=DEV)
    ts = x.lang_ids.shape[1] if B0 else 0
    p = lambda t: t.data_ptr() if t is not None else None
    fwd = lambda o: check(lib.spacap_mixed_cap_loss_fwd_f32(
        logits.data_ptr(), ids.data_ptr() + 8 if B0 else None, ts, p(good), B0, W0, words.data_ptr(), length.data_ptr(), reward.data_ptr(),
        p(base), count.data_ptr(), Rn, S, W, V, case.w_xe, pair.data_ptr(), hit.data_ptr(), adv.data_ptr(), rowlogp.data_ptr(),
        o.data_ptr(), st), "spacap_mixed_cap_loss_fwd_f32")
    fwd(out)
    check(lib.spacap_mixed_cap_loss_bwd_f32(logits.data_ptr(), ids.data_ptr() + 8 if B0 else None, ts, p(good), B0, W0, words.data_ptr(),
                                            length.data_ptr(), pair.data_ptr(), adv.data_ptr(), out.data_ptr(), gl.data_ptr(), Rn, W, V,
                                            case.w_xe, dlogits.data_ptr(), st), "spacap_mixed_cap_loss_bwd_f32")
    out2 = torch.full((12,), poison, device=DEV)
    fwd(out2)                                                                          # a second call gives the same bits
    assert _bits(out) == _bits(out2)
    # the sample rows through spacap_scst_loss_* on their slice of the same image
    s_pair, s_hit = torch.full((Rn, W, 2), poison, device=DEV), torch.full((Rn, W), 9, dtype=torch.uint8, device=DEV)
    s_adv, s_row, s_out = torch.full((Rn,), poison, device=DEV), torch.full((Rn,), poison, device=DEV), torch.full((8,), poison, device=DEV)
    s_d = torch.full((Rn, W, V), poison, device=DEV)
    tail = logits[B0:]
    check(lib.spacap_scst_loss_fwd_f32(tail.data_ptr(), words.data_ptr(), length.data_ptr(), reward.data_ptr(), p(base), count.data_ptr(),
                                       Rn, S, W, V, s_pair.data_ptr(), s_hit.data_ptr(), s_adv.data_ptr(), s_row.data_ptr(),
                                       s_out.data_ptr(), st), "spacap_scst_loss_fwd_f32")
    check(lib.spacap_scst_loss_bwd_f32(tail.data_ptr(), words.data_ptr(), length.data_ptr(), s_pair.data_ptr(), s_adv.data_ptr(),
                                       s_out.data_ptr(), gl.data_ptr(), Rn, W, V, s_d.data_ptr(), st), "spacap_scst_loss_bwd_f32")
    torch.cuda.synchronize()
    return (out, adv, rowlogp, pair, hit, dlogits), (s_out, s_adv, s_row, s_pair, s_hit, s_d)


@pytest.mark.parametrize("case", RM.LOSS_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_loss_kernels_at_their_dispatch_edges(case):
    x, ref = RM.loss_inputs(case), RM.loss_reference(case)
    B0, Rn, S, W, V = case.B0, case.R, case.S, case.W, case.V
    (out, adv, rowlogp, pair, hit, dlogits), (s_out, s_adv, s_row, s_pair, s_hit, s_d) = _call_mixed(x, case)
    o, d = out.cpu().numpy().astype(np.float64), dlogits.cpu().numpy()
    assert np.isfinite(o).all() and np.isfinite(d).all() and torch.isfinite(pair).all() and int(hit.max()) <= 1
    # the sample rows hold spacap_scst_loss_*'s bits, whatever stands in front of them
    so = s_out.cpu().numpy()
    assert [o[i] for i in (1, 3, 5, 7, 9, 10)] == [so[i] for i in range(6)]
    assert _bits(out[1]) == _bits(s_out[0]) and _bits(adv) == _bits(s_adv) and _bits(rowlogp) == _bits(s_row)
    assert _bits(pair[B0:]) == _bits(s_pair) and _bits(hit[B0:]) == _bits(s_hit) and _bits(dlogits[B0:]) == _bits(s_d)
    if B0 == 0 or case.w_xe == 0:
        assert _bits(out[0]) == _bits(s_out[0])                                        # the total IS L_rl, to the bit
    if B0 == 0:
        assert o[2] == 0 and o[4] == 0 and o[8] == 0 and o[11] == 0
    if case.w_xe == 0:
        assert not d[:B0].any()                                                        # the ground-truth rows: exact zeros
    # against the restatement, within the project's bars for the caption head
    e_loss = abs(o[0] - ref.loss) / (LR.CAP_LOSS_REL * max(1.0, ref.labs))
    e_rl = abs(o[1] - ref.l_rl) / (LR.CAP_LOSS_REL * max(1.0, ref.rl.labs))
    e_xe = abs(o[2] - ref.l_xe) / (LR.CAP_LOSS_REL * max(1.0, abs(ref.l_xe)))
    e_acc = max(abs(o[3] - ref.acc_rl), abs(o[4] - ref.acc_xe)) / LR.CAP_ACC_ABS
    grad = lambda got, want: float(np.abs(got - want).max()) / (LR.CAP_GRAD_REL * max(float(np.abs(want).max()), 1e-6) + LR.CAP_GRAD_ABS)
    e_grl = grad(d[B0:], ref.dlogits[B0:])
    e_gxe = grad(d[:B0], ref.dlogits[:B0]) if B0 else 0.0
    e_row = float(np.abs(rowlogp.cpu().numpy() - ref.rl.rowlogp).max()) / (W * LR.CAP_LOGP_ABS)
    e_lp = 0.0
    if B0:
        t = ref.xe.target
        valid = (t != 0) & x.good[:, None]
        lp = np.take_along_axis(ref.xe.logp, t[..., None], -1)[..., 0]
        got = pair[:B0, :, 1].cpu().numpy()
        e_lp = float(np.abs(got - lp)[valid].max()) / LR.CAP_LOGP_ABS if valid.any() else 0.0
        assert not got[~valid].any() and not pair[:B0, :, 0].cpu().numpy()[~valid].any()
        # exact zeros on pad targets (out-of-range ids among them) and on scenes that are not good
        assert not d[:B0][~valid].any()
        assert o[8] == ref.n_good and abs(o[6] - ref.inv_xe) <= 1e-6 * ref.inv_xe
        if case.good == "none":
            assert o[2] == 0 and not d[:B0].any()
        elif case.w_xe > 0:
            assert np.abs(d[:B0]).max() > 0 and ref.acc_xe > 0
    print(f"excess (at most 1): loss {e_loss:.3g}  L_rl {e_rl:.3g}  L_xe {e_xe:.3g}  acc {e_acc:.3g}  dlogits rl {e_grl:.3g} xe {e_gxe:.3g}  "
          f"rowlogp {e_row:.3g}  logp {e_lp:.3g}   loss {o[0]:.6g} vs {ref.loss:.6g} (scale {ref.labs:.3g})")
    assert max(e_loss, e_rl, e_xe, e_acc, e_grl, e_gxe, e_row, e_lp) <= 1
    # exact zeros behind the length, on scenes that do not count and where the advantage is 0
    live = (np.arange(W)[None, :] < x.length[:, None]) & np.repeat(x.count, S)[:, None]
    assert not d[B0:][~live].any()
    z = slice(B0 + SC.ZERO_SCENE * S, B0 + (SC.ZERO_SCENE + 1) * S)
    assert not d[z].any() and not adv.cpu().numpy()[SC.ZERO_SCENE * S:(SC.ZERO_SCENE + 1) * S].any()
    assert abs(o[5] - ref.inv_rl) <= 1e-6 * ref.inv_rl and o[7] == ref.rl.n_scenes and o[11] == 0
    assert abs(o[9] - ref.rl.mean_reward) <= 1e-6 * max(1.0, abs(ref.rl.mean_reward))
    assert abs(o[10] - ref.rl.mean_baseline) <= 1e-6 * max(1.0, abs(ref.rl.mean_baseline))
    if case.count == "none":
        assert o[1] == 0 and not d[B0:].any()


def test_mixed_loss_op_through_autograd():
    """``fused_losses.mixed_caption_loss``: the op's value and gradient are the entry points', the upstream gradient arrives."""
    from spacap3d_amd.fused_losses import mixed_caption_loss, self_critical_loss
    case = RM.MixCase(3, 9, 3, 7, 257, "some", "all", 0.5, "greedy")
    x, ref = RM.loss_inputs(case), RM.loss_reference(case)
    logits = _up(x.logits).requires_grad_(True)
    out, adv, rowlogp = mixed_caption_loss(logits, _up(x.lang_ids), _up(x.good), _up(x.words), _up(x.length), _up(x.reward),
                                           _up(x.baseline), _up(x.count), case.S, case.w_xe)
    (out[0] * RM.LOSS_UPSTREAM).backward()
    (want, *_), _ = _call_mixed(x, case)
    assert _bits(out) == _bits(want) and out.shape == (12,) and adv.shape == (case.R,)
    d = logits.grad.cpu().numpy()
    bar = LR.CAP_GRAD_REL * float(np.abs(ref.dlogits).max()) + LR.CAP_GRAD_ABS
    assert np.abs(d - ref.dlogits).max() <= bar
    # ground-truth rows of fewer word positions than the pass (W0 = 4 of W = 7): the restatement's value and gradient, exact
    # zeros behind them, the sample rows' bits untouched
    cut = RM.loss(x.logits, x.lang_ids, x.good, x.words, x.length, x.reward, x.baseline, x.count, case.S, case.w_xe, RM.LOSS_UPSTREAM, 4)
    (c_out, c_adv, _, c_pair, _, c_d), (s_out, s_adv, _, _, _, s_d) = _call_mixed(x, case, W0=4)
    o = c_out.cpu().numpy().astype(np.float64)
    assert abs(o[2] - cut.l_xe) <= LR.CAP_LOSS_REL * max(1.0, cut.l_xe) and abs(o[0] - cut.loss) <= LR.CAP_LOSS_REL * max(1.0, cut.labs)
    assert abs(o[6] - cut.inv_xe) <= 1e-6 * cut.inv_xe and abs(o[4] - cut.acc_xe) <= LR.CAP_ACC_ABS and cut.l_xe != ref.l_xe
    cd = c_d.cpu().numpy()
    assert np.abs(cd - cut.dlogits).max() <= LR.CAP_GRAD_REL * float(np.abs(cut.dlogits).max()) + LR.CAP_GRAD_ABS
    assert not cd[:case.B0, 4:].any() and not c_pair[:case.B0, 4:].any() and _bits(c_d[case.B0:]) == _bits(s_d) and _bits(c_adv) == _bits(s_adv)
    # without ground-truth rows: SelfCriticalLoss's bits
    tail = _up(x.logits[case.B0:]).requires_grad_(True)
    o0, a0, r0 = mixed_caption_loss(tail, None, None, _up(x.words), _up(x.length), _up(x.reward), _up(x.baseline), _up(x.count), case.S, 0.5)
    o1, a1, r1 = self_critical_loss(tail, _up(x.words), _up(x.length), _up(x.reward), _up(x.baseline), _up(x.count), case.S)
    assert _bits(o0[0]) == _bits(o1[0]) and _bits(a0) == _bits(a1) and _bits(r0) == _bits(r1)


# ---- (c) the training forward, end to end, in both proposal modes ----------------------------------------------------------
SEED, SAMPLE_SEED, CORPUS_SEED, S_SAMPLES, M_SLOTS, NEAR, N_WORDS = 0, 20261020, 20261021, 3, 4, 0.3, 31
KEYED_SLOTS = ((0, 1, 2, 3, 4), (1, 3, 5))         # tests/test_scene_scst_gpu.py's scenes: the object slots with a key row
ID_OFFSET = 3
MODES = ("referred", "matched")


@pytest.fixture(scope="module")
def world():
    """The model and scenes of tests/test_sampling_gpu.py in train() mode with dropout 0 (ground-truth boxes anchored on the
    proposals, as tests/test_scene_scst_gpu.py has them, so that both proposal modes find their objects), the corpus, and per
    mode everything the checks of (c) share, computed once: the CIDEr-only forward, the mixed forward twice, the cross-entropy
    forward before and afterwards, and the float64 oracles on the CPU oracle backend."""
    from oracle.attention_ref import OracleBackend
    from spacap3d_amd import backend, caption_decode
    from spacap3d_amd import synthetic as SY
    from spacap3d_amd.caption_eval import CaptionCorpus
    from spacap3d_amd.engine import synthetic_batch
    from spacap3d_amd.loss_helper import compute_cap_loss
    from spacap3d_amd.self_critical import SelfCritical
    from spacap3d_amd.spacapnet import build_default
    import scene_scst_restated as SS
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
    ep["object_id"] = torch.tensor([KEYED_SLOTS[b][0] + ID_OFFSET for b in range(B)], device=DEV)
    table = np.full((B, G + ID_OFFSET), -1, np.int32)
    keys = [(b, j) for b in range(B) for j in KEYED_SLOTS[b]]
    for row, (b, j) in enumerate(keys):
        table[b, j + ID_OFFSET] = row
    sos, eos = cap.word_to_idx["sos"], cap.word_to_idx["eos"]
    idx2word = {i: w for w, i in cap.word_to_idx.items()}
    xyz = ep["aggregated_vote_xyz"].cpu().numpy()
    assert len({tuple(p) for p in xyz.reshape(-1, 3)}) == B * K                       # the proposals are distinct points
    res = {"cap": cap, "ep": ep, "B": B, "sos": sos, "eos": eos}

    res["ce_before"] = _run(cap, ep)
    te, dec, gen = cap.model.tgt_embed, cap.model.decoder, cap.model.generator
    with torch.no_grad():
        src = ep["aggregated_vote_features"]
        memory = cap.model.encode(src, cap._src_pos(ep), ep["bbox_mask"].unsqueeze(1))
        both = src + memory
        near_k = [SS.nearest(xyz[b], ep["center_label"][b, j].cpu().numpy())[0] for b, j in keys]
        ind = torch.stack([both[b, k] for (b, _), k in zip(keys, near_k)])
        other = caption_decode.sample_decode(dec, gen, te[0], te[1].pe, ind, sos, eos, N_WORDS, S_SAMPLES, 1.0, 0, CORPUS_SEED)[0]
        greedy = caption_decode.greedy_decode(dec, gen, te[0], te[1].pe, ind, sos, N_WORDS)
    other, greedy = other.cpu().numpy(), greedy.cpu().numpy()
    refs = [[R.decode(w, sos, eos) for w in other[i]] + [R.decode(greedy[i], sos, eos)] for i in range(len(keys))]
    corpus = {"k%d" % i: [" ".join(idx2word[t] for t in r) for r in refs[i]] for i in range(len(keys))}
    cc = CaptionCorpus(corpus, cap.word_to_idx, key_of=table)
    rc = SC.Corpus(refs)
    mk = lambda mode, **kw: SelfCritical(cc, sos, eos, num_samples=S_SAMPLES, seed=SAMPLE_SEED, proposals=mode, max_proposals=M_SLOTS,
                                         near_threshold=NEAR, **kw)
    res["mk"] = mk

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
    gt_ids = ep64["lang_ids"].numpy()
    Tg = ep64["lang_label"].shape[1]
    assert Tg == N_WORDS + 2 and gt_ids.shape[1] >= N_WORDS + 1                       # (the two token widths agree in these scenes)

    for mode in MODES:
        m = {}
        try:
            cap.self_critical = mk(mode)
            m["cider_only"] = _run(cap, ep)
            cap.self_critical = mk(mode, reward=REWARD, xe_weight=XE_WEIGHT)
            m["mixed"] = _run(cap, ep)
            m["mixed_again"] = _run(cap, ep)[0]["_cap_loss"][0].detach().clone()
        finally:
            del cap.self_critical
        out = m["mixed"][0]
        # the groups: B scenes with their referred object's proposal, or the B M slots of the selection (an empty slot: -1)
        if mode == "referred":
            prop, obj = out["match_idx"].cpu().numpy().reshape(B, 1), ep["object_id"].cpu().numpy().reshape(B, 1)
        else:
            prop, obj = out["scst_proposal"].cpu().numpy(), out["scst_object_id"].cpu().numpy()
        Mg = prop.shape[1]
        NG = B * Mg
        count = out["scst_count"].cpu().numpy().reshape(-1).astype(bool)
        samples = out["scst_samples"].cpu().numpy().reshape(NG * S_SAMPLES, N_WORDS)
        didx, oid = np.repeat(np.arange(B), Mg), obj.reshape(-1)
        with torch.no_grad():
            p_ = _up(prop)
            ind_g = both[torch.arange(B, device=DEV)[:, None], p_.clamp(min=0)].masked_fill((p_ < 0).unsqueeze(-1), 0.0).reshape(NG, D)
            greedy_g = caption_decode.greedy_decode(dec, gen, te[0], te[1].pe, ind_g, sos, N_WORDS).cpu().numpy()
        rw = RM.rewards(rc, samples, S_SAMPLES, didx, oid, table, sos, eos, WEIGHTS)
        bs = RM.rewards(rc, greedy_g, 1, didx, oid, table, sos, eos, WEIGHTS)
        m.update(rw=rw, bs=bs, count=count, samples=samples, Mg=Mg)
        # the float64 oracle: B ground-truth rows, then the NG S sample rows, every scene repeated equally often (the encoder's
        # position embedding holds a BatchNorm1d in training mode: equal repeats keep the statistics of the B scenes)
        grp = np.arange(NG * S_SAMPLES) // S_SAMPLES
        rows_scene = torch.from_numpy(np.concatenate([np.arange(B), grp // Mg]))
        ref_xyz = torch.cat([ep64["ref_center_label"], torch.from_numpy(xyz[grp // Mg, np.maximum(prop.reshape(-1)[grp], 0)]).double()])
        A64, _ = SC.advantage(rw.reward, bs.reward, count, S_SAMPLES)
        A = torch.from_numpy(A64.astype(np.float32).astype(np.float64))
        length = torch.from_numpy(rw.length.astype(np.int64))
        words = torch.from_numpy(samples)
        den = float(LR._den(float(rw.length[np.repeat(count, S_SAMPLES)].sum())))
        tok = torch.cat([torch.ones(len(grp), 1, dtype=torch.long), torch.from_numpy(rw.tf_tok[:, :-1])], 1)
        all_tok = torch.cat([ep64["lang_label"], tok])
        good = out["good_bbox_masks"].cpu().numpy().astype(bool)
        tgt = torch.from_numpy(gt_ids[:, 1:N_WORDS + 1])
        valid = torch.from_numpy(good)[:, None] & (tgt != 0)
        den_xe = float(LR._den(float(good.sum() * N_WORDS)))                          # (the good (scene, word) rows)

        def mixed_loss64(o):
            lp = o["lang_cap"]
            lps = lp[B:].gather(2, words.unsqueeze(-1)).squeeze(-1)
            live = (torch.arange(N_WORDS)[None, :] < length[:, None]).double()
            l_rl = -(A * (lps * live).sum(1)).sum() / den
            l_xe = -(lp[:B].gather(2, tgt.unsqueeze(-1)).squeeze(-1) * valid.double()).sum() / den_xe
            return l_rl + XE_WEIGHT * l_xe

        ids_rows = torch.cat([ep64["lang_ids"][:, :Tg], torch.nn.functional.pad(tok[:, 1:], (0, 1))])
        m["f64"] = run64(rows_scene, {"lang_label": all_tok, "lang_ids": ids_rows, "ref_center_label": ref_xyz}, mixed_loss64)
        live_rows = torch.from_numpy(np.concatenate([np.ones(B, bool), np.repeat(count, S_SAMPLES)]))
        want_idx = torch.from_numpy(np.concatenate([out["match_idx"].cpu().numpy(), prop.reshape(-1)[grp]]))
        assert torch.equal(m["f64"][0]["match_idx"][live_rows], want_idx[live_rows])
        m["ref"] = RM.loss(m["f64"][0]["lang_cap"].detach().numpy(), gt_ids, good, samples, rw.length, rw.reward, bs.reward, count,
                           S_SAMPLES, XE_WEIGHT)
        res[mode] = m
    res["ce_after"] = _run(cap, ep)

    # lang_label narrower than the samples' token rows: the ground-truth rows are padded with the pad id 0
    cut = dict(ep, lang_label=ep["lang_label"][:, :20].contiguous())
    res["ce_cut"] = _run(cap, cut)
    try:
        cap.self_critical = mk("referred", reward=REWARD, xe_weight=XE_WEIGHT)
        res["mixed_cut"] = _run(cap, cut)
    finally:
        del cap.self_critical
    return res


@pytest.mark.parametrize("mode", MODES)
def test_training_forward_samples_and_rewards(world, mode):
    m, B = world[mode], world["B"]
    out, base_out = m["mixed"][0], m["cider_only"][0]
    rw, bs, Mg, S = m["rw"], m["bs"], m["Mg"], S_SAMPLES
    lead = (B, Mg) if mode == "matched" else (B,)
    assert "lang_cap" not in out and "_cap_vec" not in out
    assert tuple(out["scst_reward_terms"].shape) == lead + (S, 3) and tuple(out["scst_baseline_terms"].shape) == lead + (3,)
    assert out["scst_reward_terms"].dtype == torch.float64 and tuple(out["scst_stats"].shape) == (12,)
    assert "scst_reward_terms" not in base_out and "scst_xe_loss" not in base_out and tuple(base_out["scst_stats"].shape) == (8,)
    # the samples do not depend on the reward: bit-equal to the CIDEr-only run's, and so is the CIDEr column
    assert torch.equal(out["scst_samples"], base_out["scst_samples"])
    assert _bits(out["scst_reward_terms"][..., 0]) == _bits(base_out["scst_reward"])
    assert _bits(out["scst_baseline_terms"][..., 0]) == _bits(base_out["scst_baseline"])
    terms = out["scst_reward_terms"].cpu().numpy().reshape(-1, 3)
    bterms = out["scst_baseline_terms"].cpu().numpy().reshape(-1, 3)
    assert out["scst_reward"].cpu().numpy().reshape(-1).tobytes() == RM.combine(terms, WEIGHTS).tobytes()
    assert out["scst_baseline"].cpu().numpy().reshape(-1).tobytes() == RM.combine(bterms, WEIGHTS).tobytes()
    e_t, e_b = float(np.abs(terms - rw.scores).max()), float(np.abs(bterms - bs.scores).max())
    print(f"{mode}: largest |scst_reward_terms - restated| = {e_t:.3e}, baseline terms {e_b:.3e}; mean terms {terms.mean(0).round(4).tolist()}")
    assert e_t <= REWARD_TOL and e_b <= REWARD_TOL and (terms > 0).any(0).all()
    count = m["count"]
    assert count.any() and (mode == "referred" or not count.all())                    # (the matched scenes leave a slot empty)
    adv = out["scst_advantage"].cpu().numpy().reshape(-1)
    A64, _ = SC.advantage(rw.reward, bs.reward, count, S)
    assert np.abs(adv - A64).max() <= 2.0 ** -24 * np.abs(A64).max() + 4 * REWARD_TOL
    assert (np.abs(adv) > 1e-3).mean() >= 0.4
    # what the cross-entropy path leaves, as it leaves it
    ce = world["ce_before"][0]
    for k in ("match_idx", "good_bbox_masks", "pred_ious"):
        assert torch.equal(out[k], ce[k]), k
    assert bool(out["good_bbox_masks"].any())


@pytest.mark.parametrize("mode", MODES)
def test_training_forward_loss_and_gradients(world, mode):
    m = world[mode]
    (out, grads), ref = m["mixed"], m["ref"]
    o64, v64, g64 = m["f64"]
    assert abs(float(v64) - ref.loss) <= LR.F64_BAR * max(1.0, ref.labs)               # torch float64 and numpy float64 agree
    loss, stats = float(out["_cap_loss"][0].detach()), out["scst_stats"].cpu().numpy().astype(np.float64)
    e = abs(loss - ref.loss) / (LR.CAP_LOSS_REL * max(1.0, ref.labs))
    # the cross-entropy term against the plain cross-entropy forward's own loss
    ce_loss = float(world["ce_before"][0]["_cap_loss"][0])
    e_xe = abs(float(out["scst_xe_loss"]) - ce_loss) / (LR.CAP_LOSS_REL * max(1.0, abs(ce_loss)))
    e_acc = abs(float(out["scst_xe_acc"]) - float(world["ce_before"][0]["_cap_loss"][1]))
    print(f"{mode}: loss {loss:.7g} vs float64 {ref.loss:.7g} (scale {ref.labs:.3g}): excess {e:.3g}; L_rl {stats[1]:.6g} vs {ref.l_rl:.6g}, "
          f"L_xe {stats[2]:.6g} vs {ref.l_xe:.6g} and the cross-entropy forward's {ce_loss:.6g}: excess {e_xe:.3g}; acc_xe off by {e_acc:.2g}")
    assert e <= 1 and e_xe <= 1 and e_acc <= LR.CAP_ACC_ABS
    assert loss == float(out["scst_stats"][0]) and float(out["_cap_loss"][1]) == float(out["scst_stats"][3])
    assert abs(stats[1] - ref.l_rl) <= LR.CAP_LOSS_REL * max(1.0, ref.rl.labs) and abs(stats[2] - ref.l_xe) <= LR.CAP_LOSS_REL * max(1.0, ref.l_xe)
    assert torch.equal(m["mixed_again"], out["_cap_loss"][0].detach())                 # the same bits at the same seed
    # gradients: four times the deviation of the existing cross-entropy path from ITS float64 oracle, per tensor (section 7j's)
    ce_g, ce64_g = world["ce_before"][1], world["ce64"][2]
    assert abs(ce_loss - float(world["ce64"][1])) <= LR.CAP_LOSS_REL * max(1.0, abs(float(world["ce64"][1])))
    bad = []
    for k in GRAD_TENSORS:
        f_ce = LR.figure(ce_g[k].cpu().numpy(), ce64_g[k].numpy())
        f_mx = LR.figure(grads[k].cpu().numpy(), g64[k].numpy())
        print(f"{mode} {k}: cross-entropy path {f_ce:.3e}, mixed self-critical path {f_mx:.3e} (allowed {4 * f_ce:.3e}); "
              f"largest reference entry {float(g64[k].abs().max()):.3e}")
        if not f_mx <= 4 * f_ce:
            bad.append(k)
    assert not bad, bad


def test_narrower_ground_truth_rows_are_padded(world):
    """``lang_label`` of 20 columns beside the samples' 33: the cross-entropy term is the plain forward's on the same batch."""
    ce, mx = world["ce_cut"][0], world["mixed_cut"][0]
    a, b = float(ce["_cap_loss"][0]), float(mx["scst_xe_loss"])
    print(f"cross-entropy over 18 word positions: plain forward {a:.7g}, mixed forward {b:.7g}")
    assert abs(a - b) <= LR.CAP_LOSS_REL * max(1.0, abs(a)) and abs(float(ce["_cap_loss"][1]) - float(mx["scst_xe_acc"])) <= LR.CAP_ACC_ABS
    assert torch.equal(mx["scst_samples"], world["referred"]["mixed"][0]["scst_samples"])


def test_without_the_attribute_forward_train_is_bit_equal(world):
    (o0, g0), (o1, g1) = world["ce_before"], world["ce_after"]
    assert world["cap"].self_critical is None
    for k in ("lang_cap", "_cap_vec", "match_idx", "good_bbox_masks", "pred_ious"):
        assert torch.equal(o0[k], o1[k]), k
    assert torch.equal(o0["_cap_loss"][0], o1["_cap_loss"][0]) and torch.equal(o0["_cap_loss"][1], o1["_cap_loss"][1])
    for k in GRAD_TENSORS:
        assert torch.equal(g0[k], g1[k]), k
    assert not any(k.startswith("scst_") for k in o1)


# ---- (d) Trainer -----------------------------------------------------------------------------------------------------------
def _mixed_settings(mode):
    def make(cap, B):
        from spacap3d_amd.caption_eval import CaptionCorpus
        from spacap3d_amd.self_critical import SelfCritical
        idx2word = {i: w for w, i in cap.word_to_idx.items()}
        rng = np.random.default_rng(3)
        nkeys = 2 * B
        corpus = {"k%d" % i: ["sos " + " ".join(idx2word[int(t)] for t in rng.integers(4, 120, 12)) + " eos" for _ in range(2)]
                  for i in range(nkeys)}
        table = np.full((B, 64 + ID_OFFSET), -1, np.int32)
        for i in range(nkeys):
            table[i % B, ID_OFFSET + 2 * (i // B)] = i
        return SelfCritical(CaptionCorpus(corpus, cap.word_to_idx, key_of=table), cap.word_to_idx["sos"], cap.word_to_idx["eos"],
                            num_samples=3, seed=11, proposals=mode, max_proposals=3, reward=REWARD, xe_weight=XE_WEIGHT)
    return make


@pytest.mark.parametrize("mode", MODES)
def test_trainer_steps_eagerly_with_the_mixed_settings(mode):
    from spacap3d_amd import synthetic as SY
    model, tr, data = _small_trainer(None)
    with torch.no_grad():
        probe = model(dict(data))
    data = SY.anchor_boxes_on_proposals(data, probe["aggregated_vote_xyz"])
    B, G = data["box_label_mask"].shape
    data["dataset_idx"] = torch.arange(B, device=DEV)
    data["object_id"] = torch.full((B,), ID_OFFSET, device=DEV)
    data["scene_object_ids"] = (torch.arange(G, device=DEV) + ID_OFFSET).repeat(B, 1)
    model.caption.self_critical = _mixed_settings(mode)(model.caption, B)
    w_cap, w_det = model.caption.model.generator.proj.weight, model.proposal.proposal[-1].weight
    before = (w_cap.detach().clone(), w_det.detach().clone())
    losses = []
    for _ in range(2):                                   # (the deferred weight-gradient check of _core runs in both)
        tr.step(data)
        losses.append({k: float(v) for k, v in tr.last_losses.items()})
    print(f"two eager {mode} steps with the mixed settings: {losses}")
    assert tr.graph is None and tr._eager_checks == 0
    assert all(np.isfinite(v) for h in losses for v in h.values())
    assert not torch.equal(before[0], w_cap) and not torch.equal(before[1], w_det)


def test_default_trainer_is_untouched_by_a_mixed_run():
    from spacap3d_amd import attention

    def two_steps():
        attention._CALL_COUNTER[0] = 1 << 20
        attention.rng_state(torch.device(DEV)).zero_()
        model, tr, data = _small_trainer(None)
        return [tr.step(data).clone() for _ in range(2)]
    first = two_steps()
    model, tr, data = _small_trainer(lambda cap, B: _mixed_settings("referred")(cap, B))
    tr.step(data)
    second = two_steps()
    torch.cuda.synchronize()
    print(f"default losses: {[float(v) for v in first]} and after a mixed self-critical step {[float(v) for v in second]}")
    assert all(torch.equal(a, b) for a, b in zip(first, second))


# ---- (e) refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(world):
    cap, ep, mk = world["cap"], world["ep"], world["mk"]
    try:
        for mode in MODES:
            cap.self_critical = mk(mode, reward=REWARD, xe_weight=XE_WEIGHT)
            for k in ("lang_label", "lang_ids", "ref_center_label"):
                with pytest.raises(KeyError, match=k):
                    cap.forward_train({n: v for n, v in ep.items() if n != k})
        cap.self_critical = mk("referred", reward=REWARD)                             # no cross-entropy term: the caption is not read
        out = cap.forward_train({n: v for n, v in ep.items() if n not in ("lang_label", "lang_ids")})
        assert "scst_reward_terms" in out and "scst_xe_loss" not in out
        cap.self_critical = mk("referred", reward=REWARD, xe_weight=XE_WEIGHT)
        with pytest.raises(RuntimeError, match="self_critical.*not supported"):
            _cpu_copy(cap).forward_train({k: v.cpu() for k, v in ep.items()})
        cap.early_guide = False                                                       # the late guide
        try:
            with pytest.raises(RuntimeError, match="self_critical.*not supported"):
                cap.forward_train(dict(ep))
        finally:
            cap.early_guide = True
        enc = cap.model.encoder                                                       # a captioner without the encoder
        cap.model.encoder = None
        try:
            with pytest.raises(RuntimeError, match="self_critical.*not supported"):
                cap.forward_train(dict(ep))
        finally:
            cap.model.encoder = enc
        cap.eval()                                                                    # eval mode does not read the attribute
        with torch.no_grad():
            assert "scst_reward" not in cap.forward_train(dict(ep))
    finally:
        cap.train()
        del cap.self_critical
