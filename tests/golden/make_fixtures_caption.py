"""Generates tests/golden/caption_eval_ref.npz by RUNNING THE REFERENCE'S OWN caption evaluation in this container:
``Bleu(4)``, ``Cider()`` and ``Rouge()`` of lib/capeval (with ``BleuScorer`` once more for the per-key components) and, for
the selection case, ``feed_scene_cap`` itself (lib/eval_helper.py:78-245) followed by ``check_candidates`` /
``organize_candidates``.  Nothing of the reference is copied.

``feed_scene_cap`` runs under stubs in the manner of make_fixtures_postprocess.install_stubs: ``ScannetDatasetConfig`` is
replaced before lib/eval_helper.py is imported (its constructor reads a ScanNet label file), the model is the identity,
``get_scene_cap_loss`` passes the dict through, ``parse_predictions`` stores the recorded NMS mask as ``pred_mask``,
``Tensor.cuda`` is the identity, and the dataset is a namespace with ``scanrefer`` and ``vocabulary``.  The reference's
``box3d_iou_batch_tensor`` still runs: a proposal's box is its assigned ground-truth box (IoU 1) or that box moved away
(IoU 0), which gives the recorded ``good_bbox_masks``.

Words: ids 0..3 are pad_ / unk / sos / eos, every other id i is the word ``w<i>``; ids at or above a case's ``vocab`` are
words outside the vocabulary (tests/caption_eval_restated.py: ``word``).  Per case ``<case>/...``:
  ref_tok, ref_len, key_nref   the references as ids (CSR, keys in corpus order), vocab
  cand_tok (NKEYS,64), cand_len   the candidates scored
  bleu_comp (NKEYS,10)         testlen, closest reflen, guess[4], correct[4] of the reference's BleuScorer
  bleu (4,), cider, cider_scores, rouge, rouge_scores   what the three scorers return
Cases:
  edge    hand-built keys: placeholder candidate; candidate shorter / longer than every reference; a closest-length tie
          (references of testlen-1 and testlen+1); a repeated n-gram clipped (a a a a against a a); a reference word outside
          the vocabulary (twice, in two keys: it counts in the document frequency); a candidate containing unk; keys with 1
          and with 9 references; a candidate equal to a reference; a 64-token candidate against a 64-token reference; a
          candidate sharing only sos / eos with its references;
  random  300 keys over 40 words (n-grams collide across keys), 1-8 references, 20 % placeholders;
  select  K = 64, L = 31, two steps of 2 scenes: tokens, nms_masks, good_bbox_masks, dataset_idx, scene_object_ids,
          object_assignment (leading axis = step), keys / scene_ids / organized rows (scene, object id, object name),
          key_table, and the candidate table after step 1 (cand_tok_step1, cand_len_step1) and after both.  Covered: two
          passing proposals of one key in a scene, one key in both scenes of a batch, one key in both steps, a key row of
          -1 (an object outside ``organized``: KeyError; and one whose key is not in the corpus), each mask off in turn, no
          eos, eos first, junk after eos, keys never hit.
Asserted while generating: the numpy restatement reproduces every recorded value (integers and ROUGE exactly, CIDEr within
1e-12); per case a key with CIDEr > 0, a key with ROUGE strictly between 0 and 1 and a key with brevity ratio < 1.

Run:  python tests/golden/make_fixtures_caption.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_fixtures_postprocess import REF, corners_of, install_stubs  # noqa: E402
import caption_eval_restated as R  # noqa: E402

SOS, EOS, UNK = R.SOS, R.EOS, R.UNK


def wrap(body):
    return [SOS] + [int(x) for x in body] + [EOS]


def edge_case():
    V = 60
    a, b, c, d, e, f = 10, 11, 12, 13, 14, 15
    oov1, oov2 = V + 5, V + 9
    long64 = list(range(4, 4 + 31)) + list(range(4, 4 + 31))                # 62 words + sos + eos = 64 tokens
    long64_ref = long64[:20] + [50] + long64[21:40] + [51] + long64[41:]
    keys = [
        ([SOS, EOS], [wrap([a, b, c]), wrap([a, b])]),                                    # placeholder
        (wrap([a, b]), [wrap([a, b, c, d, e]), wrap([a, b, c, d, e, f, a])]),            # shorter than every reference
        (wrap([a, b, c, d, e, f, a, b]), [wrap([a, b]), wrap([a, c, d])]),               # longer than every reference
        (wrap([a, b, c, d]), [wrap([a, b, c]), wrap([a, b, c, d, e])]),                  # closest-length tie: 5 and 7 around 6
        (wrap([a, a, a, a]), [wrap([a, a]), wrap([b, a])]),                              # clipping
        (wrap([a, b, c]), [wrap([a, oov1, c]), wrap([oov1, oov2])]),                     # words outside the vocabulary
        (wrap([b, c]), [wrap([b, oov1, c])]),                                            # ... the same word in another key
        (wrap([a, UNK, c, UNK]), [wrap([a, b, c, d]), wrap([a, UNK, c])]),               # candidate with unk
        (wrap([d, e, f]), [wrap([d, e, f, a])]),                                         # one reference
        (wrap([a, b, c, d, e]), [wrap([a, b, c, d, e][:n] + [f] * (n % 3)) for n in range(1, 10)]),   # nine references
        (wrap([c, d, e, f]), [wrap([a, b]), wrap([c, d, e, f]), wrap([f, e, d, c])]),    # equal to a reference
        (wrap(long64), [wrap(long64_ref), wrap(long64[:30])]),                           # LMAX edge
        (wrap([20, 21, 22]), [wrap([a, b, c]), wrap([d, e])]),                           # shares only sos / eos
        (wrap([a, b, a, b, a, b]), [wrap([a, b, a, b]), wrap([b, a, b, a, b, a, b])]),   # repeated bigrams on both sides
        (wrap([e, d, c, b, a]), [wrap([a, b, c, d, e]), wrap([e, d, a, b, c])]),         # reordered: LCS < length
        (wrap([a]), [wrap([a]), wrap([a, a])]),                                          # three tokens: no 4-gram
    ]
    assert len(keys[11][0]) == 64 and len(keys[11][1][0]) == 64
    return V, [k[0] for k in keys], [k[1] for k in keys]


def random_case(nk=300, seed=3, V=40):
    rng = np.random.default_rng(seed)
    cands, refs = [], []
    for _ in range(nk):
        nr = int(rng.integers(1, 9))
        cur = []
        base = rng.integers(4, V, int(rng.integers(3, 31)))
        for _ in range(nr):
            t = base.copy()
            m = rng.random(len(t)) < 0.3
            t[m] = rng.integers(4, V, m.sum())
            cur.append(wrap(t[: int(rng.integers(1, len(t) + 1))]))
        refs.append(cur)
        if rng.random() < 0.2:
            cands.append([SOS, EOS])
        else:
            t = base.copy()
            m = rng.random(len(t)) < 0.3
            t[m] = rng.integers(4, V, m.sum())
            cands.append(wrap(t[: int(rng.integers(1, len(t) + 1))]))
    return V, cands, refs


def score_case(name, V, cands, refs, out):
    """Runs the reference's scorers on the word strings and records inputs and outputs."""
    import lib.capeval.bleu.bleu as capbleu
    import lib.capeval.cider.cider as capcider
    import lib.capeval.rouge.rouge as caprouge
    from lib.capeval.bleu.bleu_scorer import BleuScorer

    keys = ["k%d" % i for i in range(len(cands))]
    corpus = {k: [R.sentence(r) for r in rs] for k, rs in zip(keys, refs)}
    cand = {k: [R.sentence(c)] for k, c in zip(keys, cands)}
    bleu, _ = capbleu.Bleu(4).compute_score(corpus, cand)
    cider, cider_scores = capcider.Cider().compute_score(corpus, cand)
    rouge, rouge_scores = caprouge.Rouge().compute_score(corpus, cand)
    bs = BleuScorer(n=4)
    for k in keys:
        bs += (cand[k][0], corpus[k])
    comp = np.array([[t["testlen"], bs._single_reflen(t["reflen"], "closest", t["testlen"])] + t["guess"] + t["correct"]
                     for t in bs.ctest], np.int64)

    tok = np.zeros((len(cands), R.LMAX), np.int32)
    ln = np.array([len(c) for c in cands], np.int32)
    for i, c in enumerate(cands):
        tok[i, :len(c)] = c
    got = R.score_all(tok, ln, refs)
    np.testing.assert_array_equal(got["bleu_comp"], comp)
    assert got["bleu"] == list(bleu), (got["bleu"], bleu)
    assert got["rouge_scores"].tobytes() == np.asarray(rouge_scores, np.float64).tobytes()
    assert got["rouge"] == float(rouge)
    assert np.max(np.abs(got["cider_scores"] - cider_scores)) <= 1e-12, np.max(np.abs(got["cider_scores"] - cider_scores))
    assert abs(got["cider"] - float(cider)) <= 1e-12
    assert (cider_scores > 0).any() and ((rouge_scores > 0) & (rouge_scores < 1)).any()
    assert (comp[:, 0] < comp[:, 1]).any(), "no key with a brevity ratio < 1"
    out.update({f"{name}/vocab": np.array(V), f"{name}/ref_tok": np.array([t for rs in refs for r in rs for t in r], np.int32),
                f"{name}/ref_len": np.array([len(r) for rs in refs for r in rs], np.int32),
                f"{name}/key_nref": np.array([len(rs) for rs in refs], np.int32), f"{name}/cand_tok": tok,
                f"{name}/cand_len": ln, f"{name}/bleu_comp": comp.astype(np.int32), f"{name}/bleu": np.array(bleu, np.float64),
                f"{name}/cider": np.array(float(cider)), f"{name}/cider_scores": np.asarray(cider_scores, np.float64),
                f"{name}/rouge": np.array(float(rouge)), f"{name}/rouge_scores": np.asarray(rouge_scores, np.float64)})
    print(f"{name}: {len(keys)} keys, BLEU {['%.4f' % b for b in bleu]}, CIDEr {cider:.4f} ({int((cider_scores > 0).sum())} keys > 0), "
          f"ROUGE {rouge:.4f} ({int((rouge_scores < 1).sum())} keys < 1), ratio < 1 on {int((comp[:, 0] < comp[:, 1]).sum())} keys")


def select_case(out):
    import torch
    import data.scannet.model_util_scannet as mus
    mus.ScannetDatasetConfig = lambda: types.SimpleNamespace(num_class=18)     # its constructor reads a ScanNet label file
    import lib.eval_helper as EH

    torch.Tensor.cuda = lambda self, *a, **k: self
    V, K, L, M = 50, 64, 31, 8
    rng = np.random.default_rng(5)
    # corpus keys (scene, object id, name); "sB|9|lamp" is in organized but NOT in the corpus; object 7 of sA is in neither
    rows = [("sA", 0, "chair"), ("sA", 1, "table"), ("sA", 2, "sofa"), ("sA", 3, "desk"), ("sB", 0, "bed"), ("sB", 4, "door"),
            ("sB", 5, "sink"), ("sC", 2, "shelf")]
    org_rows = rows + [("sB", 9, "lamp")]
    keys = ["%s|%d|%s" % r for r in rows]
    corpus = {k: [R.sentence(wrap(rng.integers(4, V, int(rng.integers(3, 9))))) for _ in range(int(rng.integers(1, 4)))]
              for k in keys}
    organized = {}
    for s, o, n in org_rows:
        organized.setdefault(s, {})[str(o)] = {"0": {"object_name": n}, "1": {"object_name": n + "_other"}}
    scene_ids = ["sA", "sB", "sA", "sC", "sB"]                     # dataset items 0..4 (two items per scene, as annotations)
    n_obj = 10
    key_table = np.full((len(scene_ids), n_obj), -1, np.int32)
    for i, s in enumerate(scene_ids):
        for row, (rs, o, n) in enumerate(rows):
            if rs == s:
                key_table[i, o] = row

    tokens = rng.integers(4, V, (2, 2, K, L)).astype(np.int64)
    eos_at = rng.integers(2, L, (2, 2, K))
    for idx in np.ndindex(2, 2, K):
        tokens[idx][eos_at[idx]] = EOS                           # one eos somewhere; what follows is junk (more words)
    nms = np.zeros((2, 2, K), np.int64)
    good = np.zeros((2, 2, K), bool)
    bbox_mask = np.ones((2, 2, K), np.int64)
    pred_mask = np.zeros((2, 2, K), np.int64)
    oa = rng.integers(0, M, (2, 2, K)).astype(np.int64)
    dataset_idx = np.array([[0, 1], [2, 0]], np.int64)           # step 0: sA, sB; step 1: sA (another item) and sA again
    ids = np.zeros((2, 2, M), np.int64)
    ids[:, :] = [0, 1, 2, 3, 7, 7, 7, 7]                         # sA: slots 4.. hold object 7 (KeyError -> -1)
    ids[0, 1] = [0, 4, 5, 9, 9, 0, 4, 11]                        # sB: object 9 has no corpus key, 11 is outside the table

    def hit(s, b, k, slot, pm=1, bm=1, gd=True):
        pred_mask[s, b, k], bbox_mask[s, b, k], good[s, b, k], oa[s, b, k] = pm, bm, gd, slot

    hit(0, 0, 3, 0); hit(0, 0, 40, 0)                            # two passing proposals of sA|0 in one scene: 40 wins ...
    hit(1, 0, 5, 0)                                              # ... until step 1 hits sA|0 again (through item 2)
    hit(0, 0, 10, 1); hit(0, 0, 11, 2, pm=0); hit(0, 0, 12, 2, bm=0); hit(0, 0, 13, 2, gd=False)   # each mask off in turn
    hit(0, 0, 20, 4); hit(0, 1, 21, 3); hit(0, 1, 22, 7)         # key row -1: KeyError, key outside the corpus, id outside
    hit(0, 1, 7, 1); hit(0, 1, 30, 6)                            # sB|4 twice in one scene (slots 1 and 6)
    hit(1, 1, 2, 0)                                              # ... and once more in the OTHER scene of that batch
    hit(1, 0, 9, 3); hit(1, 1, 50, 2)                            # sA|3, sA|2 in step 1
    hit(0, 1, 33, 5)                                             # sB|0 through slot 5, step 0 only
    tokens[0, 0, 10, :] = rng.integers(4, V, L)                  # no eos at all
    tokens[1, 0, 9, 0] = EOS                                     # eos first
    tokens[1, 1, 50, 2] = EOS; tokens[1, 1, 50, 3:] = rng.integers(4, V, L - 3)   # junk after an early eos
    nms[:] = pred_mask * bbox_mask

    gt = corners_of(rng.uniform(-3, 3, (M, 3)), rng.uniform(0.4, 1.0, (M, 3))).astype(np.float32)

    def batch(s):
        assigned = gt[oa[s]].astype(np.float64)                   # (2, K, 8, 3)
        corners = assigned + np.where(good[s], 0.0, 50.0)[..., None, None]
        return {"lang_cap": torch.from_numpy(tokens[s]), "dataset_idx": torch.from_numpy(dataset_idx[s]),
                "pred_mask_in": torch.from_numpy(pred_mask[s]), "bbox_mask": torch.from_numpy(bbox_mask[s]),
                "scene_object_ids": torch.from_numpy(ids[s]), "object_assignment": torch.from_numpy(oa[s]),
                "gt_box_corner_label": torch.from_numpy(np.broadcast_to(gt, (2, M, 8, 3)).copy()),
                "bbox_corner": torch.from_numpy(corners)}

    def fake_parse(d, cfg):
        d["pred_mask"] = d["pred_mask_in"].numpy()
        return None

    EH.get_scene_cap_loss = lambda d, *a, **k: d
    EH.parse_predictions = fake_parse
    dataset = types.SimpleNamespace(scanrefer=[{"scene_id": s} for s in scene_ids],
                                    vocabulary={"idx2word": {str(i): R.word(i) for i in range(V)}})
    model = lambda d, is_eval: d
    w2i = R.vocabulary(V)

    def run(steps):
        cand = EH.feed_scene_cap(model, "cpu", dataset, [batch(s) for s in steps], "unused", organized=organized)
        raw = set(cand)
        cand = EH.organize_candidates(corpus, EH.check_candidates(corpus, cand))
        assert list(cand) == keys
        tok = np.zeros((len(keys), R.LMAX), np.int32)
        ln = np.zeros(len(keys), np.int32)
        for i, k in enumerate(keys):
            t = [w2i[w] for w in cand[k][0].split()]
            tok[i, :len(t)], ln[i] = t, len(t)
        return tok, ln, raw

    tok1, ln1, _ = run([0])
    tok2, ln2, raw = run([0, 1])
    assert "sB|9|lamp" in raw                                     # built by the reference, dropped by organize_candidates
    table = R.new_table(len(keys), SOS, EOS)
    R.select(table, tokens[0], nms[0], good[0], dataset_idx[0], ids[0], oa[0], key_table, SOS, EOS)
    np.testing.assert_array_equal(table[0], tok1)
    np.testing.assert_array_equal(table[1], ln1)
    R.select(table, tokens[1], nms[1], good[1], dataset_idx[1], ids[1], oa[1], key_table, SOS, EOS)
    np.testing.assert_array_equal(table[0], tok2)
    np.testing.assert_array_equal(table[1], ln2)
    row = {k: i for i, k in enumerate(keys)}
    assert list(tok2[row["sA|1|table"], :ln2[row["sA|1|table"]]]) == [SOS] + list(tokens[0, 0, 10]) + [EOS] and ln2[row["sA|1|table"]] == L + 2
    assert list(tok2[row["sA|3|desk"], :2]) == [SOS, EOS] and ln2[row["sA|3|desk"]] == 2     # eos first = the placeholder's tokens
    assert ln1[row["sA|2|sofa"]] == 2 and ln2[row["sA|2|sofa"]] == 4                        # masks off in step 1; junk after eos
    assert list(tok1[row["sA|0|chair"], 1:4]) == list(tokens[0, 0, 40, :3]) and list(tok2[row["sA|0|chair"], 1:4]) == list(tokens[1, 1, 2, :3])
    assert list(tok2[row["sB|4|door"], 1:4]) == list(tokens[0, 1, 30, :3])
    assert list(tok1[row["sB|0|bed"], 1:4]) == list(tokens[0, 1, 33, :3]) and np.array_equal(tok1[row["sB|0|bed"]], tok2[row["sB|0|bed"]])
    assert ln2[row["sB|5|sink"]] == 2 and ln2[row["sC|2|shelf"]] == 2                       # never hit
    refs = [[[w2i[w] for w in s.split()] for s in corpus[k]] for k in keys]
    out.update({"select/vocab": np.array(V), "select/keys": np.array(keys), "select/scene_ids": np.array(scene_ids),
                "select/organized": np.array([[s, str(o), n] for s, o, n in org_rows]), "select/key_table": key_table,
                "select/ref_tok": np.array([t for rs in refs for r in rs for t in r], np.int32),
                "select/ref_len": np.array([len(r) for rs in refs for r in rs], np.int32),
                "select/key_nref": np.array([len(rs) for rs in refs], np.int32),
                "select/tokens": tokens, "select/nms_masks": nms, "select/good_bbox_masks": good,
                "select/dataset_idx": dataset_idx, "select/scene_object_ids": ids, "select/object_assignment": oa,
                "select/cand_tok_step1": tok1, "select/cand_len_step1": ln1, "select/cand_tok": tok2, "select/cand_len": ln2})
    print(f"select: {len(keys)} keys, lengths after step 1 {ln1.tolist()}, after step 2 {ln2.tolist()}")
    return V, tok2, ln2, refs


def main():
    install_stubs()
    os.chdir(REF)
    sys.path.insert(0, REF)
    out = {}
    score_case("edge", *edge_case(), out)
    score_case("random", *random_case(), out)
    select_case(out)
    path = os.path.join(HERE, "caption_eval_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
