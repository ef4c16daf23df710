"""Generates tests/golden/caption_reward_ref.npz by RUNNING THE REFERENCE'S OWN ``BleuScorer`` (lib/capeval/bleu/bleu_scorer.py) and
``Rouge`` (lib/capeval/rouge/rouge.py) on the CPU over the caption rows of self-critical training's tests: per row set of
tests/reward_mix_restated.py (``ROW_SETS``: the rows tests/test_self_critical_cpu.py builds from the ``edge`` and ``random`` cases of
caption_eval_ref.npz, plain and with ``extra``; ``hand``: the hand-made rows) the row's caption -- sos, the decoded words through
the first eos, an eos appended when there was none -- is scored against the references of its key row.  Nothing of the
reference is copied; only numbers are recorded.

Per row set ``<set>/...``:
  key (rows,) i32          the key row of every row (-1: none; such a row records zeros)
  bleu_comp (rows,10) i32  testlen, closest reflen, guess[4], correct[4] of the scorer's ``ctest`` entry
  bleu4 (rows,) f64        ``bleu_list[3]`` of ``compute_score(option="closest")``
  rouge (rows,) f64        ``Rouge().calc_score``
The row tokens are not stored: tests/reward_mix_restated.py rebuilds them from caption_eval_ref.npz with fixed seeds, and the
recorded ``key`` is compared first.

Asserted while generating, so that the fixture cannot pass vacuously -- at least one row each with: the brevity penalty active
(testlen < reflen); a tie in the closest reference length; a clipped count (correct_k below the caption's own count of its
n-grams that occur in some reference); the two-token caption sos eos (guess[2] = guess[3] = 0); the 64-token caption; ROUGE
strictly between 0 and 1; no key row.  And: the numpy restatement reproduces every recorded integer and ROUGE exactly and
BLEU-4 within 1e-12.

Run:  python tests/golden/make_fixtures_reward.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # (tests/losses_restated.py reads the package's constants)
from make_fixtures_postprocess import REF  # noqa: E402
import caption_eval_restated as R  # noqa: E402
import reward_mix_restated as RM  # noqa: E402
import self_critical_restated as SC  # noqa: E402


def score_rows(fix, name):
    from lib.capeval.bleu.bleu_scorer import BleuScorer
    from lib.capeval.rouge.rouge import Rouge

    tokens, didx, oid, table, want_key, case = RM.row_set(fix, name)
    refs = R.refs_of(fix, case)
    rows = len(tokens)
    key = np.asarray([SC.key_row(didx[r], oid[r], table, len(refs)) for r in range(rows)], np.int32)
    np.testing.assert_array_equal(key, want_key)
    caps = [R.decode(tokens[r], R.SOS, R.EOS) for r in range(rows)]
    keyed = [r for r in range(rows) if key[r] >= 0]
    bs, rouge_scorer = BleuScorer(n=4), Rouge()
    rouge = np.zeros(rows)
    for r in keyed:
        ref_s = [R.sentence(x) for x in refs[key[r]]]
        bs += (R.sentence(caps[r]), ref_s)
        rouge[r] = rouge_scorer.calc_score([R.sentence(caps[r])], ref_s)
    _, bleu_list = bs.compute_score(option="closest")
    comp, bleu4 = np.zeros((rows, 10), np.int32), np.zeros(rows)
    flags = dict.fromkeys(("brevity", "tie", "clipped", "two_token", "lmax", "rouge_between", "no_key"), 0)
    for i, r in enumerate(keyed):
        t = bs.ctest[i]
        comp[r] = [t["testlen"], bs._single_reflen(t["reflen"], "closest", t["testlen"])] + t["guess"] + t["correct"]
        bleu4[r] = bleu_list[3][i]
        lens = [len(x) for x in refs[key[r]]]
        diffs = sorted(abs(l - len(caps[r])) for l in set(lens))
        own = R.ngrams(caps[r])
        in_refs = set(g for x in refs[key[r]] for g in R.ngrams(x))
        own_k = [sum(c for g, c in own.items() if len(g) == k + 1 and g in in_refs) for k in range(4)]
        flags["brevity"] += comp[r, 0] < comp[r, 1]
        flags["tie"] += len(diffs) > 1 and diffs[0] == diffs[1]
        flags["clipped"] += any(comp[r, 6 + k] < own_k[k] for k in range(4))
        flags["two_token"] += len(caps[r]) == 2 and comp[r, 4] == 0 and comp[r, 5] == 0
        flags["lmax"] += len(caps[r]) == R.LMAX
        flags["rouge_between"] += 0.0 < rouge[r] < 1.0
    flags["no_key"] = int((key < 0).sum())

    # the restatement reproduces what was recorded
    got = RM.rewards(SC.Corpus(refs), tokens, 1, didx, oid, table, R.SOS, R.EOS, (0.0, 1.0, 1.0))
    np.testing.assert_array_equal(got.bleu_comp, comp)
    assert got.scores[:, 2].tobytes() == rouge.tobytes()
    err = float(np.abs(got.scores[:, 1] - bleu4).max())
    assert err <= 1e-12, err
    print(f"{name}: {rows} rows, {len(keyed)} with a key row, BLEU-4 up to {bleu4.max():.4f} (restated within {err:.2e}), "
          f"ROUGE up to {rouge.max():.4f}; rows with {flags}")
    return {f"{name}/key": key, f"{name}/bleu_comp": comp, f"{name}/bleu4": bleu4, f"{name}/rouge": rouge}, flags


def main():
    fix = np.load(os.path.join(HERE, "caption_eval_ref.npz"))
    os.chdir(REF)
    sys.path.insert(0, REF)
    out, total = {}, {}
    for name in RM.ROW_SET_NAMES:
        o, flags = score_rows(fix, name)
        out.update(o)
        for k, v in flags.items():
            total[k] = total.get(k, 0) + int(v)
    missing = [k for k, v in total.items() if v == 0]
    assert not missing, f"no row with: {missing}"
    path = os.path.join(HERE, "caption_reward_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", sum(len(v) for k, v in out.items() if k.endswith("/key")), "rows;", total)


if __name__ == "__main__":
    main()
