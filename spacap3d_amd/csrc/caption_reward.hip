// Rewards for self-critical caption training on gfx950 (MI355X): up to three scores per DRAWN caption -- CIDEr-D, sentence-level
// BLEU-4 and ROUGE-L -- and their weighted sum, where caption_score_kernel (caption_eval.hip) scores one candidate per corpus
// key.  The reference has no self-critical training; the semantics are the project's own (DESIGN.md sections 7j and 7l,
// restated in tests/self_critical_restated.py and tests/reward_mix_restated.py).
//
// caption_reward_kernel (spacap_caption_reward_mix_f64; spacap_caption_reward_f64 is the same launch at weights (1, 0, 0)), one
// wave per row, one lane per token position, one launch, no atomics, no state between rows.  Row r belongs to scene
// b = r / rows_per_scene; the scene's key row is key_table[dataset_idx[b]][object_id[b]] (any index outside its table, or an
// entry outside 0..nkeys-1: no row -- caption_row's rule, caption_eval.hip).  The row's caption is decode_caption
// (eval_common.hpp) of its L decoded words: sos, the words through the first eos, an eos appended when there was none.  Against
// the references of the key row:
//   cider   CIDEr-D (n = 4, sigma = 6, x 10 / references): the arithmetic of cider_common.hpp in caption_score_kernel's order,
//           the same bits that kernel writes for this caption as the key's candidate;
//   bleu4   the sentence-level BLEU-4 the reference's scorer appends to bleu_list[3] (bleu_scorer.py:232-240) from the ten
//           components caption_score_kernel writes (closest reference length, clipped counts), float64;
//   rouge   ROUGE-L F-measure (rouge.py:45-75, beta 1.2), the bit-parallel LCS and the same bits caption_score_kernel writes;
//   reward  ((w_cider cider) + (w_bleu bleu4)) + (w_rouge rouge), float64, un-contracted.
// A term whose weight is exactly 0 is not computed: its output is +0.0 and it adds +0.0 (the ten components are zeros when
// w_bleu is 0).  The weights are kernel arguments, so every branch on them is uniform over the grid.  Next to the scores the
// row's teacher-forcing tokens are written: sos, the words through the first eos, zeros behind them (the pad id 0 is what
// caption_prep builds its mask from).
#include <math.h>

#include "bleu_rouge_common.hpp"

namespace {

using namespace spacap::eval;

struct RewardArgs {
  const int64_t *tokens;        // [rows, L]
  const int64_t *dataset_idx;   // [rows / rows_per_scene]
  const int64_t *object_id;     // [rows / rows_per_scene]
  const int32_t *key_table;     // [n_items, n_obj]
  int rows_per_scene, L, n_items, n_obj, nkeys, sos, eos;
  CiderRefs refs;
  CiderTables df;
  double w_cider, w_bleu, w_rouge;
  double *cider;                // [rows]  (each of the four score outputs and bleu_comp may be null: not written)
  double *bleu4;                // [rows]
  double *rouge;                // [rows]
  double *reward;               // [rows]
  int32_t *bleu_comp;           // [rows, 10]: testlen, reflen, guess[4], correct[4]
  int32_t *key;                 // [rows]: -1 = no key row
  int32_t *length;              // [rows]: decoded words through the first eos (L: none)
  int64_t *tf_tok;              // [rows, L + 2]
};

// MIX = false is the body with CIDEr-D alone, for weights (w_cider != 0, 0, 0): the BLEU and ROUGE branches fold away at compile
// time and the launch keeps the registers and the time it had before there were three terms.  Same functions, same order, same
// bits either way.
template <bool MIX>
__global__ __launch_bounds__(CE_LMAX) void caption_reward_kernel(RewardArgs a) {
  __shared__ int s_tok[CE_LMAX];
  __shared__ uint64_t s_cc[4][CE_LMAX];             // candidate n-gram codes
  __shared__ uint64_t s_rc[4][CE_LMAX];             // reference n-gram codes
  const int row = blockIdx.x, lane = threadIdx.x, b = row / a.rows_per_scene;
  const bool do_c = MIX ? a.w_cider != 0.0 : true, do_b = MIX && a.w_bleu != 0.0, do_r = MIX && a.w_rouge != 0.0;   // uniform over the grid

  int key = -1;                                      // uniform over the wave
  {
    const int64_t item = a.dataset_idx[b], oid = a.object_id[b];
    if (item >= 0 && item < a.n_items && oid >= 0 && oid < a.n_obj) {
      const int k = a.key_table[(size_t)item * a.n_obj + oid];
      key = k >= 0 && k < a.nkeys ? k : -1;
    }
  }

  const int tok = lane < a.L ? (int)a.tokens[(size_t)row * a.L + lane] : 0;   // (a token is compared as the int it is stored as)
  int lc;
  const int word = decode_caption(tok, lane, a.L, a.sos, a.eos, lc);           // lc = 1 + words through eos (+ 1: eos appended)
  const int len = lc - 1 > a.L ? a.L : lc - 1;                                 // decoded words through the first eos
  if (lane < a.L + 2) a.tf_tok[(size_t)row * (a.L + 2) + lane] = lane <= len ? (int64_t)word : 0;
  if (lane == 0) {
    a.key[row] = key;
    a.length[row] = len;
  }
  if (key < 0) {
    if (lane == 0) {
      if (a.cider) a.cider[row] = 0.0;
      if (a.bleu4) a.bleu4[row] = 0.0;
      if (a.rouge) a.rouge[row] = 0.0;
      if (a.reward) a.reward[row] = 0.0;
    }
    if (a.bleu_comp && lane < 10) a.bleu_comp[(size_t)row * 10 + lane] = 0;
    return;
  }

  const int ctok = lane < lc ? word : -1;
  s_tok[lane] = ctok;
  __syncthreads();
  uint64_t cc[4];
  ngram_codes(s_tok, lane, cc);
#pragma unroll
  for (int n = 0; n < 4; ++n) s_cc[n][lane] = cc[n];
  __syncthreads();

  CiderCand c;
  if (do_c) cider_candidate(a.df, s_cc, cc, lc, lane, c);
  else if (do_b) ngram_candidate_counts(s_cc, cc, lc, lane, c);
  int maxref[4];
  double score[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) maxref[n] = 0, score[n] = 0.0;

  long long r0 = a.refs.key_ref_off[key], r1 = a.refs.key_ref_off[key + 1];
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > a.refs.n_ref ? a.refs.n_ref : r1;
  BleuClosest closest;
  RougeL rl;
  for (long long r = r0; r < r1; ++r) {              // (uniform over the wave)
    uint64_t rc[4];
    const int lr = cider_stage_reference(a.refs, r, lane, s_tok, s_rc, rc);
    if (do_b) closest.add(lc, lr);
    if (do_r) rl.add(lcs_bitparallel(s_tok, lr, lc, ctok, lane), lc, lr);
    if (do_c) {
      const double penalty = cider_penalty(lc, lr);
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        int cr;
        double val = cider_reference(a.df, s_rc, rc, cc, c, lr, lane, n, cr);
        if (do_b) bleu_clip_add(c, n, cr, maxref);
        val *= penalty;
        score[n] += val;
      }
    } else if (do_b) {
#pragma unroll
      for (int n = 0; n < 4; ++n) bleu_clip_add(c, n, ngram_reference_count(s_rc, cc, lr, n), maxref);
    }
  }

  int correct[4] = {0, 0, 0, 0};
  if (do_b) {
#pragma unroll
    for (int n = 0; n < 4; ++n) correct[n] = bleu_correct(c, n, maxref);
  }
  if (a.bleu_comp && !do_b && lane < 10) a.bleu_comp[(size_t)row * 10 + lane] = 0;
  if (lane != 0) return;
  if (a.bleu_comp && do_b) bleu_components(lc, closest.best_len, correct, a.bleu_comp + (size_t)row * 10);
  const double cider = do_c ? cider_finish(score, r1 - r0) : 0.0;
  const double bleu4 = do_b ? bleu4_sentence(lc, closest.best_len, correct) : 0.0;
  const double rouge = do_r ? rl.finish() : 0.0;
  if (a.cider) a.cider[row] = cider;
  if (a.bleu4) a.bleu4[row] = bleu4;
  if (a.rouge) a.rouge[row] = rouge;
  if (a.reward) {
    const double tc = do_c ? a.w_cider * cider : 0.0, tb = do_b ? a.w_bleu * bleu4 : 0.0, tr = do_r ? a.w_rouge * rouge : 0.0;
    a.reward[row] = (tc + tb) + tr;
  }
}

// the checks and the launch both entries share
int launch_reward(const char *what, const int64_t *tokens, int rows, int rows_per_scene, int L, const int64_t *dataset_idx,
                  const int64_t *object_id, const int32_t *key_table, int n_items, int n_obj, int nkeys, int sos, int eos,
                  const int32_t *ref_tok, int64_t n_tok, const int32_t *ref_off, const int32_t *ref_len, int64_t n_ref,
                  const int32_t *key_ref_off, const uint64_t *df_code, const double *df_idf, const int64_t *df_off, double log_nkeys,
                  double w_cider, double w_bleu, double w_rouge, bool mixed, double *cider, int32_t *key, int32_t *length,
                  int64_t *tf_tok, double *bleu4, double *rouge, double *reward, int32_t *bleu_comp, spacap_stream_t stream) {
  SPACAP_REQUIRE(rows >= 0 && rows_per_scene >= 1 && rows % rows_per_scene == 0 && L >= 1 && L + 2 <= CE_LMAX && n_items >= 1 &&
                     n_obj >= 1 && nkeys >= 1 && n_tok >= 0 && n_ref >= 0,
                 "%s: bad sizes (rows=%d rows_per_scene=%d L=%d n_items=%d n_obj=%d nkeys=%d n_tok=%lld n_ref=%lld; rows a multiple "
                 "of rows_per_scene, L + 2 <= %d)",
                 what, rows, rows_per_scene, L, n_items, n_obj, nkeys, (long long)n_tok, (long long)n_ref, CE_LMAX);
  SPACAP_REQUIRE(sos >= 0 && sos <= 65535 && eos >= 0 && eos <= 65535, "%s: bad sizes (sos=%d eos=%d: ids are 16 bits)", what, sos,
                 eos);
  SPACAP_REQUIRE(w_cider >= 0.0 && w_bleu >= 0.0 && w_rouge >= 0.0 && isfinite(w_cider) && isfinite(w_bleu) && isfinite(w_rouge),
                 "%s: bad weights (w_cider=%g w_bleu=%g w_rouge=%g: finite and not negative)", what, w_cider, w_bleu, w_rouge);
  if (rows == 0) return SPACAP_OK;
  SPACAP_REQUIRE(tokens && dataset_idx && object_id && key_table && ref_tok && ref_off && ref_len && key_ref_off && df_code && df_idf &&
                     df_off && cider && key && length && tf_tok && (!mixed || (bleu4 && rouge && reward && bleu_comp)),
                 "%s: null pointer", what);
  SPACAP_REQUIRE(df_off[0] == 0 && df_off[0] <= df_off[1] && df_off[1] <= df_off[2] && df_off[2] <= df_off[3] && df_off[3] <= df_off[4],
                 "%s: bad sizes (df_off must ascend from 0)", what);
  RewardArgs a;
  a.tokens = tokens;
  a.dataset_idx = dataset_idx;
  a.object_id = object_id;
  a.key_table = key_table;
  a.rows_per_scene = rows_per_scene;
  a.L = L;
  a.n_items = n_items;
  a.n_obj = n_obj;
  a.nkeys = nkeys;
  a.sos = sos;
  a.eos = eos;
  a.refs.ref_tok = ref_tok;
  a.refs.ref_off = ref_off;
  a.refs.ref_len = ref_len;
  a.refs.key_ref_off = key_ref_off;
  a.refs.n_tok = n_tok;
  a.refs.n_ref = n_ref;
  a.df.df_code = df_code;
  a.df.df_idf = df_idf;
  for (int i = 0; i < 5; ++i) a.df.df_off[i] = df_off[i];
  a.df.log_nkeys = log_nkeys;
  a.w_cider = w_cider;
  a.w_bleu = w_bleu;
  a.w_rouge = w_rouge;
  a.cider = cider;
  a.bleu4 = bleu4;
  a.rouge = rouge;
  a.reward = reward;
  a.bleu_comp = bleu_comp;
  a.key = key;
  a.length = length;
  a.tf_tok = tf_tok;
  if (w_cider != 0.0 && w_bleu == 0.0 && w_rouge == 0.0)
    hipLaunchKernelGGL(caption_reward_kernel<false>, dim3(rows), dim3(CE_LMAX), 0, spacap::as_stream(stream), a);
  else
    hipLaunchKernelGGL(caption_reward_kernel<true>, dim3(rows), dim3(CE_LMAX), 0, spacap::as_stream(stream), a);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

}  // namespace

extern "C" int spacap_caption_reward_f64(const int64_t *tokens, int rows, int rows_per_scene, int L, const int64_t *dataset_idx,
                                         const int64_t *object_id, const int32_t *key_table, int n_items, int n_obj, int nkeys,
                                         int sos, int eos, const int32_t *ref_tok, int64_t n_tok, const int32_t *ref_off,
                                         const int32_t *ref_len, int64_t n_ref, const int32_t *key_ref_off, const uint64_t *df_code,
                                         const double *df_idf, const int64_t *df_off, double log_nkeys, double *cider, int32_t *key,
                                         int32_t *length, int64_t *tf_tok, spacap_stream_t stream) {
  return launch_reward("spacap_caption_reward_f64", tokens, rows, rows_per_scene, L, dataset_idx, object_id, key_table, n_items, n_obj,
                       nkeys, sos, eos, ref_tok, n_tok, ref_off, ref_len, n_ref, key_ref_off, df_code, df_idf, df_off, log_nkeys, 1.0,
                       0.0, 0.0, false, cider, key, length, tf_tok, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int spacap_caption_reward_mix_f64(const int64_t *tokens, int rows, int rows_per_scene, int L, const int64_t *dataset_idx,
                                             const int64_t *object_id, const int32_t *key_table, int n_items, int n_obj, int nkeys,
                                             int sos, int eos, const int32_t *ref_tok, int64_t n_tok, const int32_t *ref_off,
                                             const int32_t *ref_len, int64_t n_ref, const int32_t *key_ref_off,
                                             const uint64_t *df_code, const double *df_idf, const int64_t *df_off, double log_nkeys,
                                             double w_cider, double w_bleu, double w_rouge, double *cider, int32_t *key,
                                             int32_t *length, int64_t *tf_tok, double *bleu4, double *rouge, double *reward,
                                             int32_t *bleu_comp, spacap_stream_t stream) {
  return launch_reward("spacap_caption_reward_mix_f64", tokens, rows, rows_per_scene, L, dataset_idx, object_id, key_table, n_items,
                       n_obj, nkeys, sos, eos, ref_tok, n_tok, ref_off, ref_len, n_ref, key_ref_off, df_code, df_idf, df_off, log_nkeys,
                       w_cider, w_bleu, w_rouge, true, cider, key, length, tf_tok, bleu4, rouge, reward, bleu_comp, stream);
}
