// Caption metrics for gfx950 (MI355X): the candidate bookkeeping of the reference's feed_scene_cap (lib/eval_helper.py:
// 178-222 with decode_caption, :46-57, and check_candidates, :59-69) and the per-object parts of BLEU-4, CIDEr-D and ROUGE-L
// (lib/capeval/bleu/bleu_scorer.py:60-84, cider/cider_scorer.py:106-181, rouge/rouge.py:45-75) over word IDS: once a word is
// an id (< 65 536) an n-gram is n x 16 bits in a u64 and nothing below is string processing.
//
//  1. caption_stamp_kernel + caption_write_kernel (spacap_caption_select_i32), per batch.  The reference assigns
//     candidates[key] = [caption] in a loop over step, scene, proposal: the LAST write wins.  Pass one gives every counting
//     proposal the stamp base + b*K + k + 1 (base = the proposals of all earlier calls, kept ON THE DEVICE so that a captured
//     call replays with the right value) and takes the maximum per key row (global integer atomicMax: the result is the same
//     for every schedule).  Pass two, one wave per proposal, lets only the holder of a row's stamp write the row: sos, the
//     tokens up to and including the first eos, an eos appended when there was none (decode_caption of eval_common.hpp, as
//     predictions.hip writes its captions); one lane per position, plain stores.
//     The two cells of `counter` hand the base from call to call without a race: pass one reads [0] and writes [1] =
//     base + B*K, pass two reads [1] and writes [0] = [1].
//  2. caption_score_kernel (spacap_caption_score_f64), one wave per key row, one lane per token position, no state between
//     keys.  The candidate and one reference at a time sit in LDS as four arrays of packed n-gram codes.  Per lane and n:
//     whether the position is the first occurrence of its n-gram and how often the n-gram occurs (64 LDS compares), its idf
//     by binary search in the sorted document-frequency table of that n (the only global reads inside the loop; absent =
//     df 0 = log(NKEYS)).  BLEU's clipped counts, CIDEr's clipped tf-idf products and the norms are wave sums over the
//     first-occurrence lanes; the longest common subsequence is the bit-parallel recurrence V' = (V + (V & M)) | (V & ~M)
//     on one u64 (64 tokens are one word), M = the wave's ballot of "candidate token == this reference token".
//
// Arithmetic: -ffp-contract=off (Makefile default).  ROUGE-L is a chain of IEEE divisions, two multiplies and an add in the
// reference's order: bit-equal to Python's.  CIDEr's sums run in wave-reduction order, not the reference's dict order.
#include <math.h>

#include "bleu_rouge_common.hpp"

namespace {

using namespace spacap::eval;

// (CE_LMAX = 64 tokens per sentence = lanes of a wave = bits of the LCS word: cider_common.hpp; the closest reference length,
// the LCS, the clipping and the ROUGE finish: bleu_rouge_common.hpp, shared with caption_reward.hip)

struct SelectArgs {
  const int64_t *tokens;             // [B,K,L]
  const int64_t *nms_mask;           // [B,K]
  const uint8_t *good;               // [B,K]
  const int64_t *dataset_idx;        // [B]
  const int64_t *scene_object_ids;   // [B,M]
  const int64_t *object_assignment;  // [B,K]
  const int32_t *key_table;          // [n_items, n_obj]
  int B, K, L, M, n_items, n_obj, nkeys, sos, eos;
  unsigned long long *stamp;         // [NKEYS]
  unsigned long long *counter;       // [2]
  int32_t *cand_tok;                 // [NKEYS, 64]
  int32_t *cand_len;                 // [NKEYS]
};

// key row of proposal p = b*K + k when it counts, else -1
__device__ __forceinline__ int caption_row(const SelectArgs &a, int b, int p) {
  if (a.nms_mask[p] != 1 || a.good[p] == 0) return -1;
  const int64_t item = a.dataset_idx[b], oa = a.object_assignment[p];
  if (item < 0 || item >= a.n_items || oa < 0 || oa >= a.M) return -1;
  const int64_t oid = a.scene_object_ids[(size_t)b * a.M + oa];
  if (oid < 0 || oid >= a.n_obj) return -1;
  const int row = a.key_table[(size_t)item * a.n_obj + oid];
  return row >= 0 && row < a.nkeys ? row : -1;
}

__global__ __launch_bounds__(256) void caption_stamp_kernel(SelectArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x, n = a.B * a.K;
  const unsigned long long base = a.counter[0];
  if (p == 0) a.counter[1] = base + (unsigned long long)n;
  if (p >= n) return;
  const int row = caption_row(a, p / a.K, p);
  if (row >= 0) atomicMax(&a.stamp[row], base + (unsigned long long)p + 1ull);
}

__global__ __launch_bounds__(CE_LMAX) void caption_write_kernel(SelectArgs a) {
  const int p = blockIdx.x, lane = threadIdx.x, n = a.B * a.K;
  const unsigned long long next = a.counter[1];
  if (p == 0 && lane == 0) a.counter[0] = next;                    // (nobody reads [0] in this pass)
  const int row = caption_row(a, p / a.K, p);                      // uniform over the wave
  if (row < 0 || a.stamp[row] != next - (unsigned long long)n + (unsigned long long)p + 1ull) return;
  const int tok = lane < a.L ? (int)a.tokens[(size_t)p * a.L + lane] : 0;   // (a token is compared as the int it is stored as)
  int len;
  a.cand_tok[(size_t)row * CE_LMAX + lane] = decode_caption(tok, lane, a.L, a.sos, a.eos, len);
  if (lane == 0) a.cand_len[row] = len;
}

// ---- scoring ---------------------------------------------------------------------------------------------------------

struct ScoreArgs {
  const int32_t *cand_tok;      // [NKEYS, 64]
  const int32_t *cand_len;      // [NKEYS]
  CiderRefs refs;               // the references (CSR) and the key rows' ranges
  CiderTables df;               // the document-frequency tables
  int32_t *bleu;                // [NKEYS, 10]: testlen, reflen, guess[4], correct[4]
  double *rouge;                // [NKEYS]
  double *cider;                // [NKEYS]
};

// (the n-gram codes, the idf lookup and CIDEr's per-candidate and per-reference bodies: cider_common.hpp, shared with
// caption_reward.hip)
__global__ __launch_bounds__(CE_LMAX) void caption_score_kernel(ScoreArgs a) {
  __shared__ int s_tok[CE_LMAX];
  __shared__ uint64_t s_cc[4][CE_LMAX];             // candidate n-gram codes
  __shared__ uint64_t s_rc[4][CE_LMAX];             // reference n-gram codes
  const int key = blockIdx.x, lane = threadIdx.x;
  int lc = a.cand_len[key];
  lc = lc < 0 ? 0 : (lc > CE_LMAX ? CE_LMAX : lc);
  const int ctok = lane < lc ? a.cand_tok[(size_t)key * CE_LMAX + lane] : -1;
  s_tok[lane] = ctok;
  __syncthreads();
  uint64_t cc[4];
  ngram_codes(s_tok, lane, cc);
#pragma unroll
  for (int n = 0; n < 4; ++n) s_cc[n][lane] = cc[n];
  __syncthreads();

  CiderCand c;
  cider_candidate(a.df, s_cc, cc, lc, lane, c);
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
    closest.add(lc, lr);
    rl.add(lcs_bitparallel(s_tok, lr, lc, ctok, lane), lc, lr);

    const double penalty = cider_penalty(lc, lr);
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      int cr;
      double val = cider_reference(a.df, s_rc, rc, cc, c, lr, lane, n, cr);
      bleu_clip_add(c, n, cr, maxref);
      val *= penalty;
      score[n] += val;
    }
  }

  int correct[4];
#pragma unroll
  for (int n = 0; n < 4; ++n)
    correct[n] = bleu_correct(c, n, maxref);
  if (lane == 0) {
    bleu_components(lc, closest.best_len, correct, a.bleu + (size_t)key * 10);
    a.rouge[key] = rl.finish();
    a.cider[key] = cider_finish(score, r1 - r0);
  }
}

}  // namespace

extern "C" int spacap_caption_select_i32(const int64_t *tokens, const int64_t *nms_mask, const uint8_t *good_bbox_mask,
                                         const int64_t *dataset_idx, const int64_t *scene_object_ids,
                                         const int64_t *object_assignment, int B, int K, int L, int M, const int32_t *key_table,
                                         int n_items, int n_obj, int nkeys, int sos, int eos, uint64_t *stamp, uint64_t *counter,
                                         int32_t *cand_tok, int32_t *cand_len, spacap_stream_t stream) {
  const char *what = "spacap_caption_select_i32";
  SPACAP_REQUIRE(B >= 0 && B <= 65535 && K >= 1 && K <= 16384 && L >= 1 && L + 2 <= CE_LMAX && M >= 1 && n_items >= 1 && n_obj >= 1 &&
                     nkeys >= 1,
                 "%s: bad sizes (B=%d K=%d L=%d M=%d n_items=%d n_obj=%d nkeys=%d; L + 2 <= %d)", what, B, K, L, M, n_items,
                 n_obj, nkeys, CE_LMAX);
  SPACAP_REQUIRE(sos >= 0 && sos <= 65535 && eos >= 0 && eos <= 65535, "%s: bad sizes (sos=%d eos=%d: ids are 16 bits)", what, sos,
                 eos);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(tokens && nms_mask && good_bbox_mask && dataset_idx && scene_object_ids && object_assignment && key_table && stamp &&
                     counter && cand_tok && cand_len,
                 "%s: null pointer", what);
  SelectArgs a;
  a.tokens = tokens;
  a.nms_mask = nms_mask;
  a.good = good_bbox_mask;
  a.dataset_idx = dataset_idx;
  a.scene_object_ids = scene_object_ids;
  a.object_assignment = object_assignment;
  a.key_table = key_table;
  a.B = B;
  a.K = K;
  a.L = L;
  a.M = M;
  a.n_items = n_items;
  a.n_obj = n_obj;
  a.nkeys = nkeys;
  a.sos = sos;
  a.eos = eos;
  a.stamp = reinterpret_cast<unsigned long long *>(stamp);
  a.counter = reinterpret_cast<unsigned long long *>(counter);
  a.cand_tok = cand_tok;
  a.cand_len = cand_len;
  const int n = B * K;
  hipLaunchKernelGGL(caption_stamp_kernel, dim3((n + 255) / 256), dim3(256), 0, spacap::as_stream(stream), a);
  SPACAP_CHECK_LAUNCH(what);
  hipLaunchKernelGGL(caption_write_kernel, dim3(n), dim3(CE_LMAX), 0, spacap::as_stream(stream), a);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_caption_score_f64(const int32_t *cand_tok, const int32_t *cand_len, int nkeys, const int32_t *ref_tok,
                                        int64_t n_tok, const int32_t *ref_off, const int32_t *ref_len, int64_t n_ref,
                                        const int32_t *key_ref_off, const uint64_t *df_code, const double *df_idf,
                                        const int64_t *df_off, double log_nkeys, int32_t *bleu, double *rouge, double *cider,
                                        spacap_stream_t stream) {
  const char *what = "spacap_caption_score_f64";
  SPACAP_REQUIRE(nkeys >= 0 && n_tok >= 0 && n_ref >= 0, "%s: bad sizes (nkeys=%d n_tok=%lld n_ref=%lld)", what, nkeys,
                 (long long)n_tok, (long long)n_ref);
  if (nkeys == 0) return SPACAP_OK;
  SPACAP_REQUIRE(cand_tok && cand_len && ref_tok && ref_off && ref_len && key_ref_off && df_code && df_idf && df_off && bleu &&
                     rouge && cider,
                 "%s: null pointer", what);
  SPACAP_REQUIRE(df_off[0] == 0 && df_off[0] <= df_off[1] && df_off[1] <= df_off[2] && df_off[2] <= df_off[3] && df_off[3] <= df_off[4],
                 "%s: bad sizes (df_off must ascend from 0)", what);
  ScoreArgs a;
  a.cand_tok = cand_tok;
  a.cand_len = cand_len;
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
  a.bleu = bleu;
  a.rouge = rouge;
  a.cider = cider;
  hipLaunchKernelGGL(caption_score_kernel, dim3(nkeys), dim3(CE_LMAX), 0, spacap::as_stream(stream), a);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
