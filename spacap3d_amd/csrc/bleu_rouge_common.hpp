// The per-caption parts of BLEU-4 (bleu_scorer.py:60-84, :232-240) and ROUGE-L (rouge.py:45-75, beta 1.2) over word ids, by one
// wave with one lane per token position: what caption_score_kernel (caption_eval.hip, one candidate per key row) and
// caption_reward_kernel (caption_reward.hip, one candidate per drawn caption) share, so that each number has ONE definition, as
// cider_common.hpp gives CIDEr-D one.  Both kernels call the functions below per staged reference in the same order and give
// the same bits for the same caption and references.  Compiled with -ffp-contract=off (Makefile default).
#pragma once
#include <math.h>

#include "cider_common.hpp"

namespace spacap::eval {

constexpr double CE_BETA2 = 1.2 * 1.2;              // rouge.py: self.beta ** 2
constexpr double BLEU_SMALL = 1e-9;                 // bleu_scorer.py:201-202
constexpr double BLEU_TINY = 1e-15;

// BLEU's "closest" reference length: min over (|l - testlen|, l), one reference at a time
struct BleuClosest {
  int best_diff = 0x7fffffff, best_len = 0;
  __device__ __forceinline__ void add(int lc, int lr) {
    const int diff = lr > lc ? lr - lc : lc - lr;
    if (diff < best_diff || (diff == best_diff && lr < best_len)) {
      best_diff = diff;
      best_len = lr;
    }
  }
};

// Longest common subsequence of the candidate (lane i holds token ctok, lc tokens) and the reference staged in s_tok (lr
// tokens), bit-parallel over the candidate's positions: V' = (V + (V & M)) | (V & ~M) on one u64, M = the wave's ballot of
// "candidate token == this reference token".  Every lane of the wave calls it and gets the same value.
__device__ __forceinline__ int lcs_bitparallel(const int *s_tok, int lr, int lc, int ctok, int lane) {
  uint64_t V = ~0ull;
  for (int i = 0; i < lr; ++i) {
    const int t = s_tok[i];
    const uint64_t M = __ballot(lane < lc && ctok == t);
    const uint64_t U = V & M;
    V = (V + U) | (V & ~M);
  }
  const uint64_t low = lc >= 64 ? ~0ull : ((1ull << lc) - 1ull);
  return __popcll(~V & low);
}

// ROUGE-L: the largest precision and the largest recall over the references, then the F-measure -- a chain of IEEE divisions,
// two multiplies and an add in the reference's order: bit-equal to Python's
struct RougeL {
  double pmax = 0.0, rmax = 0.0;
  __device__ __forceinline__ void add(int lcs, int lc, int lr) {
    const double prec = (double)lcs / (double)lc, rec = (double)lcs / (double)lr;
    pmax = prec > pmax ? prec : pmax;
    rmax = rec > rmax ? rec : rmax;
  }
  __device__ __forceinline__ double finish() const {
    double rouge = 0.0;
    if (pmax != 0.0 && rmax != 0.0) rouge = ((1.0 + CE_BETA2) * pmax * rmax) / (rmax + CE_BETA2 * pmax);
    return rouge;
  }
};

// The candidate's n-gram bookkeeping without the tf-idf side (cider_candidate's first / count, the same loops): for a wave that
// computes BLEU's clipped counts but no CIDEr.  Fills c.first and c.count only.
__device__ __forceinline__ void ngram_candidate_counts(const uint64_t (*s_cc)[CE_LMAX], const uint64_t cc[4], int lc, int lane,
                                                       CiderCand &c) {
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int valid = lc - n;
    int cnt = 0, before = 0;
    for (int j = 0; j < valid; ++j) {
      const bool eq = s_cc[n][j] == cc[n];
      cnt += eq ? 1 : 0;
      before += (eq && j < lane) ? 1 : 0;
    }
    c.first[n] = lane < valid && before == 0;
    c.count[n] = cnt;
  }
}

// how often this lane's candidate n-gram occurs in the staged reference (cider_reference's cr, without the products)
__device__ __forceinline__ int ngram_reference_count(const uint64_t (*s_rc)[CE_LMAX], const uint64_t cc[4], int lr, int n) {
  int cr = 0;
  for (int j = 0; j < lr - n; ++j) cr += s_rc[n][j] == cc[n] ? 1 : 0;
  return cr;
}

// BLEU's clipping: per n the largest count over the references of this lane's candidate n-gram (first occurrences only) ...
__device__ __forceinline__ void bleu_clip_add(const CiderCand &c, int n, int cr, int maxref[4]) {
  if (c.first[n]) maxref[n] = cr > maxref[n] ? cr : maxref[n];
}

// ... and correct[n] = the sum over the candidate's distinct n-grams of min(count, that maximum)
__device__ __forceinline__ int bleu_correct(const CiderCand &c, int n, const int maxref[4]) {
  return spacap::wave_sum(c.first[n] ? (c.count[n] < maxref[n] ? c.count[n] : maxref[n]) : 0);
}

// the ten components as spacap_caption_score_f64 lays them out: testlen, reflen, guess[4], correct[4]
__device__ __forceinline__ void bleu_components(int lc, int reflen, const int correct[4], int32_t *o) {
  o[0] = lc;
  o[1] = reflen;
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    o[2 + n] = lc - n > 0 ? lc - n : 0;
    o[6 + n] = correct[n];
  }
}

// Sentence-level BLEU-4 as the reference's scorer appends it to bleu_list[3] (bleu_scorer.py:232-240): the product of the four
// smoothed precisions to the power 1/4 (two correctly rounded square roots), times the brevity penalty when the caption is
// shorter than the closest reference.  float64 throughout.
__device__ __forceinline__ double bleu4_sentence(int lc, int reflen, const int correct[4]) {
  double bleu = 1.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int guess = lc - k > 0 ? lc - k : 0;
    bleu *= ((double)correct[k] + BLEU_TINY) / ((double)guess + BLEU_SMALL);
  }
  bleu = sqrt(sqrt(bleu));
  const double ratio = ((double)lc + BLEU_TINY) / ((double)reflen + BLEU_SMALL);
  if (ratio < 1.0) bleu *= exp(1.0 - 1.0 / ratio);
  return bleu;
}

}  // namespace spacap::eval
