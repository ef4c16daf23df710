// The CIDEr-D arithmetic (cider_scorer.py:106-181 with n = 4, sigma = 6) over word ids, by one wave with one lane per token
// position: what caption_score_kernel (caption_eval.hip, one candidate per key row) and caption_reward_kernel
// (caption_reward.hip, one candidate per drawn caption) share, so that the number has ONE definition: both kernels call the
// functions below in the same order and give the same bits for the same caption, references and tables.
// Compiled with -ffp-contract=off (Makefile default); the sums run in wave-reduction order.
#pragma once
#include <math.h>

#include "eval_common.hpp"

namespace spacap::eval {

constexpr int CE_LMAX = 64;                         // tokens per sentence = lanes of a wave
constexpr double CE_TWO_SIGMA2 = 2.0 * 6.0 * 6.0;   // cider_scorer.py: 2 * sigma ** 2

struct CiderTables {
  const uint64_t *df_code;      // the four sorted document-frequency tables, one after the other
  const double *df_idf;         // log(NKEYS) - log(max(1, df)) per entry
  long long df_off[5];          // table n (n-grams of n words) = entries df_off[n-1] .. df_off[n]
  double log_nkeys;
};

struct CiderRefs {
  const int32_t *ref_tok;       // CSR over the references
  const int32_t *ref_off;       // [NREF]
  const int32_t *ref_len;       // [NREF]
  const int32_t *key_ref_off;   // [NKEYS + 1]
  long long n_tok, n_ref;
};

// the candidate's side of the products, per lane and n (index n-1)
struct CiderCand {
  bool first[4];                // this position is the first occurrence of its n-gram
  int count[4];                 // how often the n-gram occurs in the candidate
  double idf[4], vec[4], norm[4];
};

// n-gram codes of the sentence in s_tok (len tokens) at this lane's position: code[n-1] is valid when lane + n <= len
__device__ __forceinline__ void ngram_codes(const int *s_tok, int lane, uint64_t code[4]) {
  uint64_t c = 0;
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int t = lane + n < CE_LMAX ? s_tok[lane + n] : 0;
    c = (c << 16) | (uint64_t)(t & 0xFFFF);
    code[n] = c;
  }
}

__device__ __forceinline__ double idf_lookup(const CiderTables &a, int n, uint64_t code) {
  long long lo = a.df_off[n], hi = a.df_off[n + 1];
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (a.df_code[mid] < code) lo = mid + 1;
    else hi = mid;
  }
  return (lo < a.df_off[n + 1] && a.df_code[lo] == code) ? a.df_idf[lo] : a.log_nkeys;
}

// candidate: first occurrence, term frequency, tf-idf, norm per n.  s_cc holds the candidate's codes of every lane
// (written and synchronised by the caller), cc are this lane's, lc the candidate's length.
__device__ __forceinline__ void cider_candidate(const CiderTables &a, const uint64_t (*s_cc)[CE_LMAX], const uint64_t cc[4], int lc,
                                                int lane, CiderCand &c) {
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int valid = lc - n;                        // positions 0 .. valid-1 hold an (n+1)-gram
    const bool in = lane < valid;
    int cnt = 0, before = 0;
    for (int j = 0; j < valid; ++j) {
      const bool eq = s_cc[n][j] == cc[n];
      cnt += eq ? 1 : 0;
      before += (eq && j < lane) ? 1 : 0;
    }
    c.first[n] = in && before == 0;
    c.count[n] = cnt;
    c.idf[n] = in ? idf_lookup(a, n, cc[n]) : 0.0;
    c.vec[n] = (double)cnt * c.idf[n];
    c.norm[n] = sqrt(spacap::wave_sum(c.first[n] ? c.vec[n] * c.vec[n] : 0.0));
  }
}

// Reference r into LDS: its tokens in s_tok (-2 behind its end), its n-gram codes in s_rc; this lane's codes in rc.  Returns
// the reference's length.  Every lane of the wave calls it; the readers of the previous reference are done on entry.
__device__ __forceinline__ int cider_stage_reference(const CiderRefs &a, long long r, int lane, int *s_tok, uint64_t (*s_rc)[CE_LMAX],
                                                     uint64_t rc[4]) {
  int lr = a.ref_len[r];
  lr = lr < 0 ? 0 : (lr > CE_LMAX ? CE_LMAX : lr);
  const long long off = a.ref_off[r];
  const bool ok = off >= 0 && off + lr <= a.n_tok;
  __syncthreads();                                 // the previous reference's readers are done
  s_tok[lane] = (ok && lane < lr) ? a.ref_tok[off + lane] : -2;
  __syncthreads();
  ngram_codes(s_tok, lane, rc);
#pragma unroll
  for (int n = 0; n < 4; ++n) s_rc[n][lane] = rc[n];
  __syncthreads();
  return lr;
}

// exp(-(delta ** 2) / (2 sigma ** 2)) with the reference's `length`: the number of BIGRAMS of either sentence
__device__ __forceinline__ double cider_penalty(int lc, int lr) {
  const int len_h = lc > 1 ? lc - 1 : 0, len_r = lr > 1 ? lr - 1 : 0;
  const double delta = (double)(len_h - len_r);
  return exp(-(delta * delta) / CE_TWO_SIGMA2);
}

// One n of one staged reference: the clipped tf-idf product over the two norms, before the length penalty.  cr = how often
// this lane's CANDIDATE n-gram occurs in the reference (BLEU's clipping reads it).
__device__ __forceinline__ double cider_reference(const CiderTables &a, const uint64_t (*s_rc)[CE_LMAX], const uint64_t rc[4],
                                                  const uint64_t cc[4], const CiderCand &c, int lr, int lane, int n, int &cr) {
  const int rvalid = lr - n;
  // the reference's own vector: norm over its distinct n-grams
  int rcnt = 0, rbefore = 0;
  cr = 0;
  for (int j = 0; j < rvalid; ++j) {
    const uint64_t x = s_rc[n][j];
    const bool eq = x == rc[n];
    rcnt += eq ? 1 : 0;
    rbefore += (eq && j < lane) ? 1 : 0;
    cr += x == cc[n] ? 1 : 0;
  }
  const bool rfirst = lane < rvalid && rbefore == 0;
  double rv = 0.0;
  if (rfirst) rv = (double)rcnt * idf_lookup(a, n, rc[n]);
  const double rnorm = sqrt(spacap::wave_sum(rfirst ? rv * rv : 0.0));
  double term = 0.0;
  if (c.first[n]) {
    const double vr = (double)cr * c.idf[n];
    term = (c.vec[n] < vr ? c.vec[n] : vr) * vr;
  }
  double val = spacap::wave_sum(term);
  if (c.norm[n] != 0.0 && rnorm != 0.0) val /= c.norm[n] * rnorm;
  return val;
}

// the mean over n, over the references, times 10
__device__ __forceinline__ double cider_finish(const double score[4], long long nref) {
  double avg = (((score[0] + score[1]) + score[2]) + score[3]) / 4.0;
  if (nref > 0) avg /= (double)nref;
  return avg * 10.0;
}

}  // namespace spacap::eval
