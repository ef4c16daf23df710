// Self-critical caption loss on gfx950 (MI355X): the drawn words' log-probabilities weighted with the advantage of their
// caption's reward over a baseline (the reference has no such loss, tests/self_critical_restated.py is
// the specification).  Modelled on the caption head of losses.hip (cap_rows_kernel / cap_final_kernel / cap_bwd_kernel), which
// it leaves alone; unlike it, NO (rows, W, V) log-probability image is written: per (row, position) the forward keeps the
// log-sum-exp and the drawn word's log-probability, and the backward forms the softmax from the logits again.
//
//   R rows = R / S scenes x S samples (row r = b S + s), W word positions, V words;  length_r <= W positions of row r count.
//   A_r   = c_b (reward_r - base_r),  base_r = baseline[b]  or, with baseline == NULL, the mean of the scene's OTHER rewards
//           (float64, rounded to fp32 once);  c_b = count[b] != 0
//   loss  = - sum_r A_r sum_{t < length_r} logp[r, t, w_rt]  /  (sum_r c_b length_r + 1e-6)
//   a word id outside [0, V) contributes nothing (as an out-of-range target in cap_rows_kernel)
//
//   scst_rows_kernel   one workgroup per (row, position); t >= length_r returns without reading its V logits
//   scst_final_kernel  one wave: advantages, per-row sums and the totals in a fixed order (bitwise reproducible)
//   scst_bwd_kernel    dlogits[r,t,v] = g (-A_r inv_den) ([v == w_rt] - softmax_rtv) for t < length_r, exact zeros elsewhere
//
// Below them the mixed loss: the same rows behind B0 teacher-forced ground-truth rows of ONE logit image,
// L_rl + w_xe L_xe.  Each kernel body above is a device function that both sets of kernels call.
#include <math.h>

#include "common.hpp"

namespace {
constexpr int SC_T = 256;

// One row of V logits by one workgroup of SC_T threads: the maximum, the FIRST arg-max (torch.argmax returns the first) and the
// log-sum-exp.  Returns true on thread 0 only, which alone holds the results.  The one definition of the row arithmetic of
// scst_rows_kernel and mixed_rows_kernel: the same bits from both.
__device__ __forceinline__ bool row_lse_argmax(const float *__restrict__ x, int V, float *s_f, int *s_i, float &lse, int &AM) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float m = -INFINITY;
  int am = 0;
  for (int v = tid; v < V; v += SC_T) {
    const float a = x[v];
    if (a > m) m = a, am = v;        // first maximum per thread (ascending v)
  }
  // block arg-max with the lowest index among equal maxima
  float wm = spacap::wave_max(m);
  int cand = (m == wm) ? am : 0x7fffffff;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) cand = min(cand, __shfl_xor(cand, o));
  if (lane == 0) s_f[wv] = wm, s_i[wv] = cand;
  __syncthreads();
  float M = s_f[0];
  for (int i = 1; i < SC_T / 64; ++i) M = fmaxf(M, s_f[i]);
  AM = 0x7fffffff;
  for (int i = 0; i < SC_T / 64; ++i)
    if (s_f[i] == M) AM = min(AM, s_i[i]);
  __syncthreads();
  float s = 0.f;
  for (int v = tid; v < V; v += SC_T) s += expf(x[v] - M);
  s = spacap::wave_sum(s);
  if (lane == 0) s_f[wv] = s;
  __syncthreads();
  if (tid != 0) return false;
  float Z = 0.f;
  for (int i = 0; i < SC_T / 64; ++i) Z += s_f[i];
  lse = M + logf(Z);
  return true;
}

// (row, position) q of the drawn captions: words / length / pair / hit are indexed from the first SAMPLE row
__device__ __forceinline__ void scst_row(const float *__restrict__ x, const int64_t *__restrict__ words,
                                         const int32_t *__restrict__ length, int q, int W, int V, float *__restrict__ pair,
                                         uint8_t *__restrict__ hit, float *s_f, int *s_i) {
  const int r = q / W, t = q - r * W, tid = threadIdx.x;
  if (t >= length[r]) {                              // (uniform over the workgroup) not counted: nothing of its row is read
    if (tid == 0) pair[(size_t)q * 2] = 0.f, pair[(size_t)q * 2 + 1] = 0.f, hit[q] = 0;
    return;
  }
  float lse;
  int AM;
  if (!row_lse_argmax(x, V, s_f, s_i, lse, AM)) return;
  const int64_t w = words[q];
  const bool in = (uint64_t)w < (uint64_t)V;         // out-of-range id: contributes nothing (never read out of bounds)
  pair[(size_t)q * 2] = lse;
  pair[(size_t)q * 2 + 1] = in ? x[w] - lse : 0.f;
  hit[q] = (in && AM == (int)w) ? 1 : 0;
}

__global__ __launch_bounds__(SC_T) void scst_rows_kernel(const float *__restrict__ logits, const int64_t *__restrict__ words,
                                                        const int32_t *__restrict__ length, int W, int V, float *__restrict__ pair,
                                                        uint8_t *__restrict__ hit) {
  __shared__ float s_f[SC_T / 64];
  __shared__ int s_i[SC_T / 64];
  const int q = blockIdx.x;
  scst_row(logits + (size_t)q * V, words, length, q, W, V, pair, hit, s_f, s_i);
}

// the totals of the reward-weighted term, on every lane of the one wave that formed them
struct ScstTotals {
  float loss, acc, inv, scenes, mean_reward, mean_base;
};

// One wavefront: advantages, per-row sums and the totals over the R sample rows (pair / hit indexed from the first sample row).
// The one definition of scst_final_kernel's and mixed_final_kernel's sums: the same bits from both.
__device__ __forceinline__ ScstTotals scst_totals(const float *__restrict__ pair, const uint8_t *__restrict__ hit,
                                                  const int32_t *__restrict__ length, const double *__restrict__ reward,
                                                  const double *__restrict__ baseline, const uint8_t *__restrict__ count, int R, int S,
                                                  int W, float *__restrict__ adv, float *__restrict__ rowlogp) {
  // lane l takes rows l, l + 64, ... in order, then a fixed shuffle tree (bitwise reproducible)
  double num = 0.0, rsum = 0.0, bsum = 0.0;
  int den = 0, hits = 0, nrow = 0;
  for (int r = threadIdx.x; r < R; r += 64) {
    const int b = r / S;
    const bool c = count[b] != 0;
    double base;
    if (baseline) {
      base = baseline[b];
    } else {                                         // the mean of the scene's other samples, in sample order (S >= 2)
      double o = 0.0;
      for (int s = 0; s < S; ++s)
        if (b * S + s != r) o += reward[b * S + s];
      base = o / (double)(S - 1);
    }
    const float A = c ? (float)(reward[r] - base) : 0.f;
    int len = length[r];
    len = len < 0 ? 0 : (len > W ? W : len);
    float lp = 0.f;
    int h = 0;
    for (int t = 0; t < len; ++t) lp += pair[((size_t)r * W + t) * 2 + 1], h += hit[(size_t)r * W + t];
    adv[r] = A;
    rowlogp[r] = lp;
    if (c) {
      num += (double)A * (double)lp;
      den += len;
      hits += h;
      nrow += 1;
      rsum += reward[r];
      bsum += base;
    }
  }
  num = spacap::wave_sum(num), rsum = spacap::wave_sum(rsum), bsum = spacap::wave_sum(bsum);
  den = spacap::wave_sum(den), hits = spacap::wave_sum(hits), nrow = spacap::wave_sum(nrow);
  ScstTotals o;
  o.inv = 1.0f / ((float)den + 1e-6f);
  o.loss = (float)(-num * (double)o.inv);
  o.acc = (float)hits / fmaxf((float)den, 1.0f);
  o.scenes = (float)(nrow / S);
  o.mean_reward = (float)(rsum / (double)(nrow > 0 ? nrow : 1));
  o.mean_base = (float)(bsum / (double)(nrow > 0 ? nrow : 1));
  return o;
}

__global__ __launch_bounds__(64) void scst_final_kernel(const float *__restrict__ pair, const uint8_t *__restrict__ hit,
                                                        const int32_t *__restrict__ length, const double *__restrict__ reward,
                                                        const double *__restrict__ baseline, const uint8_t *__restrict__ count, int R,
                                                        int S, int W, float *__restrict__ adv, float *__restrict__ rowlogp,
                                                        float *__restrict__ out) {
  const ScstTotals o = scst_totals(pair, hit, length, reward, baseline, count, R, S, W, adv, rowlogp);
  if (threadIdx.x != 0) return;
  out[0] = o.loss;
  out[1] = o.acc;
  out[2] = o.inv;
  out[3] = o.scenes;
  out[4] = o.mean_reward;
  out[5] = o.mean_base;
  out[6] = 0.f;
  out[7] = 0.f;
}

// (row, position) q of the drawn captions, indexed from the first SAMPLE row as in scst_row; inv = 1 / (counted positions + 1e-6)
__device__ __forceinline__ void scst_row_bwd(const float *__restrict__ x, const int64_t *__restrict__ words,
                                             const int32_t *__restrict__ length, const float *__restrict__ pair,
                                             const float *__restrict__ adv, float inv, float g, int q, int W, int V,
                                             float *__restrict__ d) {
  const int r = q / W, t = q - r * W, tid = threadIdx.x;
  const int64_t w = words[q];
  const float A = adv[r];
  if (t >= length[r] || A == 0.f || (uint64_t)w >= (uint64_t)V) {   // (uniform) no term of the loss: exact zeros, logits unread
    for (int v = tid; v < V; v += SC_T) d[v] = 0.f;
    return;
  }
  const float k = g * (-A * inv), lse = pair[(size_t)q * 2];
  for (int v = tid; v < V; v += SC_T) d[v] = k * ((v == (int)w ? 1.f : 0.f) - expf(x[v] - lse));
}

__global__ __launch_bounds__(SC_T) void scst_bwd_kernel(const float *__restrict__ logits, const int64_t *__restrict__ words,
                                                       const int32_t *__restrict__ length, const float *__restrict__ pair,
                                                       const float *__restrict__ adv, const float *__restrict__ out,
                                                       const float *__restrict__ gloss, int W, int V, float *__restrict__ dlogits) {
  const int q = blockIdx.x;
  scst_row_bwd(logits + (size_t)q * V, words, length, pair, adv, out[2], gloss[0], q, W, V, dlogits + (size_t)q * V);
}

// ---- the mixed loss: cross-entropy rows and reward rows over ONE logit image --------------------------
//   logits (B0 + R, W, V): rows 0 .. B0-1 are teacher-forced ground-truth captions, one per scene (target[b, t], row stride
//   tstride; good[b]; their own W0 <= W word positions: t >= W0 is padding and never counts), rows B0 .. are the R = G S drawn
//   captions of G groups.
//   L_rl  = the loss of the head of this file over rows B0 .., to the bit
//   L_xe  = sum_b good_b sum_{t < W0: target_bt != 0} -logp[b, t, target_bt] / (W0 sum_b good_b + 1e-6)    (compute_cap_loss,
//           lib/loss_helper.py:212-219, whose sum of good_bbox_masks runs over the (scene, word) rows: cap_rows_kernel /
//           cap_final_kernel of losses.hip on a (B0, W0, V) image; a target outside [0, V) is ignored like the pad id 0);
//           accuracy = first-arg-max hits over the counted positions (:226-233)
//   loss  = L_rl + w_xe L_xe    (L_rl alone, to the bit, when B0 = 0 or w_xe = 0)
//   mixed_rows_kernel   one workgroup per (row, position): a ground-truth position that does not count (scene not good, pad
//                       target) and a sample position behind its length return without reading their V logits
//   mixed_final_kernel  one wave: scst_totals, then the ground-truth rows' sums in float64, lane l scenes l, l + 64, ... in
//                       order and a fixed shuffle tree (bitwise reproducible)
//   mixed_bwd_kernel    sample rows: scst_row_bwd;  ground-truth rows: g w_xe good_b inv_good (softmax - onehot) at counted
//                       positions;  exact zeros everywhere else, every element written
// out f32 [12] = (loss, L_rl, L_xe, accuracy of the sample rows, accuracy of the ground-truth rows, 1 / (counted sample
//                positions + 1e-6), 1 / (W0 good scenes + 1e-6), counting groups, good scenes, mean reward, mean baseline, 0)
constexpr int MX_OUT = 12;

// The ground-truth rows of the image: target[b, t] (row stride tstride), good[b], and their own W0 <= W word positions -- a
// position t >= W0 of such a row is padding: its target is not read and it never counts.
struct XeRows {
  const int64_t *target;
  const uint8_t *good;
  int tstride, B0, W0;
};

__device__ __forceinline__ int64_t xe_target(const XeRows &g, int b, int t, int V) {
  if (t >= g.W0) return 0;
  const int64_t w = g.target[(size_t)b * g.tstride + t];
  return (uint64_t)w >= (uint64_t)V ? 0 : w;         // out-of-range id: ignored like the pad id (never read out of bounds)
}

__global__ __launch_bounds__(SC_T) void mixed_rows_kernel(const float *__restrict__ logits, XeRows g,
                                                         const int64_t *__restrict__ words, const int32_t *__restrict__ length,
                                                         int W, int V, float *__restrict__ pair, uint8_t *__restrict__ hit) {
  __shared__ float s_f[SC_T / 64];
  __shared__ int s_i[SC_T / 64];
  const int q = blockIdx.x, q0 = g.B0 * W;
  const float *x = logits + (size_t)q * V;
  if (q >= q0) {                                     // (uniform over the workgroup) a drawn caption's position
    scst_row(x, words, length, q - q0, W, V, pair + (size_t)q0 * 2, hit + q0, s_f, s_i);
    return;
  }
  const int b = q / W, t = q - b * W;
  const int64_t w = xe_target(g, b, t, V);
  if (w == 0 || g.good[b] == 0) {                    // (uniform) not counted: nothing of its row is read
    if (threadIdx.x == 0) pair[(size_t)q * 2] = 0.f, pair[(size_t)q * 2 + 1] = 0.f, hit[q] = 0;
    return;
  }
  float lse;
  int AM;
  if (!row_lse_argmax(x, V, s_f, s_i, lse, AM)) return;
  pair[(size_t)q * 2] = lse;
  pair[(size_t)q * 2 + 1] = x[w] - lse;
  hit[q] = AM == (int)w ? 1 : 0;
}

__global__ __launch_bounds__(64) void mixed_final_kernel(const float *__restrict__ pair, const uint8_t *__restrict__ hit, XeRows g,
                                                         const int32_t *__restrict__ length, const double *__restrict__ reward,
                                                         const double *__restrict__ baseline, const uint8_t *__restrict__ count,
                                                         int R, int S, int W, int V, float w_xe, float *__restrict__ adv,
                                                         float *__restrict__ rowlogp, float *__restrict__ out) {
  const int B0 = g.B0;
  const ScstTotals o = scst_totals(pair + (size_t)B0 * W * 2, hit + (size_t)B0 * W, length, reward, baseline, count, R, S, W, adv,
                                   rowlogp);
  double nll = 0.0;
  int ngood = 0, hits = 0, valid = 0;
  for (int b = threadIdx.x; b < B0; b += 64) {
    if (g.good[b] == 0) continue;
    ngood += 1;
    for (int t = 0; t < g.W0; ++t) {
      if (xe_target(g, b, t, V) == 0) continue;
      nll -= (double)pair[((size_t)b * W + t) * 2 + 1];
      hits += hit[(size_t)b * W + t];
      valid += 1;
    }
  }
  nll = spacap::wave_sum(nll);
  ngood = spacap::wave_sum(ngood), hits = spacap::wave_sum(hits), valid = spacap::wave_sum(valid);
  if (threadIdx.x != 0) return;
  const float inv_good = 1.0f / ((float)(ngood * g.W0) + 1e-6f);   // (compute_cap_loss sums good over the (scene, word) rows)
  const float l_xe = (float)(nll * (double)inv_good);
  out[0] = (B0 > 0 && w_xe != 0.f) ? o.loss + w_xe * l_xe : o.loss;
  out[1] = o.loss;
  out[2] = l_xe;
  out[3] = o.acc;
  out[4] = (float)hits / fmaxf((float)valid, 1.0f);
  out[5] = o.inv;
  out[6] = inv_good;
  out[7] = o.scenes;
  out[8] = (float)ngood;
  out[9] = o.mean_reward;
  out[10] = o.mean_base;
  out[11] = 0.f;
}

__global__ __launch_bounds__(SC_T) void mixed_bwd_kernel(const float *__restrict__ logits, XeRows g,
                                                        const int64_t *__restrict__ words, const int32_t *__restrict__ length,
                                                        const float *__restrict__ pair, const float *__restrict__ adv,
                                                        const float *__restrict__ out, const float *__restrict__ gloss, int W, int V,
                                                        float w_xe, float *__restrict__ dlogits) {
  const int q = blockIdx.x, q0 = g.B0 * W, tid = threadIdx.x;
  const float *x = logits + (size_t)q * V;
  float *d = dlogits + (size_t)q * V;
  if (q >= q0) {                                     // (uniform over the workgroup)
    scst_row_bwd(x, words, length, pair + (size_t)q0 * 2, adv, out[5], gloss[0], q - q0, W, V, d);
    return;
  }
  const int b = q / W, t = q - b * W;
  const int64_t w = xe_target(g, b, t, V);
  if (w == 0 || g.good[b] == 0 || w_xe == 0.f) {     // (uniform) no term of the loss: exact zeros, logits unread
    for (int v = tid; v < V; v += SC_T) d[v] = 0.f;
    return;
  }
  const float k = gloss[0] * w_xe * out[6], lse = pair[(size_t)q * 2];
  for (int v = tid; v < V; v += SC_T) d[v] = k * (expf(x[v] - lse) - (v == (int)w ? 1.f : 0.f));
}
}  // namespace

extern "C" int spacap_scst_loss_fwd_f32(const float *logits, const int64_t *words, const int32_t *length, const double *reward,
                                        const double *baseline, const uint8_t *count, int R, int S, int W, int V, float *pair,
                                        uint8_t *hit, float *adv, float *rowlogp, float *out, spacap_stream_t stream) {
  const char *what = "spacap_scst_loss_fwd_f32";
  SPACAP_REQUIRE(R >= 0 && S >= 1 && R % S == 0 && W >= 1 && V >= 2 && (long long)R * W <= 0x7fffffffLL,
                 "%s: bad sizes (R=%d S=%d W=%d V=%d; R a multiple of S)", what, R, S, W, V);
  SPACAP_REQUIRE(baseline || S >= 2, "%s: bad sizes (S=%d: the leave-one-out baseline needs two samples per scene)", what, S);
  hipStream_t s = spacap::as_stream(stream);
  if (R == 0) {   // no rows: loss 0 and every reported figure 0
    if (out) SPACAP_CHECK_HIP(hipMemsetAsync(out, 0, 8 * sizeof(float), s), what);
    return SPACAP_OK;
  }
  SPACAP_REQUIRE(logits && words && length && reward && count && pair && hit && adv && rowlogp && out, "%s: null pointer", what);
  hipLaunchKernelGGL(scst_rows_kernel, dim3(R * W), dim3(SC_T), 0, s, logits, words, length, W, V, pair, hit);
  hipLaunchKernelGGL(scst_final_kernel, dim3(1), dim3(64), 0, s, pair, hit, length, reward, baseline, count, R, S, W, adv, rowlogp,
                     out);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_scst_loss_bwd_f32(const float *logits, const int64_t *words, const int32_t *length, const float *pair,
                                        const float *adv, const float *out, const float *gloss, int R, int W, int V, float *dlogits,
                                        spacap_stream_t stream) {
  const char *what = "spacap_scst_loss_bwd_f32";
  SPACAP_REQUIRE(R >= 0 && W >= 1 && V >= 2 && (long long)R * W <= 0x7fffffffLL, "%s: bad sizes (R=%d W=%d V=%d)", what, R, W, V);
  if (R == 0) return SPACAP_OK;
  SPACAP_REQUIRE(logits && words && length && pair && adv && out && gloss && dlogits, "%s: null pointer", what);
  hipLaunchKernelGGL(scst_bwd_kernel, dim3(R * W), dim3(SC_T), 0, spacap::as_stream(stream), logits, words, length, pair, adv, out,
                     gloss, W, V, dlogits);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_mixed_cap_loss_fwd_f32(const float *logits, const int64_t *target, int tstride, const uint8_t *good, int B0,
                                             int W0, const int64_t *words, const int32_t *length, const double *reward,
                                             const double *baseline, const uint8_t *count, int R, int S, int W, int V, float w_xe,
                                             float *pair, uint8_t *hit, float *adv, float *rowlogp, float *out,
                                             spacap_stream_t stream) {
  const char *what = "spacap_mixed_cap_loss_fwd_f32";
  SPACAP_REQUIRE(B0 >= 0 && R >= 0 && S >= 1 && R % S == 0 && W >= 1 && V >= 2 && ((long long)B0 + R) * W <= 0x7fffffffLL &&
                     (B0 == 0 || (W0 >= 1 && W0 <= W && tstride >= W0)),
                 "%s: bad sizes (B0=%d W0=%d R=%d S=%d W=%d V=%d tstride=%d; R a multiple of S, 1 <= W0 <= W, tstride >= W0)", what, B0,
                 W0, R, S, W, V, tstride);
  SPACAP_REQUIRE(baseline || S >= 2, "%s: bad sizes (S=%d: the leave-one-out baseline needs two samples per scene)", what, S);
  SPACAP_REQUIRE(w_xe >= 0.f && isfinite(w_xe), "%s: bad weight (w_xe=%g: finite and not negative)", what, (double)w_xe);
  hipStream_t s = spacap::as_stream(stream);
  if (B0 + R == 0) {   // no rows: loss 0 and every reported figure 0
    if (out) SPACAP_CHECK_HIP(hipMemsetAsync(out, 0, MX_OUT * sizeof(float), s), what);
    return SPACAP_OK;
  }
  SPACAP_REQUIRE(logits && pair && hit && out && (B0 == 0 || (target && good)) &&
                     (R == 0 || (words && length && reward && count && adv && rowlogp)),
                 "%s: null pointer", what);
  const XeRows g{target, good, tstride, B0, B0 ? W0 : 0};
  hipLaunchKernelGGL(mixed_rows_kernel, dim3((B0 + R) * W), dim3(SC_T), 0, s, logits, g, words, length, W, V, pair, hit);
  hipLaunchKernelGGL(mixed_final_kernel, dim3(1), dim3(64), 0, s, pair, hit, g, length, reward, baseline, count, R, S, W, V, w_xe, adv,
                     rowlogp, out);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_mixed_cap_loss_bwd_f32(const float *logits, const int64_t *target, int tstride, const uint8_t *good, int B0,
                                             int W0, const int64_t *words, const int32_t *length, const float *pair, const float *adv,
                                             const float *out, const float *gloss, int R, int W, int V, float w_xe, float *dlogits,
                                             spacap_stream_t stream) {
  const char *what = "spacap_mixed_cap_loss_bwd_f32";
  SPACAP_REQUIRE(B0 >= 0 && R >= 0 && W >= 1 && V >= 2 && ((long long)B0 + R) * W <= 0x7fffffffLL &&
                     (B0 == 0 || (W0 >= 1 && W0 <= W && tstride >= W0)),
                 "%s: bad sizes (B0=%d W0=%d R=%d W=%d V=%d tstride=%d; 1 <= W0 <= W, tstride >= W0)", what, B0, W0, R, W, V, tstride);
  SPACAP_REQUIRE(w_xe >= 0.f && isfinite(w_xe), "%s: bad weight (w_xe=%g: finite and not negative)", what, (double)w_xe);
  if (B0 + R == 0) return SPACAP_OK;
  SPACAP_REQUIRE(logits && pair && out && gloss && dlogits && (B0 == 0 || (target && good)) && (R == 0 || (words && length && adv)),
                 "%s: null pointer", what);
  const XeRows g{target, good, tstride, B0, B0 ? W0 : 0};
  hipLaunchKernelGGL(mixed_bwd_kernel, dim3((B0 + R) * W), dim3(SC_T), 0, spacap::as_stream(stream), logits, g, words, length, pair, adv,
                     out, gloss, W, V, w_xe, dlogits);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
