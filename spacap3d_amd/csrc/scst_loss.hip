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
#include <math.h>

#include "common.hpp"

namespace {
constexpr int SC_T = 256;

__global__ __launch_bounds__(SC_T) void scst_rows_kernel(const float *__restrict__ logits, const int64_t *__restrict__ words,
                                                        const int32_t *__restrict__ length, int W, int V, float *__restrict__ pair,
                                                        uint8_t *__restrict__ hit) {
  __shared__ float s_f[SC_T / 64];
  __shared__ int s_i[SC_T / 64];
  const int q = blockIdx.x, r = q / W, t = q - r * W, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (t >= length[r]) {                              // (uniform over the workgroup) not counted: nothing of its row is read
    if (tid == 0) pair[(size_t)q * 2] = 0.f, pair[(size_t)q * 2 + 1] = 0.f, hit[q] = 0;
    return;
  }
  const float *x = logits + (size_t)q * V;
  float m = -INFINITY;
  int am = 0;
  for (int v = tid; v < V; v += SC_T) {
    const float a = x[v];
    if (a > m) m = a, am = v;        // first maximum per thread (ascending v)
  }
  // block arg-max with the lowest index among equal maxima (torch.argmax returns the first)
  float wm = spacap::wave_max(m);
  int cand = (m == wm) ? am : 0x7fffffff;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) cand = min(cand, __shfl_xor(cand, o));
  if (lane == 0) s_f[wv] = wm, s_i[wv] = cand;
  __syncthreads();
  float M = s_f[0];
  for (int i = 1; i < SC_T / 64; ++i) M = fmaxf(M, s_f[i]);
  int AM = 0x7fffffff;
  for (int i = 0; i < SC_T / 64; ++i)
    if (s_f[i] == M) AM = min(AM, s_i[i]);
  __syncthreads();
  float s = 0.f;
  for (int v = tid; v < V; v += SC_T) s += expf(x[v] - M);
  s = spacap::wave_sum(s);
  if (lane == 0) s_f[wv] = s;
  __syncthreads();
  if (tid != 0) return;
  float Z = 0.f;
  for (int i = 0; i < SC_T / 64; ++i) Z += s_f[i];
  const float lse = M + logf(Z);
  const int64_t w = words[q];
  const bool in = (uint64_t)w < (uint64_t)V;         // out-of-range id: contributes nothing (never read out of bounds)
  pair[(size_t)q * 2] = lse;
  pair[(size_t)q * 2 + 1] = in ? x[w] - lse : 0.f;
  hit[q] = (in && AM == (int)w) ? 1 : 0;
}

__global__ __launch_bounds__(64) void scst_final_kernel(const float *__restrict__ pair, const uint8_t *__restrict__ hit,
                                                        const int32_t *__restrict__ length, const double *__restrict__ reward,
                                                        const double *__restrict__ baseline, const uint8_t *__restrict__ count, int R,
                                                        int S, int W, float *__restrict__ adv, float *__restrict__ rowlogp,
                                                        float *__restrict__ out) {
  // one wavefront: lane l takes rows l, l + 64, ... in order, then a fixed shuffle tree (bitwise reproducible)
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
  if (threadIdx.x != 0) return;
  const float inv = 1.0f / ((float)den + 1e-6f);
  out[0] = (float)(-num * (double)inv);
  out[1] = (float)hits / fmaxf((float)den, 1.0f);
  out[2] = inv;
  out[3] = (float)(nrow / S);
  out[4] = (float)(rsum / (double)(nrow > 0 ? nrow : 1));
  out[5] = (float)(bsum / (double)(nrow > 0 ? nrow : 1));
  out[6] = 0.f;
  out[7] = 0.f;
}

__global__ __launch_bounds__(SC_T) void scst_bwd_kernel(const float *__restrict__ logits, const int64_t *__restrict__ words,
                                                       const int32_t *__restrict__ length, const float *__restrict__ pair,
                                                       const float *__restrict__ adv, const float *__restrict__ out,
                                                       const float *__restrict__ gloss, int W, int V, float *__restrict__ dlogits) {
  const int q = blockIdx.x, r = q / W, t = q - r * W, tid = threadIdx.x;
  float *d = dlogits + (size_t)q * V;
  const int64_t w = words[q];
  const float A = adv[r];
  if (t >= length[r] || A == 0.f || (uint64_t)w >= (uint64_t)V) {   // (uniform) no term of the loss: exact zeros, logits unread
    for (int v = tid; v < V; v += SC_T) d[v] = 0.f;
    return;
  }
  const float k = gloss[0] * (-A * out[2]), lse = pair[(size_t)q * 2];
  const float *x = logits + (size_t)q * V;
  for (int v = tid; v < V; v += SC_T) d[v] = k * ((v == (int)w ? 1.f : 0.f) - expf(x[v] - lse));
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
