// Score decoding of the proposal head for gfx950 (MI355X): models/proposal_module.py:106-158 (decode_scores) and :81-104
// (decode_pred_box; the reference takes a GPU -> CPU -> numpy -> GPU round trip there).
//
// The head's output (B, CH, K) -- CH = 2 + 3 + 2 NH + 4 NS + NC channels per proposal -- is sliced into objectness scores,
// centre offset, heading scores / residuals, size scores / residuals and class scores; PyTorch runs the transpose, the centre
// add, two residual scalings, four arg-maxes, a gather and the float64 box corners as ~20 launches of a few microseconds on a
// 200 K-element tensor (and as many again for the slice gradients).  Here: one launch forward (one thread per proposal,
// channel-major reads coalesced over the proposals), one launch for the gradient.  Arithmetic as the composition: fp32 centre
// add and residual products (one rounding each), first-maximum arg-max, corners in float64.
#include <math.h>

#include "common.hpp"

namespace {

__global__ __launch_bounds__(256) void proposal_decode_fwd_kernel(const float *__restrict__ net, const float *__restrict__ agg_xyz,
                                                                  const float *__restrict__ msa, const double *__restrict__ msa64,
                                                                  int K, int NH, int NS, int NC,
                                                                  float *__restrict__ nt, float *__restrict__ center,
                                                                  float *__restrict__ hres, float *__restrict__ sres,
                                                                  double *__restrict__ corners, int64_t *__restrict__ bbox_mask,
                                                                  int64_t *__restrict__ sem_cls, int64_t *__restrict__ size_cls) {
  // 64 proposals per workgroup of 256 threads.  Phase A (all threads): the proposals' channels through LDS -- channel-major
  // reads and proposal-major writes both coalesced.  Phase B (one thread per proposal): arg-maxes and the centre.  Phase C
  // (all threads): the per-proposal output rows (size residuals, corners) written cooperatively.
  extern __shared__ float s_x[];                         // [64][CH + 1], then [64][4] (centre x, y, z, size class)
  const int b = blockIdx.y, k0 = blockIdx.x * 64, tid = threadIdx.x;
  const int CH = 5 + 2 * NH + 4 * NS + NC, LD = CH + 1, nk = min(64, K - k0);
  float *s_c = s_x + 64 * LD;
  for (int i = tid; i < CH * 64; i += 256) {
    const int c = i >> 6, kk = i & 63;
    if (kk < nk) s_x[kk * LD + c] = net[((size_t)b * CH + c) * K + k0 + kk];
  }
  __syncthreads();
  for (int i = tid; i < nk * CH; i += 256) nt[((size_t)b * K + k0) * CH + i] = s_x[(i / CH) * LD + i % CH];
  if (tid < nk) {
    const float *row = s_x + tid * LD;
    const size_t p = (size_t)b * K + k0 + tid;
    bbox_mask[p] = row[1] > row[0] ? 1 : 0;               // argmax over (no object, object): first maximum
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float c = agg_xyz[p * 3 + d] + row[2 + d];
      center[p * 3 + d] = c;
      s_c[tid * 4 + d] = c;
    }
    const float *ss = row + 5 + 2 * NH;
    int sc = 0;
    float best = ss[0];
    for (int j = 1; j < NS; ++j)
      if (ss[j] > best) best = ss[j], sc = j;
    size_cls[p] = sc;
    s_c[tid * 4 + 3] = __int_as_float(sc);
    const float *cl = ss + 4 * NS;
    int am = 0;
    best = cl[0];
    for (int j = 1; j < NC; ++j)
      if (cl[j] > best) best = cl[j], am = j;
    sem_cls[p] = am;
  }
  __syncthreads();
  const float hs = (float)(M_PI / (double)NH);
  const size_t p0 = (size_t)b * K + k0;
  for (int i = tid; i < nk * NH; i += 256) hres[p0 * NH + i] = s_x[(i / NH) * LD + 5 + NH + i % NH] * hs;
  const int S3 = 3 * NS, so = 5 + 2 * NH + NS;
  for (int i = tid; i < nk * S3; i += 256) sres[p0 * S3 + i] = s_x[(i / S3) * LD + so + i % S3] * msa[i % S3];
  // utils/box_util.py:377-379 corner order (l on x, w on y, h on z); heading is 0 for this dataset configuration
  for (int i = tid; i < nk * 24; i += 256) {
    const int kk = i / 24, e = i % 24, c = e / 3, d = e % 3;
    const int sc = __float_as_int(s_c[kk * 4 + 3]);
    const float mine = s_x[kk * LD + so + 3 * sc + d] * msa[3 * sc + d];
    const double half = ((msa64 ? msa64[3 * sc + d] : (double)msa[3 * sc + d]) + (double)mine) / 2.0;
    const double sgn = d == 0 ? ((c & 3) < 2 ? 1.0 : -1.0) : d == 1 ? (((c & 3) == 0 || (c & 3) == 3) ? 1.0 : -1.0) : (c < 4 ? 1.0 : -1.0);
    corners[p0 * 24 + i] = (double)s_c[kk * 4 + d] + sgn * half;
  }
}

// d net[b, c, k] = g_nt[b, k, c] (+ g_center on channels 2..4, + g_hres * pi / NH on the heading residuals, + g_sres * mean
// size on the size residuals); every gradient pointer may be null
__global__ __launch_bounds__(256) void proposal_decode_bwd_kernel(const float *__restrict__ g_nt, const float *__restrict__ g_center,
                                                                 const float *__restrict__ g_hres, const float *__restrict__ g_sres,
                                                                 const float *__restrict__ msa, int K, int NH, int NS, int NC,
                                                                 float *__restrict__ d_net) {
  extern __shared__ float s_x[];                         // [64][CH + 1]
  const int b = blockIdx.y, k0 = blockIdx.x * 64;
  const int CH = 5 + 2 * NH + 4 * NS + NC, LD = CH + 1, nk = min(64, K - k0);
  const float hs = (float)(M_PI / (double)NH);
  const int s0 = 5 + 2 * NH + NS;
  for (int i = threadIdx.x; i < nk * CH; i += 256) {     // proposal-major reads, coalesced
    const int kk = i / CH, c = i % CH;
    const size_t p = (size_t)b * K + k0 + kk;
    float v = g_nt ? g_nt[p * CH + c] : 0.f;
    if (g_center && c >= 2 && c < 5) v += g_center[p * 3 + (c - 2)];
    if (g_hres && c >= 5 + NH && c < 5 + 2 * NH) v += g_hres[p * NH + (c - 5 - NH)] * hs;
    if (g_sres && c >= s0 && c < s0 + 3 * NS) v += g_sres[p * NS * 3 + (c - s0)] * msa[c - s0];
    s_x[kk * LD + c] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CH * 64; i += 256) {     // channel-major stores, coalesced over the proposals
    const int c = i >> 6, kk = i & 63;
    if (kk < nk) d_net[((size_t)b * CH + c) * K + k0 + kk] = s_x[kk * LD + c];
  }
}

}  // namespace

extern "C" int spacap_proposal_decode_fwd_f32(const float *net, const float *agg_xyz, const float *mean_size,
                                              const double *mean_size_f64, int B, int K, int NH, int NS, int NC, float *nt, float *center, float *heading_res, float *size_res,
                                              double *corners, int64_t *bbox_mask, int64_t *sem_cls, int64_t *size_cls,
                                              spacap_stream_t stream) {
  const char *what = "spacap_proposal_decode_fwd_f32";
  SPACAP_REQUIRE(B >= 0 && K >= 1 && NH >= 1 && NS >= 1 && NC >= 1, "%s: bad sizes", what);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(net && agg_xyz && mean_size && nt && center && heading_res && size_res && corners && bbox_mask && sem_cls && size_cls,
                 "%s: null pointer", what);
  const int CH = 5 + 2 * NH + 4 * NS + NC;
  SPACAP_REQUIRE((size_t)64 * (CH + 1) * sizeof(float) <= 64 * 1024, "%s: too many channels (%d)", what, CH);
  hipLaunchKernelGGL(proposal_decode_fwd_kernel, dim3((K + 63) / 64, B), dim3(256), (size_t)(64 * (CH + 1) + 256) * sizeof(float),
                     spacap::as_stream(stream), net, agg_xyz, mean_size,
                     mean_size_f64, K, NH, NS, NC, nt, center, heading_res, size_res, corners, bbox_mask, sem_cls, size_cls);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_proposal_decode_bwd_f32(const float *g_nt, const float *g_center, const float *g_heading_res,
                                              const float *g_size_res, const float *mean_size, int B, int K, int NH, int NS, int NC,
                                              float *d_net, spacap_stream_t stream) {
  const char *what = "spacap_proposal_decode_bwd_f32";
  SPACAP_REQUIRE(B >= 0 && K >= 1 && NH >= 1 && NS >= 1 && NC >= 1, "%s: bad sizes", what);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(mean_size && d_net, "%s: null pointer", what);
  const int CH = 5 + 2 * NH + 4 * NS + NC;
  SPACAP_REQUIRE((size_t)64 * (CH + 1) * sizeof(float) <= 64 * 1024, "%s: too many channels (%d)", what, CH);
  hipLaunchKernelGGL(proposal_decode_bwd_kernel, dim3((K + 63) / 64, B), dim3(256), (size_t)64 * (CH + 1) * sizeof(float),
                     spacap::as_stream(stream), g_nt, g_center,
                     g_heading_res, g_size_res, mean_size, K, NH, NS, NC, d_net);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// ---- votes from the voting module's last convolution (models/voting_module.py:49-60) ---------------------------------------
// net f32 [B, 3 + C, N] (channel-major conv output, vote_factor 1), seed_xyz f32 [B, N, 3], seed_features f32 [B, C, N] ->
//   vote_xyz [B, N, 3] = seed_xyz + net[:, 0:3]^T,   vote_features [B, N, C] (point-major) = seed_features^T + net[:, 3:]^T
// As tensor operations: a transposed view, two slices, two broadcast adds, two contiguous copies forward, and slice / add /
// transpose copies with zero fills in the backward.  32 x 32 tiles through LDS, reads coalesced over n, writes over c.
namespace {
__global__ __launch_bounds__(256) void vote_assemble_fwd_kernel(const float *__restrict__ net, const float *__restrict__ seed_xyz,
                                                                const float *__restrict__ seed_feat, int C, int N,
                                                                float *__restrict__ vote_xyz, float *__restrict__ vote_feat) {
  __shared__ float s[32][33];
  const int b = blockIdx.z, c0 = blockIdx.y * 32, n0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const float *nb = net + (size_t)b * (3 + C) * N;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, n = n0 + tx;
    s[ty + 8 * i][tx] = (c < C && n < N) ? seed_feat[((size_t)b * C + c) * N + n] + nb[(size_t)(3 + c) * N + n] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + ty + 8 * i, c = c0 + tx;
    if (n < N && c < C) vote_feat[((size_t)b * N + n) * C + c] = s[tx][ty + 8 * i];
  }
  if (blockIdx.y == 0 && threadIdx.x < 96) {
    const int n = n0 + threadIdx.x / 3, k = threadIdx.x % 3;
    if (n < N) vote_xyz[((size_t)b * N + n) * 3 + k] = seed_xyz[((size_t)b * N + n) * 3 + k] + nb[(size_t)k * N + n];
  }
}

// d net [B, 3 + C, N] and d seed_features [B, C, N] (= d net[:, 3:]) from g_xyz [B, N, 3] (may be null: zeros) and g_feat [B, N, C]
__global__ __launch_bounds__(256) void vote_assemble_bwd_kernel(const float *__restrict__ g_xyz, const float *__restrict__ g_feat,
                                                                int C, int N, float *__restrict__ d_net, float *__restrict__ d_seed) {
  __shared__ float s[32][33];
  const int b = blockIdx.z, c0 = blockIdx.y * 32, n0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  float *nb = d_net + (size_t)b * (3 + C) * N;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + ty + 8 * i, c = c0 + tx;
    s[ty + 8 * i][tx] = (n < N && c < C && g_feat) ? g_feat[((size_t)b * N + n) * C + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, n = n0 + tx;
    if (c < C && n < N) {
      const float v = s[tx][ty + 8 * i];
      nb[(size_t)(3 + c) * N + n] = v;
      if (d_seed) d_seed[((size_t)b * C + c) * N + n] = v;
    }
  }
  if (blockIdx.y == 0 && threadIdx.x < 96) {
    const int k = threadIdx.x >> 5, n = n0 + (threadIdx.x & 31);
    if (n < N) nb[(size_t)k * N + n] = g_xyz ? g_xyz[((size_t)b * N + n) * 3 + k] : 0.f;
  }
}
}  // namespace

extern "C" int spacap_vote_assemble_fwd_f32(const float *net, const float *seed_xyz, const float *seed_feat, int B, int C, int N,
                                            float *vote_xyz, float *vote_feat, spacap_stream_t stream) {
  const char *what = "spacap_vote_assemble_fwd_f32";
  SPACAP_REQUIRE(B >= 0 && C >= 1 && N >= 1 && B <= 65535, "%s: bad sizes", what);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(net && seed_xyz && seed_feat && vote_xyz && vote_feat, "%s: null pointer", what);
  hipLaunchKernelGGL(vote_assemble_fwd_kernel, dim3((N + 31) / 32, (C + 31) / 32, B), dim3(256), 0, spacap::as_stream(stream), net,
                     seed_xyz, seed_feat, C, N, vote_xyz, vote_feat);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_vote_assemble_bwd_f32(const float *g_xyz, const float *g_feat, int B, int C, int N, float *d_net, float *d_seed,
                                            spacap_stream_t stream) {
  const char *what = "spacap_vote_assemble_bwd_f32";
  SPACAP_REQUIRE(B >= 0 && C >= 1 && N >= 1 && B <= 65535, "%s: bad sizes", what);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(d_net, "%s: null pointer", what);
  hipLaunchKernelGGL(vote_assemble_bwd_kernel, dim3((N + 31) / 32, (C + 31) / 32, B), dim3(256), 0, spacap::as_stream(stream), g_xyz,
                     g_feat, C, N, d_net, d_seed);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

