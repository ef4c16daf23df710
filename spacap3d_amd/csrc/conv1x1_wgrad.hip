// spacap_conv1x1_wgrad_*, for gfx950 (MI355X): one launch per layer, or the layers of a backward pass in one batched launch.
// The forward and data-gradient products of the same layers are in conv1x1.hip, which is built with contraction off; this
// file is built with -ffp-contract=fast (csrc/Makefile: CONTRACT_FAST), as these kernels always were.
//
// Weight gradient of a 1x1 convolution on CHANNEL-MAJOR tensors (the vote net and the feature-propagation MLPs:
// models/voting_module.py:33-60, lib/pointnet2/pointnet2_modules.py:376-421; Conv1d/Conv2d k = 1 on (B, C, N)):
//   dW[co, ci] = sum_b sum_n g[b, co, n] x[b, ci, n]
// The convolution library runs this as an implicit-GEMM weight-gradient kernel (46 - 60 us for 256 x 256 over
// 8 x 1 024 points) or as one small GEMM per scene; here both operands are read as [channel][32 points] panels
// (contiguous along n), each (scene, point range) slab accumulates a 128 x 128 block by MFMA and writes a partial
// result; the caller adds the slabs in order (spacap_sum_slabs_f32).
#include "common.hpp"
#include "launch.hpp"
#include "mfma.hpp"

namespace {
using namespace spacap::mfma;

// with_bias: the partial row is [CO * CI | CO rounded up to 4] and its tail receives db[co] = sum over the slab's points of g
// (a column of ones beside x; written by the workgroups of the first input-channel block)
__device__ __forceinline__ void conv1x1_wgrad_body(const float *__restrict__ g, const float *__restrict__ x, int CO, int CI,
                                                   int N, int nsplit, float *__restrict__ part, int bx, int by, int bz,
                                                   int with_bias = 0) {
  constexpr int CB = 128, KT = 32, LDK = KT + 4;
  __shared__ __attribute__((aligned(16))) float s_g[CB * LDK];
  __shared__ __attribute__((aligned(16))) float s_x[CB * LDK];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int b = bx / nsplit, sl = bx % nsplit;
  const int co0 = by * CB, ci0 = bz * CB;
  const int tiles = N / KT, t_begin = (int)((long)tiles * sl / nsplit), t_end = (int)((long)tiles * (sl + 1) / nsplit);
  const float *gb = g + ((size_t)b * CO + co0) * N, *xb = x + ((size_t)b * CI + ci0) * N;
  const int k4 = tid & 7, c0 = tid >> 3;   // 8 float4 per 32-point row, 32 channels per pass
  f32x4 acc[2][8];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 8; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 accb[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const bool wb = with_bias && bz == 0;
  for (int t = t_begin; t < t_end; ++t) {
    const int n0 = t * KT;
#pragma unroll
    for (int i = 0; i < CB / 32; ++i) {
      const int c = c0 + 32 * i;   // (channels past the end re-read the last one: their products are never stored)
      st4(&s_g[c * LDK + k4 * 4], ld4(gb + (size_t)min(c, CO - 1 - co0) * N + n0 + k4 * 4));
      st4(&s_x[c * LDK + k4 * 4], ld4(xb + (size_t)min(c, CI - 1 - ci0) * N + n0 + k4 * 4));
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < KT / 4; ++ks) {
      float af[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) af[m] = s_g[((w * 2 + m) * 16 + l15) * LDK + ks * 4 + lg];
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const float bb = s_x[(n * 16 + l15) * LDK + ks * 4 + lg];
#pragma unroll
        for (int m = 0; m < 2; ++m) acc[m][n] = MFMA16(af[m], bb, acc[m][n]);
      }
      if (wb) {
#pragma unroll
        for (int m = 0; m < 2; ++m) accb[m] = MFMA16(af[m], 1.0f, accb[m]);
      }
    }
    __syncthreads();
  }
  float *o = part + (size_t)bx * ((size_t)CO * CI + (with_bias ? (size_t)((CO + 3) & ~3) : 0));
  if (wb && l15 == 0) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int row = co0 + (w * 2 + m) * 16 + 4 * lg + u;
        if (row < ((CO + 3) & ~3)) o[(size_t)CO * CI + row] = row < CO ? accb[m][u] : 0.f;
      }
  }
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 8; ++n)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int row = co0 + (w * 2 + m) * 16 + 4 * lg + u, col = ci0 + n * 16 + l15;
        if (row < CO && col < CI) o[(size_t)row * CI + col] = acc[m][n][u];
      }
}

__global__ __launch_bounds__(256) void conv1x1_wgrad_kernel(const float *__restrict__ g, const float *__restrict__ x, int CO,
                                                            int CI, int N, int nsplit, float *__restrict__ part) {
  conv1x1_wgrad_body(g, x, CO, CI, N, nsplit, part, blockIdx.x, blockIdx.y, blockIdx.z);
}

// Several 1x1-convolution weight gradients in one launch (end of a backward pass: see linear_wgrad_batched_kernel)
constexpr int CV_JOB_MAX = 64;
struct ConvJob {
  const float *g, *x;
  float *part;
  int CO, CI, N, nsplit, gx, gy, block0, with_bias;
};
struct ConvTable {
  int njobs, pad;
  ConvJob job[CV_JOB_MAX];
};
__global__ __launch_bounds__(256) void conv1x1_wgrad_batched_kernel(const ConvTable T) {
  int lo = 0, hi = T.njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (T.job[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const ConvJob J = T.job[lo];
  const int local = (int)blockIdx.x - J.block0;
  const int bx = local % J.gx, by = (local / J.gx) % J.gy, bz = local / (J.gx * J.gy);
  conv1x1_wgrad_body(J.g, J.x, J.CO, J.CI, J.N, J.nsplit, J.part, bx, by, bz, J.with_bias);
}

// ---- the same on the bf16 matrix cores with fp32-equivalent accuracy (split-bf16, mfma.hpp; the Linear layers' counterpart is
// linear_wgrad_bf3_body in linear_grad.hip) ------------------------------------------------------------------------------------
// (conv1x1_wgrad_body's tiling and partial layout.)  The contraction index n is the contiguous one here, so the images are
// [channel][32 points] with 80-byte rows (conflict-free 16-byte reads) and a fragment is one ds_read_b128; unlike the fp32 body
// the next tile's panels are in flight in registers while this tile is multiplied.
constexpr int CWB_LD = 32 + 8;               // bf16 elements per image row (80 bytes)
constexpr int CWB_IMG = 128 * CWB_LD;

__device__ __forceinline__ void conv1x1_wgrad_bf3_body(const float *__restrict__ g, const float *__restrict__ x, int CO, int CI, int N,
                                                       int nsplit, float *__restrict__ part, int bx, int by, int bz, int with_bias) {
  constexpr int CB = 128, KT = 32;
  __shared__ __attribute__((aligned(16))) __bf16 s_g[3 * CWB_IMG];
  __shared__ __attribute__((aligned(16))) __bf16 s_x[3 * CWB_IMG];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int b = bx / nsplit, sl = bx % nsplit;
  const int co0 = by * CB, ci0 = bz * CB;
  const int tiles = N / KT, t_begin = (int)((long)tiles * sl / nsplit), t_end = (int)((long)tiles * (sl + 1) / nsplit);
  const float *gb = g + ((size_t)b * CO + co0) * N, *xb = x + ((size_t)b * CI + ci0) * N;
  const int k4 = tid & 7, c0 = tid >> 3;   // 8 float4 per 32-point row, 32 channels per pass
  f32x4 acc[2][8];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 8; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 accb[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const bool wb = with_bias && bz == 0;
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.0f;
  f32x4 pa[CB / 32], pb[CB / 32];
  auto fetch = [&](int t) {
    const int n0 = (t < t_end ? t : t_end - 1) * KT;   // (past the end: a harmless re-read, never staged)
#pragma unroll
    for (int i = 0; i < CB / 32; ++i) {
      const int c = c0 + 32 * i;   // (channels past the end re-read the last one: their products are never stored)
      pa[i] = ld4(gb + (size_t)min(c, CO - 1 - co0) * N + n0 + k4 * 4);
      pb[i] = ld4(xb + (size_t)min(c, CI - 1 - ci0) * N + n0 + k4 * 4);
    }
  };
  if (t_begin < t_end) fetch(t_begin);
  for (int t = t_begin; t < t_end; ++t) {
#pragma unroll
    for (int i = 0; i < CB / 32; ++i) {
      const int o = (c0 + 32 * i) * CWB_LD + k4 * 4;
      bf16x4 p0, p1, p2;
      split4(pa[i], p0, p1, p2);
      *reinterpret_cast<bf16x4 *>(&s_g[o]) = p0;
      *reinterpret_cast<bf16x4 *>(&s_g[CWB_IMG + o]) = p1;
      *reinterpret_cast<bf16x4 *>(&s_g[2 * CWB_IMG + o]) = p2;
      split4(pb[i], p0, p1, p2);
      *reinterpret_cast<bf16x4 *>(&s_x[o]) = p0;
      *reinterpret_cast<bf16x4 *>(&s_x[CWB_IMG + o]) = p1;
      *reinterpret_cast<bf16x4 *>(&s_x[2 * CWB_IMG + o]) = p2;
    }
    __syncthreads();
    if (t + 1 < t_end) fetch(t + 1);
    bf16x8 a[2][3];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int q = 0; q < 3; ++q)
        a[m][q] = *reinterpret_cast<const bf16x8 *>(&s_g[q * CWB_IMG + ((w * 2 + m) * 16 + l15) * CWB_LD + 8 * lg]);
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      bf16x8 bq[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) bq[q] = *reinterpret_cast<const bf16x8 *>(&s_x[q * CWB_IMG + (n * 16 + l15) * CWB_LD + 8 * lg]);
#pragma unroll
      for (int m = 0; m < 2; ++m) acc[m][n] = mfma6(a[m], bq, acc[m][n]);
    }
    if (wb) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 2; q >= 0; --q) accb[m] = MFMA_B(a[m][q], ones, accb[m]);
    }
    __syncthreads();
  }
  float *o = part + (size_t)bx * ((size_t)CO * CI + (with_bias ? (size_t)((CO + 3) & ~3) : 0));
  if (wb && l15 == 0) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int row = co0 + (w * 2 + m) * 16 + 4 * lg + u;
        if (row < ((CO + 3) & ~3)) o[(size_t)CO * CI + row] = row < CO ? accb[m][u] : 0.f;
      }
  }
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 8; ++n)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int row = co0 + (w * 2 + m) * 16 + 4 * lg + u, col = ci0 + n * 16 + l15;
        if (row < CO && col < CI) o[(size_t)row * CI + col] = acc[m][n][u];
      }
}

// (the split-bf16 bodies: the default; SPACAP_SA_F32MFMA=1 keeps the fp32-MFMA ones)
__global__ __launch_bounds__(256) void conv1x1_wgrad_bf3_kernel(const float *__restrict__ g, const float *__restrict__ x, int CO,
                                                                int CI, int N, int nsplit, float *__restrict__ part) {
  conv1x1_wgrad_bf3_body(g, x, CO, CI, N, nsplit, part, blockIdx.x, blockIdx.y, blockIdx.z, 0);
}
__global__ __launch_bounds__(256) void conv1x1_wgrad_bf3_batched_kernel(const ConvTable T) {
  int lo = 0, hi = T.njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (T.job[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const ConvJob J = T.job[lo];
  const int local = (int)blockIdx.x - J.block0;
  const int bx = local % J.gx, by = (local / J.gx) % J.gy, bz = local / (J.gx * J.gy);
  conv1x1_wgrad_bf3_body(J.g, J.x, J.CO, J.CI, J.N, J.nsplit, J.part, bx, by, bz, J.with_bias);
}

inline int conv1x1_nsplit(int B, int CO, int CI, int N) {
  const long yz = (long)((CO + 127) / 128) * ((CI + 127) / 128), tiles = N / 32;
  long n = 512 / (yz * B), cap = (4L << 20) / ((long)CO * CI * B);
  if (n > cap) n = cap;
  if (n > tiles) n = tiles;
  return (int)(n < 1 ? 1 : n);
}
}  // namespace

// number of partial results (= B x point ranges) for a (B, CO, CI, N) problem; 0 when the shape has no kernel
extern "C" int spacap_conv1x1_wgrad_slabs(int B, int CO, int CI, int N) {
  if (B < 1 || N < 32 || N % 32 || CO < 1 || CI < 1) return 0;   // (any widths: 128 x 128 tiles with clamped tails)
  return B * conv1x1_nsplit(B, CO, CI, N);
}

// slabs per job inside a batch (the batch fills the chip: ~16 point tiles per workgroup)
extern "C" int spacap_conv1x1_wgrad_slabs_batched(int B, int CO, int CI, int N) {
  if (spacap_conv1x1_wgrad_slabs(B, CO, CI, N) == 0) return 0;
  // (512 points per workgroup: half the partial-sum traffic of 256 -- 65 instead of 130 MB per step at cfg2 -- and still ~1 000
  // workgroups in the step's batch; 6.60 -> 6.57 ms same box, 1 024 points gives it back)
  int nsplit = N / 512;
  if (nsplit < 1) nsplit = 1;
  const int single = conv1x1_nsplit(B, CO, CI, N);
  return B * (nsplit < single ? nsplit : single);
}

// njobs independent 1x1-convolution weight gradients in one launch; all arrays are HOST arrays (read before the call
// returns); part[i] receives nslabs[i] = B[i] x (point ranges) partial results (add in order).
extern "C" int spacap_conv1x1_wgrad_batched_f32(const float *const *g, const float *const *x, const int *B, const int *CO,
                                                const int *CI, const int *N, const int *nslabs, const int *with_bias,
                                                float *const *part, int njobs, spacap_stream_t stream) {
  const char *what = "spacap_conv1x1_wgrad_batched_f32";
  SPACAP_REQUIRE(njobs >= 0 && (njobs == 0 || (g && x && B && CO && CI && N && nslabs && part)), "%s: bad arguments", what);
  hipStream_t s = spacap::as_stream(stream);
  int i = 0;
  while (i < njobs) {
    ConvTable T;
    T.njobs = 0, T.pad = 0;
    long blocks = 0;
    for (; i < njobs && T.njobs < CV_JOB_MAX; ++i) {
      SPACAP_REQUIRE(spacap_conv1x1_wgrad_slabs(B[i], CO[i], CI[i], N[i]) > 0 && nslabs[i] >= B[i] && nslabs[i] % B[i] == 0 &&
                         g[i] && x[i] && part[i],
                     "%s: job %d: (B=%d, CO=%d, CI=%d, N=%d, slabs=%d) unsupported or null pointer", what, i, B[i], CO[i], CI[i],
                     N[i], nslabs[i]);
      ConvJob &J = T.job[T.njobs++];
      J.g = g[i], J.x = x[i], J.part = part[i], J.CO = CO[i], J.CI = CI[i], J.N = N[i];
      J.nsplit = nslabs[i] / B[i], J.gx = nslabs[i], J.gy = (CO[i] + 127) / 128, J.block0 = (int)blocks, J.with_bias = with_bias ? with_bias[i] : 0;
      blocks += (long)nslabs[i] * ((CO[i] + 127) / 128) * ((CI[i] + 127) / 128);
      SPACAP_REQUIRE(blocks < 2147483647L, "%s: too many blocks", what);
    }
    if (!spacap::sa_f32_mfma_only()) hipLaunchKernelGGL(conv1x1_wgrad_bf3_batched_kernel, dim3((unsigned)blocks), dim3(256), 0, s, T);
    else hipLaunchKernelGGL(conv1x1_wgrad_batched_kernel, dim3((unsigned)blocks), dim3(256), 0, s, T);
  }
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// g f32 [B,CO,N], x f32 [B,CI,N] dense; part f32 [spacap_conv1x1_wgrad_slabs(B,CO,CI,N)][CO*CI]
extern "C" int spacap_conv1x1_wgrad_f32(const float *g, const float *x, int B, int CO, int CI, int N, float *part,
                                        spacap_stream_t stream) {
  const char *what = "spacap_conv1x1_wgrad_f32";
  const int nslab = spacap_conv1x1_wgrad_slabs(B, CO, CI, N);
  SPACAP_REQUIRE(nslab > 0, "%s: (B=%d, CO=%d, CI=%d, N=%d) unsupported", what, B, CO, CI, N);
  SPACAP_REQUIRE(g && x && part, "%s: null pointer", what);
  if (!spacap::sa_f32_mfma_only())
    hipLaunchKernelGGL(conv1x1_wgrad_bf3_kernel, dim3(nslab, (CO + 127) / 128, (CI + 127) / 128), dim3(256), 0, spacap::as_stream(stream), g, x,
                       CO, CI, N, nslab / B, part);
  else
    hipLaunchKernelGGL(conv1x1_wgrad_kernel, dim3(nslab, (CO + 127) / 128, (CI + 127) / 128), dim3(256), 0, spacap::as_stream(stream), g, x, CO, CI,
                       N, nslab / B, part);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
