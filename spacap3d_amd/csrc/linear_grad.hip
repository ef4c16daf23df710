// Backward of torch.nn.Linear on row-major activations, for gfx950 (MI355X): the weight + bias gradient
// (spacap_linear_wgrad_*: one launch per layer, or every layer of a training step in one batched launch through a job table)
// and the feed-forward block's w_2 data gradient fused with the relu + dropout mask (spacap_linear_dgrad_mask_f32).
// Callers: the Linear autograd functions, the fused Transformer layer and the end-of-backward flush of the Python package.
// Built with -ffp-contract=fast (csrc/Makefile: CONTRACT_FAST), as these kernels always were.
#include "common.hpp"
#include "launch.hpp"
#include "mfma.hpp"

namespace {
using namespace spacap::mfma;
constexpr int TM = 64;      // rows per tile of the data-gradient product
constexpr int TW = 32;      // rows per tile of the weight-gradient products
}  // namespace

// Weight + bias gradient of a Linear layer:  dW[ck, cp] = sum_r g[r, ck] x[r, cp],  db[ck] = sum_r g[r, ck]
// (torch.nn.Linear backward: models/transformer_captioner.py's projections and feed-forward layers).  The BLAS
// path runs these [<= 2048 rows] x [128..2048]^2 reductions as a memset + a split-K GEMM + a separate column-sum
// kernel (30 us of mostly latency for 67 MFLOP); here one launch produces per-slab partials of both (the bias
// gradient falls out of the same staged tile as one more MFMA column against a constant 1), summed in slab order
// by the caller.
namespace {
// (bx, gx): slab index / number of slabs; by, bz: 128-wide blocks of CK and CP
template <bool WITH_BIAS>
__device__ __forceinline__ void linear_wgrad_body(const float *__restrict__ g, const float *__restrict__ x, int CK, int CP,
                                                  long R, float *__restrict__ part, int bx, int by, int bz, int gx) {
  constexpr int CB = 128, LDG = CB + 16;
  __shared__ __attribute__((aligned(16))) float s_g[TW * LDG];
  __shared__ __attribute__((aligned(16))) float s_x[TW * LDG];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int ck0 = by * CB, cp0 = bz * CB;
  const int c4 = tid & 31, r0 = tid >> 5;  // 32 float4 per 128-wide row, 8 rows per pass
  f32x4 acc[2][8], accb[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    accb[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < 8; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const long ntiles = (R + TW - 1) / TW;
  // register pipeline: the next tile's rows are in flight while this tile's MFMAs run (a workgroup per CU has nobody
  // else to hide the load latency behind)
  f32x4 pa[TW / 8], pb[TW / 8];
  auto fetch = [&](long t) {
    const long row0 = t * TW;
#pragma unroll
    for (int i = 0; i < TW / 8; ++i) {
      const int row = r0 + 8 * i;
      pa[i] = pb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t < ntiles && row0 + row < R) {
        pa[i] = ld4(g + (size_t)(row0 + row) * CK + ck0 + c4 * 4);
        pb[i] = ld4(x + (size_t)(row0 + row) * CP + cp0 + c4 * 4);
      }
    }
  };
  fetch(bx);
  for (long t = bx; t < ntiles; t += gx) {
#pragma unroll
    for (int i = 0; i < TW / 8; ++i) {
      const int row = r0 + 8 * i;
      st4(&s_g[row * LDG + c4 * 4], pa[i]);
      st4(&s_x[row * LDG + c4 * 4], pb[i]);
    }
    __syncthreads();
    fetch(t + gx);
#pragma unroll
    for (int ks = 0; ks < TW / 4; ++ks) {
      float af[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) af[m] = s_g[(ks * 4 + lg) * LDG + (w * 2 + m) * 16 + l15];
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const float b = s_x[(ks * 4 + lg) * LDG + n * 16 + l15];
#pragma unroll
        for (int m = 0; m < 2; ++m) acc[m][n] = MFMA16(af[m], b, acc[m][n]);
      }
      if (WITH_BIAS) {
#pragma unroll
        for (int m = 0; m < 2; ++m) accb[m] = MFMA16(af[m], 1.0f, accb[m]);
      }
    }
    __syncthreads();
  }
  // partial layout per slab: [CK][CP] weights, then [CK] bias
  float *o = part + (size_t)bx * ((size_t)CK * CP + (WITH_BIAS ? CK : 0));
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 8; ++n)
#pragma unroll
      for (int u = 0; u < 4; ++u)
        o[(size_t)(ck0 + (w * 2 + m) * 16 + 4 * lg + u) * CP + cp0 + n * 16 + l15] = acc[m][n][u];
  if (WITH_BIAS && bz == 0 && l15 == 0) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int u = 0; u < 4; ++u) o[(size_t)CK * CP + ck0 + (w * 2 + m) * 16 + 4 * lg + u] = accb[m][u];
  }
}
template <bool WITH_BIAS>
__global__ __launch_bounds__(256) void linear_wgrad_kernel(const float *__restrict__ g, const float *__restrict__ x, int CK,
                                                           int CP, long R, float *__restrict__ part) {
  linear_wgrad_body<WITH_BIAS>(g, x, CK, CP, R, part, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x);
}

// Many weight gradients in ONE launch: the backward of a training step produces ~50 of them, most far too small to
// fill the chip (the decoder's: 8 slabs x 1 - 16 blocks) and each a launch of its own; nothing but the optimizer
// reads them, so they can all run together when the backward is over.  Job table by value in the kernel arguments
// (hipGraph-capturable as it is); a workgroup finds its job by binary search over the first-block prefix.  (The lookup is
// written out in each batched kernel, here and in conv1x1_wgrad.hip: behind a shared helper the compiler orders it differently.)
constexpr int WG_JOB_MAX = 72;
struct WgradJob {
  const float *g, *x;
  float *part;
  long R;
  int CK, CP, gx, gy, with_bias, block0;
};
struct WgradTable {
  int njobs, pad;
  WgradJob job[WG_JOB_MAX];
};

// ---- the same on the bf16 matrix cores with fp32-equivalent accuracy (split-bf16, mfma.hpp) ------------------------------------
//   dW[ck, cp] = sum_r g[r, ck] x[r, cp],   db[ck] = sum_r g[r, ck]           (torch.nn.Linear backward; the projections and
//   feed-forward layers of models/transformer_captioner.py:52-81, the relation head's :319-326 at d_model = 512)
//
// The fp32-MFMA body (linear_wgrad_body) is matrix-pipe bound: 16.5 GFLOP per training step at 1/16 of the bf16 rate.  Here
// both operands of a 32-row tile are split into three bf16 pieces (x = x1 + x2 + x3, 24 significant bits) while they are
// staged, and a product is the six piece products above 2^-24 on v_mfma_f32_16x16x32_bf16: 6/16 of the fp32-MFMA time.
// The contraction runs over the ROWS, i.e. across the direction both operands are stored in: the LDS images stay row-major
// [row][channel] (8-byte stores straight from the staging registers) and the fragments are read with ds_read_b64_tr_b16, the
// transposing LDS read of gfx950 -- a lane gets four consecutive rows of its channel per read, two reads per operand piece.
// (Plain padded rows: the two 4-row blocks a 32-lane half reads are 8 rows apart and meet on the same banks, a 2-way
// conflict on 60 reads per tile against 96 matrix instructions: not worth a swizzle.)
// Same tiling, slab structure and partial layout as linear_wgrad_body: one workgroup = one 128 x 128 block of dW over a row
// slab, wave w owns rows 32 w .. 32 w + 31 of the block.
constexpr int WB_LD = 128 + 8;               // bf16 elements per image row (272 bytes)
constexpr int WB_IMG = TW * WB_LD;           // one piece of one operand

// (WITH_BIAS is a run-time flag on purpose: two instantiations in the batched kernel would each bring their own 52 KB of LDS)
__device__ __forceinline__ void linear_wgrad_bf3_body(const bool WITH_BIAS, const float *__restrict__ g, const float *__restrict__ x, int CK,
                                                      int CP, long R, float *__restrict__ part, int bx, int by, int bz, int gx) {
  constexpr int CB = 128;
  __shared__ __attribute__((aligned(16))) __bf16 s_g[3 * WB_IMG];
  __shared__ __attribute__((aligned(16))) __bf16 s_x[3 * WB_IMG];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int ck0 = by * CB, cp0 = bz * CB;
  const int c4 = tid & 31, r0 = tid >> 5;  // 32 float4 per 128-wide row, 8 rows per pass
  f32x4 acc[2][8], accb[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    accb[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < 8; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const long ntiles = (R + TW - 1) / TW;
  f32x4 pa[TW / 8], pb[TW / 8];
  auto fetch = [&](long t) {
    const long row0 = t * TW;
#pragma unroll
    for (int i = 0; i < TW / 8; ++i) {
      const int row = r0 + 8 * i;
      pa[i] = pb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t < ntiles && row0 + row < R) {
        pa[i] = ld4(g + (size_t)(row0 + row) * CK + ck0 + c4 * 4);
        pb[i] = ld4(x + (size_t)(row0 + row) * CP + cp0 + c4 * 4);
      }
    }
  };
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.0f;
  fetch(bx);
  for (long t = bx; t < ntiles; t += gx) {
#pragma unroll
    for (int i = 0; i < TW / 8; ++i) {
      const int o = (r0 + 8 * i) * WB_LD + c4 * 4;
      bf16x4 p0, p1, p2;
      split4(pa[i], p0, p1, p2);
      *reinterpret_cast<bf16x4 *>(&s_g[o]) = p0;
      *reinterpret_cast<bf16x4 *>(&s_g[WB_IMG + o]) = p1;
      *reinterpret_cast<bf16x4 *>(&s_g[2 * WB_IMG + o]) = p2;
      split4(pb[i], p0, p1, p2);
      *reinterpret_cast<bf16x4 *>(&s_x[o]) = p0;
      *reinterpret_cast<bf16x4 *>(&s_x[WB_IMG + o]) = p1;
      *reinterpret_cast<bf16x4 *>(&s_x[2 * WB_IMG + o]) = p2;
    }
    __syncthreads();
    fetch(t + gx);
    bf16x8 a[2][3];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int q = 0; q < 3; ++q) a[m][q] = tr_frag<WB_LD>(s_g + q * WB_IMG, (w * 2 + m) * 16, lane);
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      bf16x8 b[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) b[q] = tr_frag<WB_LD>(s_x + q * WB_IMG, n * 16, lane);
#pragma unroll
      for (int m = 0; m < 2; ++m) acc[m][n] = mfma6(a[m], b, acc[m][n]);
    }
    if (WITH_BIAS) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 2; q >= 0; --q) accb[m] = MFMA_B(a[m][q], ones, accb[m]);
    }
    __syncthreads();
  }
  // partial layout per slab: [CK][CP] weights, then [CK] bias
  float *o = part + (size_t)bx * ((size_t)CK * CP + (WITH_BIAS ? CK : 0));
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 8; ++n)
#pragma unroll
      for (int u = 0; u < 4; ++u)
        o[(size_t)(ck0 + (w * 2 + m) * 16 + 4 * lg + u) * CP + cp0 + n * 16 + l15] = acc[m][n][u];
  if (WITH_BIAS && bz == 0 && l15 == 0) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int u = 0; u < 4; ++u) o[(size_t)CK * CP + ck0 + (w * 2 + m) * 16 + 4 * lg + u] = accb[m][u];
  }
}
template <bool WITH_BIAS>
__global__ __launch_bounds__(256) void linear_wgrad_bf3_kernel(const float *__restrict__ g, const float *__restrict__ x, int CK,
                                                               int CP, long R, float *__restrict__ part) {
  linear_wgrad_bf3_body(WITH_BIAS, g, x, CK, CP, R, part, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x);
}

// (the split-bf16 body: the default; SPACAP_SA_F32MFMA=1 keeps the fp32-MFMA body)
__global__ __launch_bounds__(256) void linear_wgrad_bf3_batched_kernel(const WgradTable T) {
  int lo = 0, hi = T.njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (T.job[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const WgradJob J = T.job[lo];
  const int local = (int)blockIdx.x - J.block0;
  const int bx = local % J.gx, by = (local / J.gx) % J.gy, bz = local / (J.gx * J.gy);
  linear_wgrad_bf3_body(J.with_bias != 0, J.g, J.x, J.CK, J.CP, J.R, J.part, bx, by, bz, J.gx);
}
__global__ __launch_bounds__(256) void linear_wgrad_batched_kernel(const WgradTable T) {
  int lo = 0, hi = T.njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (T.job[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const WgradJob J = T.job[lo];
  const int local = (int)blockIdx.x - J.block0;
  const int bx = local % J.gx, by = (local / J.gx) % J.gy, bz = local / (J.gx * J.gy);
  if (J.with_bias) linear_wgrad_body<true>(J.g, J.x, J.CK, J.CP, J.R, J.part, bx, by, bz, J.gx);
  else linear_wgrad_body<false>(J.g, J.x, J.CK, J.CP, J.R, J.part, bx, by, bz, J.gx);
}
}  // namespace

// number of row slabs (= partial results) for a (rows, CK, CP) problem; 0 when the shape has no kernel
extern "C" int spacap_linear_wgrad_slabs(long R, int CK, int CP) {
  if (R < 1 || CK < 128 || CP < 128 || CK % 128 || CP % 128) return 0;
  const long tiles = (R + TW - 1) / TW, yz = (long)(CK / 128) * (CP / 128);
  long n = 1024 / yz, cap = (4L << 20) / ((long)CK * CP);
  if (n > cap) n = cap;
  if (n > tiles) n = tiles;
  return (int)(n < 1 ? 1 : n);
}

// part f32 [spacap_linear_wgrad_slabs(R,CK,CP)][CK*CP (+ CK when with_bias)]
extern "C" int spacap_linear_wgrad_f32(const float *g, const float *x, long R, int CK, int CP, int with_bias, float *part,
                                       spacap_stream_t stream) {
  const char *what = "spacap_linear_wgrad_f32";
  const int nslab = spacap_linear_wgrad_slabs(R, CK, CP);
  SPACAP_REQUIRE(nslab > 0, "%s: (R=%ld, CK=%d, CP=%d) unsupported", what, R, CK, CP);
  SPACAP_REQUIRE(g && x && part, "%s: null pointer", what);
  hipStream_t s = spacap::as_stream(stream);
  const dim3 grid(nslab, CK / 128, CP / 128);
  if (!spacap::sa_f32_mfma_only()) {
    if (with_bias) hipLaunchKernelGGL((linear_wgrad_bf3_kernel<true>), grid, dim3(256), 0, s, g, x, CK, CP, R, part);
    else hipLaunchKernelGGL((linear_wgrad_bf3_kernel<false>), grid, dim3(256), 0, s, g, x, CK, CP, R, part);
  } else if (with_bias) hipLaunchKernelGGL((linear_wgrad_kernel<true>), grid, dim3(256), 0, s, g, x, CK, CP, R, part);
  else hipLaunchKernelGGL((linear_wgrad_kernel<false>), grid, dim3(256), 0, s, g, x, CK, CP, R, part);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// The same with the number of row slabs chosen by the caller (1 <= nslab <= row tiles): part f32 [nslab][CK*CP (+ CK)].  For the
// wide relation head of the stress configuration (4.2 M pair rows x 512 x 512): 64 slabs fill the chip twice over, where
// spacap_linear_wgrad_slabs' 4 M-element cap on a partial set would leave it 16.
extern "C" int spacap_linear_wgrad_nslab_f32(const float *g, const float *x, long R, int CK, int CP, int with_bias, int nslab, float *part,
                                             spacap_stream_t stream) {
  const char *what = "spacap_linear_wgrad_nslab_f32";
  SPACAP_REQUIRE(spacap_linear_wgrad_slabs(R, CK, CP) > 0 && nslab >= 1 && nslab <= 65535 && nslab <= (R + TW - 1) / TW,
                 "%s: (R=%ld, CK=%d, CP=%d, nslab=%d) unsupported", what, R, CK, CP, nslab);
  SPACAP_REQUIRE(g && x && part, "%s: null pointer", what);
  hipStream_t s = spacap::as_stream(stream);
  const dim3 grid(nslab, CK / 128, CP / 128);
  if (!spacap::sa_f32_mfma_only()) {
    if (with_bias) hipLaunchKernelGGL((linear_wgrad_bf3_kernel<true>), grid, dim3(256), 0, s, g, x, CK, CP, R, part);
    else hipLaunchKernelGGL((linear_wgrad_bf3_kernel<false>), grid, dim3(256), 0, s, g, x, CK, CP, R, part);
  } else if (with_bias) hipLaunchKernelGGL((linear_wgrad_kernel<true>), grid, dim3(256), 0, s, g, x, CK, CP, R, part);
  else hipLaunchKernelGGL((linear_wgrad_kernel<false>), grid, dim3(256), 0, s, g, x, CK, CP, R, part);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// njobs independent weight gradients in one launch (same values as njobs calls of spacap_linear_wgrad_f32 with the
// same arguments when nslabs[i] = spacap_linear_wgrad_slabs(...); any other slab count only changes how the rows are
// grouped).  All arrays are HOST arrays, read before the call returns; part[i] holds nslabs[i] partial results.
// slabs per job when many jobs share one launch: the batch fills the chip, so a workgroup can take 8 row tiles
// (fewer partial results to write and to add up; one slab = the result itself for the decoder's 256 rows)
extern "C" int spacap_linear_wgrad_slabs_batched(long R, int CK, int CP) {
  const int single = spacap_linear_wgrad_slabs(R, CK, CP);
  if (single == 0) return 0;
  const long tiles = (R + TW - 1) / TW;
  long n = tiles / 8;
  if (n < 1) n = 1;
  return (int)(n < single ? n : single);
}

extern "C" int spacap_linear_wgrad_batched_f32(const float *const *g, const float *const *x, const long *R, const int *CK,
                                               const int *CP, const int *with_bias, const int *nslabs, float *const *part,
                                               int njobs, spacap_stream_t stream) {
  const char *what = "spacap_linear_wgrad_batched_f32";
  SPACAP_REQUIRE(njobs >= 0 && (njobs == 0 || (g && x && R && CK && CP && with_bias && nslabs && part)), "%s: bad arguments",
                 what);
  hipStream_t s = spacap::as_stream(stream);
  int i = 0;
  while (i < njobs) {
    WgradTable T;
    T.njobs = 0, T.pad = 0;
    long blocks = 0;
    for (; i < njobs && T.njobs < WG_JOB_MAX; ++i) {
      const int nslab = nslabs[i];
      SPACAP_REQUIRE(spacap_linear_wgrad_slabs(R[i], CK[i], CP[i]) > 0 && nslab >= 1 && g[i] && x[i] && part[i],
                     "%s: job %d: (R=%ld, CK=%d, CP=%d, slabs=%d) unsupported or null pointer", what, i, R[i], CK[i], CP[i], nslab);
      WgradJob &J = T.job[T.njobs++];
      J.g = g[i], J.x = x[i], J.part = part[i], J.R = R[i], J.CK = CK[i], J.CP = CP[i];
      J.gx = nslab, J.gy = CK[i] / 128, J.with_bias = with_bias[i], J.block0 = (int)blocks;
      blocks += (long)nslab * (CK[i] / 128) * (CP[i] / 128);
      SPACAP_REQUIRE(blocks < 2147483647L, "%s: too many blocks", what);
    }
    if (!spacap::sa_f32_mfma_only()) hipLaunchKernelGGL(linear_wgrad_bf3_batched_kernel, dim3((unsigned)blocks), dim3(256), 0, s, T);
    else hipLaunchKernelGGL(linear_wgrad_batched_kernel, dim3((unsigned)blocks), dim3(256), 0, s, T);
  }
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// ---- feed-forward data gradient --------------------------------------------------------------------------------------------
// Data gradient of the feed-forward block's second Linear fused with the backward of relu + dropout:
//   dx[r, n] = (y[r, n] > 0) ? scale * sum_k g[r, k] W[k, n] : 0        g [R, 128], W [128, CP] (= w_2.weight), y [R, CP]
// (models/transformer_captioner.py:117-126: w_2(dropout(relu(w_1 x))); y is the saved dropout(relu(.)) output, which is
// positive exactly where the unit was active and kept).  The BLAS library runs this row-major x row-major product at
// 28 TFLOP/s (37 us for 2048 x 2048 x 128) and the mask is one more pass over the 16 MB result.  Here: weights
// stationary in registers (K = 128), one 64-row tile per workgroup and column block, accumulators transposed through
// LDS so that y is read and dx written as full rows.
namespace {
__global__ __launch_bounds__(256) void linear_dgrad_mask_kernel(const float *__restrict__ g, const float *__restrict__ W,
                                                                const float *__restrict__ y, float scale, long R, int CP,
                                                                float *__restrict__ dx) {
  constexpr int CK = 128, NT = 2, LD = CK + 4, KS = CK / 4, C4 = CK / 4, NV = TM * C4 / 256, RSTEP = 256 / C4;
  constexpr int COB = 64 * NT, LDO = COB + 4, O4 = COB / 4, NO = TM * O4 / 256, OSTEP = 256 / O4;
  __shared__ __attribute__((aligned(16))) float s_a[TM * LD];
  __shared__ __attribute__((aligned(16))) float s_o[TM * LDO];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int cbb = blockIdx.y * COB, wc = w * 16 * NT, cb = cbb + wc;
  const long row0 = (long)blockIdx.x * TM;
  const int c4 = tid % C4, r0 = tid / C4, o4 = tid % O4, or0 = tid / O4;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int row = r0 + i * RSTEP;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (row0 + row < R) a = ld4(g + (size_t)(row0 + row) * CK + c4 * 4);
    st4(&s_a[row * LD + c4 * 4], a);
  }
  float wf[NT][KS];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) wf[j][ks] = W[(size_t)(ks * 4 + lg) * CP + cb + 16 * j + l15];
  __syncthreads();
  f32x4 acc[TM / 16][NT];
#pragma unroll
  for (int mt = 0; mt < TM / 16; ++mt)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
    for (int mt = 0; mt < TM / 16; ++mt) {
      const float b = s_a[(mt * 16 + l15) * LD + ks * 4 + lg];
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[mt][j] = MFMA16(wf[j][ks], b, acc[mt][j]);
    }
  }
#pragma unroll
  for (int mt = 0; mt < TM / 16; ++mt)
#pragma unroll
    for (int j = 0; j < NT; ++j) st4(&s_o[(mt * 16 + l15) * LDO + wc + 16 * j + 4 * lg], acc[mt][j]);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NO; ++i) {
    const int row = or0 + i * OSTEP;
    if (row0 + row < R) {
      const size_t o = (size_t)(row0 + row) * CP + cbb + o4 * 4;
      const f32x4 d = ld4(&s_o[row * LDO + o4 * 4]), yv = ld4(y + o);
      f32x4 r;
#pragma unroll
      for (int u = 0; u < 4; ++u) r[u] = yv[u] > 0.f ? d[u] * scale : 0.f;
      st4(dx + o, r);
    }
  }
}
}  // namespace

// g f32 [R,128], W f32 [128,CP] (CP a multiple of 128), y f32 [R,CP], dx f32 [R,CP]; all dense
extern "C" int spacap_linear_dgrad_mask_f32(const float *g, const float *W, const float *y, float scale, long R, int CK,
                                            int CP, float *dx, spacap_stream_t stream) {
  const char *what = "spacap_linear_dgrad_mask_f32";
  SPACAP_REQUIRE(R >= 0 && CK == 128 && CP >= 128 && CP % 128 == 0, "%s: (R=%ld, CK=%d, CP=%d) unsupported", what, R, CK, CP);
  if (R == 0) return SPACAP_OK;
  SPACAP_REQUIRE(g && W && y && dx, "%s: null pointer", what);
  const long tiles = (R + TM - 1) / TM;
  SPACAP_REQUIRE(tiles <= 2147483647L, "%s: too many rows", what);
  hipLaunchKernelGGL(linear_dgrad_mask_kernel, dim3((unsigned)tiles, CP / 128), dim3(256), 0, spacap::as_stream(stream), g, W, y,
                     scale, R, CP, dx);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
