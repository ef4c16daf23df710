// spacap_rel_tail_bwd_*, for gfx950 (MI355X).  Built with -ffp-contract=fast (csrc/Makefile: CONTRACT_FAST).
//
// Relation head, layers 2 and 3 (models/transformer_captioner.py:319-326, 392-397) on R = B*K*K pair rows:
//   hid2 = relu(hid1 W2^T + b2) [R,128],  pred = hid2 W3^T + b3 [R,NO3 = 9]
// Forward: sa_mid_fwd_kernel<128, 2, TAIL> in sa_fwd.hip (one pass: read hid1, write hid2 and pred; the composition of a BLAS GEMM,
// a ReLU pass and a second GEMM moves 5x the bytes).  Backward, first stage (this kernel): one streaming pass over
// hid2 that produces dz2 = (dpred W3) * (hid2 > 0) and per-workgroup partial sums of dW3 = dpred^T hid2,
// db2 = sum dz2 and db3 = sum dpred -- replacing a GEMM, a transposed GEMM, a masking pass and two column sums, each
// a full pass over a 268 MB tensor.  dhid1 = dz2 W2 and dW2 = dz2^T hid1 stay BLAS GEMMs (MFMA-bound).
// The forward's entry point, spacap_rel_tail_fwd_f32, sits beside the sa_mid_fwd_kernel template in sa_fwd.hip.
#include "common.hpp"
#include "mfma.hpp"

namespace {
using namespace spacap::mfma;

constexpr int RT_NO = 9, RT_TM = 64;
// part f32 [gridDim.x][RT_NO*128 + 128 + 16]: dW3 (row-major [9][128]), db2 [128], db3 [9 (+7 pad)]
__global__ __launch_bounds__(256) void rel_tail_bwd_kernel(const float *__restrict__ dpred, const float *__restrict__ W3,
                                                           const float *__restrict__ hid2, long R, float *__restrict__ dz2,
                                                           float *__restrict__ part) {
  constexpr int C = 128, PW = RT_NO * C + C + 16;
  __shared__ __attribute__((aligned(16))) float s_dp[RT_TM * RT_NO];
  __shared__ float s_red[8 * 32 * 41];
  const int tid = threadIdx.x, c4 = tid & 31, r0 = tid >> 5;
  float w3[RT_NO][4], aw[RT_NO][4], ab2[4] = {0.f, 0.f, 0.f, 0.f}, ab3[RT_NO];
#pragma unroll
  for (int o = 0; o < RT_NO; ++o) {
    ab3[o] = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) w3[o][u] = W3[o * C + c4 * 4 + u], aw[o][u] = 0.f;
  }
  const long ntiles = (R + RT_TM - 1) / RT_TM;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long row0 = t * RT_TM;
    __syncthreads();
    for (int i = tid; i < RT_TM * RT_NO; i += 256) s_dp[i] = (row0 * RT_NO + i < R * RT_NO) ? dpred[row0 * RT_NO + i] : 0.f;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RT_TM / 8; ++i) {
      const int row = r0 + 8 * i;
      if (row0 + row >= R) continue;
      const f32x4 h = ld4(hid2 + (size_t)(row0 + row) * C + c4 * 4);
      float d[RT_NO];
#pragma unroll
      for (int o = 0; o < RT_NO; ++o) d[o] = s_dp[row * RT_NO + o];
      f32x4 dz = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int o = 0; o < RT_NO; ++o)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          dz[u] = fmaf(d[o], w3[o][u], dz[u]);
          aw[o][u] = fmaf(d[o], h[u], aw[o][u]);
        }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        dz[u] = h[u] > 0.f ? dz[u] : 0.f;
        ab2[u] += dz[u];
      }
      st4(dz2 + (size_t)(row0 + row) * C + c4 * 4, dz);
      if (c4 == 0) {
#pragma unroll
        for (int o = 0; o < RT_NO; ++o) ab3[o] += d[o];
      }
    }
  }
  // the 8 row groups of a column quad, added in a fixed order
  __syncthreads();
  float *mine = &s_red[(r0 * 32 + c4) * 41];
#pragma unroll
  for (int o = 0; o < RT_NO; ++o)
#pragma unroll
    for (int u = 0; u < 4; ++u) mine[o * 4 + u] = aw[o][u];
#pragma unroll
  for (int u = 0; u < 4; ++u) mine[36 + u] = ab2[u];
  __syncthreads();
  float *o_part = part + (size_t)blockIdx.x * PW;
  for (int i = tid; i < 32 * 40; i += 256) {
    const int q = i / 40, e = i % 40;
    float a = 0.f;
#pragma unroll
    for (int g = 0; g < 8; ++g) a += s_red[(g * 32 + q) * 41 + e];
    if (e < 36) o_part[(e >> 2) * C + q * 4 + (e & 3)] = a;
    else o_part[RT_NO * C + q * 4 + (e - 36)] = a;
  }
  __syncthreads();
  if (c4 == 0) {
#pragma unroll
    for (int o = 0; o < RT_NO; ++o) s_red[r0 * 16 + o] = ab3[o];
  }
  __syncthreads();
  if (tid < 16) {
    float a = 0.f;
    if (tid < RT_NO)
#pragma unroll
      for (int g = 0; g < 8; ++g) a += s_red[g * 16 + tid];
    o_part[RT_NO * C + C + tid] = a;
  }
}
}  // namespace

// number of partial rows the backward writes (each 9*128 + 128 + 16 floats)
extern "C" int spacap_rel_tail_bwd_nparts(long R) {
  const long tiles = (R + RT_TM - 1) / RT_TM;
  return (int)(tiles < 1024 ? (tiles < 1 ? 1 : tiles) : 1024);
}

// dpred f32 [R,9], W3 f32 [9,128], hid2 f32 [R,128] -> dz2 f32 [R,128], part f32 [nparts][9*128 + 128 + 16]
extern "C" int spacap_rel_tail_bwd_f32(const float *dpred, const float *W3, const float *hid2, long R, float *dz2, float *part,
                                       spacap_stream_t stream) {
  const char *what = "spacap_rel_tail_bwd_f32";
  SPACAP_REQUIRE(dpred && W3 && hid2 && dz2 && part && R >= 1, "%s: bad arguments", what);
  hipLaunchKernelGGL(rel_tail_bwd_kernel, dim3(spacap_rel_tail_bwd_nparts(R)), dim3(256), 0, spacap::as_stream(stream), dpred, W3,
                     hid2, R, dz2, part);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
