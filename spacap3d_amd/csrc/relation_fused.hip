// The relation head of the spatiality-guided encoder end to end on chip, forward and backward, for gfx950 (MI355X).
//
// Reference: models/transformer_captioner.py:319-326 (relation_proposal = Linear(128,128)-ReLU-Linear(128,128)-ReLU-Linear(128,9))
// and :392-397 (relation feature R[b,i,j,h*16+d] = P[b,h,i,j] V[b,h,j,d] of the last encoder layer, then the MLP on all B*K*K
// proposal pairs).  With U[b,j,h,:] = V[b,h,j,:] W1[:, 16h:16h+16]^T (a tiny product done by the caller, csrc/relation.hip):
//     hid1[b,i,j,:] = relu(b1 + sum_h P[b,h,i,j] U[b,j,h,:])      hid2 = relu(hid1 W2^T + b2)      pred = hid2 W3^T + b3
// As separate operators the head moves hid1 (268 MB at B = 8, K = 256) five times and the equally large dz2 / dhid1 twice
// each: 2.9 GB of HBM traffic around 51 GFLOP.  Here a workgroup owns 8 key columns j of one scene (U[b, j-block] stays in
// registers for the whole launch) and walks the queries in blocks of 8: one tile = 8 x 8 = 64 pair rows.
//   forward   hid1 tile -> LDS -> layer 2 (weights in registers) -> + b2, ReLU -> hid2 (stored: the backward's only large
//             input) -> layer 3 (9 outputs) from the same registers -> pred.
//   backward  hid1 tile recomputed from P, U; dz2 = (dpred W3) * [hid2 > 0] -> LDS; dW3 += dpred^T hid2; dW2 += dz2^T hid1;
//             dhid1 = dz2 W2; dz1 = dhid1 * [hid1 > 0]; then layer 1's gradients from the tile: dP[b,h,i,j] =
//             dz1 . U[b,j,h,:] (stored), dU[b,j,h,:] += P dz1 (registers, written once at the end); the bias sums ride the
//             same products as a column of ones; all parameter sums leave as per-workgroup partials (fixed order, no atomics).
//   backward over the selected pairs (spacap_relation_fused_bwd_sel_f32): dpred is zero unless both proposals of a pair are
//             selected by the relation loss; the active query rows and key columns are found from dpred, compacted into lists
//             and the same tile body runs over (8 list rows) x (8 list columns): n_sel^2 work instead of K^2.
// Every product, the small per-key ones included (block-diagonal operands, two key columns per 16-row tile), runs on the
// matrix cores: the backward has one wave per SIMD, so VALU phases would leave the matrix pipe idle.
// Arithmetic: the three 128 x 128 products (layer 2, dhid1, dW2: 94 % of the flops) as split-bf16, three bf16 pieces per
// operand and the six piece products above 2^-24 on v_mfma_f32_16x16x32_bf16 (fp32-equivalent, 6/16 of the fp32-MFMA time);
// the operands are split once by their producer and live in LDS as bf16 images, row-major where the contraction runs over
// channels and channel-major (the producing MFMA issued with its operands swapped) where it runs over the rows.  The small
// products use v_mfma_f32_16x16x4_f32 (exact fp32).  H = 8 heads, 128 channels, 9 outputs, K a multiple of 8.
#include <stdlib.h>
#include <atomic>

#include "common.hpp"
#include "launch.hpp"
#include "mfma.hpp"

namespace {

using namespace spacap::mfma;

constexpr int H = 8, C = 128, NO = 9, LDT = C + 8, TI = 8, TJ = 8, TR = TI * TJ;   // 64 pair rows per tile
constexpr int DPL = 12;                      // row stride of 9-wide tiles in LDS (9 values + 3 zeros: three k steps of 4)
constexpr int LDB = C + 8, IMG = TR * LDB;   // row-major bf16 piece [64 rows][128 + 8]: 272-byte rows, 16-byte reads conflict free
constexpr int LDR = TR + 8, IMGT = C * LDR;  // channel-major bf16 piece [128 channels][64 + 8]: 144-byte rows
constexpr int PART = C * C + NO * C + C + C + 16;   // per-workgroup partial: dW2 | dW3 | db1 | db2 | db3 (padded)

__device__ __forceinline__ f32x4 relu4(f32x4 v) { return f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)}; }

// Tile rows are ordered key-major: row rr = jj * 8 + ii is the pair (query i0 + ii, key j0 + jj), so a 16-row matrix-core tile
// holds the 8 queries of two key columns and wave w owns the key columns 2 w, 2 w + 1 in every per-key product.
__device__ __forceinline__ size_t pair_row(int b, int K, int i0, int j0, int rr) { return ((size_t)b * K + i0 + (rr & 7)) * K + j0 + (rr >> 3); }

// ---- split-bf16 operands: x = x0 + x1 + x2 (three bf16 pieces, 24 mantissa bits), a product = the six piece products whose
// weight is above 2^-24, each exact in the fp32 accumulator of v_mfma_f32_16x16x32_bf16: 6/16 of the fp32-MFMA time ----------
// (split4, split8, mfma6: mfma.hpp)
__device__ __forceinline__ void st_pieces(__bf16 *dst, int piece_stride, f32x4 v) {   // 3 x 8 bytes
  bf16x4 p0, p1, p2;
  split4(v, p0, p1, p2);
  *reinterpret_cast<bf16x4 *>(dst) = p0;
  *reinterpret_cast<bf16x4 *>(dst + piece_stride) = p1;
  *reinterpret_cast<bf16x4 *>(dst + 2 * piece_stride) = p2;
}
__device__ __forceinline__ void ld_pieces(const __bf16 *src, int piece_stride, bf16x8 *p) {   // 3 x 16 bytes
#pragma unroll
  for (int q = 0; q < 3; ++q) p[q] = *reinterpret_cast<const bf16x8 *>(src + q * piece_stride);
}

// the attention values of the next tile, two per thread (key index fastest in memory), stored as s_p[h][jj * 8 + ii]
__device__ __forceinline__ void p_tile_request(const float *__restrict__ P, int b, int K, int i0, int j0, float *pp) {
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int idx = threadIdx.x + 256 * e, h = idx >> 6, ii = (idx >> 3) & 7, jj = idx & 7;
    pp[e] = P[(((size_t)b * H + h) * K + i0 + ii) * K + j0 + jj];
  }
}
// the same for a thread that knows its query row and key column (the selected backward: rows and columns come from lists)
__device__ __forceinline__ void p_tile_request_at(const float *__restrict__ P, int b, int K, int qrow, int kcol, float *pp) {
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int h = (threadIdx.x + 256 * e) >> 6;
    pp[e] = P[(((size_t)b * H + h) * K + qrow) * K + kcol];
  }
}
__device__ __forceinline__ void p_tile_store(const float *pp, float *s_p) {
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int idx = threadIdx.x + 256 * e, h = idx >> 6, ii = (idx >> 3) & 7, jj = idx & 7;
    s_p[h * TR + jj * TI + ii] = pp[e];
  }
}

// hid1 rows 16 w .. 16 w + 15 = relu(b1 + sum_h P U) on the matrix cores (exact fp32 products): contraction index k = (key
// column of the pair, head) with the attention operand block diagonal (zero where the row's key column is not k's) and the
// bias as a fifth k step.  uA[n][ks] = U[b, j0 + 2 w + (ks >> 1), 4 (ks & 1) + lg, 16 n + l15], bA[n] = lg == 0 ? b1[16 n + l15] : 0.
// TRANSPOSED = false: the lane gets 4 channels of row l15 -> row-major bf16 pieces [64][LDB]; true: 4 rows of channel l15 ->
// channel-major pieces [128][LDR].
template <bool TRANSPOSED>
__device__ __forceinline__ void hid1_rows(const float (*uA)[4], const float *bA, const float *s_p, int w, int l15, int lg, __bf16 *img) {
  const float p0 = s_p[lg * TR + 16 * w + l15], p1 = s_p[(4 + lg) * TR + 16 * w + l15];
  const bool hi = l15 >> 3;
  const float pB[4] = {hi ? 0.f : p0, hi ? 0.f : p1, hi ? p0 : 0.f, hi ? p1 : 0.f};
  const float one = lg == 0 ? 1.f : 0.f;
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (TRANSPOSED) {
      acc = MFMA16(one, bA[n], acc);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) acc = MFMA16(pB[ks], uA[n][ks], acc);
      st_pieces(img + (16 * n + l15) * LDR + 16 * w + 4 * lg, IMGT, relu4(acc));
    } else {
      acc = MFMA16(bA[n], one, acc);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) acc = MFMA16(uA[n][ks], pB[ks], acc);
      st_pieces(img + (16 * w + l15) * LDB + 16 * n + 4 * lg, IMG, relu4(acc));
    }
  }
}

__global__ __launch_bounds__(256) void rel_fused_fwd_kernel(const float *__restrict__ P, const float *__restrict__ Um,
                                                            const float *__restrict__ b1, const float *__restrict__ W2,
                                                            const float *__restrict__ b2, const float *__restrict__ W3,
                                                            const float *__restrict__ b3, int B, int K, float *__restrict__ hid2,
                                                            float *__restrict__ pred) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __bf16 *s_a = reinterpret_cast<__bf16 *>(smem_raw);                       // hid1 pieces [3][64][LDB]
  float *s_pr = reinterpret_cast<float *>(smem_raw + 3 * IMG * 2);          // layer 3 partial sums [4 waves][64][DPL]
  float *s_p = s_pr + 4 * TR * DPL;                                         // [8][64]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  // this workgroup's contiguous range of tile units (unit = (scene, key block, query block), query block fastest)
  const int NI = K / TI, NJ = K / TJ;
  const long U = (long)B * NJ * NI, u_beg = (long)blockIdx.x * U / gridDim.x, u_end = ((long)blockIdx.x + 1) * U / gridDim.x;
  // layer 2 weights of the wave's 32 output channels as pieces: wA[t][kc] = W2[32 w + 16 t + l15][32 kc + 8 lg .. + 7]
  bf16x8 wA[2][4][3];
  float w3r[2][4];
  f32x4 bb[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float *wp = W2 + (size_t)(32 * w + 16 * t + l15) * C + 8 * lg;
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) split8(ld4(wp + 32 * kc), ld4(wp + 32 * kc + 4), wA[t][kc]);
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) w3r[t][uu] = l15 < NO ? W3[l15 * C + 32 * w + 16 * t + 4 * lg + uu] : 0.f;
    bb[t] = ld4(b2 + 32 * w + 16 * t + 4 * lg);
  }
  float pp[2];
  for (long u = u_beg; u < u_end;) {
    const int grp = (int)(u / NI), ib0 = (int)(u - (long)grp * NI), ibe = (int)min((long)NI, ib0 + (u_end - u));
    const int b = grp / NJ, j0 = (grp - b * NJ) * TJ, ibeg = ib0 * TI, iend = ibe * TI;
    u += ibe - ib0;
    float uA[8][4], bA[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) uA[n][ks] = Um[(((size_t)b * K + j0 + 2 * w + (ks >> 1)) * H + 4 * (ks & 1) + lg) * C + 16 * n + l15];
      bA[n] = lg == 0 ? b1[16 * n + l15] : 0.f;
    }
    p_tile_request(P, b, K, ibeg, j0, pp);
    auto pred_out = [&](int i0) {   // the four waves' layer 3 partial sums + b3 -> pred, 8 runs (one per query) of 72 floats
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const int idx = tid + 256 * e, ii = idx / (TJ * NO), off = idx - ii * (TJ * NO), j = off / NO, o = off - j * NO;
        if (idx < TR * NO) {
          const float *q = s_pr + (j * TI + ii) * DPL + o;
          pred[(((size_t)b * K + i0 + ii) * K + j0) * NO + off] = ((q[0] + q[TR * DPL]) + (q[2 * TR * DPL] + q[3 * TR * DPL])) + b3[o];
        }
      }
    };

    for (int i0 = ibeg; i0 < iend; i0 += TI) {
      __syncthreads();   // the previous tile's readers of s_p / s_a and writers of s_pr are done
      p_tile_store(pp, s_p);
      if (i0 > ibeg) pred_out(i0 - TI);
      if (i0 + TI < iend) p_tile_request(P, b, K, i0 + TI, j0, pp);
      __syncthreads();
      hid1_rows<false>(uA, bA, s_p, w, l15, lg, s_a);
      __syncthreads();
#pragma unroll 2
      for (int mt = 0; mt < TR / 16; ++mt) {
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
          bf16x8 a[3];
          ld_pieces(s_a + (mt * 16 + l15) * LDB + 32 * kc + 8 * lg, IMG, a);
          acc[0] = mfma6(wA[0][kc], a, acc[0]);
          acc[1] = mfma6(wA[1][kc], a, acc[1]);
        }
        const int rr = mt * 16 + l15;
        float *hrow = hid2 + pair_row(b, K, i0, j0, rr) * C + 32 * w + 4 * lg;
        f32x4 a3 = {0.f, 0.f, 0.f, 0.f}, a3b = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const f32x4 h = relu4(acc[t] + bb[t]);
          st4(hrow + 16 * t, h);
          // layer 3 straight from the registers: k = the wave's channel 32 w + 16 t + 4 lg + uu
          a3 = MFMA16(w3r[t][0], h[0], a3);
          a3b = MFMA16(w3r[t][1], h[1], a3b);
          a3 = MFMA16(w3r[t][2], h[2], a3);
          a3b = MFMA16(w3r[t][3], h[3], a3b);
        }
        if (lg < 3) st4(&s_pr[(w * TR + rr) * DPL + 4 * lg], a3 + a3b);
      }
    }
    __syncthreads();
    pred_out(iend - TI);
  }
}

// ---- the selected backward's workspace (int32 words; include/spacap_hip.h documents it): per-scene counts, the compacted
// lists, the flags they are made from ------------------------------------------------------------------------------------
__host__ __device__ inline size_t sel_cnt_off(int, int) { return 0; }                                        // [B][4]
__host__ __device__ inline size_t sel_qi_off(int B, int) { return (size_t)4 * B; }                           // [B][K]
__host__ __device__ inline size_t sel_kj_off(int B, int K) { return (size_t)4 * B + (size_t)B * K; }         // [B][K]
__host__ __device__ inline size_t sel_rowflag_off(int B, int K) { return (size_t)4 * B + (size_t)2 * B * K; }   // [B][K]
__host__ __device__ inline size_t sel_colflag_off(int B, int K) { return (size_t)4 * B + (size_t)3 * B * K; }   // [B][K]
__host__ __device__ inline size_t sel_colbits_off(int B, int K) { return (size_t)4 * B + (size_t)4 * B * K; }   // 64-bit [B][K][NW]
__host__ __device__ inline int sel_nw(int K) { return (K + 63) >> 6; }
// per scene {active row blocks, active column blocks, row-block flags [K/8], column-block flags [K/8]}: 8-aligned blocks of
// proposals that hold an active one (the tiles of the dense kernel that can be non-zero)
__host__ __device__ inline size_t sel_blk_off(int B, int K) { return sel_colbits_off(B, K) + (size_t)2 * B * K * sel_nw(K); }
__host__ __device__ inline int sel_blk_stride(int K) { return 2 + 2 * (K / 8); }
__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

// The backward of one workgroup.  SEL = false: all B K K pairs, a static partition of the (scene, key block, query block) units.
// SEL = true, one of two walks, chosen from the counts in the workspace `ws` (rel_sel_scan_kernel, rel_sel_compact_kernel below):
//   in place    the tiles, partition and dU slots of SEL = false, but only tiles whose query block and key block hold an active
//               proposal are visited.  A tile without an active pair adds exact zeros to every sum, so the results are the
//               bits of SEL = false.  Taken while it costs no more tiles than the lists (everything active) or at most 1/16
//               of all tiles (a handful of selected proposals per scene).
//   over lists  the units are (8 entries of the scene's query list) x (8 entries of its key list); rows of P, hid2, dpred, U
//               and of dP, dU are addressed through the lists: n_sel^2 work where most 8-blocks hold a selected proposal.
//               Workgroup g takes the units [g L, (g + 1) L), L = max(ceil(NU / G), ceil(NI_max / (Z - 1))): a key block
//               (at most NI_max units) then meets at most Z workgroups.  Same products per pair, another summation order.
// dP and dU outside the visited tiles are the caller's zeros (the scan kernel writes them).
template <bool SEL>
__device__ __forceinline__ void rel_bwd_body(const float *__restrict__ dpred, const float *__restrict__ hid2,
                                             const float *__restrict__ P, const float *__restrict__ U,
                                             const float *__restrict__ b1, const float *__restrict__ W2,
                                             const float *__restrict__ W3, int B, int K, int Z, const int *__restrict__ ws,
                                             float *__restrict__ dP, float *__restrict__ dU, float *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __bf16 *s_h1T = reinterpret_cast<__bf16 *>(smem_raw);                  // hid1 pieces, channel-major [3][128][LDR]
  __bf16 *s_zT = s_h1T + 3 * IMGT;                                       // dz2 pieces, channel-major; the same bytes later
  __bf16 *s_z = s_zT;                                                    //   hold them row-major [3][64][LDB]
  float *s_x = reinterpret_cast<float *>(smem_raw + 2 * 3 * IMGT * 2);   // [64][LDT]: the hid2 tile, then dz1
  float *s_p = s_x + TR * LDT, *s_dp = s_p + H * TR;                     // [8][64], [64][DPL]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int jj = tid >> 5, c4 = tid & 31;
  // this workgroup's contiguous range of tile units (unit = (scene, key block, query block), query block fastest)
  const int NI = K / TI, NJ = K / TJ;
  long NU = (long)B * NJ * NI, u_beg = (long)blockIdx.x * NU / gridDim.x, u_end = ((long)blockIdx.x + 1) * NU / gridDim.x;
  long L = 0;          // SEL, not all active: the length of every workgroup's range
  bool dense = true;   // the static partition above holds
  const int *cnt = SEL ? ws + sel_cnt_off(B, K) : nullptr, *blk = SEL ? ws + sel_blk_off(B, K) : nullptr;
  const int BS = sel_blk_stride(K);
  if (SEL) {
    // units, the longest query list and "everything active" over the scenes; every count clamped to what the lists can hold
    long long nu = 0, tb = 0;   // tiles over the compacted lists; tiles of the dense kernel that hold an active pair
    int nim = 0;
    for (int s = tid; s < B; s += 256) {
      const int ni = clampi(cnt[4 * s + 2], NI), nj = clampi(cnt[4 * s + 3], NJ);
      nu += (long long)ni * nj;
      nim = max(nim, ni);
      tb += (long long)clampi(blk[(size_t)s * BS], NI) * clampi(blk[(size_t)s * BS + 1], NJ);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      nu += __shfl_xor(nu, m);
      tb += __shfl_xor(tb, m);
      nim = max(nim, __shfl_xor(nim, m));
    }
    long long *s_nu = reinterpret_cast<long long *>(s_x);
    int *s_ni = reinterpret_cast<int *>(s_nu + 8);
    if (lane == 0) s_nu[w] = nu, s_nu[4 + w] = tb, s_ni[w] = nim;
    __syncthreads();
    nu = (s_nu[0] + s_nu[1]) + (s_nu[2] + s_nu[3]);
    tb = (s_nu[4] + s_nu[5]) + (s_nu[6] + s_nu[7]);
    nim = max(max(s_ni[0], s_ni[1]), max(s_ni[2], s_ni[3]));
    // In place (the dense kernel's tiles, partition and slots, inactive tiles skipped: the dense kernel's bits, since a tile
    // without an active pair adds exact zeros) while that costs no more tiles than the lists (everything active) or at most
    // 1/16 of the dense kernel; over the lists (fewer tiles, other summation order) beyond that.
    dense = tb <= nu || tb * 16 <= NU;
    if (!dense) {
      NU = nu;
      L = max((NU + gridDim.x - 1) / gridDim.x, (long)(nim + max(Z - 1, 1) - 1) / max(Z - 1, 1));
      u_beg = min(NU, (long)blockIdx.x * L);
      u_end = min(NU, ((long)blockIdx.x + 1) * L);
    }
    if (u_beg >= u_end) {   // nothing selected in this range: zero partial sums
      float *po = part + (size_t)blockIdx.x * PART;
      for (int idx = tid; idx < PART; idx += 256) po[idx] = 0.f;
      return;
    }
  }
  // ---- operands that stay in registers for the whole launch ------------------------------------------------------------
  float bA[8], w3A[8][3];
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    bA[n] = lg == 0 ? b1[16 * n + l15] : 0.f;
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) w3A[n][ks] = 4 * ks + lg < NO ? W3[(4 * ks + lg) * C + 16 * n + l15] : 0.f;
  }
  // dhid1 = dz2 W2 for the wave's 32 INPUT channels: wA[t][kc] = W2[32 kc + 8 lg .. + 7][32 w + 16 t + l15] as pieces
  bf16x8 wA[2][4][3];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      const float *wp = W2 + (size_t)(32 * kc + 8 * lg) * C + 32 * w + 16 * t + l15;
      split8(f32x4{wp[0], wp[C], wp[2 * C], wp[3 * C]}, f32x4{wp[4 * C], wp[5 * C], wp[6 * C], wp[7 * C]}, wA[t][kc]);
    }
  const bf16x8 ones = {(__bf16)1.f, (__bf16)1.f, (__bf16)1.f, (__bf16)1.f, (__bf16)1.f, (__bf16)1.f, (__bf16)1.f, (__bf16)1.f};
  // ---- running sums ----------------------------------------------------------------------------------------------------
  f32x4 gw[2][8], gb2[2], g3[2], d1[2], gb3 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    gb2[t] = g3[t] = d1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < 8; ++n) gw[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int idx = tid; idx < TR * DPL; idx += 256) s_dp[idx] = 0.f;   // (the three pad columns stay zero)

  // ---- the next tile's inputs travel while the current one is worked on -------------------------------------------------
  f32x4 hp[TI];
  float pp[2], dq[3];
  int sc = 0, NIs = SEL ? clampi(cnt[2], NI) : NI, NJs = SEL ? clampi(cnt[3], NJ) : NJ;   // SEL: the scene of unit u,
  long sbeg = 0;                                                                           //   its first unit
  for (long u = u_beg; u < u_end;) {
  // ---- one key block (8 key columns of one scene): the stretch of its query blocks that falls into this workgroup's range --
  int b, j0, ib0, ibe;
  long kstart;   // the key block's first unit
  if (SEL && !dense) {
    while (sc + 1 < B && u >= sbeg + (long)NIs * NJs) {   // (scenes with nothing selected hold no units)
      sbeg += (long)NIs * NJs;
      ++sc;
      NIs = clampi(cnt[4 * sc + 2], NI), NJs = clampi(cnt[4 * sc + 3], NJ);
    }
    const long v = u - sbeg;
    const int jb = (int)(v / NIs);
    ib0 = (int)(v - (long)jb * NIs), ibe = (int)min((long)NIs, ib0 + (u_end - u));
    b = sc, j0 = jb * TJ, kstart = sbeg + (long)jb * NIs;
  } else {
    const int grp = (int)(u / NI);
    ib0 = (int)(u - (long)grp * NI), ibe = (int)min((long)NI, ib0 + (u_end - u));
    b = grp / NJ, j0 = (grp - b * NJ) * TJ, kstart = (long)grp * NI;
  }
  u += ibe - ib0;
  // SEL in place: only the tiles whose query block and key block hold an active proposal
  const int *rfl = SEL ? blk + (size_t)b * BS + 2 : nullptr;
  auto next_tile = [&](int ib) -> int {
    if (SEL && dense)
      while (ib < ibe && !rfl[ib]) ++ib;
    return ib;
  };
  if (SEL && dense && !rfl[NI + (j0 >> 3)]) continue;
  int ib = next_tile(ib0);
  if (ib >= ibe) continue;   // (dU of an unvisited stretch: the scan kernel's zeros)
  int ibn = next_tile(ib + 1), ibn2 = ibn < ibe ? next_tile(ibn + 1) : ibe;
  // SEL: i0, j0 count list entries; rows_of / KJ give the proposal behind an entry (clamped: no address leaves the scene)
  const int *ql = SEL ? ws + sel_qi_off(B, K) + (size_t)b * K : nullptr, *kl = SEL ? ws + sel_kj_off(B, K) + (size_t)b * K : nullptr;
  auto KJ = [&](int x) -> int { return SEL && !dense ? clampi(kl[j0 + x], K - 1) : j0 + x; };
  const int kP = KJ(tid & 7), kH = KJ(jj), kU[2] = {KJ(2 * w), KJ(2 * w + 1)}, kR = KJ(2 * w + (l15 >> 3)), kZ = KJ(2 * w + (lg >> 1));
  int kD[3], iD[3], oD[3];   // the thread's three dpred elements of a tile: key column, query entry, output
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int idx = tid + 256 * e, ii = idx / (TJ * NO), off = idx - ii * (TJ * NO), j = off / NO;
    iD[e] = ii, oD[e] = off - j * NO, kD[e] = idx < TR * NO ? KJ(j) : 0;
  }
  float uA[8][4];
  f32x4 uP[8], du[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) uA[n][ks] = U[(((size_t)b * K + kU[ks >> 1]) * H + 4 * (ks & 1) + lg) * C + 16 * n + l15];
    // dP: row (key column l15 >> 3, head l15 & 7) of U, contraction over the channels
    uP[n] = ld4(U + (((size_t)b * K + kR) * H + (l15 & 7)) * C + 16 * n + 4 * lg);
    du[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // SEL: the proposals behind the 8 query entries of a tile, entry (lane & 7) in every lane: read from the list one tile before
  // the loads that use them are issued, so that no load waits for an index; a lane fetches its rows from its wave's lanes 0 .. 7
  int ha = 0, hb = 0;   // the tile in flight, the tile after it
  auto rows_of = [&](int i0) -> int { return !SEL ? 0 : dense ? i0 + (lane & 7) : clampi(ql[i0 + (lane & 7)], K - 1); };
  auto row = [&](int i0, int h, int x) -> int { return SEL ? __shfl(h, x & 7) : i0 + x; };
  auto request = [&](int i0, int h) {
    p_tile_request_at(P, b, K, row(i0, h, (tid >> 3) & 7), kP, pp);
    int rD[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) rD[e] = row(i0, h, iD[e]);
#pragma unroll
    for (int e = 0; e < 3; ++e)   // dpred rows of the tile: 8 runs (one per query) of 72 contiguous floats
      dq[e] = tid + 256 * e < TR * NO ? dpred[(((size_t)b * K + rD[e]) * K + kD[e]) * NO + oD[e]] : 0.f;
#pragma unroll
    for (int ii = 0; ii < TI; ++ii) {
      const int r = SEL ? __builtin_amdgcn_readlane(h, ii) : i0 + ii;
      hp[ii] = ld4(hid2 + (((size_t)b * K + r) * K + kH) * C + 4 * c4);
    }
  };
  ha = rows_of(ib * TI);
  if (ibn < ibe) hb = rows_of(ibn * TI);
  request(ib * TI, ha);

  for (; ib < ibe; ib = ibn, ibn = ibn2, ibn2 = ibn < ibe ? next_tile(ibn + 1) : ibe) {
    const int i0 = ib * TI;
    __syncthreads();   // the previous tile's readers of every LDS buffer are done
    const int qR = row(i0, ha, l15 & 7);   // the query row of this lane's dP results
    p_tile_store(pp, s_p);
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const int idx = tid + 256 * e, ii = idx / (TJ * NO), off = idx - ii * (TJ * NO), j = off / NO, o = off - j * NO;
      if (idx < TR * NO) s_dp[(j * TI + ii) * DPL + o] = dq[e];
    }
#pragma unroll
    for (int ii = 0; ii < TI; ++ii) st4(&s_x[(jj * TI + ii) * LDT + 4 * c4], hp[ii]);
    if (ibn < ibe) {
      ha = hb;
      request(ibn * TI, ha);
      if (ibn2 < ibe) hb = rows_of(ibn2 * TI);
    }
    __syncthreads();
    float dB[3];   // dpred of row 16 w + l15, three k steps of 4 outputs (either operand side: same lane structure)
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) dB[ks] = s_dp[(16 * w + l15) * DPL + 4 * ks + lg];
    hid1_rows<true>(uA, bA, s_p, w, l15, lg, s_h1T);
    {
      // dz2 = (dpred W3) * [hid2 > 0] of the wave's 16 rows, the lane holding 4 ROWS of channel 16 n + l15 -> channel-major pieces
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) acc = MFMA16(dB[ks], w3A[n][ks], acc);
        const float *hx = s_x + (16 * w + 4 * lg) * LDT + 16 * n + l15;
#pragma unroll
        for (int uu = 0; uu < 4; ++uu) acc[uu] = hx[uu * LDT] > 0.f ? acc[uu] : 0.f;
        st_pieces(s_zT + (16 * n + l15) * LDR + 16 * w + 4 * lg, IMGT, acc);
      }
      // dW3[o][c] += dpred^T hid2 for the channels 32 w .. 32 w + 31, db3 (wave 0) with a column of ones
#pragma unroll 4
      for (int ks = 0; ks < TR / 4; ++ks) {
        const float a = l15 < NO ? s_dp[(4 * ks + lg) * DPL + l15] : 0.f;
        const float *hr = s_x + (4 * ks + lg) * LDT + 32 * w + l15;
        g3[0] = MFMA16(a, hr[0], g3[0]);
        g3[1] = MFMA16(a, hr[16], g3[1]);
        if (w == 0) gb3 = MFMA16(a, 1.f, gb3);
      }
    }
    __syncthreads();   // both channel-major images complete
#pragma unroll 1
    for (int kc = 0; kc < TR / 32; ++kc) {   // dW2 += dz2^T hid1 (contraction over the 64 rows), db2 with a column of ones
      bf16x8 za[2][3];
      ld_pieces(s_zT + (32 * w + l15) * LDR + 32 * kc + 8 * lg, IMGT, za[0]);
      ld_pieces(s_zT + (32 * w + 16 + l15) * LDR + 32 * kc + 8 * lg, IMGT, za[1]);
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        bf16x8 hb[3];
        ld_pieces(s_h1T + (16 * n + l15) * LDR + 32 * kc + 8 * lg, IMGT, hb);
        gw[0][n] = mfma6(za[0], hb, gw[0][n]);
        gw[1][n] = mfma6(za[1], hb, gw[1][n]);
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 2; q >= 0; --q) gb2[t] = MFMA_B(za[t][q], ones, gb2[t]);
    }
    __syncthreads();   // the channel-major dz2 image is consumed: its bytes take the row-major one
    {
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) acc = MFMA16(w3A[n][ks], dB[ks], acc);
        const f32x4 h2 = ld4(&s_x[(16 * w + l15) * LDT + 16 * n + 4 * lg]);
#pragma unroll
        for (int uu = 0; uu < 4; ++uu) acc[uu] = h2[uu] > 0.f ? acc[uu] : 0.f;
        st_pieces(s_z + (16 * w + l15) * LDB + 16 * n + 4 * lg, IMG, acc);
      }
    }
    __syncthreads();   // row-major dz2 complete; hid2 (s_x) consumed
#pragma unroll 1
    for (int mt = 0; mt < TR / 16; ++mt) {   // dhid1 = dz2 W2, masked by hid1 > 0 -> dz1 (s_x), db1
      f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        bf16x8 z[3];
        ld_pieces(s_z + (mt * 16 + l15) * LDB + 32 * kc + 8 * lg, IMG, z);
        acc[0] = mfma6(wA[0][kc], z, acc[0]);
        acc[1] = mfma6(wA[1][kc], z, acc[1]);
      }
      const int rr = mt * 16 + l15;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        // hid1 > 0 <=> its leading piece is not zero (ReLU output; bf16 keeps the fp32 exponent range)
        const unsigned short *hb = reinterpret_cast<const unsigned short *>(s_h1T) + (32 * w + 16 * t + 4 * lg) * LDR + rr;
#pragma unroll
        for (int uu = 0; uu < 4; ++uu) acc[t][uu] = (hb[uu * LDR] & 0x7fff) ? acc[t][uu] : 0.f;
        d1[t] += acc[t];
        st4(&s_x[rr * LDT + 32 * w + 16 * t + 4 * lg], acc[t]);
      }
    }
    __syncthreads();   // dz1 complete
    {
      // dP[h, i, j] = dz1[(i, j), :] . U[j, h, :] for the wave's two key columns: result row (key column, head), valid where
      // the row's key column is the pair's
      f32x4 acc = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const f32x4 a = ld4(&s_x[(16 * w + l15) * LDT + 16 * q + 4 * lg]);
        acc = MFMA16(uP[q][0], a[0], acc);
        accb = MFMA16(uP[q][1], a[1], accb);
        acc = MFMA16(uP[q][2], a[2], acc);
        accb = MFMA16(uP[q][3], a[3], accb);
      }
      acc += accb;
      if ((lg >> 1) == (l15 >> 3)) {
        float *o = dP + (((size_t)b * H + 4 * (lg & 1)) * K + qR) * K + kR;
#pragma unroll
        for (int uu = 0; uu < 4; ++uu) o[(size_t)uu * K * K] = acc[uu];
      }
      // dU[j, h, c] += sum_i P[h, i, j] dz1[(i, j), c]: block-diagonal attention operand again, now on the row side
      const float q0 = s_p[(l15 & 7) * TR + 16 * w + (l15 >> 3) * TI + lg], q1 = s_p[(l15 & 7) * TR + 16 * w + (l15 >> 3) * TI + 4 + lg];
      const bool hi = l15 >> 3;
      const float pA[4] = {hi ? 0.f : q0, hi ? 0.f : q1, hi ? q0 : 0.f, hi ? q1 : 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const float *zr = s_x + (16 * w + 4 * ks + lg) * LDT + l15;
#pragma unroll
        for (int n = 0; n < 8; ++n) du[n] = MFMA16(pA[ks], zr[16 * n], du[n]);
      }
    }
  }
  {   // this stretch's share of dU: du[n][uu] = dU[key column 2 w + (lg >> 1), head 4 (lg & 1) + uu, channel 16 n + l15].
      // Slot = position of this workgroup among those that share the key block; the one that ends it clears the unused slots.
    const long first = (kstart + 1) * gridDim.x;
    const int slot = (int)(blockIdx.x - (SEL && !dense ? kstart / L : (first + NU - 1) / NU - 1));
    const size_t slab = (size_t)B * K * H * C;
    float *duo = dU + (size_t)slot * slab + (((size_t)b * K + kZ) * H + 4 * (lg & 1)) * C + l15;
    if (!SEL || slot < Z) {   // (SEL: the host sized Z by the rule of the partition; the test keeps a store inside dU regardless)
#pragma unroll
      for (int n = 0; n < 8; ++n)
#pragma unroll
        for (int uu = 0; uu < 4; ++uu) duo[uu * C + 16 * n] = du[n][uu];
    }
    if (!SEL && ibe == NI)
      for (int z = slot + 1; z < Z; ++z)
#pragma unroll
        for (int n = 0; n < 8; ++n)
#pragma unroll
          for (int uu = 0; uu < 4; ++uu) duo[(size_t)(z - slot) * slab + uu * C + 16 * n] = 0.f;
  }
  }
  // ---- results of the whole launch --------------------------------------------------------------------------------------
  float *po = part + (size_t)blockIdx.x * PART;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int n = 0; n < 8; ++n)
#pragma unroll
      for (int uu = 0; uu < 4; ++uu) po[(size_t)(32 * w + 16 * t + 4 * lg + uu) * C + 16 * n + l15] = gw[t][n][uu];
  float *p3 = po + C * C, *pb1 = p3 + NO * C, *pb2 = pb1 + C, *pb3 = pb2 + C;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) {
      if (4 * lg + uu < NO) p3[(4 * lg + uu) * C + 32 * w + 16 * t + l15] = g3[t][uu];
      if (l15 == 0) pb2[32 * w + 16 * t + 4 * lg + uu] = gb2[t][uu];
    }
  if (w == 0 && l15 == 0) st4(pb3 + 4 * lg, gb3);
  __syncthreads();
  float *s_sum = s_x;   // db1: the 16 row lanes' sums of channels 32 w + 16 t + 4 lg .. + 3, added in order
  st4(&s_sum[l15 * C + 32 * w + 4 * lg], d1[0]);
  st4(&s_sum[l15 * C + 32 * w + 16 + 4 * lg], d1[1]);
  __syncthreads();
  if (tid < C) {
    float a = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) a += s_sum[g * C + tid];
    pb1[tid] = a;
  }
}

__global__ __launch_bounds__(256) void rel_fused_bwd_kernel(const float *__restrict__ dpred, const float *__restrict__ hid2,
                                                            const float *__restrict__ P, const float *__restrict__ U,
                                                            const float *__restrict__ b1, const float *__restrict__ W2,
                                                            const float *__restrict__ W3, int B, int K, int Z,
                                                            float *__restrict__ dP, float *__restrict__ dU, float *__restrict__ part) {
  rel_bwd_body<false>(dpred, hid2, P, U, b1, W2, W3, B, K, Z, nullptr, dP, dU, part);
}
__global__ __launch_bounds__(256) void rel_fused_bwd_sel_kernel(const float *__restrict__ dpred, const float *__restrict__ hid2,
                                                                const float *__restrict__ P, const float *__restrict__ U,
                                                                const float *__restrict__ b1, const float *__restrict__ W2,
                                                                const float *__restrict__ W3, int B, int K, int Z,
                                                                const int *__restrict__ ws, float *__restrict__ dP,
                                                                float *__restrict__ dU, float *__restrict__ part) {
  rel_bwd_body<true>(dpred, hid2, P, U, b1, W2, W3, B, K, Z, ws, dP, dU, part);
}

// ---- which query rows and key columns of dpred carry a gradient ----------------------------------------------------------
// One workgroup per query row (b, i): its K x 9 values of dpred, read once.  Row flag = any value != 0 (-0 is not, NaN is);
// the row's key columns leave as a bit mask, OR-ed over the scene's rows by the compaction below.  Every word has one writer:
// no atomics, nothing to clear.  The same workgroup writes the zeros of its share of the outputs: dP[b, :, i, :] and
// dU[:, b, i, :, :] -- what the backward kernel does not visit stays zero.
__global__ __launch_bounds__(256) void rel_sel_scan_kernel(const float *__restrict__ dpred, int B, int K, int Z, int *__restrict__ ws,
                                                           float *__restrict__ dP, float *__restrict__ dU) {
  __shared__ int s_f[256];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, NW = sel_nw(K);
  const size_t row = blockIdx.x;
  const int b = (int)(row / K), i = (int)(row - (size_t)b * K);
  unsigned long long *colbits = reinterpret_cast<unsigned long long *>(ws + sel_colbits_off(B, K)) + row * NW;
  bool any = false;
  for (int c0 = 0; c0 < K; c0 += 256) {   // 256 key columns = 2304 contiguous floats at a time
    const int nq = min(256, K - c0) * NO / 4;
    s_f[tid] = 0;
    __syncthreads();
    const float *d = dpred + (row * K + c0) * NO;
    for (int q = tid; q < nq; q += 256) {
      const f32x4 v = ld4(d + 4 * q);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (v[c] != 0.f) s_f[(4 * q + c) / NO] = 1, any = true;   // (every writer stores the same value)
    }
    __syncthreads();
    const unsigned long long bal = __ballot(s_f[tid] != 0);
    if (lane == 0 && (c0 >> 6) + w < NW) colbits[(c0 >> 6) + w] = bal;
    __syncthreads();
  }
  const int r = __syncthreads_or(any);
  if (tid == 0) ws[sel_rowflag_off(B, K) + row] = r != 0;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int h = 0; h < H; ++h) {
    float *o = dP + (((size_t)b * H + h) * K + i) * K;
    for (int q = tid; q < K / 4; q += 256) st4(o + 4 * q, zero);
  }
  for (int z = 0; z < Z; ++z) {
    float *o = dU + ((size_t)z * B * K + row) * H * C;
    for (int q = tid; q < H * C / 4; q += 256) st4(o + 4 * q, zero);
  }
}

// flag[0 .. K) -> list: the flagged indices ascending, then (up to the next multiple of 8) the first unflagged ones ascending
__device__ __forceinline__ int compact_list(const int *flag, int K, int *list, int *s_wc) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int n = 0;
  for (int c0 = 0; c0 < K; c0 += 256) n += __syncthreads_count(c0 + tid < K && flag[c0 + tid] != 0);
  const int pad = ((n + 7) & ~7) - n;
  int base = 0;
  for (int c0 = 0; c0 < K; c0 += 256) {
    const int j = c0 + tid;
    const bool f = j < K && flag[j] != 0;
    const unsigned long long bal = __ballot(f);
    if (lane == 0) s_wc[w] = __popcll(bal);
    __syncthreads();
    int a = base + __popcll(bal & ((1ull << lane) - 1));   // flagged indices below j
    for (int ww = 0; ww < w; ++ww) a += s_wc[ww];
    if (f) list[a] = j;
    else if (j < K && j - a < pad) list[n + j - a] = j;
    base += (s_wc[0] + s_wc[1]) + (s_wc[2] + s_wc[3]);
    __syncthreads();
  }
  return n;
}

// One workgroup per scene: key-column flags from the rows' bit masks, both lists, the counts.
__global__ __launch_bounds__(256) void rel_sel_compact_kernel(int B, int K, int *__restrict__ ws) {
  __shared__ int s_wc[4];
  const int tid = threadIdx.x, b = blockIdx.x, NW = sel_nw(K);
  const unsigned long long *colbits = reinterpret_cast<const unsigned long long *>(ws + sel_colbits_off(B, K)) + (size_t)b * K * NW;
  int *colflag = ws + sel_colflag_off(B, K) + (size_t)b * K;
  for (int j = tid; j < K; j += 256) {
    unsigned long long acc = 0;
#pragma unroll 8
    for (int i = 0; i < K; ++i) acc |= colbits[(size_t)i * NW + (j >> 6)];
    colflag[j] = (int)((acc >> (j & 63)) & 1);
  }
  __threadfence_block();
  __syncthreads();
  const int nq = compact_list(ws + sel_rowflag_off(B, K) + (size_t)b * K, K, ws + sel_qi_off(B, K) + (size_t)b * K, s_wc);
  const int nk = compact_list(colflag, K, ws + sel_kj_off(B, K) + (size_t)b * K, s_wc);
  // (colflag: written above by other threads of this workgroup; compact_list's barriers lie in between)
  const int *rowflag = ws + sel_rowflag_off(B, K) + (size_t)b * K;
  int *bl = ws + sel_blk_off(B, K) + (size_t)b * sel_blk_stride(K);
  const int NB = K / 8;
  int rbn = 0, cbn = 0;
  for (int c0 = 0; c0 < NB; c0 += 256) {
    const int ib = c0 + tid;
    int rf = 0, cf = 0;
    if (ib < NB) {
#pragma unroll
      for (int k = 0; k < 8; ++k) rf |= rowflag[8 * ib + k], cf |= colflag[8 * ib + k];
      bl[2 + ib] = rf != 0, bl[2 + NB + ib] = cf != 0;
    }
    rbn += __syncthreads_count(rf != 0);
    cbn += __syncthreads_count(cf != 0);
  }
  if (tid == 0) {
    int *cnt = ws + sel_cnt_off(B, K) + 4 * b;
    cnt[0] = nq, cnt[1] = nk, cnt[2] = (nq + 7) >> 3, cnt[3] = (nk + 7) >> 3;
    bl[0] = rbn, bl[1] = cbn;
  }
}

constexpr size_t FWD_LDS = (size_t)3 * IMG * 2 + (size_t)(4 * TR * DPL + H * TR) * sizeof(float);
constexpr size_t BWD_LDS = (size_t)2 * 3 * IMGT * 2 + (size_t)(TR * LDT + H * TR + TR * DPL) * sizeof(float);

// Grid: one workgroup per CU the caller has not reserved for side-stream work (spacap_sa_reserve_cus), each with a contiguous
// range of tile units.  A grid sized to ALL CUs would leave its last workgroups waiting behind the sampling chain's (one
// scene per CU for the first half of the step) and run them as a second round: twice the time.
// CUs the head's persistent grids leave free IN ADDITION to spacap_sa_reserve_cus: a caller that runs the caption decoder on
// another stream beside the head (engine.Trainer: the decoder only needs the encoder's output) sets this to what the decoder's
// launches need to be resident at once (spacap_relation_fused_leave_cus).  Below ~56 the decoder's 64-workgroup launches queue
// behind the head's persistent workgroups and the two chains serialise again (measured: 7.25 against 6.97 ms per step).
static std::atomic<int> g_rel_leave{0};
inline int grid_size(int B, int K, int per_cu) {
  const long units = (long)B * (K / TJ) * (K / TI);
  // (with two workgroups per CU the dispatcher needs slack beyond the occupied CUs themselves: launch.hpp, fwd_cus_left_free)
  const int extra = g_rel_leave.load(std::memory_order_relaxed);   // CUs left to a stream that runs beside the head (below)
  const long g = (long)per_cu * std::max(1, spacap::device_cus() - extra - spacap::launch::fwd_cus_left_free(per_cu));
  return (int)std::min(units, g);
}
// dU slots: the largest number of workgroups whose ranges meet one key block
inline int du_slots(int B, int K, int G) {
  const long NI = K / TI, NU = (long)B * (K / TJ) * NI;
  int z = 1;
  for (long g = 0; g < (long)B * (K / TJ); ++g) {
    const long wf = ((g * NI + 1) * G + NU - 1) / NU - 1, wl = (((g + 1) * NI) * G + NU - 1) / NU - 1;
    z = std::max(z, (int)(wl - wf + 1));
  }
  return z;
}

}  // namespace

extern "C" int spacap_relation_fused_leave_cus(int n) {
  if (n < 0 || n > spacap::device_cus() / 2) return SPACAP_E_INVALID;
  g_rel_leave.store(n, std::memory_order_relaxed);
  return SPACAP_OK;
}
extern "C" int spacap_relation_fused_supported(int H_, int K, int C_, int NO_) {
  return H_ == H && C_ == C && NO_ == NO && K >= 8 && K % 8 == 0;
}
extern "C" int spacap_relation_fused_nparts(int B, int K) { return B > 0 && K >= 8 ? grid_size(B, K, 1) : 0; }
extern "C" int spacap_relation_fused_zsplit(int B, int K, int nparts) { return B > 0 && K >= 8 && nparts > 0 ? du_slots(B, K, nparts) : 0; }
extern "C" int spacap_relation_fused_part_floats(void) { return PART; }
// the selected backward's ranges are at least ceil(NI_max / (zslots - 1)) units long: three slots keep them within twice the even share
extern "C" int spacap_relation_fused_sel_zsplit(int B, int K, int nparts) {
  return B > 0 && K >= 8 && nparts > 0 ? std::max(3, du_slots(B, K, nparts)) : 0;
}
extern "C" size_t spacap_relation_fused_sel_workspace_bytes(int B, int K) {
  return B > 0 && K >= 8 ? (sel_blk_off(B, K) + (size_t)B * sel_blk_stride(K)) * sizeof(int) : 0;
}

extern "C" int spacap_relation_fused_fwd_f32(const float *P, const float *U, const float *b1, const float *W2, const float *b2,
                                             const float *W3, const float *b3, int B, int K, float *hid2, float *pred,
                                             spacap_stream_t stream) {
  const char *what = "spacap_relation_fused_fwd_f32";
  SPACAP_REQUIRE(B >= 0 && K >= 8 && K % 8 == 0 && B <= 65535, "%s: (B=%d, K=%d) unsupported", what, B, K);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(P && U && b1 && W2 && b2 && W3 && b3 && hid2 && pred, "%s: null pointer", what);
  static unsigned long long lds_ok = 0;
  SPACAP_CHECK_HIP(spacap::allow_dynamic_lds(reinterpret_cast<const void *>(&rel_fused_fwd_kernel), (int)FWD_LDS, lds_ok), what);
  // (two workgroups per CU overlap each other's phases)
  hipLaunchKernelGGL(rel_fused_fwd_kernel, dim3(grid_size(B, K, 2)), dim3(256), FWD_LDS, spacap::as_stream(stream), P, U, b1, W2, b2, W3,
                     b3, B, K, hid2, pred);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_relation_fused_bwd_f32(const float *dpred, const float *hid2, const float *P, const float *U, const float *b1,
                                             const float *W2, const float *W3, int B, int K, int nparts, int zslots, float *dP,
                                             float *dU, float *part, spacap_stream_t stream) {
  const char *what = "spacap_relation_fused_bwd_f32";
  SPACAP_REQUIRE(B >= 0 && K >= 8 && K % 8 == 0 && B <= 65535, "%s: (B=%d, K=%d) unsupported", what, B, K);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(dpred && hid2 && P && U && b1 && W2 && W3 && dP && dU && part, "%s: null pointer", what);
  static unsigned long long lds_ok = 0;
  SPACAP_CHECK_HIP(spacap::allow_dynamic_lds(reinterpret_cast<const void *>(&rel_fused_bwd_kernel), (int)BWD_LDS, lds_ok), what);
  SPACAP_REQUIRE(nparts >= 1 && nparts <= B * (K / TJ) * (K / TI) && zslots >= du_slots(B, K, nparts),
                 "%s: (nparts=%d, zslots=%d) do not fit (B=%d, K=%d)", what, nparts, zslots, B, K);
  hipLaunchKernelGGL(rel_fused_bwd_kernel, dim3(nparts), dim3(256), BWD_LDS, spacap::as_stream(stream), dpred, hid2, P, U, b1, W2, W3, B, K,
                     zslots, dP, dU, part);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

static int rel_sel_lists(const char *what, const float *dpred, int B, int K, int zslots, float *dP, float *dU, void *workspace,
                         spacap_stream_t stream) {
  SPACAP_REQUIRE(B >= 0 && K >= 8 && K % 8 == 0 && B <= 65535 && zslots >= 1, "%s: (B=%d, K=%d, zslots=%d) unsupported", what, B, K, zslots);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(dpred && dP && dU && workspace, "%s: null pointer", what);
  SPACAP_REQUIRE(((uintptr_t)dpred | (uintptr_t)dP | (uintptr_t)dU) % 16 == 0 && (uintptr_t)workspace % 8 == 0, "%s: unaligned buffer", what);
  hipLaunchKernelGGL(rel_sel_scan_kernel, dim3((unsigned)B * K), dim3(256), 0, spacap::as_stream(stream), dpred, B, K, zslots,
                     static_cast<int *>(workspace), dP, dU);
  SPACAP_CHECK_LAUNCH(what);
  hipLaunchKernelGGL(rel_sel_compact_kernel, dim3(B), dim3(256), 0, spacap::as_stream(stream), B, K, static_cast<int *>(workspace));
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_relation_fused_sel_lists_f32(const float *dpred, int B, int K, int zslots, float *dP, float *dU, void *workspace,
                                                   spacap_stream_t stream) {
  return rel_sel_lists("spacap_relation_fused_sel_lists_f32", dpred, B, K, zslots, dP, dU, workspace, stream);
}

extern "C" int spacap_relation_fused_bwd_sel_f32(const float *dpred, const float *hid2, const float *P, const float *U, const float *b1,
                                                 const float *W2, const float *W3, int B, int K, int nparts, int zslots, float *dP,
                                                 float *dU, float *part, void *workspace, spacap_stream_t stream) {
  const char *what = "spacap_relation_fused_bwd_sel_f32";
  SPACAP_REQUIRE(B >= 0 && K >= 8 && K % 8 == 0 && B <= 65535, "%s: (B=%d, K=%d) unsupported", what, B, K);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(dpred && hid2 && P && U && b1 && W2 && W3 && dP && dU && part && workspace, "%s: null pointer", what);
  static unsigned long long lds_ok = 0;
  SPACAP_CHECK_HIP(spacap::allow_dynamic_lds(reinterpret_cast<const void *>(&rel_fused_bwd_sel_kernel), (int)BWD_LDS, lds_ok), what);
  SPACAP_REQUIRE(nparts >= 1 && nparts <= B * (K / TJ) * (K / TI) && zslots >= std::max(3, du_slots(B, K, nparts)),
                 "%s: (nparts=%d, zslots=%d) do not fit (B=%d, K=%d)", what, nparts, zslots, B, K);
  if (const int rc = rel_sel_lists(what, dpred, B, K, zslots, dP, dU, workspace, stream)) return rc;
  hipLaunchKernelGGL(rel_fused_bwd_sel_kernel, dim3(nparts), dim3(256), BWD_LDS, spacap::as_stream(stream), dpred, hid2, P, U, b1, W2, W3,
                     B, K, zslots, static_cast<const int *>(workspace), dP, dU, part);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
