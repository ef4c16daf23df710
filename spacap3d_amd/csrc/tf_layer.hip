// Fused sub-layer kernels of the Transformer captioner (d_model = 128) for gfx950 (MI355X).
//
// Reference: models/transformer_captioner.py -- SublayerConnection :115-127 (x + dropout(sublayer(norm(x)))),
// LayerNorm :102-113 (unbiased std, eps on std), PositionwiseFeedForward :72-81, MultiHeadedAttention's four
// Linear(128,128) :39-70, EncoderLayer :180-191, DecoderLayer :209-225 (early guide: no cross-attention).
//
// One encoder / decoder layer is ~10 launches forward and ~14 backward as separate operators (LayerNorm, packed q|k|v
// GEMM, attention, output projection, dropout-add, LayerNorm, w_1, relu-dropout, w_2, dropout-add and their
// gradients), each a few microseconds on 1 MB tensors.  Rows (tokens) are independent everywhere except inside the
// attention kernel, so everything between two attention calls is ONE row-tile kernel here:
//
//   tf_rows_kernel<FWD>:  acc = A1 W1^T + b1            (optional GEMM, K1 = 128 .. 2048: output projection or w_2)
//                         x' = res + dropout(acc)       (stored: the residual stream)
//                         n  = LayerNorm(x')            (stored for the weight gradients; statistics for the backward)
//                         out2 = n W2^T + b2            (optional GEMM, N2 = 384: the NEXT attention's packed q|k|v)
//   tf_rows_kernel<BWD>:  dn = A1 W1                    (optional GEMM: dqkv Wqkv, or dhid W_1 with K1 = 2048)
//                         dx = LayerNorm'(dn) + addend  (stored; per-workgroup partials of the LayerNorm parameter sums)
//                         dy = dropout'(dx)             (stored: gradient of the sub-layer output in front of the residual)
//                         out2 = dy W2                  (optional GEMM, N2 = 128: through the output projection)
//   tf_gemm_kernel<EPI>:  weights stationary, 64 x 128 tiles: partial sums over slices of k for the row kernel (EPI 0),
//                         h = dropout(relu(n W_1^T + b_1)) [R, d_ff] (EPI 1) and its backward mask (EPI 2)
//   tf_ffn_kernel, tf_ffn_bf3_kernel (+ tf_ffn_split_kernel): the feed-forward block as ONE launch per direction, on fp32 MFMA
//                         or, for tall inputs, on split-bf16 products with pre-split weight images
// Kernels first, the C entry points after them.  The same kernels with dropout off run the caption decoders' layers
// (caption_decode.hip holds what only decoding needs).
//
// The weight gradients are the batched kernel of linear_grad.hip (deferred to the end of the backward pass).
//
// Arithmetic: v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate: bit-for-bit an fp32 fma chain), computed transposed
// (weights as the A operand) so that a lane ends up with consecutive columns of one row.  Operands reach the
// registers as 16-byte loads through a permutation of k inside every group of 16: lane (l15, lg) loads
// X[l15][16 q + 4 lg .. + 3] and the i-th MFMA of the group uses element i of both operands.
#include <math.h>

#include "common.hpp"
#include "dropout.hpp"
#include "mfma.hpp"

namespace {

using namespace spacap;
using namespace spacap::mfma;
using f32x2 = float __attribute__((ext_vector_type(2)));

constexpr int D = 128;        // d_model
constexpr int BM = 16;        // rows per workgroup of the row kernel
constexpr int LDT = D + 8;    // LDS row stride of a [rows][128] fp32 tile read with ds_read_b128 (conflict-free)

__device__ __forceinline__ f32x2 ld2(const float *p) { return *reinterpret_cast<const f32x2 *>(p); }

struct TfRowsArgs {
  long R;
  const float *A1;       // [R][K1], or [nparts][R][128] partial sums of the first product when nparts > 0, or null
  const float *W1;       // FWD: [128][K1];  BWD: [K1][128]
  const float *bias1;    // FWD: [128] or null
  int K1;
  unsigned drop_thresh;  // 0: no dropout
  float drop_scale;
  float eps;
  unsigned long long seed;
  const unsigned long long *seed_dev;
  const float *res;      // FWD: residual rows [R][128];  BWD: addend [R][128] or null
  float *x_out;          // FWD: res + dropout(gemm1) or null;  BWD: dx
  const float *ln_a, *ln_b;
  float *n_out;          // FWD: LayerNorm output rows or null;  BWD: dy = dropout'(dx) or null
  float *stats;          // FWD: out [R][2] (mean, 1 / (std + eps)) or null;  BWD: in
  const float *x_ln;     // BWD: the rows the LayerNorm normalised
  const float *G;        // BWD with A1 == null: gradient w.r.t. the LayerNorm output [R][128]
  float *part;           // BWD: [gridDim.x][256] partial sums of (d ln_a, d ln_b)
  const float *W2;       // FWD: [N2][128];  BWD: [128][N2 = 128]
  const float *bias2;    // FWD: [N2] or null
  float *out2;           // [R][N2]
  int N2;                // 0: no second product
  int nparts;            // > 0: A1 holds that many partial results of the first product (added in order), no GEMM here
  const float *attn_out; // BWD with N2 == 128 (out2 = gradient of the attention output a): a itself [R][128], and
  float *delta_out;      //   delta_out [R / Lq][8][Lq] receives sum_d out2[r, 16 head + d] a[r, 16 head + d] per (row, head):
  int Lq;                //   the softmax-backward row term of the attention kernel (h = 8 heads of 16), rows r = b Lq + q
};

// Row-tile kernel: see the file header.  256 threads = 4 waves; wave w owns columns [32 w, 32 w + 32) of the
// 128-wide row through GEMM1 and the row epilogue, and N2 / 4 columns of the second product.
template <bool BWD>
__global__ __launch_bounds__(256) void tf_rows_kernel(const TfRowsArgs P) {
  __shared__ __attribute__((aligned(16))) float s_t[BM * LDT];
  __shared__ float s_red[2][4][BM];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const long row0 = (long)blockIdx.x * BM, row = row0 + l15;
  const bool valid = row < P.R;
  const long rowc = valid ? row : P.R - 1;

  // ---- GEMM1 -> v[g][t]: the lane's 8 values of row l15, two groups of 4 consecutive columns cb[g] .. cb[g] + 3
  float v[2][4];
  int cb[2];
#pragma unroll
  for (int g = 0; g < 2; ++g) cb[g] = BWD ? 32 * w + 8 * lg + 4 * g : 32 * w + 16 * g + 4 * lg;
  if (P.nparts > 0) {
    // the first product was formed by tf_gemm_kernel as partial sums over slices of k: add them in slice order
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const float *pp = P.A1 + (size_t)rowc * D + cb[g];
      const size_t ps = (size_t)P.R * D;
      f32x4 a = ld4(pp);
      int sidx = 1;
      for (; sidx + 7 < P.nparts; sidx += 8) {   // eight loads in flight (one round trip for d_ff = 2048's 16 slices, both column
        f32x4 t[8];                              // groups interleaved), added in slice order
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = ld4(pp + (sidx + u) * ps);
#pragma unroll
        for (int u = 0; u < 8; ++u) a += t[u];
      }
      for (; sidx + 3 < P.nparts; sidx += 4) {   // four loads in flight
        const f32x4 t0 = ld4(pp + sidx * ps), t1 = ld4(pp + (sidx + 1) * ps), t2 = ld4(pp + (sidx + 2) * ps),
                    t3 = ld4(pp + (sidx + 3) * ps);
        a += t0, a += t1, a += t2, a += t3;
      }
      for (; sidx < P.nparts; ++sidx) a += ld4(pp + sidx * ps);
#pragma unroll
      for (int t = 0; t < 4; ++t) v[g][t] = a[t];
    }
  } else if (P.A1 != nullptr) {
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const int K1 = P.K1;
    const float *ap = P.A1 + (size_t)rowc * K1 + 4 * lg;
    if (!BWD) {
      // weights [128][K1]: tile j of the wave = output columns 32 w + 16 j + (0..15)
      const float *wp0 = P.W1 + (size_t)(32 * w + l15) * K1 + 4 * lg, *wp1 = wp0 + (size_t)16 * K1;
      // two register sets, loaded one chunk (128 of k) ahead of their use: no copies, so the loads of chunk c + 1 stay in
      // flight under the MFMAs of chunk c
      f32x4 a0[8], p0[8], q0[8], a1[8], p1[8], q1[8];
      auto load = [&](f32x4 *a, f32x4 *x, f32x4 *y, int kc) {
#pragma unroll
        for (int q = 0; q < 8; ++q) a[q] = ld4(ap + kc + 16 * q), x[q] = ld4(wp0 + kc + 16 * q), y[q] = ld4(wp1 + kc + 16 * q);
      };
      auto mma = [&](const f32x4 *a, const f32x4 *x, const f32x4 *y) {
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            acc[0] = MFMA16(x[q][i], a[q][i], acc[0]);
            acc[1] = MFMA16(y[q][i], a[q][i], acc[1]);
          }
      };
      load(a0, p0, q0, 0);
      for (int kc = 0; kc < K1; kc += 256) {
        if (kc + 128 < K1) load(a1, p1, q1, kc + 128);
        mma(a0, p0, q0);
        if (kc + 128 < K1) {
          if (kc + 256 < K1) load(a0, p0, q0, kc + 256);
          mma(a1, p1, q1);
        }
      }
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int u = 0; u < 4; ++u) v[g][u] = acc[g][u];
    } else {
      // weights [K1][128]: the wave's 32 columns as two interleaved tiles, tile i = columns 32 w + 2 n + i
      const float *wp = P.W1 + (size_t)(4 * lg) * D + 32 * w + 2 * l15;
      f32x4 a0[8], a1[8];
      f32x2 x0[32], x1[32];
      auto load = [&](f32x4 *a, f32x2 *x, int kc) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          a[q] = ld4(ap + kc + 16 * q);
#pragma unroll
          for (int i = 0; i < 4; ++i) x[q * 4 + i] = ld2(wp + (size_t)(kc + 16 * q + i) * D);
        }
      };
      auto mma = [&](const f32x4 *a, const f32x2 *x) {
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            acc[0] = MFMA16(x[q * 4 + i][0], a[q][i], acc[0]);
            acc[1] = MFMA16(x[q * 4 + i][1], a[q][i], acc[1]);
          }
      };
      load(a0, x0, 0);
      for (int kc = 0; kc < K1; kc += 256) {
        if (kc + 128 < K1) load(a1, x1, kc + 128);
        mma(a0, x0);
        if (kc + 128 < K1) {
          if (kc + 256 < K1) load(a0, x0, kc + 256);
          mma(a1, x1);
        }
      }
      // acc[i][u] is column 32 w + 2 (4 lg + u) + i = cb[u >> 1] + 2 (u & 1) + i
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u >> 1][2 * (u & 1) + i] = acc[i][u];
    }
  }

  // The second product's weights depend on nothing computed here: its first registers are requested NOW, so that their
  // latency runs under the row epilogue (three barriers and a round of global loads) instead of after it.
  f32x4 x0[8], y0[8];   // FWD: first pair of 16-column tiles of W2
  f32x2 wv2[32];        // BWD: W2 [128][128], the wave's two interleaved tiles
  // forward with N2 > 128: blockIdx.y owns N2 / gridDim.y of the second product's columns (the rows' first part is then formed
  // by every one of those workgroups, stored by the first)
  const int n2y = P.N2 / (int)gridDim.y, nw2 = n2y >> 2, n00 = (int)blockIdx.y * n2y + w * nw2;
  const bool first_y = blockIdx.y == 0;
  const float *wp2 = BWD ? P.W2 + (size_t)(4 * lg) * D + 32 * w + 2 * l15 : P.W2 + (size_t)(n00 + l15) * D + 4 * lg;
  if (P.N2 != 0) {
    if (!BWD) {
#pragma unroll
      for (int q = 0; q < 8; ++q) x0[q] = ld4(wp2 + 16 * q), y0[q] = ld4(wp2 + 16 * D + 16 * q);
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) wv2[q * 4 + i] = ld2(wp2 + (size_t)(16 * q + i) * D);
    }
  }

  const DropSeed sd = make_seed(P.seed, P.seed_dev);
  float t_out[2][4];   // what the second product consumes: FWD LayerNorm output, BWD dy

  if (!BWD) {
    // ---- x' = res + dropout(acc + b1);  n = LayerNorm(x') ----------------------------------------------------------
    float xo[2][4], s = 0.f;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const f32x4 r4 = ld4(P.res + (size_t)rowc * D + cb[g]);
      if (P.A1 != nullptr) {
        f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
        if (P.bias1) b4 = ld4(P.bias1 + cb[g]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          float a = v[g][t] + b4[t];
          if (P.drop_thresh != 0u) {
            const bool keep = hash32((unsigned long long)row * D + cb[g] + t, sd) >= P.drop_thresh;
            a = keep ? a * P.drop_scale : 0.f;
          }
          xo[g][t] = r4[t] + a;
        }
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) xo[g][t] = r4[t];
      }
      if (P.x_out && valid && first_y) st4(P.x_out + (size_t)row * D + cb[g], f32x4{xo[g][0], xo[g][1], xo[g][2], xo[g][3]});
#pragma unroll
      for (int t = 0; t < 4; ++t) s += xo[g][t];
    }
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (lg == 0) s_red[0][w][l15] = s;
    __syncthreads();
    const float mu = ((s_red[0][0][l15] + s_red[0][1][l15]) + (s_red[0][2][l15] + s_red[0][3][l15])) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float c = xo[g][t] - mu;
        q += c * c;
      }
    q += __shfl_xor(q, 16);
    q += __shfl_xor(q, 32);
    if (lg == 0) s_red[1][w][l15] = q;
    __syncthreads();
    const float var = ((s_red[1][0][l15] + s_red[1][1][l15]) + (s_red[1][2][l15] + s_red[1][3][l15])) / (float)(D - 1);
    const float r = 1.0f / (sqrtf(var) + P.eps);
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const f32x4 a4 = ld4(P.ln_a + cb[g]), b4 = ld4(P.ln_b + cb[g]);
#pragma unroll
      for (int t = 0; t < 4; ++t) t_out[g][t] = a4[t] * ((xo[g][t] - mu) * r) + b4[t];
      if (P.n_out && valid && first_y)
        st4(P.n_out + (size_t)row * D + cb[g], f32x4{t_out[g][0], t_out[g][1], t_out[g][2], t_out[g][3]});
    }
    if (P.stats && valid && w == 0 && lg == 0 && first_y) {
      P.stats[row * 2] = mu;
      P.stats[row * 2 + 1] = r;
    }
  } else {
    // ---- dx = LayerNorm'(dn) + addend;  partial sums of the LayerNorm parameter gradients;  dy = dropout'(dx) -----
    const float mu = P.stats[rowc * 2], r = P.stats[rowc * 2 + 1];
    float dn[2][4], xc[2][4], dxh[2][4], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      if (P.A1 == nullptr) {
        const f32x4 g4 = ld4(P.G + (size_t)rowc * D + cb[g]);
#pragma unroll
        for (int t = 0; t < 4; ++t) v[g][t] = g4[t];
      }
      const f32x4 x4 = ld4(P.x_ln + (size_t)rowc * D + cb[g]), a4 = ld4(P.ln_a + cb[g]);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        dn[g][t] = valid ? v[g][t] : 0.f;
        xc[g][t] = x4[t] - mu;
        dxh[g][t] = dn[g][t] * a4[t];
        s1 += dxh[g][t];
        s2 += dxh[g][t] * xc[g][t];
      }
    }
    s1 += __shfl_xor(s1, 16);
    s1 += __shfl_xor(s1, 32);
    s2 += __shfl_xor(s2, 16);
    s2 += __shfl_xor(s2, 32);
    if (lg == 0) s_red[0][w][l15] = s1, s_red[1][w][l15] = s2;
    __syncthreads();
    s1 = (s_red[0][0][l15] + s_red[0][1][l15]) + (s_red[0][2][l15] + s_red[0][3][l15]);
    s2 = (s_red[1][0][l15] + s_red[1][1][l15]) + (s_red[1][2][l15] + s_red[1][3][l15]);
    const float sdv = 1.0f / r - P.eps;                            // the unbiased std
    // (a constant row: std == 0, where autograd masks the gradient through the std to zero; unmasked this is 0/0 = NaN)
    const float c2 = sdv == 0.f ? 0.f : -(s2 * r * r) / (sdv * (float)(D - 1));
    const float c1 = r * s1 / (float)D;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      f32x4 ad = {0.f, 0.f, 0.f, 0.f};
      if (P.res) ad = ld4(P.res + (size_t)rowc * D + cb[g]);
      float dx[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        dx[t] = r * dxh[g][t] + c2 * xc[g][t] - c1 + ad[t];
        float y = dx[t];
        if (P.drop_thresh != 0u) {
          const bool keep = hash32((unsigned long long)row * D + cb[g] + t, sd) >= P.drop_thresh;
          y = keep ? y * P.drop_scale : 0.f;
        }
        t_out[g][t] = valid ? y : 0.f;
      }
      if (valid) {
        st4(P.x_out + (size_t)row * D + cb[g], f32x4{dx[0], dx[1], dx[2], dx[3]});
        if (P.n_out) st4(P.n_out + (size_t)row * D + cb[g], f32x4{t_out[g][0], t_out[g][1], t_out[g][2], t_out[g][3]});
      }
      // column sums over the 16 rows of the tile (lanes l15 = 0..15 of one lg), fixed tree order
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float pa = dn[g][t] * (xc[g][t] * r), pb = dn[g][t];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          pa += __shfl_xor(pa, o);
          pb += __shfl_xor(pb, o);
        }
        if (l15 == 0) {
          P.part[(size_t)blockIdx.x * 2 * D + cb[g] + t] = pa;
          P.part[(size_t)blockIdx.x * 2 * D + D + cb[g] + t] = pb;
        }
      }
    }
  }

  if (P.N2 == 0) return;   // (uniform: kernel argument)

  // ---- second product on the rows just formed -------------------------------------------------------------------------
#pragma unroll
  for (int g = 0; g < 2; ++g) st4(&s_t[l15 * LDT + cb[g]], f32x4{t_out[g][0], t_out[g][1], t_out[g][2], t_out[g][3]});
  __syncthreads();
  f32x4 at[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) at[q] = ld4(&s_t[l15 * LDT + 16 * q + 4 * lg]);
  if (!BWD) {
    // W2 [N2][128], N2 a multiple of 128: the wave's N2 / 4 columns in pairs of 16-column tiles
    const int N2 = P.N2, nw = nw2;
    const float *wp = wp2;
    // pairs of tiles, two register sets loaded one pair ahead (no copies: the loads stay in flight under the MFMAs)
    f32x4 x1[8], y1[8];
    auto load = [&](f32x4 *x, f32x4 *y, int jt) {
#pragma unroll
      for (int q = 0; q < 8; ++q) x[q] = ld4(wp + (size_t)jt * D + 16 * q), y[q] = ld4(wp + (size_t)(jt + 16) * D + 16 * q);
    };
    auto pair = [&](const f32x4 *x, const f32x4 *y, int jt) {
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc0 = MFMA16(x[q][i], at[q][i], acc0);
          acc1 = MFMA16(y[q][i], at[q][i], acc1);
        }
      const int c0 = n00 + jt + 4 * lg;
      if (P.bias2) acc0 += ld4(P.bias2 + c0), acc1 += ld4(P.bias2 + c0 + 16);
      if (valid) {
        st4(P.out2 + (size_t)row * N2 + c0, acc0);
        st4(P.out2 + (size_t)row * N2 + c0 + 16, acc1);
      }
    };
    for (int jt = 0; jt < nw; jt += 64) {   // (pair 0 was requested before the row epilogue)
      if (jt + 32 < nw) load(x1, y1, jt + 32);
      pair(x0, y0, jt);
      if (jt + 32 < nw) {
        if (jt + 64 < nw) load(x0, y0, jt + 64);
        pair(x1, y1, jt + 32);
      }
    }
  } else {
    // W2 [128][128] (N2 == 128): out2 = dy W2, the wave's 32 columns as two interleaved tiles
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[0] = MFMA16(wv2[q * 4 + i][0], at[q][i], acc[0]);
        acc[1] = MFMA16(wv2[q * 4 + i][1], at[q][i], acc[1]);
      }
    float dsum = 0.f;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      // columns cb[g] + e: e = 2 (u & 1) + i with u >> 1 == g
      const f32x4 o = {acc[0][2 * g], acc[1][2 * g], acc[0][2 * g + 1], acc[1][2 * g + 1]};
      if (valid) st4(P.out2 + (size_t)row * D + cb[g], o);
      if (P.delta_out) {
        const f32x4 a4 = ld4(P.attn_out + (size_t)rowc * D + cb[g]);
        dsum += (o[0] * a4[0] + o[1] * a4[1]) + (o[2] * a4[2] + o[3] * a4[3]);
      }
    }
    if (P.delta_out) {
      // the lane's 8 columns 32 w + 8 lg .. + 7 are half of head 2 w + (lg >> 1); the other half sits in lane ^ 16
      dsum += __shfl_xor(dsum, 16);
      if (valid && (lg & 1) == 0) {
        const long bi = row / P.Lq, qi = row - bi * P.Lq;
        P.delta_out[((size_t)bi * 8 + 2 * w + (lg >> 1)) * P.Lq + qi] = dsum;
      }
    }
  }
}

// Tiled product with the weights stationary in registers and a choice of epilogue (fp32 MFMA, 64-row x 128-column tile
// per workgroup, K walked in chunks of 128 through LDS; blockIdx.z = slice of K for the split products):
//   EPI 0  out[z][r][n] = sum_{k in slice z} x[r][k] Wop[k][n]            partial sums, added in order by tf_rows_kernel
//          (w_2 / the data gradient through w_1: K = d_ff = 2 048 and only 128 output columns -- a row-tile kernel alone would
//          occupy R / 16 workgroups for 2 048 dependent k-steps each; split over K the product fills the chip)
//   EPI 1  out[r][n] = dropout(relu(. + bias[n]))                          models/transformer_captioner.py:80 (w_1)
//   EPI 2  out[r][n] = y[r][n] > 0 ? scale * . : 0                         backward of EPI 1 through w_2 (y = the saved EPI-1 output)
// NN: Wop[k][n] = W[k][n] (W [K][ldw >= N]: data gradients), else Wop[k][n] = W[n][k] (W [N][ldw >= K]: forward products).
constexpr int FM = 64;
struct TfGemmArgs {
  const float *x, *W, *bias, *y;
  float *out;
  long R;
  int ldx, ldw, N, KS;
  unsigned thresh;
  float scale;
  unsigned long long seed;
  const unsigned long long *seed_dev;
};
template <int EPI, bool NN>
__global__ __launch_bounds__(256) void tf_gemm_kernel(const TfGemmArgs P) {
  __shared__ __attribute__((aligned(16))) float s_a[FM * LDT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const long row0 = (long)blockIdx.x * FM;
  const int n0 = blockIdx.y * 128 + 32 * w;
  const int k0 = blockIdx.z * P.KS;
  const int c4 = tid & 31, r0 = tid >> 5;
  f32x4 acc[FM / 16][2];
#pragma unroll
  for (int mt = 0; mt < FM / 16; ++mt) acc[mt][0] = acc[mt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kc = k0; kc < k0 + P.KS; kc += 128) {
    if (kc != k0) __syncthreads();
    {
      // (rows past the end read the last row: branch-free, so the eight loads are in flight together; those rows of the
      // tile are computed and never stored)
      f32x4 stg[FM / 8];
#pragma unroll
      for (int i = 0; i < FM / 8; ++i) {
        const long rr = min(row0 + r0 + 8 * i, P.R - 1);
        stg[i] = ld4(P.x + (size_t)rr * P.ldx + kc + c4 * 4);
      }
#pragma unroll
      for (int i = 0; i < FM / 8; ++i) st4(&s_a[(r0 + 8 * i) * LDT + c4 * 4], stg[i]);
    }
    f32x4 w0[8], w1[8];   // NN: w0[q][i] / w1[q][i] = the two interleaved tiles' weights for k = kc + 16 q + 4 lg + i
    if (!NN) {
      const float *wp = P.W + (size_t)(n0 + l15) * P.ldw + kc + 4 * lg;
#pragma unroll
      for (int q = 0; q < 8; ++q) w0[q] = ld4(wp + 16 * q), w1[q] = ld4(wp + (size_t)16 * P.ldw + 16 * q);
    } else {
      const float *wp = P.W + (size_t)(kc + 4 * lg) * P.ldw + n0 + 2 * l15;
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x2 t = ld2(wp + (size_t)(16 * q + i) * P.ldw);
          w0[q][i] = t[0], w1[q][i] = t[1];
        }
    }
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < FM / 16; ++mt)
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const f32x4 a = ld4(&s_a[(mt * 16 + l15) * LDT + 16 * q + 4 * lg]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[mt][0] = MFMA16(w0[q][i], a[i], acc[mt][0]);
          acc[mt][1] = MFMA16(w1[q][i], a[i], acc[mt][1]);
        }
      }
  }
  // the lane's columns of row (mt, l15): two runs of four, starting at c0 and c1
  const int c0 = NN ? n0 + 8 * lg : n0 + 4 * lg, c1 = NN ? c0 + 4 : c0 + 16;
  f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = {0.f, 0.f, 0.f, 0.f};
  if (EPI == 1 && P.bias) b0 = ld4(P.bias + c0), b1 = ld4(P.bias + c1);
  const DropSeed sd = make_seed(P.seed, P.seed_dev);
  float *out = P.out + (EPI == 0 ? (size_t)blockIdx.z * P.R * P.N : (size_t)0);
#pragma unroll
  for (int mt = 0; mt < FM / 16; ++mt) {
    const long row = row0 + mt * 16 + l15;
    if (row >= P.R) continue;
    f32x4 o0, o1;
    if (NN) {
      o0 = f32x4{acc[mt][0][0], acc[mt][1][0], acc[mt][0][1], acc[mt][1][1]};
      o1 = f32x4{acc[mt][0][2], acc[mt][1][2], acc[mt][0][3], acc[mt][1][3]};
    } else {
      o0 = acc[mt][0], o1 = acc[mt][1];
    }
    if (EPI == 1) {
      o0 += b0, o1 += b1;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float a0 = fmaxf(o0[u], 0.f), a1 = fmaxf(o1[u], 0.f);
        if (P.thresh != 0u) {
          const unsigned long long e = (unsigned long long)row * P.N;
          a0 = hash32(e + c0 + u, sd) >= P.thresh ? a0 * P.scale : 0.f;
          a1 = hash32(e + c1 + u, sd) >= P.thresh ? a1 * P.scale : 0.f;
        }
        o0[u] = a0, o1[u] = a1;
      }
    } else if (EPI == 2) {
      const f32x4 y0 = ld4(P.y + (size_t)row * P.N + c0), y1 = ld4(P.y + (size_t)row * P.N + c1);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        o0[u] = y0[u] > 0.f ? o0[u] * P.scale : 0.f;
        o1[u] = y1[u] > 0.f ? o1[u] * P.scale : 0.f;
      }
    }
    st4(out + (size_t)row * P.N + c0, o0);
    st4(out + (size_t)row * P.N + c1, o1);
  }
}

// The feed-forward block as ONE launch per direction, chained through LDS (models/transformer_captioner.py:72-81):
//   forward   h_c = dropout(relu(n W1_c^T + b1_c))   [64 rows x 128 hidden units c]   stored (the backward needs it)
//             part[c] = h_c W2[:, c]^T                [64 x 128]   partial sum of w_2's output over this slice of d_ff
//   backward  dhid_c = (dy W2[:, c]) * [h_c > 0] * scale            stored (the weight gradient of w_1 needs it)
//             part[c] = dhid_c W1_c                   [64 x 128]   partial sum of the gradient w.r.t. the LayerNorm output
// One workgroup per (64-row tile, 128-wide slice of d_ff): the hidden tile goes from the first product's accumulators
// through the epilogue into LDS and is the second product's activation tile; both weight blocks are in registers
// before the first MFMA (the second block's load latency hides under the first product).  tf_rows_kernel adds the
// d_ff / 128 partial sums in slice order.
struct TfFfnArgs {
  const float *x, *Wa, *Wb, *bias, *y;
  float *hid, *part;
  long R;
  int dff;
  unsigned thresh;
  float scale;
  unsigned long long seed;
  const unsigned long long *seed_dev;
};
template <bool BWD, int MT>   // MT row tiles of 16 per workgroup: 4, or 1 for the few hundred rows of the caption decoder
__global__ __launch_bounds__(256) void tf_ffn_kernel(const TfFfnArgs P) {
  constexpr int FM = 16 * MT, NST = FM >= 8 ? FM / 8 : 1;
  __shared__ __attribute__((aligned(16))) float s_a[FM * LDT];
  __shared__ __attribute__((aligned(16))) float s_h[FM * LDT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const long row0 = (long)blockIdx.x * FM;
  const int c0 = blockIdx.y * 128, dff = P.dff;
  const int c4 = tid & 31, r0 = tid >> 5;
  f32x4 stg[NST];   // (rows past the end read the last row: branch-free, all loads in flight together; never stored)
#pragma unroll
  for (int i = 0; i < NST; ++i) stg[i] = ld4(P.x + (size_t)min(row0 + r0 + 8 * i, P.R - 1) * D + c4 * 4);
  // element [q][i] of a weight register = Wop[k = 16 q + 4 lg + i][the wave's column l15 of tile 0 / 1]
  f32x4 a0[8], a1[8], b0[8], b1[8];
  if (!BWD) {
    const float *wa = P.Wa + (size_t)(c0 + 32 * w + l15) * D + 4 * lg;          // W1 [dff][128]: rows = hidden units
    const float *wb = P.Wb + (size_t)(32 * w + l15) * dff + c0 + 4 * lg;        // W2 [128][dff]: k = hidden units
#pragma unroll
    for (int q = 0; q < 8; ++q) a0[q] = ld4(wa + 16 * q), a1[q] = ld4(wa + 16 * D + 16 * q);
#pragma unroll
    for (int q = 0; q < 8; ++q) b0[q] = ld4(wb + 16 * q), b1[q] = ld4(wb + (size_t)16 * dff + 16 * q);
  } else {
    const float *wa = P.Wa + (size_t)(4 * lg) * dff + c0 + 32 * w + 2 * l15;    // W2 [128][dff]: k = model channels
    const float *wb = P.Wb + (size_t)(c0 + 4 * lg) * D + 32 * w + 2 * l15;      // W1 [dff][128]: k = hidden units
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x2 t = ld2(wa + (size_t)(16 * q + i) * dff);
        a0[q][i] = t[0], a1[q][i] = t[1];
      }
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x2 t = ld2(wb + (size_t)(16 * q + i) * D);
        b0[q][i] = t[0], b1[q][i] = t[1];
      }
  }
#pragma unroll
  for (int i = 0; i < NST; ++i) st4(&s_a[(r0 + 8 * i) * LDT + c4 * 4], stg[i]);
  // the lane's columns inside the 128-wide block: two runs of four starting at e0 and e1
  const int e0 = BWD ? 32 * w + 8 * lg : 32 * w + 4 * lg, e1 = BWD ? e0 + 4 : e0 + 16;
  f32x4 bb0 = {0.f, 0.f, 0.f, 0.f}, bb1 = {0.f, 0.f, 0.f, 0.f};
  if (!BWD && P.bias) bb0 = ld4(P.bias + c0 + e0), bb1 = ld4(P.bias + c0 + e1);
  const DropSeed sd = make_seed(P.seed, P.seed_dev);
  __syncthreads();
#pragma unroll
  for (int mt = 0; mt < FM / 16; ++mt) {
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const f32x4 a = ld4(&s_a[(mt * 16 + l15) * LDT + 16 * q + 4 * lg]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc0 = MFMA16(a0[q][i], a[i], acc0);
        acc1 = MFMA16(a1[q][i], a[i], acc1);
      }
    }
    const long row = row0 + mt * 16 + l15;
    const bool valid = row < P.R;
    f32x4 o0, o1;
    if (BWD) {
      o0 = f32x4{acc0[0], acc1[0], acc0[1], acc1[1]};
      o1 = f32x4{acc0[2], acc1[2], acc0[3], acc1[3]};
      f32x4 y0 = {0.f, 0.f, 0.f, 0.f}, y1 = {0.f, 0.f, 0.f, 0.f};
      if (valid) y0 = ld4(P.y + (size_t)row * dff + c0 + e0), y1 = ld4(P.y + (size_t)row * dff + c0 + e1);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        o0[u] = y0[u] > 0.f ? o0[u] * P.scale : 0.f;
        o1[u] = y1[u] > 0.f ? o1[u] * P.scale : 0.f;
      }
    } else {
      o0 = acc0 + bb0, o1 = acc1 + bb1;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float v0 = fmaxf(o0[u], 0.f), v1 = fmaxf(o1[u], 0.f);
        if (P.thresh != 0u) {
          const unsigned long long e = (unsigned long long)row * dff + c0;
          v0 = hash32(e + e0 + u, sd) >= P.thresh ? v0 * P.scale : 0.f;
          v1 = hash32(e + e1 + u, sd) >= P.thresh ? v1 * P.scale : 0.f;
        }
        o0[u] = valid ? v0 : 0.f, o1[u] = valid ? v1 : 0.f;
      }
    }
    if (valid && P.hid) {   // (inference passes no buffer: nothing is kept for a backward)
      st4(P.hid + (size_t)row * dff + c0 + e0, o0);
      st4(P.hid + (size_t)row * dff + c0 + e1, o1);
    }
    st4(&s_h[(mt * 16 + l15) * LDT + e0], o0);
    st4(&s_h[(mt * 16 + l15) * LDT + e1], o1);
  }
  __syncthreads();
  float *out = P.part + (size_t)blockIdx.y * P.R * D;
#pragma unroll
  for (int mt = 0; mt < FM / 16; ++mt) {
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const f32x4 a = ld4(&s_h[(mt * 16 + l15) * LDT + 16 * q + 4 * lg]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc0 = MFMA16(b0[q][i], a[i], acc0);
        acc1 = MFMA16(b1[q][i], a[i], acc1);
      }
    }
    const long row = row0 + mt * 16 + l15;
    if (row < P.R) {
      if (BWD) {
        st4(out + (size_t)row * D + e0, f32x4{acc0[0], acc1[0], acc0[1], acc1[1]});
        st4(out + (size_t)row * D + e1, f32x4{acc0[2], acc1[2], acc0[3], acc1[3]});
      } else {
        st4(out + (size_t)row * D + e0, acc0);
        st4(out + (size_t)row * D + e1, acc1);
      }
    }
  }
}

// ---- the chained feed-forward kernel on split-bf16 products (tall inputs: the encoder's 2 048 rows, greedy decoding) ---------
// Same contract as tf_ffn_kernel; both products as bf16 x 3 (three bf16 pieces per operand, the six piece products above 2^-24
// on v_mfma_f32_16x16x32_bf16: fp32-equivalent at 6/16 of the fp32-MFMA time).  The WEIGHTS arrive pre-split (four piece
// images per layer, made by one batched launch per stack and forward: spacap_tf_ffn_split_f32) in the two layouts the products
// need -- rows = the product's output unit, 8 consecutive contraction indices per 16-byte operand load -- and go from L2 straight
// into matrix-core operand registers, one 32-deep contraction step ahead; the 64-row activation tile is split once into three
// LDS images [64][128 + 8] which the hidden tile overwrites between the two products (everything of product 1 is in
// accumulators by then).  52 KB of LDS, ~130 registers: three workgroups per CU.
constexpr int FF_LD = D + 8, FF_IMG = 64 * FF_LD;
struct TfFfnBf3Args {
  const float *x, *bias, *y;
  const __bf16 *Wa, *Wb;   // the two products' weight piece images [3][dff 128], in operand order (tf_ffn_split_kernel)
  float *hid, *part;
  long R;
  int dff;
  unsigned thresh;
  float scale;
  unsigned long long seed;
  const unsigned long long *seed_dev;
};
template <bool BWD>
__global__ __launch_bounds__(256, 3) void tf_ffn_bf3_kernel(const TfFfnBf3Args P) {
  __shared__ __attribute__((aligned(16))) __bf16 s_t[3 * FF_IMG];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  // workgroup -> (row tile, slice of d_ff): workgroups are dealt round robin to the 8 XCDs, each with its own L2.  An XCD takes
  // nslice / 8 slices for ALL row tiles, so it fetches 2 x 2 x 96 KB of weight images and the 1 MB of rows instead of every
  // slice's images (3 MB per XCD: 24 MB of the launch's fetches, rocprofv3 FETCH_SIZE) for a few row tiles.
  const int dff = P.dff, nslice = dff / 128;
  int slice;
  long tile;
  if (nslice % 8 == 0) {
    const int spx = nslice / 8;
    const long j = blockIdx.x / 8;
    slice = (int)(blockIdx.x % 8) * spx + (int)(j % spx);
    tile = j / spx;
  } else {
    const long ntiles = (P.R + 63) / 64;
    tile = blockIdx.x % ntiles, slice = (int)(blockIdx.x / ntiles);
  }
  const long row0 = tile * 64;
  const int c0 = slice * 128;
  const int c4 = tid & 31, r0 = tid >> 5;
  // ---- the rows' tile: fp32 -> three bf16 images
  {
    f32x4 stg[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) stg[i] = ld4(P.x + (size_t)min(row0 + r0 + 8 * i, P.R - 1) * D + c4 * 4);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      bf16x4 p0, p1, p2;
      split4(stg[i], p0, p1, p2);
      __bf16 *d = s_t + (r0 + 8 * i) * FF_LD + 4 * c4;
      *reinterpret_cast<bf16x4 *>(d) = p0;
      *reinterpret_cast<bf16x4 *>(d + FF_IMG) = p1;
      *reinterpret_cast<bf16x4 *>(d + 2 * FF_IMG) = p2;
    }
  }
  // weight operand of a product, step kc: wq[t][piece] = 8 consecutive contraction indices of output unit 32 w + 16 t + l15.  The
  // piece images are stored in OPERAND ORDER (tf_ffn_split_kernel): the 64 lanes of one load read 1 KB of consecutive bytes
  // (per-lane 16-byte reads at a row pitch of 256 B / 4 KB ran the kernel at the L1's line rate, not the matrix rate)
  auto wload = [&](const __bf16 *base, size_t img, int kc, bf16x8 (*wq)[3]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int p = 0; p < 3; ++p) wq[t][p] = *reinterpret_cast<const bf16x8 *>(base + p * img + (size_t)(((t * 4 + kc) * 64 + lane) * 8));
  };
  // one product: acc[t][mt][u] = out[row 16 mt + l15][unit 32 w + 16 t + 4 lg + u] (weights as the A operand: a lane ends up with
  // four consecutive units of one row)
  auto product = [&](const __bf16 *wbase, size_t img, f32x4 (*acc)[4]) {
    bf16x8 wq[2][2][3];
    wload(wbase, img, 0, wq[0]);
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      if (kc + 1 < 4) wload(wbase, img, kc + 1, wq[(kc + 1) & 1]);
      bf16x8 a[4][3];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int p = 0; p < 3; ++p) a[mt][p] = *reinterpret_cast<const bf16x8 *>(s_t + p * FF_IMG + (16 * mt + l15) * FF_LD + 32 * kc + 8 * lg);
#pragma unroll
      for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) acc[t][mt] = MFMA_B(wq[kc & 1][t][PA[q]], a[mt][PB[q]], acc[t][mt]);
    }
  };
  f32x4 acc[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  const size_t wimg = (size_t)dff * D, wofs = (size_t)(slice * 4 + w) * 4096;   // (slice, wave) block of 2 x 4 x 64 x 8 elements
  product(P.Wa + wofs, wimg, acc);
  f32x4 bb[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  if (!BWD && P.bias) bb[0] = ld4(P.bias + c0 + 32 * w + 4 * lg), bb[1] = ld4(P.bias + c0 + 32 * w + 16 + 4 * lg);
  const DropSeed sd = make_seed(P.seed, P.seed_dev);
  __syncthreads();   // every wave has read the rows' images for the last time: the hidden tile takes their place
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const long row = row0 + 16 * mt + l15;
    const bool valid = row < P.R;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int e = 32 * w + 16 * t + 4 * lg;   // the lane's four hidden units inside the slice
      f32x4 o = acc[t][mt];
      if (BWD) {
        f32x4 yv = {0.f, 0.f, 0.f, 0.f};
        if (valid) yv = ld4(P.y + (size_t)row * dff + c0 + e);
#pragma unroll
        for (int u = 0; u < 4; ++u) o[u] = yv[u] > 0.f ? o[u] * P.scale : 0.f;
      } else {
        o += bb[t];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          float v = fmaxf(o[u], 0.f);
          if (P.thresh != 0u) v = hash32((unsigned long long)row * dff + c0 + e + u, sd) >= P.thresh ? v * P.scale : 0.f;
          o[u] = valid ? v : 0.f;
        }
      }
      if (valid && P.hid) st4(P.hid + (size_t)row * dff + c0 + e, o);
      bf16x4 p0, p1, p2;
      split4(o, p0, p1, p2);
      __bf16 *d = s_t + (16 * mt + l15) * FF_LD + e;
      *reinterpret_cast<bf16x4 *>(d) = p0;
      *reinterpret_cast<bf16x4 *>(d + FF_IMG) = p1;
      *reinterpret_cast<bf16x4 *>(d + 2 * FF_IMG) = p2;
      acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  __syncthreads();
  product(P.Wb + wofs, wimg, acc);
  float *out = P.part + (size_t)slice * P.R * D;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const long row = row0 + 16 * mt + l15;
    if (row < P.R) {
#pragma unroll
      for (int t = 0; t < 2; ++t) st4(out + (size_t)row * D + 32 * w + 16 * t + 4 * lg, acc[t][mt]);
    }
  }
}

// the four piece images of up to 16 feed-forward layers in one launch: per layer W1 f32 [dff][128], W2 f32 [128][dff] ->
//   out + 0 img: first-product operands of the forward  (unit = hidden h, contraction k = model channel:  W1[h][k])
//   out + 1 img: second-product operands of the forward (unit = model channel m, contraction k = hidden:  W2[m][k])
//   out + 2 img: first-product operands of the backward (unit = hidden h, contraction k = model channel:  W2[k][h])
//   out + 3 img: second-product operands of the backward (unit = model channel m, contraction k = hidden: W1[k][m])
// img = 3 dff 128 elements (three pieces of dff 128).  Inside a piece the elements are in OPERAND ORDER of tf_ffn_bf3_kernel:
//   index = ((((slice c, wave w), t, kc), lane), e)  <->  unit 32 w + 16 t + (lane % 16) [+ 128 c for hidden units],
//   contraction index 32 kc + 8 (lane / 16) + e [+ 128 c when it runs over hidden units]
constexpr int FF_SPLIT_MAX = 16;
struct FfSplitTable {
  int nlayers, dff;
  const float *w1[FF_SPLIT_MAX], *w2[FF_SPLIT_MAX];
  __bf16 *out[FF_SPLIT_MAX];
};
__global__ __launch_bounds__(256) void tf_ffn_split_kernel(const FfSplitTable T) {
  const int layer = blockIdx.y, dff = T.dff;
  const size_t n = (size_t)dff * D, img = 3 * n;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int e = (int)(idx & 7), lane = (int)((idx >> 3) & 63), kc = (int)((idx >> 9) & 3), t = (int)((idx >> 11) & 1),
            w = (int)((idx >> 12) & 3), c = (int)(idx >> 14);
  const int unit = 32 * w + 16 * t + (lane & 15), kk = 32 * kc + 8 * (lane >> 4) + e;   // inside the 128 x 128 block of slice c
  const float *W1 = T.w1[layer], *W2 = T.w2[layer];
  const int h_u = 128 * c + unit, h_k = 128 * c + kk;
  const float v[4] = {W1[(size_t)h_u * D + kk], W2[(size_t)unit * dff + h_k], W2[(size_t)kk * dff + h_u], W1[(size_t)h_k * D + unit]};
  __bf16 *o = T.out[layer];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // (split3 of mfma.hpp, spelled out: each piece is stored as soon as it exists, and the instruction order follows the source)
    const __bf16 hh = (__bf16)v[i];
    const float r = v[i] - (float)hh;
    const __bf16 m = (__bf16)r;
    __bf16 *d = o + i * img + idx;
    d[0] = hh, d[n] = m, d[2 * n] = (__bf16)(r - (float)m);
  }
}

// the one launch of tf_gemm_kernel behind its three entry points (host)
template <int EPI>
int launch_gemm(const char *what, const TfGemmArgs &P, bool nn, long R, int N, int nsplit, hipStream_t s) {
  const long tiles = (R + FM - 1) / FM;
  SPACAP_REQUIRE(tiles <= 2147483647L, "%s: too many rows", what);
  const dim3 grid((unsigned)tiles, N / 128, nsplit);
  if (nn) hipLaunchKernelGGL((tf_gemm_kernel<EPI, true>), grid, dim3(256), 0, s, P);
  else hipLaunchKernelGGL((tf_gemm_kernel<EPI, false>), grid, dim3(256), 0, s, P);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

}  // namespace

extern "C" int spacap_tf_rows_f32(const spacap_tf_rows_args *a, spacap_stream_t stream) {
  const char *what = "spacap_tf_rows_f32";
  SPACAP_REQUIRE(a != nullptr, "%s: null argument block", what);
  SPACAP_REQUIRE(a->R >= 0 && (a->mode == 0 || a->mode == 1), "%s: bad R / mode", what);
  if (a->R == 0) return SPACAP_OK;
  TfRowsArgs P;
  P.R = a->R;
  P.A1 = a->a1, P.W1 = a->w1, P.bias1 = a->bias1, P.K1 = a->k1;
  SPACAP_REQUIRE(drop_params(a->drop_p, P.drop_thresh, P.drop_scale), "%s: bad dropout probability %f", what, (double)a->drop_p);
  P.eps = a->eps, P.seed = a->seed, P.seed_dev = reinterpret_cast<const unsigned long long *>(a->seed_dev);
  P.res = a->res, P.x_out = a->x_out, P.ln_a = a->ln_a, P.ln_b = a->ln_b, P.n_out = a->n_out, P.stats = a->stats;
  P.x_ln = a->x_ln, P.G = a->g, P.part = a->part, P.W2 = a->w2, P.bias2 = a->bias2, P.out2 = a->out2, P.N2 = a->n2;
  P.nparts = a->nparts;
  P.attn_out = a->attn_out, P.delta_out = a->delta_out, P.Lq = a->lq;
  SPACAP_REQUIRE(!P.delta_out || (a->mode == 1 && P.N2 == 128 && P.attn_out && P.Lq >= 1 && a->R % P.Lq == 0 && aligned16(P.attn_out)),
                 "%s: delta_out needs mode 1, n2 = 128, attn_out and lq dividing R", what);
  SPACAP_REQUIRE(P.nparts >= 0 && (P.nparts == 0 || P.A1), "%s: nparts = %d needs the partial sums in a1", what, P.nparts);
  const bool bwd = a->mode == 1;
  if (P.A1 && P.nparts == 0) SPACAP_REQUIRE(P.W1 && P.K1 >= 128 && P.K1 % 128 == 0, "%s: first product needs weights and K1 a multiple of 128 (K1=%d)", what, P.K1);
  SPACAP_REQUIRE(P.ln_a && (bwd || P.ln_b), "%s: LayerNorm parameters missing", what);
  if (!bwd) {
    SPACAP_REQUIRE(P.res, "%s: forward needs the residual rows", what);
    SPACAP_REQUIRE(P.N2 == 0 || (P.N2 % 128 == 0 && P.W2 && P.out2), "%s: N2=%d unsupported (multiple of 128) or null pointer", what, P.N2);
  } else {
    SPACAP_REQUIRE(P.A1 || P.G, "%s: backward needs a1 or g", what);
    SPACAP_REQUIRE(P.x_ln && P.stats && P.x_out && P.part, "%s: backward needs x_ln, stats, x_out (dx) and part", what);
    SPACAP_REQUIRE(P.N2 == 0 || (P.N2 == 128 && P.W2 && P.out2), "%s: backward N2 must be 0 or 128", what);
  }
  SPACAP_REQUIRE(aligned16(P.A1, P.W1, P.bias1, P.res, P.x_out, P.ln_a, P.ln_b, P.n_out, P.x_ln, P.G, P.W2, P.bias2, P.out2),
                 "%s: pointers must be 16-byte aligned", what);
  const long tiles = (P.R + BM - 1) / BM;
  SPACAP_REQUIRE(tiles <= 2147483647L, "%s: too many rows", what);
  hipStream_t s = spacap::as_stream(stream);
  // forward, N2 = 384 (the next attention's packed q|k|v) on FEW row tiles (the decoder's 8 x ~30 tokens = 16 tiles): its three
  // 128-column blocks on three workgroups per row tile -- 17 -> 11 us per launch there; with the encoder's 128 row tiles the
  // repeated first part costs what the shorter second part saves (measured 17.5 us both ways), so those stay one workgroup
  const unsigned ny = (!bwd && P.N2 > 128 && tiles <= 64) ? (unsigned)(P.N2 / 128) : 1u;
  if (bwd) hipLaunchKernelGGL((tf_rows_kernel<true>), dim3((unsigned)tiles), dim3(256), 0, s, P);
  else hipLaunchKernelGGL((tf_rows_kernel<false>), dim3((unsigned)tiles, ny), dim3(256), 0, s, P);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_tf_rows_parts(long R) { return (int)((R + BM - 1) / BM); }

extern "C" int spacap_tf_ffn1_f32(const float *x, const float *W, const float *bias, long R, int N, float drop_p, uint64_t seed,
                                  const uint64_t *seed_dev, float *h, spacap_stream_t stream) {
  const char *what = "spacap_tf_ffn1_f32";
  TfGemmArgs P = {};
  SPACAP_REQUIRE(R >= 0 && N >= 128 && N % 128 == 0 && drop_params(drop_p, P.thresh, P.scale), "%s: (R=%ld, N=%d, p=%f) unsupported",
                 what, R, N, (double)drop_p);
  if (R == 0) return SPACAP_OK;
  SPACAP_REQUIRE(x && W && h && aligned16(x, W, bias, h), "%s: null or unaligned pointer", what);
  P.x = x, P.W = W, P.bias = bias, P.out = h, P.R = R, P.ldx = D, P.ldw = D, P.N = N, P.KS = D;
  P.seed = seed, P.seed_dev = reinterpret_cast<const unsigned long long *>(seed_dev);
  return launch_gemm<1>(what, P, false, R, N, 1, spacap::as_stream(stream));
}

// mode 0: hid = dropout(relu(x Wa^T + bias)) [R,dff] (Wa = w_1 [dff,128]), part[c] = hid[:, c] Wb[:, c]^T (Wb = w_2 [128,dff]);
// mode 1: hid = (x Wa[:, c]) * [y > 0] / (1 - p) (Wa = w_2, y = the saved forward hid), part[c] = hid[:, c] Wb[c] (Wb = w_1).
extern "C" int spacap_tf_ffn_f32(int mode, const float *x, const float *Wa, const float *Wb, const float *bias, const float *y, long R,
                                 int dff, float drop_p, uint64_t seed, const uint64_t *seed_dev, float *hid, float *part,
                                 spacap_stream_t stream) {
  const char *what = "spacap_tf_ffn_f32";
  TfFfnArgs P = {};
  SPACAP_REQUIRE((mode == 0 || mode == 1) && R >= 0 && dff >= 128 && dff % 128 == 0 && drop_params(drop_p, P.thresh, P.scale),
                 "%s: (mode=%d, R=%ld, dff=%d, p=%f) unsupported", what, mode, R, dff, (double)drop_p);
  if (R == 0) return SPACAP_OK;
  SPACAP_REQUIRE(x && Wa && Wb && (hid || mode == 0) && part && (mode == 0 || y) && aligned16(x, Wa, Wb, bias, y, hid, part), "%s: null or unaligned pointer", what);
  P.x = x, P.Wa = Wa, P.Wb = Wb, P.bias = bias, P.y = y, P.hid = hid, P.part = part, P.R = R, P.dff = dff;
  P.seed = seed, P.seed_dev = reinterpret_cast<const unsigned long long *>(seed_dev);
  const bool small = R <= 512;   // few rows: 16-row tiles, so that the launch still has a few hundred workgroups
  const long tiles = small ? (R + 15) / 16 : (R + 63) / 64;
  SPACAP_REQUIRE(tiles <= 2147483647L, "%s: too many rows", what);
  const dim3 grid((unsigned)tiles, dff / 128);
  hipStream_t s = spacap::as_stream(stream);
  if (mode == 0) {
    if (small) hipLaunchKernelGGL((tf_ffn_kernel<false, 1>), grid, dim3(256), 0, s, P);
    else hipLaunchKernelGGL((tf_ffn_kernel<false, 4>), grid, dim3(256), 0, s, P);
  } else {
    if (small) hipLaunchKernelGGL((tf_ffn_kernel<true, 1>), grid, dim3(256), 0, s, P);
    else hipLaunchKernelGGL((tf_ffn_kernel<true, 4>), grid, dim3(256), 0, s, P);
  }
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

/* bf16 elements of the piece images of ONE feed-forward layer (four images of 3 dff 128 elements, see tf_ffn_split_kernel) */
extern "C" long spacap_tf_ffn_pieces_elems(int dff) { return dff >= 128 && dff % 128 == 0 ? 4L * 3 * dff * D : 0; }
/* pieces[l] (device, spacap_tf_ffn_pieces_elems(dff) bf16 elements each) <- the split images of w1[l] f32 [dff,128], w2[l] f32 [128,dff];
   the pointer arrays are HOST arrays, read before the call returns; one launch per 16 layers. */
extern "C" int spacap_tf_ffn_split_f32(const float *const *w1, const float *const *w2, void *const *pieces, int nlayers, int dff,
                                       spacap_stream_t stream) {
  const char *what = "spacap_tf_ffn_split_f32";
  SPACAP_REQUIRE(nlayers >= 0 && dff >= 128 && dff % 128 == 0 && (nlayers == 0 || (w1 && w2 && pieces)), "%s: bad arguments", what);
  hipStream_t s = spacap::as_stream(stream);
  for (int l0 = 0; l0 < nlayers; l0 += FF_SPLIT_MAX) {
    FfSplitTable T;
    T.nlayers = std::min(FF_SPLIT_MAX, nlayers - l0), T.dff = dff;
    for (int l = 0; l < T.nlayers; ++l) {
      SPACAP_REQUIRE(w1[l0 + l] && w2[l0 + l] && pieces[l0 + l], "%s: null pointer (layer %d)", what, l0 + l);
      T.w1[l] = w1[l0 + l], T.w2[l] = w2[l0 + l], T.out[l] = static_cast<__bf16 *>(pieces[l0 + l]);
    }
    hipLaunchKernelGGL(tf_ffn_split_kernel, dim3((unsigned)((size_t)dff * D / 256), T.nlayers), dim3(256), 0, s, T);
  }
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
/* spacap_tf_ffn_f32 on split-bf16 products (fp32-equivalent), for R > 512 rows: `pieces` = the layer's images from
   spacap_tf_ffn_split_f32 (mode 0 reads the W1 / W2 images, mode 1 the transposed ones); everything else as spacap_tf_ffn_f32. */
extern "C" int spacap_tf_ffn_bf3_f32(int mode, const float *x, const void *pieces, const float *bias, const float *y, long R, int dff,
                                     float drop_p, uint64_t seed, const uint64_t *seed_dev, float *hid, float *part, spacap_stream_t stream) {
  const char *what = "spacap_tf_ffn_bf3_f32";
  TfFfnBf3Args P = {};
  SPACAP_REQUIRE((mode == 0 || mode == 1) && R >= 0 && dff >= 128 && dff % 128 == 0 && drop_params(drop_p, P.thresh, P.scale),
                 "%s: (mode=%d, R=%ld, dff=%d, p=%f) unsupported", what, mode, R, dff, (double)drop_p);
  if (R == 0) return SPACAP_OK;
  SPACAP_REQUIRE(x && pieces && (hid || mode == 0) && part && (mode == 0 || y) && aligned16(x, pieces, bias, y, hid, part), "%s: null or unaligned pointer", what);
  const size_t img = (size_t)3 * dff * D;
  const __bf16 *pc = static_cast<const __bf16 *>(pieces);
  P.x = x, P.bias = bias, P.y = y, P.hid = hid, P.part = part, P.R = R, P.dff = dff;
  P.Wa = pc + (mode == 0 ? 0 : 2) * img, P.Wb = pc + (mode == 0 ? 1 : 3) * img;
  P.seed = seed, P.seed_dev = reinterpret_cast<const unsigned long long *>(seed_dev);
  const long tiles = (R + 63) / 64;
  SPACAP_REQUIRE(tiles * (dff / 128) <= 2147483647L, "%s: too many rows", what);
  const dim3 grid((unsigned)(tiles * (dff / 128)));
  hipStream_t s = spacap::as_stream(stream);
  if (mode == 0) hipLaunchKernelGGL((tf_ffn_bf3_kernel<false>), grid, dim3(256), 0, s, P);
  else hipLaunchKernelGGL((tf_ffn_bf3_kernel<true>), grid, dim3(256), 0, s, P);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// number of K slices that fills the chip with 64 x 128 tiles (a divisor of K / 128)
extern "C" int spacap_tf_gemm_splits(long R, int K, int N) {
  if (R < 1 || K < 128 || K % 128 || N < 128 || N % 128) return 0;
  const long tiles = ((R + FM - 1) / FM) * (N / 128);
  const int chunks = K / 128;
  long want = 512 / tiles;
  if (want < 1) want = 1;
  int best = 1;
  for (int sidx = 1; sidx <= chunks; ++sidx)
    if (chunks % sidx == 0 && sidx <= want) best = sidx;
  return best;
}

extern "C" int spacap_tf_gemm_f32(const float *a, const float *W, long R, int K, int N, int trans_w, int nsplit, float *out,
                                  spacap_stream_t stream) {
  const char *what = "spacap_tf_gemm_f32";
  SPACAP_REQUIRE(R >= 0 && K >= 128 && K % 128 == 0 && N >= 128 && N % 128 == 0 && nsplit >= 1 && (K / 128) % nsplit == 0,
                 "%s: (R=%ld, K=%d, N=%d, nsplit=%d) unsupported", what, R, K, N, nsplit);
  if (R == 0) return SPACAP_OK;
  SPACAP_REQUIRE(a && W && out && aligned16(a, W, out), "%s: null or unaligned pointer", what);
  TfGemmArgs P = {};
  P.x = a, P.W = W, P.out = out, P.R = R, P.ldx = K, P.ldw = trans_w ? K : N, P.N = N, P.KS = K / nsplit;
  return launch_gemm<0>(what, P, !trans_w, R, N, nsplit, spacap::as_stream(stream));
}

extern "C" int spacap_tf_dgrad_mask_f32(const float *g, const float *W, const float *y, float scale, long R, int K, int N,
                                        float *out, spacap_stream_t stream) {
  const char *what = "spacap_tf_dgrad_mask_f32";
  SPACAP_REQUIRE(R >= 0 && K == 128 && N >= 128 && N % 128 == 0, "%s: (R=%ld, K=%d, N=%d) unsupported", what, R, K, N);
  if (R == 0) return SPACAP_OK;
  SPACAP_REQUIRE(g && W && y && out && aligned16(g, W, y, out), "%s: null or unaligned pointer", what);
  TfGemmArgs P = {};
  P.x = g, P.W = W, P.y = y, P.out = out, P.R = R, P.ldx = K, P.ldw = N, P.N = N, P.KS = K, P.scale = scale;
  return launch_gemm<2>(what, P, true, R, N, 1, spacap::as_stream(stream));
}
