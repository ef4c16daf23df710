// Fused multi-head attention for gfx950 (MI355X): forward, and a deterministic two-kernel backward.
//
// Replaces the reference's Python `attention()` (models/transformer_captioner.py:27-37)
//     scores = Q K^T / sqrt(d_k);  scores.masked_fill(mask == 0, -1e9);  p = softmax(scores, -1);
//     p = dropout(p);  return p V, p
// which runs as two batched matmuls and four elementwise kernels that stream the (B,h,L,L) score matrix
// through HBM at least four times.  Here a 16-row tile of one (scene, head) is owned by W wavefronts: the
// logits, the softmax and the P V product live in registers; P is written once, and only if asked for.
//
// Matrix cores: v_mfma_f32_16x16x4_f32 (fp32 in / fp32 accumulate, bit-exact fmaf chain).  The model's
// parity bar is 1e-3 on the attention LOGITS (BASELINE.json north_star); single-pass bf16 inputs miss
// it by 15x on this model, and at d_k = 16, L <= 512 the kernel is bound by launch
// latency and the P write, not by the matrix pipe, so the exact fp32 MFMA costs nothing measurable.
//
// Register-resident dataflow (no transposes): the logits are produced TRANSPOSED, S^T = K Q^T,
// so that in the C/D layout of the 16x16 MFMA (col = lane & 15, row = 4 * (lane >> 4) + reg) the query is on
// the lane and the keys run over registers.  A register of that accumulator is then directly the A operand
// (A[row = lane & 15][k = lane >> 4]) of the next product that sums over keys -- P V in forward, dS K in
// backward -- provided the B operand is fetched with the same key permutation
// (k-step (t, r) covers keys 16 t + 4 * (lane >> 4) + r).
//
// Backward: kernel A (16 queries per tile) recomputes P from the saved row statistics, forms
// dS = P o (dP - delta) and dQ, and stores delta; kernel B (16 keys per tile) recomputes the same tiles
// in the un-transposed orientation and accumulates dK and dV over all queries in registers -- no atomics,
// bitwise reproducible (the reference's backward is deterministic too).
//
// The forward (mha_fwd_kernel itself) and dQ (bwd_dq_body) have one body each at two widths W; dK / dV has one body per
// width (bwd_dkv_body, bwd_dkv4_body: see there for why), at the same two widths:
//   W = 1  (Lk <= 64, for dK / dV Lq <= 64): one wave owns the 16 rows and ALL of the other dimension; no LDS.
//   W = 4  (longer): at B*h = 64 and L = 256 one wave per tile is 1 024 wavefronts, one per SIMD, each a serial chain
//          over 16 tiles (40-65 us for 0.27 GFLOP).  The four waves of a workgroup share the 16 rows and split the other
//          dimension; row maxima / sums / delta / partial products are combined through LDS in the fixed order
//          (a + b) + (c + d) (deterministic), identical arithmetic per element.
// What exists only for W = 4 sits under `if constexpr (W > 1)`.  The two widths also differ in the order in which one MFMA
// sums the channels of a dot product (fetch4): that order is part of the result and stays per width.
#include <math.h>

#include "common.hpp"
#include "dropout.hpp"
#include "mfma.hpp"

namespace {

using namespace spacap;
using spacap::mfma::f32x4;

struct MhaArgs {
  const float *q, *k, *v;
  long q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, v_sb, v_sh, v_sl;
  const uint8_t *mask;
  long mask_sb, mask_sq;
  const float *bias;
  long bias_sb, bias_sh, bias_sq;
  int B, h, Lq, Lk;
  float scale, keep_scale;  // keep_scale = 1 / (1 - p)
  unsigned drop_thresh;     // drop iff hash < drop_thresh ; 0 = no dropout
  unsigned long long seed;
  const unsigned long long *seed_dev;  // optional device-resident word added to `seed` (hipGraph replays)
  float *out, *p_out, *stats;       // forward outputs
  const float *d_out, *d_p;         // backward inputs
  float *dq, *dk, *dv, *delta;      // backward outputs / scratch
  long g_sl;                        // row stride (floats) of dq / dk / dv: h * d_k when dense
  int vec;                          // q / k / v rows are 16-byte aligned (bases and strides): operands by 16-byte loads
  int dvec;                         // the same for the rows of d_out (dense: its base decides)
};

// Dropout keep decision of element (b, head, q, key): the counter hash of dropout.hpp over the flat index into p, the
// same in forward and backward.  The seed is formed once per kernel (make_seed): a 64-bit splitmix finaliser per element
// cost ~10 us of VALU time in each of the three kernels of an encoder layer.
__device__ __forceinline__ bool keep_elem(const MhaArgs &A, DropSeed sd, int b, int hh, int q, int key) {
  if (A.drop_thresh == 0u) return true;
  const unsigned long long idx = (((unsigned long long)b * A.h + hh) * A.Lq + q) * (unsigned long long)A.Lk + key;
  return hash32(idx, sd) >= A.drop_thresh;
}

// the mask bytes of 4 consecutive keys of one query as one 32-bit load where the row allows it (else 4 byte loads):
// byte r = mask of key0 + r; 0xff.. for positions past Lk (those logits are -inf anyway)
__device__ __forceinline__ unsigned mask4(const MhaArgs &A, int b, int qc, int key0) {
  if (!A.mask) return 0x01010101u;
  const uint8_t *m = A.mask + b * A.mask_sb + qc * A.mask_sq;
  if (key0 + 3 < A.Lk && ((reinterpret_cast<uintptr_t>(m) + key0) & 3) == 0) return *reinterpret_cast<const unsigned *>(m + key0);
  unsigned r = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) r |= (unsigned)m[key0 + i < A.Lk ? key0 + i : A.Lk - 1] << (8 * i);
  return r;
}

// logit of (q, key) from the raw dot product: scale, optional bias, key mask (-1e9; `mbyte` = the mask byte of the element),
// padding (-inf)
__device__ __forceinline__ float logit(const MhaArgs &A, float dot, int b, int hh, int q, int key, unsigned mbyte, bool &masked) {
  float s = dot * A.scale;
  if (A.bias) {
    const int qc = q < A.Lq ? q : A.Lq - 1, kc = key < A.Lk ? key : A.Lk - 1;
    s += A.bias[b * A.bias_sb + hh * A.bias_sh + qc * A.bias_sq + kc];
  }
  masked = false;
  if (A.mask && mbyte == 0) {
    s = -1e9f;
    masked = true;
  }
  if (key >= A.Lk) s = -INFINITY;
  return s;
}

// The same for one element whose mask byte is read here (dK / dV: the four elements of a lane are four queries of one key).
// Stated a second time on purpose: written as a call of logit() with the loaded byte, the compiler schedules
// mha_bwd_both_kernel<2, 16, 1> into 76 registers instead of 72 and the kernel loses a wave per SIMD.
__device__ __forceinline__ float logit_at(const MhaArgs &A, float dot, int b, int hh, int q, int key, bool &masked) {
  float s = dot * A.scale;
  const int qc = q < A.Lq ? q : A.Lq - 1;
  const int kc = key < A.Lk ? key : A.Lk - 1;
  if (A.bias) s += A.bias[b * A.bias_sb + hh * A.bias_sh + qc * A.bias_sq + kc];
  masked = false;
  if (A.mask && A.mask[b * A.mask_sb + qc * A.mask_sq + kc] == 0) {
    s = -1e9f;
    masked = true;
  }
  if (key >= A.Lk) s = -INFINITY;
  return s;
}

__device__ __forceinline__ f32x4 ldv(const float *p, int vec) {
  if (vec) return *reinterpret_cast<const f32x4 *>(p);
  return f32x4{p[0], p[1], p[2], p[3]};
}

// Four consecutive MFMA steps, 4 j .. 4 j + 3, of one row of q, k, v or d_out for lane group lg; a row is the DK / 16 of
// them in order of j.  One MFMA sums the channels its four lane groups hold, so the grouping is part of the result and each
// width keeps its own:
//   W = 1: step i covers channel 4 i + lg              (scalar loads; one MFMA sums {4 i, .., 4 i + 3})
//   W = 4: step (j, s) covers channel 16 j + 4 lg + s  (one 16-byte load where `vec`; sums {16 j + s, + 4, + 8, + 12})
// Both operands of a product are fetched at the same width, so either order pairs the channels correctly.
template <int W>
__device__ __forceinline__ f32x4 fetch4(const float *p, int j, int lg, int vec) {
  if constexpr (W > 1) return ldv(p + 16 * j + 4 * lg, vec);
  else return f32x4{p[16 * j + lg], p[16 * j + 4 + lg], p[16 * j + 8 + lg], p[16 * j + 12 + lg]};
}

// A finished 16 x DK accumulator tile (row 4 lg + rr, column 16 db + lq in acc[db][rr]):
// W = 1: straight to memory, rows below `nrows`, row stride `rs` floats
template <int DK>
__device__ __forceinline__ void store_tile(const f32x4 (&acc)[DK / 16], float *dst, long rs, int nrows, int lq, int lg) {
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    if (4 * lg + rr < nrows) {
#pragma unroll
      for (int db = 0; db < DK / 16; ++db) dst[(4 * lg + rr) * rs + 16 * db + lq] = acc[db][rr];
    }
  }
}
// W = 4: this wave's partial tile into its LDS slab, and the four slabs summed in the fixed order
template <int DK>
__device__ __forceinline__ void park_tile(const f32x4 (&acc)[DK / 16], float (&slab)[16][DK + 1], int lq, int lg) {
#pragma unroll
  for (int rr = 0; rr < 4; ++rr)
#pragma unroll
    for (int db = 0; db < DK / 16; ++db) slab[4 * lg + rr][16 * db + lq] = acc[db][rr];
}
template <int DK>
__device__ __forceinline__ float sum4(const float (&s)[4][16][DK + 1], int row, int d) {
  return (s[0][row][d] + s[1][row][d]) + (s[2][row][d] + s[3][row][d]);
}

// ------------------------------------------------------------------------------------------------
// forward: 16 queries x all keys of one (b, head).  W = 1: one wave per tile, four independent tiles per workgroup;
// W = 4: the four waves of a workgroup take NT key tiles each.  (Nothing else calls this body, so it is the kernel: behind a
// one-line wrapper <8, 64, 4> takes 132 registers instead of 128 and loses a wave per SIMD.)
// ------------------------------------------------------------------------------------------------
template <int NT, int DK, int W>
__global__ __launch_bounds__(256) void mha_fwd_kernel(const MhaArgs A) {
  const DropSeed sd = make_seed(A.seed, A.seed_dev);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.z, hh = blockIdx.y;
  const int q0 = (W > 1 ? blockIdx.x : blockIdx.x * 4 + wave) * 16;
  if (W == 1 && q0 >= A.Lq) return;
  const int w = W > 1 ? wave : 0, t0 = w * NT;   // this wave's first key tile
  const int lq = lane & 15, lg = lane >> 4;
  const int q = q0 + lq;                       // the query this lane carries in the S^T layout
  const int qc = q < A.Lq ? q : A.Lq - 1;

  const float *qp = A.q + b * A.q_sb + hh * A.q_sh + qc * A.q_sl;
  f32x4 qv[DK / 16];
#pragma unroll
  for (int j = 0; j < DK / 16; ++j) qv[j] = fetch4<W>(qp, j, lg, A.vec);

  f32x4 acc[NT];
  const float *kbase = A.k + b * A.k_sb + hh * A.k_sh;
#pragma unroll
  for (int tt = 0; tt < NT; ++tt) {
    const int t = t0 + tt;
    acc[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (16 * t < A.Lk) {
      const int key = 16 * t + lq;
      const float *kp = kbase + (key < A.Lk ? key : A.Lk - 1) * A.k_sl;
#pragma unroll
      for (int j = 0; j < DK / 16; ++j) {
        const f32x4 kv = fetch4<W>(kp, j, lg, A.vec);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[tt] = MFMA16(kv[s], qv[j][s], acc[tt]);
      }
    }
  }

  float m = -INFINITY;
#pragma unroll
  for (int tt = 0; tt < NT; ++tt) {
    const int key0 = 16 * (t0 + tt) + 4 * lg;
    const unsigned m4 = mask4(A, b, qc, key0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bool masked;
      acc[tt][r] = logit(A, acc[tt][r], b, hh, q, key0 + r, (m4 >> (8 * r)) & 0xffu, masked);
      m = fmaxf(m, acc[tt][r]);
    }
  }
  m = fmaxf(m, __shfl_xor(m, 16));
  m = fmaxf(m, __shfl_xor(m, 32));
  if constexpr (W > 1) {
    __shared__ float s_m[4][16];
    if (lg == 0) s_m[w][lq] = m;
    __syncthreads();
    m = fmaxf(fmaxf(s_m[0][lq], s_m[1][lq]), fmaxf(s_m[2][lq], s_m[3][lq]));
  }
  float l = 0.f;
#pragma unroll
  for (int tt = 0; tt < NT; ++tt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc[tt][r] = expf(acc[tt][r] - m);
      l += acc[tt][r];
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if constexpr (W > 1) {
    __shared__ float s_l[4][16];
    if (lg == 0) s_l[w][lq] = l;
    __syncthreads();
    l = (s_l[0][lq] + s_l[1][lq]) + (s_l[2][lq] + s_l[3][lq]);
  }
  if (w == 0 && lg == 0 && q < A.Lq) {
    float *st = A.stats + (((size_t)b * A.h + hh) * A.Lq + q) * 2;
    st[0] = m;
    st[1] = l;
  }
  const bool vec_ok = (A.Lk & 3) == 0;
  float *prow = A.p_out ? A.p_out + (((size_t)b * A.h + hh) * A.Lq + qc) * A.Lk : nullptr;
#pragma unroll
  for (int tt = 0; tt < NT; ++tt) {
    const int key0 = 16 * (t0 + tt) + 4 * lg;
    f32x4 p;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float pv = acc[tt][r] / l;
      if (!keep_elem(A, sd, b, hh, q, key0 + r)) pv = 0.f; else pv *= A.keep_scale;
      p[r] = pv;
    }
    acc[tt] = p;
    if (prow && q < A.Lq) {
      if (vec_ok) {
        if (key0 < A.Lk) *reinterpret_cast<f32x4 *>(prow + key0) = p;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (key0 + r < A.Lk) prow[key0 + r] = p[r];
      }
    }
  }

  // O = P V : A operand = a register of P^T, B operand = V[key(t, r, lane >> 4)][d = lane & 15]
  f32x4 o[DK / 16];
#pragma unroll
  for (int db = 0; db < DK / 16; ++db) o[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float *vbase = A.v + b * A.v_sb + hh * A.v_sh;
#pragma unroll
  for (int tt = 0; tt < NT; ++tt) {
    if (16 * (t0 + tt) < A.Lk) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * (t0 + tt) + 4 * lg + r;
        const float *vp = vbase + (key < A.Lk ? key : A.Lk - 1) * A.v_sl;
#pragma unroll
        for (int db = 0; db < DK / 16; ++db) o[db] = MFMA16(acc[tt][r], vp[16 * db + lq], o[db]);
      }
    }
  }
  float *orow = A.out + (((size_t)b * A.Lq + q0) * A.h + hh) * DK;
  if constexpr (W > 1) {
    __shared__ float s_o[4][16][DK + 1];
    park_tile<DK>(o, s_o[w], lq, lg);
    __syncthreads();
    for (int e = threadIdx.x; e < 16 * DK; e += 256) {
      const int qi = e / DK, d = e - qi * DK;
      if (q0 + qi < A.Lq) orow[(size_t)qi * A.h * DK + d] = sum4<DK>(s_o, qi, d);
    }
  } else {
    store_tile<DK>(o, orow, (long)A.h * DK, A.Lq - q0, lq, lg);
  }
}


// ------------------------------------------------------------------------------------------------
// backward A: dQ and delta.  One workgroup of W waves per 16 queries; each wave takes NT key tiles.
// ------------------------------------------------------------------------------------------------
// PRE: delta[b, head, q] = sum_k p d(p) was formed by the caller (= sum_d out d_out when no gradient arrives on p_attn
// itself): the dQ and the dK / dV halves are then independent and run as ONE launch (mha_bwd_both_kernel).
template <int NT, int DK, int W, bool PRE>
__device__ __forceinline__ void bwd_dq_body(const MhaArgs &A, int bx) {
  const DropSeed sd = make_seed(A.seed, A.seed_dev);
  const int lane = W > 1 ? threadIdx.x & 63 : threadIdx.x, w = W > 1 ? threadIdx.x >> 6 : 0;   // (W = 1: 64-thread workgroups)
  const int b = blockIdx.z, hh = blockIdx.y;
  const int q0 = bx * 16;
  const int lq = lane & 15, lg = lane >> 4;
  const int q = q0 + lq;
  const int qc = q < A.Lq ? q : A.Lq - 1;
  const int t0 = w * NT;

  const float *qp = A.q + b * A.q_sb + hh * A.q_sh + qc * A.q_sl;
  const float *dop = A.d_out + (((size_t)b * A.Lq + qc) * A.h + hh) * DK;
  f32x4 qv[DK / 16], dov[DK / 16];
#pragma unroll
  for (int j = 0; j < DK / 16; ++j) {
    qv[j] = fetch4<W>(qp, j, lg, A.vec);
    dov[j] = fetch4<W>(dop, j, lg, A.dvec);
  }
  const float *st = A.stats + (((size_t)b * A.h + hh) * A.Lq + qc) * 2;
  const float m = st[0], inv_l = 1.0f / st[1];

  f32x4 p[NT], dp[NT];
  const float *kbase = A.k + b * A.k_sb + hh * A.k_sh;
  const float *vbase = A.v + b * A.v_sb + hh * A.v_sh;
  const float *dprow = A.d_p ? A.d_p + (((size_t)b * A.h + hh) * A.Lq + qc) * A.Lk : nullptr;
  float delta = 0.f;
#pragma unroll
  for (int tt = 0; tt < NT; ++tt) {
    const int t = t0 + tt;
    p[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    dp[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (16 * t < A.Lk) {
      const int keyl = 16 * t + lq;
      const int kcl = keyl < A.Lk ? keyl : A.Lk - 1;
      const float *kp = kbase + kcl * A.k_sl;
      const float *vp = vbase + kcl * A.v_sl;
#pragma unroll
      for (int j = 0; j < DK / 16; ++j) {
        const f32x4 kv = fetch4<W>(kp, j, lg, A.vec), vv = fetch4<W>(vp, j, lg, A.vec);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          p[tt] = MFMA16(kv[s], qv[j][s], p[tt]);      // S^T  = K Q^T
          dp[tt] = MFMA16(vv[s], dov[j][s], dp[tt]);   // dPd^T = V dO^T
        }
      }
      const unsigned m4 = mask4(A, b, qc, 16 * t + 4 * lg);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * t + 4 * lg + r;
        bool masked;
        const float s = logit(A, p[tt][r], b, hh, q, key, (m4 >> (8 * r)) & 0xffu, masked);
        const float pr = (key < A.Lk) ? expf(s - m) * inv_l : 0.f;
        float g = dp[tt][r];
        if (dprow && key < A.Lk) g += dprow[key];
        g = keep_elem(A, sd, b, hh, q, key) ? g * A.keep_scale : 0.f;  // dP (pre-dropout)
        delta += g * pr;
        p[tt][r] = pr;
        dp[tt][r] = (masked || key >= A.Lk) ? NAN : g;  // NaN marks "no gradient to the logit"
      }
    }
  }
  if (PRE) {
    delta = A.delta[((size_t)b * A.h + hh) * A.Lq + qc];
  } else {
    delta += __shfl_xor(delta, 16);
    delta += __shfl_xor(delta, 32);
    if constexpr (W > 1) {
      __shared__ float s_d[4][16];
      if (lg == 0) s_d[w][lq] = delta;
      __syncthreads();
      delta = (s_d[0][lq] + s_d[1][lq]) + (s_d[2][lq] + s_d[3][lq]);
    }
    if (w == 0 && lg == 0 && q < A.Lq) A.delta[((size_t)b * A.h + hh) * A.Lq + q] = delta;
  }

  f32x4 dq[DK / 16];
#pragma unroll
  for (int db = 0; db < DK / 16; ++db) dq[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int tt = 0; tt < NT; ++tt) {
    const int t = t0 + tt;
    if (16 * t < A.Lk) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * t + 4 * lg + r;
        const float g = dp[tt][r];
        const float ds = (g != g) ? 0.f : p[tt][r] * (g - delta) * A.scale;
        const float *kp = kbase + (key < A.Lk ? key : A.Lk - 1) * A.k_sl;
#pragma unroll
        for (int db = 0; db < DK / 16; ++db) dq[db] = MFMA16(ds, kp[16 * db + lq], dq[db]);
      }
    }
  }
  float *orow = A.dq + ((size_t)b * A.Lq + q0) * A.g_sl + hh * DK;
  if constexpr (W > 1) {
    __shared__ float s_o[4][16][DK + 1];
    park_tile<DK>(dq, s_o[w], lq, lg);
    __syncthreads();
    for (int e = threadIdx.x; e < 16 * DK; e += 256) {
      const int qi = e / DK, d = e - qi * DK;
      if (q0 + qi < A.Lq) orow[qi * A.g_sl + d] = sum4<DK>(s_o, qi, d);
    }
  } else {
    store_tile<DK>(dq, orow, A.g_sl, A.Lq - q0, lq, lg);
  }
}

template <int NT, int DK, int W>
__global__ __launch_bounds__(64 * W) void mha_bwd_dq_kernel(const MhaArgs A) {
  bwd_dq_body<NT, DK, W, false>(A, blockIdx.x);
}

// ------------------------------------------------------------------------------------------------
// backward B: dK and dV.  One workgroup of W waves per 16 keys, loops over query tiles; S (not S^T) orientation so the
// accumulator registers are again directly the A operands of the products that sum over queries.
//
// This role keeps one body per width.  Folded into one body (as the forward and dQ are) the same arithmetic was scheduled
// another way: the four-wave kernel ran 2.5 - 5 % slower at d_k = 32, and inside mha_bwd_both_kernel<2, 16, 1> the one-wave
// half took 80 registers instead of 72 (7 -> 6 waves per SIMD); no single formulation held the registers and the times of
// both widths at d_k 16, 32 and 64.  The two bodies differ as the widths do (fetch order, query-tile stride, LDS combine) and
// in three loads: the four-wave body reads row statistics and delta as 16-byte vectors and a key mask once per key.
// ------------------------------------------------------------------------------------------------
// W = 1: one wave per 16 keys, all query tiles
template <int DK>
__device__ __forceinline__ void bwd_dkv_body(const MhaArgs &A, int bx) {
  const DropSeed sd = make_seed(A.seed, A.seed_dev);
  const int lane = threadIdx.x;
  const int b = blockIdx.z, hh = blockIdx.y;
  const int key0 = bx * 16;
  const int lq = lane & 15, lg = lane >> 4;
  const int key = key0 + lq;  // the key this lane carries (C-layout column)
  const int kc = key < A.Lk ? key : A.Lk - 1;

  const float *kp = A.k + b * A.k_sb + hh * A.k_sh + kc * A.k_sl;
  const float *vp = A.v + b * A.v_sb + hh * A.v_sh + kc * A.v_sl;
  float kreg[DK / 4], vreg[DK / 4];
#pragma unroll
  for (int s = 0; s < DK / 4; ++s) {
    kreg[s] = kp[4 * s + lg];
    vreg[s] = vp[4 * s + lg];
  }
  f32x4 dk[DK / 16], dv[DK / 16];
#pragma unroll
  for (int db = 0; db < DK / 16; ++db) {
    dk[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
    dv[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const float *qbase = A.q + b * A.q_sb + hh * A.q_sh;
  const float *stb = A.stats + ((size_t)b * A.h + hh) * A.Lq * 2;
  const float *delb = A.delta + ((size_t)b * A.h + hh) * A.Lq;

  for (int qt = 0; qt * 16 < A.Lq; ++qt) {
    const int qa = qt * 16 + lq;
    const int qac = qa < A.Lq ? qa : A.Lq - 1;
    const float *qp = qbase + qac * A.q_sl;
    const float *dop = A.d_out + (((size_t)b * A.Lq + qac) * A.h + hh) * DK;
    f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, g4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < DK / 4; ++s) {
      s4 = MFMA16(qp[4 * s + lg], kreg[s], s4);    // S   = Q K^T   : C[q = 4 lg + r][key = lq]
      g4 = MFMA16(dop[4 * s + lg], vreg[s], g4);   // dPd = dO V^T
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = qt * 16 + 4 * lg + r;
      const int qc = q < A.Lq ? q : A.Lq - 1;
      const bool valid = (q < A.Lq) && (key < A.Lk);
      bool masked;
      const float s = logit_at(A, s4[r], b, hh, q, key, masked);
      const float pr = valid ? expf(s - stb[qc * 2]) / stb[qc * 2 + 1] : 0.f;
      float g = g4[r];
      if (A.d_p && valid) g += A.d_p[(((size_t)b * A.h + hh) * A.Lq + qc) * A.Lk + kc];
      const bool keep = keep_elem(A, sd, b, hh, q, key);
      g = keep ? g * A.keep_scale : 0.f;
      const float pd = keep ? pr * A.keep_scale : 0.f;
      const float ds = (masked || !valid) ? 0.f : pr * (g - delb[qc]) * A.scale;
      const float *qr = qbase + qc * A.q_sl;
      const float *dor = A.d_out + (((size_t)b * A.Lq + qc) * A.h + hh) * DK;
#pragma unroll
      for (int db = 0; db < DK / 16; ++db) {
        dk[db] = MFMA16(ds, qr[16 * db + lq], dk[db]);
        dv[db] = MFMA16(valid ? pd : 0.f, dor[16 * db + lq], dv[db]);
      }
    }
  }
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int ko = key0 + 4 * lg + rr;
    if (ko < A.Lk) {
      float *okp = A.dk + ((size_t)b * A.Lk + ko) * A.g_sl + hh * DK;
      float *ovp = A.dv + ((size_t)b * A.Lk + ko) * A.g_sl + hh * DK;
#pragma unroll
      for (int db = 0; db < DK / 16; ++db) {
        okp[16 * db + lq] = dk[db][rr];
        ovp[16 * db + lq] = dv[db][rr];
      }
    }
  }
}

// W = 4: 16 keys per workgroup, the query tiles interleaved over the 4 waves; partial dK / dV summed through LDS
template <int DK>
__device__ __forceinline__ void bwd_dkv4_body(const MhaArgs &A, int bx) {
  const DropSeed sd = make_seed(A.seed, A.seed_dev);
  __shared__ float s_k[4][16][DK + 1], s_v[4][16][DK + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.z, hh = blockIdx.y;
  const int key0 = bx * 16;
  const int lq = lane & 15, lg = lane >> 4;
  const int key = key0 + lq;
  const int kc = key < A.Lk ? key : A.Lk - 1;

  const float *kp = A.k + b * A.k_sb + hh * A.k_sh + kc * A.k_sl;
  const float *vp = A.v + b * A.v_sb + hh * A.v_sh + kc * A.v_sl;
  f32x4 kv[DK / 16], vv[DK / 16];   // (the steps of fetch4<4>)
#pragma unroll
  for (int j = 0; j < DK / 16; ++j) {
    kv[j] = ldv(kp + 16 * j + 4 * lg, A.vec);
    vv[j] = ldv(vp + 16 * j + 4 * lg, A.vec);
  }
  f32x4 dk[DK / 16], dv[DK / 16];
#pragma unroll
  for (int db = 0; db < DK / 16; ++db) {
    dk[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
    dv[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const float *qbase = A.q + b * A.q_sb + hh * A.q_sh;
  const float *stb = A.stats + ((size_t)b * A.h + hh) * A.Lq * 2;
  const float *delb = A.delta + ((size_t)b * A.h + hh) * A.Lq;

  for (int qt = w; qt * 16 < A.Lq; qt += 4) {
    const int qa = qt * 16 + lq;
    const int qac = qa < A.Lq ? qa : A.Lq - 1;
    const float *qp = qbase + qac * A.q_sl;
    const float *dop = A.d_out + (((size_t)b * A.Lq + qac) * A.h + hh) * DK;
    f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, g4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < DK / 16; ++j) {
      const f32x4 qq = ldv(qp + 16 * j + 4 * lg, A.vec), dd = ldv(dop + 16 * j + 4 * lg, A.dvec);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        s4 = MFMA16(qq[s], kv[j][s], s4);
        g4 = MFMA16(dd[s], vv[j][s], g4);
      }
    }
    // the four queries of this lane are consecutive: their row statistics and delta as 16-byte loads when the tile is whole
    const int qb = qt * 16 + 4 * lg;
    const bool whole = qb + 3 < A.Lq && (A.Lq & 3) == 0;
    f32x4 st0 = {0.f, 0.f, 0.f, 0.f}, st1 = st0, dl4 = st0;
    if (whole) {
      st0 = *reinterpret_cast<const f32x4 *>(stb + qb * 2);
      st1 = *reinterpret_cast<const f32x4 *>(stb + qb * 2 + 4);
      dl4 = *reinterpret_cast<const f32x4 *>(delb + qb);
    }
    const unsigned mkey = (A.mask && A.mask_sq == 0) ? A.mask[b * A.mask_sb + kc] : 1u;   // key mask: the same for every query
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = qt * 16 + 4 * lg + r;
      const int qc = q < A.Lq ? q : A.Lq - 1;
      const bool valid = (q < A.Lq) && (key < A.Lk);
      bool masked;
      const float rm = whole ? (r < 2 ? st0[2 * r] : st1[2 * r - 4]) : stb[qc * 2];
      const float rl = whole ? (r < 2 ? st0[2 * r + 1] : st1[2 * r - 3]) : stb[qc * 2 + 1];
      const float dlt = whole ? dl4[r] : delb[qc];
      const float s = (A.mask && A.mask_sq != 0) ? logit_at(A, s4[r], b, hh, q, key, masked) : logit(A, s4[r], b, hh, q, key, mkey, masked);
      const float pr = valid ? expf(s - rm) / rl : 0.f;
      float g = g4[r];
      if (A.d_p && valid) g += A.d_p[(((size_t)b * A.h + hh) * A.Lq + qc) * A.Lk + kc];
      const bool keep = keep_elem(A, sd, b, hh, q, key);
      g = keep ? g * A.keep_scale : 0.f;
      const float pd = keep ? pr * A.keep_scale : 0.f;
      const float ds = (masked || !valid) ? 0.f : pr * (g - dlt) * A.scale;
      const float *qr = qbase + qc * A.q_sl;
      const float *dor = A.d_out + (((size_t)b * A.Lq + qc) * A.h + hh) * DK;
#pragma unroll
      for (int db = 0; db < DK / 16; ++db) {
        dk[db] = MFMA16(ds, qr[16 * db + lq], dk[db]);
        dv[db] = MFMA16(valid ? pd : 0.f, dor[16 * db + lq], dv[db]);
      }
    }
  }
#pragma unroll
  for (int rr = 0; rr < 4; ++rr)
#pragma unroll
    for (int db = 0; db < DK / 16; ++db) {
      s_k[w][4 * lg + rr][16 * db + lq] = dk[db][rr];
      s_v[w][4 * lg + rr][16 * db + lq] = dv[db][rr];
    }
  __syncthreads();
  for (int e = threadIdx.x; e < 16 * DK; e += 256) {
    const int ki = e / DK, d = e - ki * DK;
    if (key0 + ki < A.Lk) {
      const size_t o = ((size_t)b * A.Lk + key0 + ki) * A.g_sl + hh * DK + d;
      A.dk[o] = (s_k[0][ki][d] + s_k[1][ki][d]) + (s_k[2][ki][d] + s_k[3][ki][d]);
      A.dv[o] = (s_v[0][ki][d] + s_v[1][ki][d]) + (s_v[2][ki][d] + s_v[3][ki][d]);
    }
  }
}

template <int DK, int W>
__device__ __forceinline__ void bwd_dkv(const MhaArgs &A, int bx) {
  if constexpr (W > 1) bwd_dkv4_body<DK>(A, bx);
  else bwd_dkv_body<DK>(A, bx);
}

template <int DK, int W>
__global__ __launch_bounds__(64 * W) void mha_bwd_dkv_kernel(const MhaArgs A) {
  bwd_dkv<DK, W>(A, blockIdx.x);
}

// both halves in one launch (delta precomputed): blocks [0, nqb) form dQ, the rest dK / dV
template <int NT, int DK, int W>
__global__ __launch_bounds__(64 * W) void mha_bwd_both_kernel(const MhaArgs A, int nqb) {
  if ((int)blockIdx.x < nqb) bwd_dq_body<NT, DK, W, true>(A, blockIdx.x);
  else bwd_dkv<DK, W>(A, (int)blockIdx.x - nqb);
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// The key-count ladder: Lk -> NT key tiles per wave and W waves per 16-query tile (Lk <= 16 NT W), handed to `f` as
// compile-time constants.
template <int NT_, int W_>
struct Tier {
  static constexpr int NT = NT_, W = W_;
};
template <class F>
void with_tier(int Lk, F &&f) {
  if (Lk <= 32) f(Tier<2, 1>{});
  else if (Lk <= 64) f(Tier<4, 1>{});
  else if (Lk <= 128) f(Tier<2, 4>{});
  else if (Lk <= 256) f(Tier<4, 4>{});
  else f(Tier<8, 4>{});
}
// dK / dV split the QUERY tiles over the waves of a workgroup: four waves above 64 queries
constexpr int kOneWaveRows = 64;

template <int DK>
void launch_fwd(const MhaArgs &A, hipStream_t s) {
  with_tier(A.Lk, [&](auto t) {
    using T = decltype(t);
    const int tiles = (A.Lq + 15) / 16;   // W = 1: four independent tiles per workgroup
    hipLaunchKernelGGL((mha_fwd_kernel<T::NT, DK, T::W>), dim3(T::W > 1 ? tiles : (tiles + 3) / 4, A.h, A.B), dim3(256), 0, s, A);
  });
}

// delta precomputed: ONE launch when both halves run at the same width (self-attention: Lq == Lk)
template <int DK>
bool launch_bwd_both(const MhaArgs &A, hipStream_t s) {
  if ((A.Lk > kOneWaveRows) != (A.Lq > kOneWaveRows)) return false;
  const int nqb = (A.Lq + 15) / 16, nkb = (A.Lk + 15) / 16;
  with_tier(A.Lk, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((mha_bwd_both_kernel<T::NT, DK, T::W>), dim3(nqb + nkb, A.h, A.B), dim3(64 * T::W), 0, s, A, nqb);
  });
  return true;
}

template <int DK>
void launch_bwd(const MhaArgs &A, hipStream_t s) {
  with_tier(A.Lk, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((mha_bwd_dq_kernel<T::NT, DK, T::W>), dim3((A.Lq + 15) / 16, A.h, A.B), dim3(64 * T::W), 0, s, A);
  });
  dim3 gk((A.Lk + 15) / 16, A.h, A.B);
  if (A.Lq <= kOneWaveRows) hipLaunchKernelGGL((mha_bwd_dkv_kernel<DK, 1>), gk, dim3(64), 0, s, A);
  else hipLaunchKernelGGL((mha_bwd_dkv_kernel<DK, 4>), gk, dim3(256), 0, s, A);
}

int fill_args(MhaArgs &A, const char *what, const float *q, const float *k, const float *v, long q_sb, long q_sh,
              long q_sl, long k_sb, long k_sh, long k_sl, long v_sb, long v_sh, long v_sl, const uint8_t *mask,
              long mask_sb, long mask_sq, const float *bias, long bias_sb, long bias_sh, long bias_sq, int B, int h,
              int Lq, int Lk, int d_k, float scale, float dropout_p, uint64_t seed, const uint64_t *seed_dev) {
  SPACAP_REQUIRE(B >= 0 && h >= 1 && Lq >= 0 && Lk >= 1, "%s: bad sizes B=%d h=%d Lq=%d Lk=%d", what, B, h, Lq, Lk);
  SPACAP_REQUIRE(d_k == 16 || d_k == 32 || d_k == 64, "%s: d_k=%d unsupported (16, 32, 64)", what, d_k);
  SPACAP_REQUIRE(Lk <= 512, "%s: Lk=%d > 512 unsupported", what, Lk);
  SPACAP_REQUIRE(h <= 65535 && B <= 65535, "%s: grid out of range", what);
  SPACAP_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "%s: dropout_p=%f out of [0,1)", what, dropout_p);
  SPACAP_REQUIRE(q && k && v, "%s: null pointer", what);
  A.q = q; A.k = k; A.v = v;
  A.q_sb = q_sb; A.q_sh = q_sh; A.q_sl = q_sl;
  A.k_sb = k_sb; A.k_sh = k_sh; A.k_sl = k_sl;
  A.v_sb = v_sb; A.v_sh = v_sh; A.v_sl = v_sl;
  A.mask = mask; A.mask_sb = mask_sb; A.mask_sq = mask_sq;
  A.bias = bias; A.bias_sb = bias_sb; A.bias_sh = bias_sh; A.bias_sq = bias_sq;
  A.B = B; A.h = h; A.Lq = Lq; A.Lk = Lk;
  A.scale = scale;
  drop_params(dropout_p, A.drop_thresh, A.keep_scale);
  A.seed = seed;
  A.seed_dev = reinterpret_cast<const unsigned long long *>(seed_dev);
  auto al = [](const void *p, long a, long b2, long c) {
    return aligned16(p) && a % 4 == 0 && b2 % 4 == 0 && c % 4 == 0;
  };
  A.vec = al(q, q_sb, q_sh, q_sl) && al(k, k_sb, k_sh, k_sl) && al(v, v_sb, v_sh, v_sl) ? 1 : 0;
  A.dvec = 0;
  A.out = A.p_out = A.stats = nullptr;
  A.d_out = A.d_p = nullptr;
  A.dq = A.dk = A.dv = A.delta = nullptr;
  return SPACAP_OK;
}

// What the two backward entry points share: the checks, the gradient row stride, the cases with nothing to launch (no
// scene; no query: dK = dV = 0) and the pointer fill.  `delta` is the workspace the dQ kernel fills or the caller's own.
// A.dq stays null where nothing is left to launch.
int fill_bwd_args(MhaArgs &A, const char *what, const float *q, const float *k, const float *v, long q_sb, long q_sh,
                  long q_sl, long k_sb, long k_sh, long k_sl, long v_sb, long v_sh, long v_sl, const uint8_t *mask,
                  long mask_sb, long mask_sq, const float *bias, long bias_sb, long bias_sh, long bias_sq, int B, int h,
                  int Lq, int Lk, int d_k, float scale, float dropout_p, uint64_t seed, const uint64_t *seed_dev,
                  const float *stats, const float *d_out, const float *d_p, float *delta, float *dq, float *dk,
                  float *dv, long grad_row_stride, hipStream_t s) {
  int rc = fill_args(A, what, q, k, v, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, v_sb, v_sh, v_sl, mask, mask_sb, mask_sq,
                     bias, bias_sb, bias_sh, bias_sq, B, h, Lq, Lk, d_k, scale, dropout_p, seed, seed_dev);
  if (rc) return rc;
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(dq && dk && dv, "%s: null output", what);
  SPACAP_REQUIRE(grad_row_stride == 0 || grad_row_stride >= (long)h * d_k, "%s: bad grad_row_stride", what);
  A.g_sl = grad_row_stride ? grad_row_stride : (long)h * d_k;
  if (Lq == 0) {
    SPACAP_REQUIRE(A.g_sl == (long)h * d_k, "%s: Lq == 0 needs dense gradients", what);
    SPACAP_CHECK_HIP(hipMemsetAsync(dk, 0, sizeof(float) * (size_t)B * Lk * h * d_k, s), what);
    SPACAP_CHECK_HIP(hipMemsetAsync(dv, 0, sizeof(float) * (size_t)B * Lk * h * d_k, s), what);
    return SPACAP_OK;
  }
  SPACAP_REQUIRE(stats && d_out && delta, "%s: null input", what);
  A.stats = const_cast<float *>(stats);
  A.d_out = d_out; A.d_p = d_p;
  A.dvec = aligned16(d_out) ? 1 : 0;
  A.dq = dq; A.dk = dk; A.dv = dv;
  A.delta = delta;
  return SPACAP_OK;
}

}  // namespace

extern "C" size_t spacap_mha_bwd_workspace_bytes(int B, int h, int Lq) {
  if (B <= 0 || h <= 0 || Lq <= 0) return 0;
  return (size_t)B * h * Lq * sizeof(float);
}

extern "C" int spacap_mha_fwd_f32(const float *q, const float *k, const float *v, long q_sb, long q_sh, long q_sl,
                                  long k_sb, long k_sh, long k_sl, long v_sb, long v_sh, long v_sl, const uint8_t *mask,
                                  long mask_sb, long mask_sq, const float *bias, long bias_sb, long bias_sh,
                                  long bias_sq, int B, int h, int Lq, int Lk, int d_k, float scale, float dropout_p,
                                  uint64_t seed, const uint64_t *seed_dev, float *out, float *p_out, float *stats,
                                  spacap_stream_t stream) {
  MhaArgs A;
  int rc = fill_args(A, "spacap_mha_fwd_f32", q, k, v, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, v_sb, v_sh, v_sl, mask,
                     mask_sb, mask_sq, bias, bias_sb, bias_sh, bias_sq, B, h, Lq, Lk, d_k, scale, dropout_p, seed,
                     seed_dev);
  if (rc) return rc;
  if (B == 0 || Lq == 0) return SPACAP_OK;
  SPACAP_REQUIRE(out && stats, "spacap_mha_fwd_f32: null output");
  A.out = out; A.p_out = p_out; A.stats = stats;
  hipStream_t s = spacap::as_stream(stream);
  if (d_k == 16) launch_fwd<16>(A, s);
  else if (d_k == 32) launch_fwd<32>(A, s);
  else launch_fwd<64>(A, s);
  SPACAP_CHECK_LAUNCH("spacap_mha_fwd_f32");
  return SPACAP_OK;
}

extern "C" int spacap_mha_bwd_f32(const float *q, const float *k, const float *v, long q_sb, long q_sh, long q_sl,
                                  long k_sb, long k_sh, long k_sl, long v_sb, long v_sh, long v_sl, const uint8_t *mask,
                                  long mask_sb, long mask_sq, const float *bias, long bias_sb, long bias_sh,
                                  long bias_sq, int B, int h, int Lq, int Lk, int d_k, float scale, float dropout_p,
                                  uint64_t seed, const uint64_t *seed_dev, const float *stats, const float *d_out,
                                  const float *d_p, void *workspace, float *dq, float *dk, float *dv,
                                  long grad_row_stride, spacap_stream_t stream) {
  const char *what = "spacap_mha_bwd_f32";
  hipStream_t s = spacap::as_stream(stream);
  MhaArgs A;
  int rc = fill_bwd_args(A, what, q, k, v, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, v_sb, v_sh, v_sl, mask, mask_sb, mask_sq,
                         bias, bias_sb, bias_sh, bias_sq, B, h, Lq, Lk, d_k, scale, dropout_p, seed, seed_dev, stats,
                         d_out, d_p, reinterpret_cast<float *>(workspace), dq, dk, dv, grad_row_stride, s);
  if (rc || !A.dq) return rc;
  if (d_k == 16) launch_bwd<16>(A, s);
  else if (d_k == 32) launch_bwd<32>(A, s);
  else launch_bwd<64>(A, s);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

/* As spacap_mha_bwd_f32 with delta[b, head, q] = sum_k p_attn d(p_attn) PRECOMPUTED by the caller (f32 [B,h,Lq]; without a
   gradient on p_attn itself it equals sum_d out[b,q,head,d] d_out[b,q,head,d]): the dQ and the dK / dV halves are then
   independent and run as one launch for self-attention shapes.  d_p must be NULL. */
extern "C" int spacap_mha_bwd_delta_f32(const float *q, const float *k, const float *v, long q_sb, long q_sh, long q_sl,
                                        long k_sb, long k_sh, long k_sl, long v_sb, long v_sh, long v_sl,
                                        const uint8_t *mask, long mask_sb, long mask_sq, const float *bias, long bias_sb,
                                        long bias_sh, long bias_sq, int B, int h, int Lq, int Lk, int d_k, float scale,
                                        float dropout_p, uint64_t seed, const uint64_t *seed_dev, const float *stats,
                                        const float *d_out, const float *delta, float *dq, float *dk, float *dv,
                                        long grad_row_stride, spacap_stream_t stream) {
  const char *what = "spacap_mha_bwd_delta_f32";
  hipStream_t s = spacap::as_stream(stream);
  MhaArgs A;
  int rc = fill_bwd_args(A, what, q, k, v, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, v_sb, v_sh, v_sl, mask, mask_sb, mask_sq,
                         bias, bias_sb, bias_sh, bias_sq, B, h, Lq, Lk, d_k, scale, dropout_p, seed, seed_dev, stats,
                         d_out, nullptr, const_cast<float *>(delta), dq, dk, dv, grad_row_stride, s);
  if (rc || !A.dq) return rc;
  const bool ok = d_k == 16 ? launch_bwd_both<16>(A, s) : d_k == 32 ? launch_bwd_both<32>(A, s) : launch_bwd_both<64>(A, s);
  SPACAP_REQUIRE(ok, "%s: (Lq=%d, Lk=%d) has no single-launch form (self-attention shapes only)", what, Lq, Lk);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
