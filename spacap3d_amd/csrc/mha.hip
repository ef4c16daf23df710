// Fused multi-head attention for gfx950 (MI355X): forward, and a deterministic two-kernel backward.
//
// Replaces the reference's Python `attention()` (models/transformer_captioner.py:27-37)
//     scores = Q K^T / sqrt(d_k);  scores.masked_fill(mask == 0, -1e9);  p = softmax(scores, -1);
//     p = dropout(p);  return p V, p
// which runs as two batched matmuls and four elementwise kernels that stream the (B,h,L,L) score matrix
// through HBM at least four times.  Here one wavefront owns 16 query rows of one (scene, head): the
// logits, the softmax and the P V product live in registers; P is written once, and only if asked for.
//
// Matrix cores: v_mfma_f32_16x16x4_f32 (fp32 in / fp32 accumulate, bit-exact fmaf chain).  The model's
// parity bar is 1e-3 on the attention LOGITS (BASELINE.json north_star); single-pass bf16 inputs miss
// it by 15x on this model, and at d_k = 16, L <= 512 the kernel is bound by launch
// latency and the P write, not by the matrix pipe, so the exact fp32 MFMA costs nothing measurable.
//
// Register-resident dataflow (no LDS, no transposes): the logits are produced TRANSPOSED, S^T = K Q^T,
// so that in the C/D layout of the 16x16 MFMA (col = lane & 15, row = 4 * (lane >> 4) + reg) the query is on
// the lane and the keys run over registers.  A register of that accumulator is then directly the A operand
// (A[row = lane & 15][k = lane >> 4]) of the next product that sums over keys -- P V in forward, dS K in
// backward -- provided the B operand is fetched with the same key permutation
// (k-step (t, r) covers keys 16 t + 4 * (lane >> 4) + r).
//
// Backward: kernel A (one wave per 16 queries) recomputes P from the saved row statistics, forms
// dS = P o (dP - delta) and dQ, and stores delta; kernel B (one wave per 16 keys) recomputes the same tiles
// in the un-transposed orientation and accumulates dK and dV over all queries in registers -- no atomics,
// bitwise reproducible (the reference's backward is deterministic too).
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

// logit of (q, key) from the raw dot product: scale, optional bias, key mask (-1e9), padding (-inf)
__device__ __forceinline__ float logit(const MhaArgs &A, float dot, int b, int hh, int q, int key, bool &masked) {
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

// the mask bytes of 4 consecutive keys of one query as one 32-bit load where the row allows it (else 4 byte loads):
// byte r = mask of key0 + r; 0xff.. for positions past Lk (those logits are -inf anyway)
static __device__ __forceinline__ unsigned mask4(const MhaArgs &A, int b, int qc, int key0) {
  if (!A.mask) return 0x01010101u;
  const uint8_t *m = A.mask + b * A.mask_sb + qc * A.mask_sq;
  if (key0 + 3 < A.Lk && ((reinterpret_cast<uintptr_t>(m) + key0) & 3) == 0) return *reinterpret_cast<const unsigned *>(m + key0);
  unsigned r = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) r |= (unsigned)m[key0 + i < A.Lk ? key0 + i : A.Lk - 1] << (8 * i);
  return r;
}
// logit with the mask byte handed in (see logit())
static __device__ __forceinline__ float logit_m(const MhaArgs &A, float dot, int b, int hh, int q, int key, unsigned mbyte, bool &masked) {
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
static __device__ __forceinline__ f32x4 ldv(const float *p, int vec) {
  if (vec) return *reinterpret_cast<const f32x4 *>(p);
  return f32x4{p[0], p[1], p[2], p[3]};
}

// ------------------------------------------------------------------------------------------------
// forward: one wave = 16 queries x all keys of one (b, head); 4 waves per workgroup
// ------------------------------------------------------------------------------------------------
template <int NT, int DK>
__global__ __launch_bounds__(256) void mha_fwd_kernel(const MhaArgs A) {
  const DropSeed sd = make_seed(A.seed, A.seed_dev);
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.z, hh = blockIdx.y;
  const int q0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
  if (q0 >= A.Lq) return;
  const int lq = lane & 15, lg = lane >> 4;
  const int q = q0 + lq;                       // the query this lane carries in the S^T layout
  const int qc = q < A.Lq ? q : A.Lq - 1;

  const float *qp = A.q + b * A.q_sb + hh * A.q_sh + qc * A.q_sl;
  float qreg[DK / 4];
#pragma unroll
  for (int s = 0; s < DK / 4; ++s) qreg[s] = qp[4 * s + lg];

  f32x4 acc[NT];
  const float *kbase = A.k + b * A.k_sb + hh * A.k_sh;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (16 * t < A.Lk) {
      const int key = 16 * t + lq;
      const float *kp = kbase + (key < A.Lk ? key : A.Lk - 1) * A.k_sl;
#pragma unroll
      for (int s = 0; s < DK / 4; ++s) acc[t] = MFMA16(kp[4 * s + lg], qreg[s], acc[t]);
    }
  }

  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bool masked;
      acc[t][r] = logit(A, acc[t][r], b, hh, q, 16 * t + 4 * lg + r, masked);
      m = fmaxf(m, acc[t][r]);
    }
  }
  m = fmaxf(m, __shfl_xor(m, 16));
  m = fmaxf(m, __shfl_xor(m, 32));
  float l = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc[t][r] = expf(acc[t][r] - m);
      l += acc[t][r];
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (lg == 0 && q < A.Lq) {
    float *st = A.stats + (((size_t)b * A.h + hh) * A.Lq + q) * 2;
    st[0] = m;
    st[1] = l;
  }
  const bool vec_ok = (A.Lk & 3) == 0;
  float *prow = A.p_out ? A.p_out + (((size_t)b * A.h + hh) * A.Lq + qc) * A.Lk : nullptr;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    f32x4 p;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float pv = acc[t][r] / l;
      if (!keep_elem(A, sd, b, hh, q, 16 * t + 4 * lg + r)) pv = 0.f; else pv *= A.keep_scale;
      p[r] = pv;
    }
    acc[t] = p;
    if (prow && q < A.Lq) {
      const int key = 16 * t + 4 * lg;
      if (vec_ok) {
        if (key < A.Lk) *reinterpret_cast<f32x4 *>(prow + key) = p;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (key + r < A.Lk) prow[key + r] = p[r];
      }
    }
  }

  // O = P V : A operand = a register of P^T, B operand = V[key(t, r, lane >> 4)][d = lane & 15]
  f32x4 o[DK / 16];
#pragma unroll
  for (int db = 0; db < DK / 16; ++db) o[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float *vbase = A.v + b * A.v_sb + hh * A.v_sh;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (16 * t < A.Lk) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * t + 4 * lg + r;
        const float *vp = vbase + (key < A.Lk ? key : A.Lk - 1) * A.v_sl;
#pragma unroll
        for (int db = 0; db < DK / 16; ++db) o[db] = MFMA16(acc[t][r], vp[16 * db + lq], o[db]);
      }
    }
  }
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int qo = q0 + 4 * lg + rr;
    if (qo < A.Lq) {
      float *op = A.out + (((size_t)b * A.Lq + qo) * A.h + hh) * DK;
#pragma unroll
      for (int db = 0; db < DK / 16; ++db) op[16 * db + lq] = o[db][rr];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// backward A: dQ and delta.  One wave (= one workgroup) per 16 queries.
// ------------------------------------------------------------------------------------------------
// PRE: delta[b, head, q] = sum_k p d(p) was formed by the caller (= sum_d out d_out when no gradient arrives on p_attn
// itself): the dQ and the dK / dV halves are then independent and run as ONE launch (mha_bwd_both_*).
template <int NT, int DK, bool PRE>
__device__ __forceinline__ void bwd_dq_body(const MhaArgs &A, int bx) {
  const DropSeed sd = make_seed(A.seed, A.seed_dev);
  const int lane = threadIdx.x;
  const int b = blockIdx.z, hh = blockIdx.y;
  const int q0 = bx * 16;
  const int lq = lane & 15, lg = lane >> 4;
  const int q = q0 + lq;
  const int qc = q < A.Lq ? q : A.Lq - 1;

  const float *qp = A.q + b * A.q_sb + hh * A.q_sh + qc * A.q_sl;
  const float *dop = A.d_out + (((size_t)b * A.Lq + qc) * A.h + hh) * DK;
  float qreg[DK / 4], doreg[DK / 4];
#pragma unroll
  for (int s = 0; s < DK / 4; ++s) {
    qreg[s] = qp[4 * s + lg];
    doreg[s] = dop[4 * s + lg];
  }
  const float *st = A.stats + (((size_t)b * A.h + hh) * A.Lq + qc) * 2;
  const float m = st[0], inv_l = 1.0f / st[1];

  f32x4 p[NT], dp[NT];
  const float *kbase = A.k + b * A.k_sb + hh * A.k_sh;
  const float *vbase = A.v + b * A.v_sb + hh * A.v_sh;
  const float *dprow = A.d_p ? A.d_p + (((size_t)b * A.h + hh) * A.Lq + qc) * A.Lk : nullptr;
  float delta = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    p[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    dp[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (16 * t < A.Lk) {
      const int keyl = 16 * t + lq;
      const int kcl = keyl < A.Lk ? keyl : A.Lk - 1;
      const float *kp = kbase + kcl * A.k_sl;
      const float *vp = vbase + kcl * A.v_sl;
#pragma unroll
      for (int s = 0; s < DK / 4; ++s) {
        p[t] = MFMA16(kp[4 * s + lg], qreg[s], p[t]);     // S^T  = K Q^T
        dp[t] = MFMA16(vp[4 * s + lg], doreg[s], dp[t]);  // dPd^T = V dO^T
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * t + 4 * lg + r;
        bool masked;
        const float s = logit(A, p[t][r], b, hh, q, key, masked);
        const float pr = (key < A.Lk) ? expf(s - m) * inv_l : 0.f;
        float g = dp[t][r];
        if (dprow && key < A.Lk) g += dprow[key];
        g = keep_elem(A, sd, b, hh, q, key) ? g * A.keep_scale : 0.f;  // dP (pre-dropout)
        delta += g * pr;
        p[t][r] = pr;
        dp[t][r] = (masked || key >= A.Lk) ? NAN : g;  // NaN marks "no gradient to the logit"
      }
    }
  }
  if (PRE) {
    delta = A.delta[((size_t)b * A.h + hh) * A.Lq + qc];
  } else {
    delta += __shfl_xor(delta, 16);
    delta += __shfl_xor(delta, 32);
    if (lg == 0 && q < A.Lq) A.delta[((size_t)b * A.h + hh) * A.Lq + q] = delta;
  }

  f32x4 dq[DK / 16];
#pragma unroll
  for (int db = 0; db < DK / 16; ++db) dq[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (16 * t < A.Lk) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * t + 4 * lg + r;
        const float g = dp[t][r];
        const float ds = (g != g) ? 0.f : p[t][r] * (g - delta) * A.scale;
        const float *kp = kbase + (key < A.Lk ? key : A.Lk - 1) * A.k_sl;
#pragma unroll
        for (int db = 0; db < DK / 16; ++db) dq[db] = MFMA16(ds, kp[16 * db + lq], dq[db]);
      }
    }
  }
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int qo = q0 + 4 * lg + rr;
    if (qo < A.Lq) {
      float *op = A.dq + ((size_t)b * A.Lq + qo) * A.g_sl + hh * DK;
#pragma unroll
      for (int db = 0; db < DK / 16; ++db) op[16 * db + lq] = dq[db][rr];
    }
  }
}

template <int NT, int DK>
__global__ __launch_bounds__(64) void mha_bwd_dq_kernel(const MhaArgs A) {
  bwd_dq_body<NT, DK, false>(A, blockIdx.x);
}

// ------------------------------------------------------------------------------------------------
// backward B: dK and dV.  One wave per 16 keys, loops over query tiles; S (not S^T) orientation so the
// accumulator registers are again directly the A operands of the products that sum over queries.
// ------------------------------------------------------------------------------------------------
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
      const float s = logit(A, s4[r], b, hh, q, key, masked);
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

template <int DK>
__global__ __launch_bounds__(64) void mha_bwd_dkv_kernel(const MhaArgs A) {
  bwd_dkv_body<DK>(A, blockIdx.x);
}

// both halves in one launch (delta precomputed): blocks [0, nqb) form dQ, the rest dK / dV
template <int NT, int DK>
__global__ __launch_bounds__(64) void mha_bwd_both_kernel(const MhaArgs A, int nqb) {
  if ((int)blockIdx.x < nqb) bwd_dq_body<NT, DK, true>(A, blockIdx.x);
  else bwd_dkv_body<DK>(A, (int)blockIdx.x - nqb);
}



// ------------------------------------------------------------------------------------------------
// Key-split / query-split variants for long sequences (Lk > 64).  The kernels above give one wavefront
// 16 queries x ALL keys (or 16 keys x all queries): at B*h = 64 and L = 256 that is 1 024 wavefronts, one
// per SIMD, each a serial chain over 16 tiles (40-65 us for 0.27 GFLOP).  Here the four waves of a
// workgroup share the 16 queries (keys) and split the other dimension; row maxima / sums / partial
// products are combined through LDS in a fixed order (deterministic), identical arithmetic per element.
// ------------------------------------------------------------------------------------------------
template <int NTW, int DK>  // NTW key tiles per wave, 4 waves: Lk <= 64 * NTW
__global__ __launch_bounds__(256) void mha_fwd_split_kernel(const MhaArgs A) {
  const DropSeed sd = make_seed(A.seed, A.seed_dev);
  __shared__ float s_m[4][16], s_l[4][16];
  __shared__ float s_o[4][16][DK + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.z, hh = blockIdx.y;
  const int q0 = blockIdx.x * 16;
  const int lq = lane & 15, lg = lane >> 4;
  const int q = q0 + lq;
  const int qc = q < A.Lq ? q : A.Lq - 1;
  const int t0 = w * NTW;

  // operands as 16-byte loads: step (j, s) of the dot product covers k = 16 j + 4 lg + s in BOTH operands (any order of k
  // gives the same sum of products; one load instruction per 16 keys x 16 channels instead of four)
  const float *qp = A.q + b * A.q_sb + hh * A.q_sh + qc * A.q_sl;
  f32x4 qv[DK / 16];
#pragma unroll
  for (int j = 0; j < DK / 16; ++j) {
    if (A.vec) qv[j] = *reinterpret_cast<const f32x4 *>(qp + 16 * j + 4 * lg);
    else qv[j] = f32x4{qp[16 * j + 4 * lg], qp[16 * j + 4 * lg + 1], qp[16 * j + 4 * lg + 2], qp[16 * j + 4 * lg + 3]};
  }

  f32x4 acc[NTW];
  const float *kbase = A.k + b * A.k_sb + hh * A.k_sh;
#pragma unroll
  for (int tt = 0; tt < NTW; ++tt) {
    const int t = t0 + tt;
    acc[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (16 * t < A.Lk) {
      const int key = 16 * t + lq;
      const float *kp = kbase + (key < A.Lk ? key : A.Lk - 1) * A.k_sl;
#pragma unroll
      for (int j = 0; j < DK / 16; ++j) {
        f32x4 kv;
        if (A.vec) kv = *reinterpret_cast<const f32x4 *>(kp + 16 * j + 4 * lg);
        else kv = f32x4{kp[16 * j + 4 * lg], kp[16 * j + 4 * lg + 1], kp[16 * j + 4 * lg + 2], kp[16 * j + 4 * lg + 3]};
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[tt] = MFMA16(kv[s], qv[j][s], acc[tt]);
      }
    }
  }
  float m = -INFINITY;
#pragma unroll
  for (int tt = 0; tt < NTW; ++tt) {
    const unsigned m4 = mask4(A, b, qc, 16 * (t0 + tt) + 4 * lg);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bool masked;
      acc[tt][r] = logit_m(A, acc[tt][r], b, hh, q, 16 * (t0 + tt) + 4 * lg + r, (m4 >> (8 * r)) & 0xffu, masked);
      m = fmaxf(m, acc[tt][r]);
    }
  }
  m = fmaxf(m, __shfl_xor(m, 16));
  m = fmaxf(m, __shfl_xor(m, 32));
  if (lg == 0) s_m[w][lq] = m;
  __syncthreads();
  m = fmaxf(fmaxf(s_m[0][lq], s_m[1][lq]), fmaxf(s_m[2][lq], s_m[3][lq]));
  float l = 0.f;
#pragma unroll
  for (int tt = 0; tt < NTW; ++tt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc[tt][r] = expf(acc[tt][r] - m);
      l += acc[tt][r];
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (lg == 0) s_l[w][lq] = l;
  __syncthreads();
  l = (s_l[0][lq] + s_l[1][lq]) + (s_l[2][lq] + s_l[3][lq]);
  if (w == 0 && lg == 0 && q < A.Lq) {
    float *st = A.stats + (((size_t)b * A.h + hh) * A.Lq + q) * 2;
    st[0] = m;
    st[1] = l;
  }
  const bool vec_ok = (A.Lk & 3) == 0;
  float *prow = A.p_out ? A.p_out + (((size_t)b * A.h + hh) * A.Lq + qc) * A.Lk : nullptr;
#pragma unroll
  for (int tt = 0; tt < NTW; ++tt) {
    f32x4 p;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float pv = acc[tt][r] / l;
      if (!keep_elem(A, sd, b, hh, q, 16 * (t0 + tt) + 4 * lg + r)) pv = 0.f; else pv *= A.keep_scale;
      p[r] = pv;
    }
    acc[tt] = p;
    if (prow && q < A.Lq) {
      const int key = 16 * (t0 + tt) + 4 * lg;
      if (vec_ok) {
        if (key < A.Lk) *reinterpret_cast<f32x4 *>(prow + key) = p;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (key + r < A.Lk) prow[key + r] = p[r];
      }
    }
  }
  f32x4 o[DK / 16];
#pragma unroll
  for (int db = 0; db < DK / 16; ++db) o[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float *vbase = A.v + b * A.v_sb + hh * A.v_sh;
#pragma unroll
  for (int tt = 0; tt < NTW; ++tt) {
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
#pragma unroll
  for (int rr = 0; rr < 4; ++rr)
#pragma unroll
    for (int db = 0; db < DK / 16; ++db) s_o[w][4 * lg + rr][16 * db + lq] = o[db][rr];
  __syncthreads();
  for (int e = threadIdx.x; e < 16 * DK; e += 256) {
    const int qi = e / DK, d = e - qi * DK;
    if (q0 + qi < A.Lq)
      A.out[(((size_t)b * A.Lq + q0 + qi) * A.h + hh) * DK + d] =
          (s_o[0][qi][d] + s_o[1][qi][d]) + (s_o[2][qi][d] + s_o[3][qi][d]);
  }
}

template <int NTW, int DK, bool PRE>
__device__ __forceinline__ void bwd_dq_split_body(const MhaArgs &A, int bx) {
  const DropSeed sd = make_seed(A.seed, A.seed_dev);
  __shared__ float s_d[4][16];
  __shared__ float s_o[4][16][DK + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.z, hh = blockIdx.y;
  const int q0 = bx * 16;
  const int lq = lane & 15, lg = lane >> 4;
  const int q = q0 + lq;
  const int qc = q < A.Lq ? q : A.Lq - 1;
  const int t0 = w * NTW;

  const float *qp = A.q + b * A.q_sb + hh * A.q_sh + qc * A.q_sl;
  const float *dop = A.d_out + (((size_t)b * A.Lq + qc) * A.h + hh) * DK;
  // (16-byte operand loads, k permuted as in the forward kernel: step (j, s) covers k = 16 j + 4 lg + s in both operands)
  f32x4 qv[DK / 16], dov[DK / 16];
#pragma unroll
  for (int j = 0; j < DK / 16; ++j) {
    qv[j] = ldv(qp + 16 * j + 4 * lg, A.vec);
    dov[j] = ldv(dop + 16 * j + 4 * lg, A.dvec);
  }
  const float *st = A.stats + (((size_t)b * A.h + hh) * A.Lq + qc) * 2;
  const float m = st[0], inv_l = 1.0f / st[1];

  f32x4 p[NTW], dp[NTW];
  const float *kbase = A.k + b * A.k_sb + hh * A.k_sh;
  const float *vbase = A.v + b * A.v_sb + hh * A.v_sh;
  const float *dprow = A.d_p ? A.d_p + (((size_t)b * A.h + hh) * A.Lq + qc) * A.Lk : nullptr;
  float delta = 0.f;
#pragma unroll
  for (int tt = 0; tt < NTW; ++tt) {
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
        const f32x4 kv = ldv(kp + 16 * j + 4 * lg, A.vec), vv = ldv(vp + 16 * j + 4 * lg, A.vec);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          p[tt] = MFMA16(kv[s], qv[j][s], p[tt]);
          dp[tt] = MFMA16(vv[s], dov[j][s], dp[tt]);
        }
      }
      const unsigned m4 = mask4(A, b, qc, 16 * t + 4 * lg);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * t + 4 * lg + r;
        bool masked;
        const float s = logit_m(A, p[tt][r], b, hh, q, key, (m4 >> (8 * r)) & 0xffu, masked);
        const float pr = (key < A.Lk) ? expf(s - m) * inv_l : 0.f;
        float g = dp[tt][r];
        if (dprow && key < A.Lk) g += dprow[key];
        g = keep_elem(A, sd, b, hh, q, key) ? g * A.keep_scale : 0.f;
        delta += g * pr;
        p[tt][r] = pr;
        dp[tt][r] = (masked || key >= A.Lk) ? NAN : g;
      }
    }
  }
  if (PRE) {
    delta = A.delta[((size_t)b * A.h + hh) * A.Lq + qc];
  } else {
    delta += __shfl_xor(delta, 16);
    delta += __shfl_xor(delta, 32);
    if (lg == 0) s_d[w][lq] = delta;
    __syncthreads();
    delta = (s_d[0][lq] + s_d[1][lq]) + (s_d[2][lq] + s_d[3][lq]);
    if (w == 0 && lg == 0 && q < A.Lq) A.delta[((size_t)b * A.h + hh) * A.Lq + q] = delta;
  }

  f32x4 dq[DK / 16];
#pragma unroll
  for (int db = 0; db < DK / 16; ++db) dq[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int tt = 0; tt < NTW; ++tt) {
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
#pragma unroll
  for (int rr = 0; rr < 4; ++rr)
#pragma unroll
    for (int db = 0; db < DK / 16; ++db) s_o[w][4 * lg + rr][16 * db + lq] = dq[db][rr];
  __syncthreads();
  for (int e = threadIdx.x; e < 16 * DK; e += 256) {
    const int qi = e / DK, d = e - qi * DK;
    if (q0 + qi < A.Lq)
      A.dq[((size_t)b * A.Lq + q0 + qi) * A.g_sl + hh * DK + d] =
          (s_o[0][qi][d] + s_o[1][qi][d]) + (s_o[2][qi][d] + s_o[3][qi][d]);
  }
}

template <int NTW, int DK>
__global__ __launch_bounds__(256) void mha_bwd_dq_split_kernel(const MhaArgs A) {
  bwd_dq_split_body<NTW, DK, false>(A, blockIdx.x);
}

// dK / dV: 16 keys per workgroup, the query tiles interleaved over the 4 waves
template <int DK>
__device__ __forceinline__ void bwd_dkv_split_body(const MhaArgs &A, int bx) {
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
  f32x4 kv[DK / 16], vv[DK / 16];   // (16-byte operand loads, k permuted: see the forward kernel)
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
      const float s = (A.mask && A.mask_sq != 0) ? logit(A, s4[r], b, hh, q, key, masked) : logit_m(A, s4[r], b, hh, q, key, mkey, masked);
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

template <int DK>
__global__ __launch_bounds__(256) void mha_bwd_dkv_split_kernel(const MhaArgs A) {
  bwd_dkv_split_body<DK>(A, blockIdx.x);
}

template <int NTW, int DK>
__global__ __launch_bounds__(256) void mha_bwd_both_split_kernel(const MhaArgs A, int nqb) {
  if ((int)blockIdx.x < nqb) bwd_dq_split_body<NTW, DK, true>(A, blockIdx.x);
  else bwd_dkv_split_body<DK>(A, (int)blockIdx.x - nqb);
}

int fill_args(MhaArgs &A, const char *what, const float *q, const float *k, const float *v, long q_sb,
              long q_sh, long q_sl, long k_sb, long k_sh, long k_sl, long v_sb, long v_sh, long v_sl,
              const uint8_t *mask, long mask_sb, long mask_sq, const float *bias, long bias_sb, long bias_sh,
              long bias_sq, int B, int h, int Lq, int Lk, int d_k, float scale, float dropout_p,
              uint64_t seed, const uint64_t *seed_dev) {
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

template <int DK>
void launch_fwd(const MhaArgs &A, hipStream_t s) {
  dim3 grid((A.Lq + 63) / 64, A.h, A.B), gs((A.Lq + 15) / 16, A.h, A.B);
  if (A.Lk <= 32) hipLaunchKernelGGL((mha_fwd_kernel<2, DK>), grid, dim3(256), 0, s, A);
  else if (A.Lk <= 64) hipLaunchKernelGGL((mha_fwd_kernel<4, DK>), grid, dim3(256), 0, s, A);
  else if (A.Lk <= 128) hipLaunchKernelGGL((mha_fwd_split_kernel<2, DK>), gs, dim3(256), 0, s, A);
  else if (A.Lk <= 256) hipLaunchKernelGGL((mha_fwd_split_kernel<4, DK>), gs, dim3(256), 0, s, A);
  else hipLaunchKernelGGL((mha_fwd_split_kernel<8, DK>), gs, dim3(256), 0, s, A);
}

// delta precomputed: ONE launch when both halves use the same kernel family (self-attention: Lq == Lk)
template <int DK>
bool launch_bwd_both(const MhaArgs &A, hipStream_t s) {
  const int nqb = (A.Lq + 15) / 16, nkb = (A.Lk + 15) / 16;
  const dim3 g(nqb + nkb, A.h, A.B);
  if (A.Lk <= 64 && A.Lq <= 64) {
    if (A.Lk <= 32) hipLaunchKernelGGL((mha_bwd_both_kernel<2, DK>), g, dim3(64), 0, s, A, nqb);
    else hipLaunchKernelGGL((mha_bwd_both_kernel<4, DK>), g, dim3(64), 0, s, A, nqb);
    return true;
  }
  if (A.Lk > 64 && A.Lq > 64) {
    if (A.Lk <= 128) hipLaunchKernelGGL((mha_bwd_both_split_kernel<2, DK>), g, dim3(256), 0, s, A, nqb);
    else if (A.Lk <= 256) hipLaunchKernelGGL((mha_bwd_both_split_kernel<4, DK>), g, dim3(256), 0, s, A, nqb);
    else hipLaunchKernelGGL((mha_bwd_both_split_kernel<8, DK>), g, dim3(256), 0, s, A, nqb);
    return true;
  }
  return false;
}

template <int DK>
void launch_bwd(const MhaArgs &A, hipStream_t s) {
  dim3 gq((A.Lq + 15) / 16, A.h, A.B);
  if (A.Lk <= 32) hipLaunchKernelGGL((mha_bwd_dq_kernel<2, DK>), gq, dim3(64), 0, s, A);
  else if (A.Lk <= 64) hipLaunchKernelGGL((mha_bwd_dq_kernel<4, DK>), gq, dim3(64), 0, s, A);
  else if (A.Lk <= 128) hipLaunchKernelGGL((mha_bwd_dq_split_kernel<2, DK>), gq, dim3(256), 0, s, A);
  else if (A.Lk <= 256) hipLaunchKernelGGL((mha_bwd_dq_split_kernel<4, DK>), gq, dim3(256), 0, s, A);
  else hipLaunchKernelGGL((mha_bwd_dq_split_kernel<8, DK>), gq, dim3(256), 0, s, A);
  dim3 gk((A.Lk + 15) / 16, A.h, A.B);
  if (A.Lq <= 64) hipLaunchKernelGGL((mha_bwd_dkv_kernel<DK>), gk, dim3(64), 0, s, A);
  else hipLaunchKernelGGL((mha_bwd_dkv_split_kernel<DK>), gk, dim3(256), 0, s, A);
}

}  // namespace

extern "C" size_t spacap_mha_bwd_workspace_bytes(int B, int h, int Lq) {
  if (B <= 0 || h <= 0 || Lq <= 0) return 0;
  return (size_t)B * h * Lq * sizeof(float);
}

extern "C" int spacap_mha_fwd_f32(const float *q, const float *k, const float *v, long q_sb, long q_sh,
                                  long q_sl, long k_sb, long k_sh, long k_sl, long v_sb, long v_sh, long v_sl,
                                  const uint8_t *mask, long mask_sb, long mask_sq, const float *bias,
                                  long bias_sb, long bias_sh, long bias_sq, int B, int h, int Lq, int Lk,
                                  int d_k, float scale, float dropout_p, uint64_t seed, const uint64_t *seed_dev,
                                  float *out, float *p_out, float *stats, spacap_stream_t stream) {
  MhaArgs A;
  int rc = fill_args(A, "spacap_mha_fwd_f32", q, k, v, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, v_sb, v_sh, v_sl, mask,
                     mask_sb, mask_sq, bias, bias_sb, bias_sh, bias_sq, B, h, Lq, Lk, d_k, scale, dropout_p, seed, seed_dev);
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

extern "C" int spacap_mha_bwd_f32(const float *q, const float *k, const float *v, long q_sb, long q_sh,
                                  long q_sl, long k_sb, long k_sh, long k_sl, long v_sb, long v_sh, long v_sl,
                                  const uint8_t *mask, long mask_sb, long mask_sq, const float *bias,
                                  long bias_sb, long bias_sh, long bias_sq, int B, int h, int Lq, int Lk,
                                  int d_k, float scale, float dropout_p, uint64_t seed, const uint64_t *seed_dev,
                                  const float *stats, const float *d_out, const float *d_p, void *workspace,
                                  float *dq, float *dk, float *dv, long grad_row_stride, spacap_stream_t stream) {
  MhaArgs A;
  int rc = fill_args(A, "spacap_mha_bwd_f32", q, k, v, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, v_sb, v_sh, v_sl, mask,
                     mask_sb, mask_sq, bias, bias_sb, bias_sh, bias_sq, B, h, Lq, Lk, d_k, scale, dropout_p, seed, seed_dev);
  if (rc) return rc;
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(dq && dk && dv, "spacap_mha_bwd_f32: null output");
  SPACAP_REQUIRE(grad_row_stride == 0 || grad_row_stride >= (long)h * d_k, "spacap_mha_bwd_f32: bad grad_row_stride");
  hipStream_t s = spacap::as_stream(stream);
  A.g_sl = grad_row_stride ? grad_row_stride : (long)h * d_k;
  if (Lq == 0) {
    SPACAP_REQUIRE(A.g_sl == (long)h * d_k, "spacap_mha_bwd_f32: Lq == 0 needs dense gradients");
    SPACAP_CHECK_HIP(hipMemsetAsync(dk, 0, sizeof(float) * (size_t)B * Lk * h * d_k, s), "spacap_mha_bwd_f32");
    SPACAP_CHECK_HIP(hipMemsetAsync(dv, 0, sizeof(float) * (size_t)B * Lk * h * d_k, s), "spacap_mha_bwd_f32");
    return SPACAP_OK;
  }
  SPACAP_REQUIRE(stats && d_out && workspace, "spacap_mha_bwd_f32: null input");
  A.stats = const_cast<float *>(stats);
  A.d_out = d_out; A.d_p = d_p;
  A.dvec = aligned16(d_out) ? 1 : 0;
  A.dq = dq; A.dk = dk; A.dv = dv;
  A.delta = reinterpret_cast<float *>(workspace);
  if (d_k == 16) launch_bwd<16>(A, s);
  else if (d_k == 32) launch_bwd<32>(A, s);
  else launch_bwd<64>(A, s);
  SPACAP_CHECK_LAUNCH("spacap_mha_bwd_f32");
  return SPACAP_OK;
}

/* As spacap_mha_bwd_f32 with delta[b, head, q] = sum_k p_attn d(p_attn) PRECOMPUTED by the caller (f32 [B,h,Lq]; without a
   gradient on p_attn itself it equals sum_d out[b,q,head,d] d_out[b,q,head,d]): the dQ and the dK / dV halves are then
   independent and run as one launch for self-attention shapes.  d_p must be NULL. */
extern "C" int spacap_mha_bwd_delta_f32(const float *q, const float *k, const float *v, long q_sb, long q_sh,
                                        long q_sl, long k_sb, long k_sh, long k_sl, long v_sb, long v_sh, long v_sl,
                                        const uint8_t *mask, long mask_sb, long mask_sq, const float *bias,
                                        long bias_sb, long bias_sh, long bias_sq, int B, int h, int Lq, int Lk,
                                        int d_k, float scale, float dropout_p, uint64_t seed, const uint64_t *seed_dev,
                                        const float *stats, const float *d_out, const float *delta,
                                        float *dq, float *dk, float *dv, long grad_row_stride, spacap_stream_t stream) {
  const char *what = "spacap_mha_bwd_delta_f32";
  MhaArgs A;
  int rc = fill_args(A, what, q, k, v, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, v_sb, v_sh, v_sl, mask,
                     mask_sb, mask_sq, bias, bias_sb, bias_sh, bias_sq, B, h, Lq, Lk, d_k, scale, dropout_p, seed, seed_dev);
  if (rc) return rc;
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(dq && dk && dv, "%s: null output", what);
  SPACAP_REQUIRE(grad_row_stride == 0 || grad_row_stride >= (long)h * d_k, "%s: bad grad_row_stride", what);
  hipStream_t s = spacap::as_stream(stream);
  A.g_sl = grad_row_stride ? grad_row_stride : (long)h * d_k;
  if (Lq == 0) {   // no query, no gradient: as spacap_mha_bwd_f32
    SPACAP_REQUIRE(A.g_sl == (long)h * d_k, "%s: Lq == 0 needs dense gradients", what);
    SPACAP_CHECK_HIP(hipMemsetAsync(dk, 0, sizeof(float) * (size_t)B * Lk * h * d_k, s), what);
    SPACAP_CHECK_HIP(hipMemsetAsync(dv, 0, sizeof(float) * (size_t)B * Lk * h * d_k, s), what);
    return SPACAP_OK;
  }
  SPACAP_REQUIRE(stats && d_out && delta, "%s: null input", what);
  A.stats = const_cast<float *>(stats);
  A.d_out = d_out; A.d_p = nullptr;
  A.dvec = aligned16(d_out) ? 1 : 0;
  A.dq = dq; A.dk = dk; A.dv = dv;
  A.delta = const_cast<float *>(delta);
  const bool ok = d_k == 16 ? launch_bwd_both<16>(A, s) : d_k == 32 ? launch_bwd_both<32>(A, s) : launch_bwd_both<64>(A, s);
  SPACAP_REQUIRE(ok, "%s: (Lq=%d, Lk=%d) has no single-launch form (self-attention shapes only)", what, Lq, Lk);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
