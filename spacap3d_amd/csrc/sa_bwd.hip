// Backward kernels of the set-abstraction shared MLP (data flow: sa_common.hpp) and their entry points: the BatchNorm-backward
// constants, the pooling backward, the data gradient (fp32-MFMA: sa_dgrad_kernel, with the first-layer fusion; streaming
// split-bf16: sa_bf3_dgrad.inc), the weight gradients (sa_wgrad_kernel; the pooled layer's from z2 alone: sa_l3bwd.inc), the first
// layer's backward, and the functions that tell a caller how many slabs / partials a launch will write.
#include "sa_common.hpp"

namespace {

// part [NPART][2][C] (sum dy, sum dy*xhat) -> coef [C][4], dgamma, dbeta
__global__ __launch_bounds__(1024) void sa_bwd_finalize_kernel(const double *__restrict__ part, int nparts, int C,
                                                              double M, const float *__restrict__ stats,
                                                              float *__restrict__ coef, float *__restrict__ dgamma,
                                                              float *__restrict__ dbeta) {
  __shared__ double s[64][16];
  const int tid = threadIdx.x, col = tid & 15, slab = tid >> 4;
  const int k = col >> 3, c = blockIdx.x * 8 + (col & 7);
  double a = 0.0;
  if (c < C) {
#pragma unroll 16
    for (int p = slab; p < nparts; p += 64) a += part[((size_t)p * 2 + k) * C + c];
  }
  s[slab][col] = a;
  __syncthreads();
  if (tid < 8 && c < C) {
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < 64; ++i) s1 += s[i][tid], s2 += s[i][tid + 8];
    const float mean = stats[c * 4], istd = stats[c * 4 + 1], g = stats[c * 4 + 2];
    const float a1 = (float)(s1 / M), b1 = (float)(s2 / M);
    const float k1 = g * b1 * istd;
    coef[c * 4 + 0] = g;
    coef[c * 4 + 1] = k1 * mean - g * a1;
    coef[c * 4 + 2] = k1;
    coef[c * 4 + 3] = 0.f;
    dgamma[c] = (float)s2;
    dbeta[c] = (float)s1;
  }
}

// ---- pooling backward, pass 1: masked gradient dym = (out > 0) ? dout : 0 and the BN sums over the arg-max rows
__global__ __launch_bounds__(256) void sa_pool_bwd_kernel(const float *__restrict__ dout, const float *__restrict__ out,
                                                          const uint8_t *__restrict__ arg, const float *__restrict__ z,
                                                          const float *__restrict__ zmax, const float *__restrict__ st, long G,
                                                          int S, int C, float *__restrict__ dym, double *__restrict__ part) {
  __shared__ float s_red[2][256];
  const int tid = threadIdx.x;
  const int c = tid % C;           // C in {64, 128, 256}: 256 / C groups per pass
  const int gs = tid / C, GP = 256 / C;
  const float mean = st[c * 4], istd = st[c * 4 + 1];
  // zmax [G][C] (the forward's pooling pass kept the arg-max rows' pre-activations) replaces a 4-byte gather per element out of
  // z [G S][C]; it equals z at the arg-max row wherever a gradient passes, except in a channel whose BatchNorm weight is exactly 0
  // (every row ties): such a channel reads z when z is given
  const bool from_max = zmax && (st[c * 4 + 2] != 0.f || !z);
  float s1 = 0.f, s2 = 0.f;
  for (long g = (long)blockIdx.x * GP + gs; g < G; g += (long)gridDim.x * GP) {
    const size_t o = (size_t)g * C + c;
    const float dy = out[o] > 0.f ? dout[o] : 0.f;
    dym[o] = dy;
    const float zz = from_max ? zmax[o] : z[((size_t)g * S + arg[o]) * C + c];
    s1 += dy;
    s2 += dy * ((zz - mean) * istd);
  }
  s_red[0][tid] = s1, s_red[1][tid] = s2;
  __syncthreads();
  if (tid < C) {
    double a = 0.0, b = 0.0;
    for (int i = 0; i < GP; ++i) a += (double)s_red[0][i * C + tid], b += (double)s_red[1][i * C + tid];
    part[((size_t)blockIdx.x * 2 + 0) * C + tid] = a;
    part[((size_t)blockIdx.x * 2 + 1) * C + tid] = b;
  }
}

// dz of the current tile element group (4 channels) from the dense or the pooled gradient source
template <bool POOLED>
__device__ __forceinline__ f32x4 load_dz(const float *__restrict__ dy, const uint8_t *__restrict__ arg, int S,
                                         const float *__restrict__ zk, long grow, int CK, int c0, f32x4 g, f32x4 k0,
                                         f32x4 k1) {
  const f32x4 z = ld4(zk + (size_t)grow * CK + c0);
  f32x4 d;
  if (POOLED) {
    // S is a power of two on the model's path (64 / 32 / 16): shift + mask instead of a 64-bit division per element
    const int lgS = (S & (S - 1)) == 0 ? __builtin_ctz((unsigned)S) : -1;
    const long grp = lgS >= 0 ? (grow >> lgS) : grow / S;
    const int s = (int)(grow - grp * S);
    const f32x4 dm = ld4(dy + (size_t)grp * CK + c0);
    const uchar4 a = *reinterpret_cast<const uchar4 *>(arg + (size_t)grp * CK + c0);
    d[0] = a.x == s ? dm[0] : 0.f;
    d[1] = a.y == s ? dm[1] : 0.f;
    d[2] = a.z == s ? dm[2] : 0.f;
    d[3] = a.w == s ? dm[3] : 0.f;
  } else {
    d = ld4(dy + (size_t)grow * CK + c0);
  }
  return g * d + k0 - k1 * z;
}

// ---- data gradient: dy_prev = (dz_k W_k) * [a_prev > 0], and the BN sums of dy_prev -----------------------------
// Same pipeline as sa_mid_fwd_kernel: the next tile's z_k (and dense dy) rows are prefetched with hand-issued loads
// while the matrix cores work, dz is formed while staging, and the accumulators go through LDS so that the epilogue
// (mask by relu'(bn(z_prev)), BN sums, store) reads z_prev and writes dy_prev as full rows.
// PREFETCH: register prefetch (off for CK = 256, where it would cost the second resident workgroup).
// ALIAS: the output tile reuses the staging buffer (one more barrier, 18 KB less LDS; CK = 256).
// L1 (first-layer fusion, SA1): z_prev is the first layer's pre-activation.  Its weight gradient
//   dW1[c, d] = sum_r dz1[r, c] in_d(r),  dz1 = g dy1 + k0 - k1 z1,  in = (rel x, rel y, rel z, inline feature)
// is linear in three sums that do not need the (not yet known) BN-backward constants g, k0, k1:
//   S1[c,d] = sum dy1 in_d,  S2[d] = sum in_d,  S3[c,d] = sum z1 in_d   =>   dW1 = g S1 + k0 S2 - k1 S3.
// The epilogue accumulates them from the tile it already holds, dy1 is never written and the separate first-layer
// backward pass (read dy1 + z1: 536 MB at SA1) disappears.
struct L1Args {
  const float *feat, *xyz, *new_xyz;
  const int32_t *idx;
  float rdiv;
  int Np, N, S;
  float *part;  // [NPART][COB*8 + 4]
  const float *rel4;   // optional: the rows' inputs as the statistics pass stored them; then z_prev is rebuilt, not read (zp unused)
  L1In li;
  float *partW;        // WG only: [gridDim.x][CK][COB] per-workgroup partial sums of dW_k = dz_k^T relu(bn(z_prev))
};

// WG (with L1 + rel4, CK = COB = 64): the layer's WEIGHT gradient from the same pass.  The tile's dz_k is in LDS for the data
// gradient and the epilogue rebuilds a_prev = relu(bn(z_prev)) for its mask anyway: it leaves a_prev in the output tile's place
// and one more product per tile, dW_k += dz_k^T a_prev (contraction over the tile's 64 rows), replaces the separate weight-gradient
// kernel and its second read of dy and z_k (536 MB at SA1).
template <int CK, int NT, bool POOLED, bool PREFETCH, bool ALIAS, bool L1 = false, bool WG = false>
// (first-layer instances: two waves per SIMD asked for explicitly.  Left to itself the compiler spreads their state over 262 - 307
// VGPRs + AGPRs, one more than half the register file: ONE 256-thread workgroup per CU, 32 KB of loads in flight per CU, 182 us
// at SA1; bounded to 256 registers the plain instance needs no scratch and runs 142 us, the fused one 256 instead of 311)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(L1 ? 2 : 1))) void sa_dgrad_kernel(const float *__restrict__ dy, const uint8_t *__restrict__ arg, int S,
                                                       const float *__restrict__ zk, const float *__restrict__ coef,
                                                       const float *__restrict__ Wk, int CP, const float *__restrict__ zp,
                                                       const float *__restrict__ st_p, long R, float *__restrict__ dyp,
                                                       double *__restrict__ part, const L1Args L = L1Args{}) {
  constexpr int LD = CK + 4, KS = CK / 4, C4 = CK / 4, NV = TM * C4 / 256, RSTEP = 256 / C4;
  constexpr int COB = 64 * NT, LDO = COB + 4, O4 = COB / 4, NO = TM * O4 / 256, OSTEP = 256 / O4;
  constexpr bool DENSE_PF = PREFETCH && !POOLED;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *s_a = smem;                               // [TM][LD]  dz (MFMA B operand)
  float *s_o = ALIAS ? smem : smem + TM * LD;      // [TM][LDO] output tile, row-major
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int cbb = blockIdx.y * COB, wc = w * 16 * NT, cb = cbb + wc;
  float wf[NT][KS];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) wf[j][ks] = Wk[(size_t)(ks * 4 + lg) * CP + cb + 16 * j + l15];
  const int c4 = tid % C4, r0 = tid / C4, o4 = tid % O4, or0 = tid / O4;
  f32x4 g, k0, k1, pm, pi, ps, pb;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float *s = coef + (size_t)(c4 * 4 + u) * 4;
    g[u] = s[0], k0[u] = s[1], k1[u] = s[2];
    const float *q = st_p + (size_t)(cbb + o4 * 4 + u) * 4;
    pm[u] = q[0], pi[u] = q[1], ps[u] = q[2], pb[u] = q[3];
  }
  f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
  const int lgS = (S > 0 && (S & (S - 1)) == 0) ? __builtin_ctz((unsigned)S) : -1;
  const long ntiles = (R + TM - 1) / TM, nfull = R / TM;
  float *s_rel = smem + (ALIAS ? TM * LD : TM * LD + TM * LDO);  // [TM][4] first-layer inputs of the tile's rows (L1)
  f32x4 q1[L1 ? 4 : 1], q3[L1 ? 4 : 1], q2 = {0.f, 0.f, 0.f, 0.f};
  f32x4 l1x = {0.f, 0.f, 0.f, 0.f}, l1y = l1x, l1z = l1x, l1f = l1x;
  if (L1 && L.rel4) l1_weights(L.li, cbb + o4 * 4, l1x, l1y, l1z, l1f);
  if (L1) {
#pragma unroll
    for (int u = 0; u < 4; ++u) q1[u] = q3[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  static_assert(!WG || (L1 && !ALIAS && CK == 64 && NT == 1), "fused weight gradient: 64 x 64 first-layer instance only");
  f32x4 accw[WG ? 4 : 1];
#pragma unroll
  for (int n = 0; n < (WG ? 4 : 1); ++n) accw[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 pz[PREFETCH ? NV : 1], pd[DENSE_PF ? NV : 1];
  auto fetch = [&](long t) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      long grow = t * TM + r0 + i * RSTEP;
      grow = grow < R ? grow : R - 1;
      const float *src = zk + (size_t)grow * CK + c4 * 4;
      asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(pz[i]) : "v"(src) : "memory");
      if (DENSE_PF) {
        const float *sd = dy + (size_t)grow * CK + c4 * 4;
        asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(pd[i]) : "v"(sd) : "memory");
      }
    }
  };
  auto tile = [&](long t, auto full, bool stores_pending) {
    constexpr bool FULL = decltype(full)::value;
    const long row0 = t * TM;
    if (PREFETCH) {
      // (L1: the epilogue stores nothing, every outstanding operation is one of the prefetched loads)
      if (stores_pending && !L1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NO) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        asm volatile("" : "+v"(pz[i]));
        if (DENSE_PF) asm volatile("" : "+v"(pd[i]));
      }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int row = r0 + i * RSTEP;
      const long grow = row0 + row;
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      if (FULL || grow < R) {
        const f32x4 z = PREFETCH ? pz[i] : ld4(zk + (size_t)grow * CK + c4 * 4);
        f32x4 d;
        if (POOLED) {
          const long grp = lgS >= 0 ? (grow >> lgS) : grow / S;
          const int sidx = (int)(grow - grp * S);
          const f32x4 dm = ld4(dy + (size_t)grp * CK + c4 * 4);
          const uchar4 am = *reinterpret_cast<const uchar4 *>(arg + (size_t)grp * CK + c4 * 4);
          d[0] = am.x == sidx ? dm[0] : 0.f;
          d[1] = am.y == sidx ? dm[1] : 0.f;
          d[2] = am.z == sidx ? dm[2] : 0.f;
          d[3] = am.w == sidx ? dm[3] : 0.f;
        } else {
          d = DENSE_PF ? pd[i] : ld4(dy + (size_t)grow * CK + c4 * 4);
        }
        a = g * d + k0 - k1 * z;
      }
      st4(&s_a[row * LD + c4 * 4], a);
    }
    if (L1 && tid < TM) {
      f32x4 in = {0.f, 0.f, 0.f, 0.f};
      const long grow = row0 + tid;
      if ((FULL || grow < R) && L.rel4) {
        in = ld4(L.rel4 + (size_t)grow * 4);
      } else if (FULL || grow < R) {
        const long b = row_div(grow, (long)L.N * L.S), gi = row_div(grow, L.S);
        const int p = L.idx[grow];
        const float *q = L.xyz + ((size_t)b * L.Np + p) * 3, *c = L.new_xyz + (size_t)gi * 3;
        in[0] = (q[0] - c[0]) / L.rdiv, in[1] = (q[1] - c[1]) / L.rdiv, in[2] = (q[2] - c[2]) / L.rdiv;
        if (L.feat) in[3] = L.feat[(size_t)b * L.Np + p];
      }
      st4(&s_rel[tid * 4], in);
      q2 += in;
    }
    __syncthreads();
    if (PREFETCH && FULL) fetch(t + gridDim.x);
    f32x4 acc[TM / 16][NT];
#pragma unroll
    for (int mt = 0; mt < TM / 16; ++mt)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
        for (int mt = 0; mt < TM / 16; ++mt) {
          const float b = s_a[(mt * 16 + l15) * LD + ks * 4 + lg];
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[mt][j] = MFMA16(wf[j][ks], b, acc[mt][j]);
        }
      }
    }
    if (ALIAS) __syncthreads();  // every wave is done reading dz before the output tile overwrites it
#pragma unroll
    for (int mt = 0; mt < TM / 16; ++mt)
#pragma unroll
      for (int j = 0; j < NT; ++j) st4(&s_o[(mt * 16 + l15) * LDO + wc + 16 * j + 4 * lg], acc[mt][j]);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NO; ++i) {
      const int row = or0 + i * OSTEP;
      if (FULL || row0 + row < R) {
        const size_t o = (size_t)(row0 + row) * CP + cbb + o4 * 4;
        const f32x4 da = ld4(&s_o[row * LDO + o4 * 4]);
        f32x4 z;
        if (L1 && L.rel4) z = l1_row(l1x, l1y, l1z, l1f, ld4(&s_rel[row * 4]), L.li.has_feat != 0);
        else z = ld4(zp + o);
        f32x4 d;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float pre = (z[u] - pm[u]) * ps[u] + pb[u];
          d[u] = pre > 0.f ? da[u] : 0.f;
          s1[u] += d[u];
          s2[u] += d[u] * ((z[u] - pm[u]) * pi[u]);
        }
        if (L1) {
          const f32x4 in = ld4(&s_rel[row * 4]);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            q1[u] += in * d[u];
            q3[u] += in * z[u];
          }
        } else {
          st4(dyp + o, d);
        }
        if (WG) {   // a_prev over this thread's own element of the output tile (nobody else reads it in this loop)
          f32x4 ap;
#pragma unroll
          for (int u = 0; u < 4; ++u) ap[u] = fmaxf((z[u] - pm[u]) * ps[u] + pb[u], 0.f);
          st4(&s_o[row * LDO + o4 * 4], ap);
        }
      } else if (WG) {
        st4(&s_o[row * LDO + o4 * 4], f32x4{0.f, 0.f, 0.f, 0.f});   // (rows past the end: dz is zero there as well)
      }
    }
    if (WG) {
      __syncthreads();
      // dW[ck = 16 w + .][cp = 16 n + .] += sum over the tile's rows of dz[row][ck] a_prev[row][cp]
#pragma unroll
      for (int ks = 0; ks < TM / 4; ++ks) {
        const float af = s_a[(ks * 4 + lg) * LD + 16 * w + l15];
#pragma unroll
        for (int n = 0; n < 4; ++n) accw[n] = MFMA16(af, s_o[(ks * 4 + lg) * LDO + 16 * n + l15], accw[n]);
      }
      __syncthreads();   // before the next tile is staged over dz / the output tile
    }
    if (ALIAS) __syncthreads();  // the output tile is consumed before the next tile is staged over it
  };
  bool pending = false;
  if (PREFETCH && (long)blockIdx.x < nfull) fetch(blockIdx.x);
  for (long t = blockIdx.x; t < nfull; t += gridDim.x) {
    tile(t, std::true_type{}, pending);
    pending = true;
  }
  if (PREFETCH) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      asm volatile("" ::"v"(pz[i]));
      if (DENSE_PF) asm volatile("" ::"v"(pd[i]));
    }
  }
  if (nfull < ntiles && (long)blockIdx.x == nfull % gridDim.x) {  // ragged last tile
    if (PREFETCH) {
      fetch(nfull);
    }
    tile(nfull, std::false_type{}, false);
  }
  // BN sums: this thread owns columns cbb + 4*o4 .. +3 for the rows or0 + k*OSTEP; combine the OSTEP row groups
  __syncthreads();
  float *s_red = smem;  // [2][OSTEP][COB]
  st4(&s_red[(0 * OSTEP + or0) * COB + o4 * 4], s1);
  st4(&s_red[(1 * OSTEP + or0) * COB + o4 * 4], s2);
  __syncthreads();
  if (tid < 2 * COB) {
    const int k = tid / COB, c = tid % COB;
    float a = 0.f;
    for (int i = 0; i < OSTEP; ++i) a += s_red[(k * OSTEP + i) * COB + c];
    part[((size_t)blockIdx.x * 2 + k) * CP + cbb + c] = (double)a;
    for (int pr = blockIdx.x + gridDim.x; pr < NPART; pr += gridDim.x) part[((size_t)pr * 2 + k) * CP + cbb + c] = 0.0;
  }
  if (WG) {
    float *o = L.partW + (size_t)blockIdx.x * CK * COB;
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int u = 0; u < 4; ++u) o[(size_t)(16 * w + 4 * lg + u) * COB + 16 * n + l15] = accw[n][u];
  }
  if (L1) {  // S1 / S3: combine the OSTEP row groups; S2: combine the TM row slots
    __syncthreads();
    float *s_q = smem;  // [OSTEP][COB][8]
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      st4(&s_q[((or0 * COB) + o4 * 4 + u) * 8], q1[u]);
      st4(&s_q[((or0 * COB) + o4 * 4 + u) * 8 + 4], q3[u]);
    }
    __syncthreads();
    float *out = L.part + (size_t)blockIdx.x * (COB * 8 + 4);
    for (int e = tid; e < COB * 8; e += 256) {
      float a = 0.f;
      for (int i = 0; i < OSTEP; ++i) a += s_q[i * COB * 8 + e];
      out[e] = a;
    }
    __syncthreads();
    if (tid < TM) st4(&s_q[tid * 4], q2);
    __syncthreads();
    if (tid < 4) {
      float a = 0.f;
      for (int i = 0; i < TM; ++i) a += s_q[i * 4 + tid];
      out[COB * 8 + tid] = a;
    }
    for (int pr = blockIdx.x + gridDim.x; pr < NPART; pr += gridDim.x)
      for (int e = tid; e < COB * 8 + 4; e += 256) L.part[(size_t)pr * (COB * 8 + 4) + e] = 0.f;
  }
}

#include "sa_bf3_dgrad.inc"

// ---- weight gradient: dW_k[ck, cp] = sum_r dz_k[r, ck] a_prev[r, cp]; one partial per row slab -----------------
template <int CKB, int CP, bool POOLED>
__global__ __launch_bounds__(256) void sa_wgrad_kernel(const float *__restrict__ dy, const uint8_t *__restrict__ arg, int S,
                                                       const float *__restrict__ zk, const float *__restrict__ coef, int CK,
                                                       const float *__restrict__ zp, const float *__restrict__ st_p, long R,
                                                       float *__restrict__ partW, L1In li = L1In{nullptr, 0, 0}) {
  constexpr int LDZ = CKB + 16, LDA = CP + 16;
  constexpr int MT = CKB / 64, NTT = CP / 16;           // m-tiles per wave, n-tiles
  constexpr int Z4 = CKB / 4, A4 = CP / 4;
  constexpr int NVZ = TW * Z4 / 256, NVA = TW * A4 / 256, RZ = 256 / Z4, RA = 256 / A4;
  __shared__ __attribute__((aligned(16))) float s_dz[TW * LDZ];
  __shared__ __attribute__((aligned(16))) float s_a[TW * LDA];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int ckb0 = blockIdx.y * CKB;
  const int z4 = tid % Z4, zr0 = tid / Z4, a4 = tid % A4, ar0 = tid / A4;
  f32x4 g, k0, k1, pm, ps, pb;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float *s = coef + (size_t)(ckb0 + z4 * 4 + u) * 4;
    g[u] = s[0], k0[u] = s[1], k1[u] = s[2];
    const float *q = st_p + (size_t)(a4 * 4 + u) * 4;
    pm[u] = q[0], ps[u] = q[2], pb[u] = q[3];
  }
  f32x4 acc[MT][NTT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NTT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const long ntiles = (R + TW - 1) / TW;
  const int lgS = (S > 0 && (S & (S - 1)) == 0) ? __builtin_ctz((unsigned)S) : -1;
  // software pipeline: the raw operands of tile t + gridDim.x are loaded into registers while tile t is multiplied
  f32x4 rz[NVZ], rd[NVZ], ra[NVA];
  uchar4 rg[POOLED ? NVZ : 1];
  int rs[POOLED ? NVZ : 1];
  auto fetch = [&](long t) {
    const long row0 = t * TW;
#pragma unroll
    for (int i = 0; i < NVZ; ++i) {
      long grow = row0 + zr0 + i * RZ;
      grow = grow < R ? grow : R - 1;
      rz[i] = ld4(zk + (size_t)grow * CK + ckb0 + z4 * 4);
      if (POOLED) {
        const long grp = lgS >= 0 ? (grow >> lgS) : grow / S;
        rs[i] = (int)(grow - grp * S);
        rd[i] = ld4(dy + (size_t)grp * CK + ckb0 + z4 * 4);
        rg[i] = *reinterpret_cast<const uchar4 *>(arg + (size_t)grp * CK + ckb0 + z4 * 4);
      } else {
        rd[i] = ld4(dy + (size_t)grow * CK + ckb0 + z4 * 4);
      }
    }
#pragma unroll
    for (int i = 0; i < NVA; ++i) {
      long grow = row0 + ar0 + i * RA;
      grow = grow < R ? grow : R - 1;
      ra[i] = li.W1 ? ld4(zp + (size_t)grow * 4) : ld4(zp + (size_t)grow * CP + a4 * 4);
    }
  };
  f32x4 l1x = {0.f, 0.f, 0.f, 0.f}, l1y = l1x, l1z = l1x, l1f = l1x;
  if (li.W1) l1_weights(li, a4 * 4, l1x, l1y, l1z, l1f);
  if ((long)blockIdx.x < ntiles) fetch(blockIdx.x);
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long row0 = t * TW;
#pragma unroll
    for (int i = 0; i < NVZ; ++i) {
      const int row = zr0 + i * RZ;
      f32x4 d = rd[i];
      if (POOLED) {
        d[0] = rg[i].x == rs[i] ? d[0] : 0.f;
        d[1] = rg[i].y == rs[i] ? d[1] : 0.f;
        d[2] = rg[i].z == rs[i] ? d[2] : 0.f;
        d[3] = rg[i].w == rs[i] ? d[3] : 0.f;
      }
      f32x4 a = g * d + k0 - k1 * rz[i];
      if (row0 + row >= R) a = f32x4{0.f, 0.f, 0.f, 0.f};
      st4(&s_dz[row * LDZ + z4 * 4], a);
    }
#pragma unroll
    for (int i = 0; i < NVA; ++i) {
      const int row = ar0 + i * RA;
      f32x4 a;
      const f32x4 zv = li.W1 ? l1_row(l1x, l1y, l1z, l1f, ra[i], li.has_feat != 0) : ra[i];
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = fmaxf((zv[u] - pm[u]) * ps[u] + pb[u], 0.f);
      if (row0 + row >= R) a = f32x4{0.f, 0.f, 0.f, 0.f};
      st4(&s_a[row * LDA + a4 * 4], a);
    }
    __syncthreads();
    if (t + gridDim.x < ntiles) fetch(t + gridDim.x);
#pragma unroll
    for (int ks = 0; ks < TW / 4; ++ks) {
      float af[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) af[m] = s_dz[(ks * 4 + lg) * LDZ + (w * MT + m) * 16 + l15];
#pragma unroll
      for (int n = 0; n < NTT; ++n) {
        const float b = s_a[(ks * 4 + lg) * LDA + n * 16 + l15];
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m][n] = MFMA16(af[m], b, acc[m][n]);
      }
    }
    __syncthreads();
  }
  float *o = partW + ((size_t)blockIdx.x * CK + ckb0) * CP;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NTT; ++n)
#pragma unroll
      for (int u = 0; u < 4; ++u) o[(size_t)((w * MT + m) * 16 + 4 * lg + u) * CP + n * 16 + l15] = acc[m][n][u];
}

#include "sa_l3bwd.inc"

// ---- layer 1 backward: dz1 (in place over dy1), dW1 partials [NPART][C1][4], optional d rel [R][3] -------------
template <int C1>
__global__ __launch_bounds__(256) void sa_l1_bwd_kernel(float *__restrict__ dy1, const float *__restrict__ z1,
                                                        const float *__restrict__ coef, const float *__restrict__ feat,
                                                        const float *__restrict__ xyz, const float *__restrict__ new_xyz,
                                                        const int32_t *__restrict__ idx, const float *__restrict__ W1,
                                                        int ldw, float rdiv, int Np, int N, int S, long R,
                                                        float *__restrict__ partW, float *__restrict__ drel, int write_dz) {
  constexpr int C4 = C1 / 4, RP = 256 / C4;
  __shared__ float s_red[4][RP][C1];
  const int tid = threadIdx.x, c4 = tid % C4, rs = tid / C4;
  f32x4 g, k0, k1, wx, wy, wz;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float *s = coef + (size_t)(c4 * 4 + u) * 4;
    g[u] = s[0], k0[u] = s[1], k1[u] = s[2];
    const float *w = W1 + (size_t)(c4 * 4 + u) * ldw;
    wx[u] = w[0], wy[u] = w[1], wz[u] = w[2];
  }
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 ax = zero, ay = zero, az = zero, af = zero;
  const long NS = (long)N * S;
  for (long r0 = (long)blockIdx.x * RP; r0 < R; r0 += (long)gridDim.x * RP) {
    const long r = r0 + rs;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (r < R) {
      const long b = row_div(r, NS), gi = row_div(r, S);
      const int p = idx[r];
      const float *q = xyz + ((size_t)b * Np + p) * 3, *c = new_xyz + (size_t)gi * 3;
      const float rx = (q[0] - c[0]) / rdiv, ry = (q[1] - c[1]) / rdiv, rz = (q[2] - c[2]) / rdiv;
      const size_t o = (size_t)r * C1 + c4 * 4;
      const f32x4 dz = g * ld4(dy1 + o) + k0 - k1 * ld4(z1 + o);
      if (write_dz) st4(dy1 + o, dz);
      ax += dz * rx, ay += dz * ry, az += dz * rz;
      if (feat) af += dz * feat[(size_t)b * Np + p];
      if (drel) {
        px = dz[0] * wx[0] + dz[1] * wx[1] + dz[2] * wx[2] + dz[3] * wx[3];
        py = dz[0] * wy[0] + dz[1] * wy[1] + dz[2] * wy[2] + dz[3] * wy[3];
        pz = dz[0] * wz[0] + dz[1] * wz[1] + dz[2] * wz[2] + dz[3] * wz[3];
      }
    }
    if (drel) {  // sum over the C4 lanes that share the row (C4 = 16 or 32, aligned inside the wave)
#pragma unroll
      for (int o = 1; o < C4; o <<= 1) px += __shfl_xor(px, o), py += __shfl_xor(py, o), pz += __shfl_xor(pz, o);
      if (c4 == 0 && r < R) drel[r * 3] = px / rdiv, drel[r * 3 + 1] = py / rdiv, drel[r * 3 + 2] = pz / rdiv;
    }
  }
  st4(&s_red[0][rs][c4 * 4], ax);
  st4(&s_red[1][rs][c4 * 4], ay);
  st4(&s_red[2][rs][c4 * 4], az);
  st4(&s_red[3][rs][c4 * 4], af);
  __syncthreads();
  for (int e = tid; e < 4 * C1; e += 256) {
    const int c = e / 4, k = e % 4;
    float a = 0.f;
    for (int i = 0; i < RP; ++i) a += s_red[k][i][c];
    partW[((size_t)blockIdx.x * C1 + c) * 4 + k] = a;
  }
}

// First-layer weight gradient of a module with point features, assembled in one launch from the two sets of partial results:
//   dW1[c][0..2]    = sum over the n1 slabs of pw1 [n1][C1][4]   (relative coordinates; column 3 = the inline feature, unused here)
//   dW1[c][3 + j]   = sum over the nf slabs of pf  [nf][C1][Cf]  (the feature product over the source points)
// with sum_slabs_kernel's grouping (four runs of slabs, combined as (s0 + s1) + (s2 + s3)): the same values as the two slab sums
// and the concatenation it replaces.
__global__ __launch_bounds__(256) void sa_dw1_assemble_kernel(const float *__restrict__ pw1, int n1, const float *__restrict__ pf, int nf,
                                                              int C1, int Cf, float *__restrict__ out) {
  __shared__ float s_g[4][64];
  const int c = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const long e = (long)blockIdx.x * 64 + c, ne = (long)C1 * (3 + Cf);
  float a = 0.f;
  if (e < ne) {
    const int ch = (int)(e / (3 + Cf)), j = (int)(e % (3 + Cf));
    const float *src = j < 3 ? pw1 + (size_t)ch * 4 + j : pf + (size_t)ch * Cf + (j - 3);
    const size_t stride = j < 3 ? (size_t)C1 * 4 : (size_t)C1 * Cf;
    const int ns = j < 3 ? n1 : nf, per = (ns + 3) / 4, s0 = grp * per, s1 = min(ns, s0 + per);
    // (a dependent chain of strided loads: 32 in flight per thread, added in slab order -- 2 round trips instead of 8 at 256 slabs)
    int k = s0;
    for (; k + 32 <= s1; k += 32) {
      float t[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) t[u] = src[(size_t)(k + u) * stride];
#pragma unroll
      for (int u = 0; u < 32; ++u) a += t[u];
    }
#pragma unroll 8
    for (; k < s1; ++k) a += src[(size_t)k * stride];
  }
  s_g[grp][c] = a;
  __syncthreads();
  if (grp == 0 && e < ne) out[e] = (s_g[0][c] + s_g[1][c]) + (s_g[2][c] + s_g[3][c]);
}

}  // namespace

// ===========================================================================================================
// row slabs (= partial results = workgroups per output tile) of the weight-gradient GEMM: what is resident at
// once, at most 64 MB of partials
namespace {
int wgrad_resident(int CK, int CP, bool pooled) {
#define WR(CKB, CPV, PV)                                                        \
  {                                                                             \
    static const int res = resident_blocks(sa_wgrad_kernel<CKB, CPV, PV>, 0);   \
    return res;                                                                 \
  }
  if (pooled && CK % 128 == 0 && CP == 64) WR(128, 64, true)
  if (pooled && CK % 128 == 0 && CP == 128) WR(128, 128, true)
  if (!pooled && CK == 64 && CP == 64) WR(64, 64, false)
  if (!pooled && CK == 128 && CP == 128) WR(128, 128, false)
#undef WR
  return 512;
}
}  // namespace
extern "C" int spacap_sa_wgrad_slabs(long R, int CK, int CP, int pooled) {
  const int gy = CK >= 128 ? CK / 128 : 1;
  long n = bwd_resident(wgrad_resident(CK, CP, pooled != 0)) / gy, cap = (16L << 20) / ((long)CK * CP), tiles = (R + TW - 1) / TW;
  if (n > cap) n = cap;
  if (n > tiles) n = tiles;
  return (int)(n < 1 ? 1 : n);
}

// Weight gradient of the second layer (64 x 64, dense) with a_prev = relu(bn1(W1 in)) rebuilt from rel4
extern "C" int spacap_sa_wgrad_l1in_f32(const float *dy, const float *zk, const float *coef, const float *rel4, const float *W1, int ldw,
                                        int has_feat, const float *st_p, long R, float *partW, spacap_stream_t stream) {
  const char *what = "spacap_sa_wgrad_l1in_f32";
  SPACAP_REQUIRE(dy && zk && coef && rel4 && W1 && st_p && partW && R >= 1 && ldw >= (has_feat ? 4 : 3), "%s: bad arguments", what);
  const int nslab = spacap_sa_wgrad_slabs(R, 64, 64, 0);
  hipLaunchKernelGGL((sa_wgrad_kernel<64, 64, false>), dim3(nslab, 1), dim3(256), 0, spacap::as_stream(stream), dy, (const uint8_t *)nullptr,
                     0, zk, coef, 64, rel4, st_p, R, partW, L1In{W1, ldw, has_feat});
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_sa_bwd_finalize_f32(const double *part, int C, long count, const float *stats, float *coef,
                                          float *dgamma, float *dbeta, spacap_stream_t stream) {
  const char *what = "spacap_sa_bwd_finalize_f32";
  SPACAP_REQUIRE(part && stats && coef && dgamma && dbeta && C >= 1 && count >= 1, "%s: bad arguments", what);
  hipLaunchKernelGGL(sa_bwd_finalize_kernel, dim3((C + 7) / 8), dim3(1024), 0, spacap::as_stream(stream), part, NPART, C,
                     (double)count, stats, coef, dgamma, dbeta);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_sa_pool_bwd_f32(const float *dout, const float *out, const uint8_t *arg, const float *z, const float *zmax,
                                      const float *stats, long G, int S, int C, float *dym, double *part,
                                      spacap_stream_t stream) {
  const char *what = "spacap_sa_pool_bwd_f32";
  SPACAP_REQUIRE(dout && out && arg && (z || zmax) && stats && dym && part && G >= 1, "%s: bad arguments", what);
  SPACAP_REQUIRE(C == 64 || C == 128 || C == 256, "%s: C=%d unsupported", what, C);
  hipLaunchKernelGGL(sa_pool_bwd_kernel, dim3(NPART), dim3(256), 0, spacap::as_stream(stream), dout, out, arg, z, zmax, stats,
                     G, S, C, dym, part);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// ---- pooled layer's weight gradient from z2 alone: partial layout + reduction (sa_l3bwd.inc) ------------------------------------
/* floats per workgroup partial of spacap_sa_wgrad_pool_f32: [C3][C2] | [C2][C2] | [C2] */
extern "C" long spacap_sa_l3bwd_part_floats(int C2, int C3) { return (long)C3 * C2 + (long)C2 * C2 + C2; }

/* dW3 [C3][C2] from the workgroups' partials: sums (double scratch, spacap_sa_l3bwd_part_floats entries) then
   dW3 = S + k0 (x) colsum(a2) - diag(k1) W3 Gram. */
extern "C" int spacap_sa_l3bwd_dw_f32(const float *partW, int nparts, const float *coef3, const float *W3, int C3, int C2, double *sums,
                                      float *dW3, spacap_stream_t stream) {
  const char *what = "spacap_sa_l3bwd_dw_f32";
  SPACAP_REQUIRE(partW && coef3 && W3 && sums && dW3 && nparts >= 1 && C3 >= 1 && C2 >= 4 && C2 % 4 == 0, "%s: bad arguments", what);
  SPACAP_REQUIRE(spacap::aligned16(partW), "%s: partW must be 16-byte aligned", what);
  const long n = spacap_sa_l3bwd_part_floats(C2, C3);
  hipStream_t s = spacap::as_stream(stream);
  SPACAP_REQUIRE(C2 <= 1024 && 1024 % C2 == 0, "%s: C2=%d unsupported", what, C2);
  hipLaunchKernelGGL(sa_l3_sum_kernel, dim3(nblocks(n, 64)), dim3(256), 0, s, partW, nparts, n, sums);
  hipLaunchKernelGGL(sa_l3_dw_kernel, dim3(C3), dim3(1024), 0, s, sums, coef3, W3, C3, C2, dW3);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// ---- pooled layer's weight gradient from z2 alone (sa_l3bwd.inc: sa_wgrad_pool_kernel) ------------------------------------
extern "C" int spacap_sa_wgrad_pool_supported(int C2, int C3, int S) { return wgrad_pool_shape(C2, C3, S) ? 1 : 0; }
namespace {
int wgrad_pool_grid(long R, int C2, int S) {
  // C2 = 64: two workgroups of four waves per CU; C2 = 128: one of eight (its partial is 197 KB: fewer, larger partials)
  long g = (long)bwd_cus() * (C2 == 64 ? 2 : 1), tiles = (R + S - 1) / S;
  if (g > NPART) g = NPART;
  if (g > tiles) g = tiles;
  return (int)(g < 1 ? 1 : g);
}
}  // namespace
/* workgroups (= partials, each spacap_sa_l3bwd_part_floats(C2, C3) floats) of spacap_sa_wgrad_pool_f32 */
extern "C" int spacap_sa_wgrad_pool_parts(long R, int C2, int C3, int S) {
  return wgrad_pool_shape(C2, C3, S) && R >= 1 ? wgrad_pool_grid(R, C2, S) : 0;
}
/* partial sums of dW3 = (g d)^T a2 + k0 (x) colsum(a2) - diag(k1) W3 (a2^T a2) of a pooled layer from (dym, arg), z2 and layer
   2's statistics: z3 is not read.  partW [spacap_sa_wgrad_pool_parts][spacap_sa_l3bwd_part_floats]; spacap_sa_l3bwd_dw_f32
   turns it into dW3. */
extern "C" int spacap_sa_wgrad_pool_f32(const float *dym, const uint8_t *arg, int S, const float *coef3, const float *z2,
                                        const float *st2, long R, int C3, int C2, float *partW, spacap_stream_t stream) {
  const char *what = "spacap_sa_wgrad_pool_f32";
  SPACAP_REQUIRE(dym && arg && coef3 && z2 && st2 && partW && R >= 1, "%s: bad arguments", what);
  SPACAP_REQUIRE(wgrad_pool_shape(C2, C3, S) && R % S == 0, "%s: (C2=%d, C3=%d, S=%d) unsupported", what, C2, C3, S);
  SPACAP_REQUIRE((reinterpret_cast<uintptr_t>(arg) & 3) == 0 && spacap::aligned16(z2, dym),
                 "%s: unaligned pointer (arg: 4 bytes, z2 / dym: 16 bytes)", what);
  const WPArgs a{dym, arg, coef3, z2, st2, R, partW};
  const int grid = wgrad_pool_grid(R, C2, S);
  hipStream_t s = spacap::as_stream(stream);
#define WP(C2V, C3V, SV) \
  hipLaunchKernelGGL((sa_wgrad_pool_kernel<C2V, C3V, SV, SV>), dim3(grid), dim3(C2V * 4), wgrad_pool_lds_bytes(C2V, C3V, SV, SV), s, a)
  if (C2 == 64) WP(64, 128, 64);
  else if (C3 == 128) WP(128, 128, 32);
  else WP(128, 256, 32);
#undef WP
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// dy: dense [R, CK] when arg == NULL, else the masked pooled gradient [R / S, CK] with its arg-max map
extern "C" int spacap_sa_dgrad_f32(const float *dy, const uint8_t *arg, int S, const float *zk, const float *coef,
                                   const float *Wk, const float *zp, const float *st_p, long R, int CK, int CP,
                                   float *dyp, double *part, spacap_stream_t stream) {
  const char *what = "spacap_sa_dgrad_f32";
  SPACAP_REQUIRE(dy && zk && coef && Wk && zp && st_p && dyp && part && R >= 1, "%s: bad arguments", what);
  SPACAP_REQUIRE(!arg || (S >= 1 && R % S == 0), "%s: bad S", what);
  hipStream_t s = spacap::as_stream(stream);
  // default: the streaming split-bf16 kernel (sa_bf3_dgrad.inc); SPACAP_SA_F32MFMA=1: the fp32-MFMA kernels
  if (!spacap::sa_f32_mfma_only() && (CK == 128 || CK == 256) && CP % 64 == 0 && R >= 49152) {   // (below: too few tiles per wave to pay for the weight staging)
    const size_t ldsd = bf3s_dgrad_lds_bytes(CK);
    const int gy = CP / 64;
    const unsigned gx = stream_grid(bwd_cus(), gy, R);
#define DS(CKV, PV)                                                                                                   \
  hipLaunchKernelGGL((sa_dgrad_bf3s_kernel<CKV, PV>), dim3(gx, gy), dim3(512), ldsd, s, dy, arg, S, zk, coef, Wk, CP, zp, \
                     st_p, R, dyp, part)
    if (CK == 128) { if (arg) DS(128, true); else DS(128, false); }
    else { if (arg) DS(256, true); else DS(256, false); }
#undef DS
    SPACAP_CHECK_LAUNCH(what);
    return SPACAP_OK;
  }
#define DG(CKV, NTV, PV, PF, AL, GY)                                                                                 \
  {                                                                                                                  \
    const size_t lds = (size_t)TM * ((CKV + 4) + ((AL) ? 0 : (64 * NTV + 4))) * sizeof(float);                       \
    static unsigned long long lds_ok = 0;                                                                            \
    if (lds > 65536)                                                                                                 \
      SPACAP_CHECK_HIP(spacap::allow_dynamic_lds(reinterpret_cast<const void *>(&sa_dgrad_kernel<CKV, NTV, PV, PF, AL>), \
                                                 (int)lds, lds_ok), what);                                           \
    static const int res = resident_blocks(sa_dgrad_kernel<CKV, NTV, PV, PF, AL>, lds);                              \
    hipLaunchKernelGGL((sa_dgrad_kernel<CKV, NTV, PV, PF, AL>), dim3(grid_rows(bwd_resident(res), GY, (R + TM - 1) / TM), GY), \
                       dim3(256), lds, s, dy, arg, S, zk, coef, Wk, CP, zp, st_p, R, dyp, part);                      \
  }
  if (arg && CK == 128 && CP == 64) DG(128, 1, true, true, false, 1)
  else if (arg && CK == 256 && CP == 128) DG(256, 1, true, false, true, 2)
  else if (arg && CK == 128 && CP == 128) DG(128, 2, true, true, false, 1)
  else if (!arg && CK == 64 && CP == 64) DG(64, 1, false, true, false, 1)
  else if (!arg && CK == 128 && CP == 128) DG(128, 2, false, true, false, 1)
  else SPACAP_REQUIRE(false, "%s: (CK=%d, CP=%d, pooled=%d) unsupported", what, CK, CP, arg ? 1 : 0);
#undef DG
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// ---- first-layer fusion of the layer-2 data gradient (sa_dgrad_kernel<64, 1, .., L1 = true, WG>): its three entry points -------
namespace {
// dz tile + output tile + the tile rows' four first-layer inputs
constexpr size_t DGRAD_L1_LDS = (size_t)TM * ((64 + 4) + (64 + 4) + 4) * sizeof(float);
template <bool WG>
int dgrad_l1_grid(long R) {
  static const int res = resident_blocks(sa_dgrad_kernel<64, 1, false, true, false, true, WG>, DGRAD_L1_LDS);
  return grid_rows(bwd_resident(res), 1, (R + TM - 1) / TM);
}
// dense dy [R, 64], CK = CP = 64; dy_prev is not written (zp: z1 as stored, or null when L.rel4 rebuilds it)
template <bool WG>
void launch_dgrad_l1(const float *dy, const float *zk, const float *coef, const float *Wk, const float *zp, const float *st_p, long R,
                     double *part, const L1Args &L, hipStream_t s) {
  hipLaunchKernelGGL((sa_dgrad_kernel<64, 1, false, true, false, true, WG>), dim3(dgrad_l1_grid<WG>(R), 1), dim3(256), DGRAD_L1_LDS, s, dy,
                     (const uint8_t *)nullptr, 0, zk, coef, Wk, 64, zp, st_p, R, (float *)nullptr, part, L);
}
}  // namespace

// Layer-2 data gradient of an SA module whose first layer reads (rel xyz, one inline feature) directly (SA1):
// as spacap_sa_dgrad_f32 with dense dy [R,64], but dy_prev is not written; instead part_l1 f32
// [spacap_sa_nparts()][64*8+4] receives per-workgroup sums (per channel c: S1[c,0:4], S3[c,0:4]; then S2[0:4]) from which
// the caller forms dW1 = g S1 + k0 S2 - k1 S3 once the layer-1 constants are known.
extern "C" int spacap_sa_dgrad_l1_f32(const float *dy, const float *zk, const float *coef, const float *Wk, const float *zp,
                                      const float *st_p, const float *feat, const float *xyz, const float *new_xyz,
                                      const int32_t *idx, float rdiv, int B, int Np, int N, int S, int CK, int CP,
                                      double *part, float *part_l1, spacap_stream_t stream) {
  const char *what = "spacap_sa_dgrad_l1_f32";
  SPACAP_REQUIRE(dy && zk && coef && Wk && zp && st_p && xyz && new_xyz && idx && part && part_l1 && rdiv > 0.f,
                 "%s: bad arguments", what);
  SPACAP_REQUIRE(CK == 64 && CP == 64, "%s: (CK=%d, CP=%d) unsupported", what, CK, CP);
  const long R = (long)B * N * S;
  hipStream_t s = spacap::as_stream(stream);
  L1Args L{feat, xyz, new_xyz, idx, rdiv, Np, N, S, part_l1, nullptr, L1In{nullptr, 0, 0}, nullptr};
  launch_dgrad_l1<false>(dy, zk, coef, Wk, zp, st_p, R, part, L, s);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// spacap_sa_dgrad_l1_f32 with the rows' inputs read from rel4 and z1 rebuilt from them (nothing of size R x 64 is read but dy, zk)
extern "C" int spacap_sa_dgrad_l1in_f32(const float *dy, const float *zk, const float *coef, const float *Wk, const float *rel4,
                                        const float *W1, int ldw, int has_feat, const float *st_p, int B, int N, int S, double *part,
                                        float *part_l1, spacap_stream_t stream) {
  const char *what = "spacap_sa_dgrad_l1in_f32";
  SPACAP_REQUIRE(dy && zk && coef && Wk && rel4 && W1 && st_p && part && part_l1 && ldw >= (has_feat ? 4 : 3), "%s: bad arguments", what);
  const long R = (long)B * N * S;
  L1Args L{nullptr, nullptr, nullptr, nullptr, 1.f, 1, N, S, part_l1, rel4, L1In{W1, ldw, has_feat}, nullptr};
  launch_dgrad_l1<false>(dy, zk, coef, Wk, nullptr, st_p, R, part, L, spacap::as_stream(stream));
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// spacap_sa_dgrad_l1in_f32 that ALSO leaves the layer's weight-gradient partials: partW f32 [spacap_sa_dgrad_wgrad_l1in_slabs(R)][64][64],
// summed by the caller in slab order (what spacap_sa_wgrad_l1in_f32 computes from a second pass over dy and zk)
extern "C" int spacap_sa_dgrad_wgrad_l1in_slabs(long R) { return R >= 1 ? dgrad_l1_grid<true>(R) : 0; }
extern "C" int spacap_sa_dgrad_wgrad_l1in_f32(const float *dy, const float *zk, const float *coef, const float *Wk, const float *rel4,
                                              const float *W1, int ldw, int has_feat, const float *st_p, int B, int N, int S,
                                              double *part, float *part_l1, float *partW, spacap_stream_t stream) {
  const char *what = "spacap_sa_dgrad_wgrad_l1in_f32";
  SPACAP_REQUIRE(dy && zk && coef && Wk && rel4 && W1 && st_p && part && part_l1 && partW && ldw >= (has_feat ? 4 : 3), "%s: bad arguments", what);
  const long R = (long)B * N * S;
  L1Args L{nullptr, nullptr, nullptr, nullptr, 1.f, 1, N, S, part_l1, rel4, L1In{W1, ldw, has_feat}, partW};
  launch_dgrad_l1<true>(dy, zk, coef, Wk, nullptr, st_p, R, part, L, spacap::as_stream(stream));
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// dW1 of the fused first-layer backward from its three sums (L1Args): part_l1 [nparts][C1 * 8 + 4] = per workgroup
// (S1 [C1][4] | S3 [C1][4]) interleaved per channel as [c][2][4], then S2 [4]; coef [C1][4] = (g, k0, k1, .) of layer 1:
//   dW1[c][d] = g[c] S1[c][d] + k0[c] S2[d] - k1[c] S3[c][d],  sums over the partials in double, d < ldw columns written.
namespace {
// one workgroup per channel c: its 12 sums (S1[c][0..3], S3[c][0..3], S2[0..3]) over the partial rows, 16 lanes per sum with
// independent loads (the first version ran the nparts loads of every sum as one dependent chain on ONE workgroup: 262 us),
// lanes combined in a fixed order in double
__global__ __launch_bounds__(256) void sa_l1_dw_kernel(const float *__restrict__ part_l1, int nparts, const float *__restrict__ coef,
                                                       int C1, int ldw, float *__restrict__ dW1) {
  __shared__ double s_lane[12][17];
  __shared__ double s_sum[12];
  const int c = blockIdx.x, tid = threadIdx.x, sidx = tid >> 4, l = tid & 15;
  const int n = C1 * 8 + 4;
  if (sidx < 12) {
    const int e = sidx < 8 ? c * 8 + sidx : C1 * 8 + (sidx - 8);   // [c][2][4] then S2 [4]
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int p = l;
    for (; p + 48 < nparts; p += 64) {
      a0 += (double)part_l1[(size_t)p * n + e];
      a1 += (double)part_l1[(size_t)(p + 16) * n + e];
      a2 += (double)part_l1[(size_t)(p + 32) * n + e];
      a3 += (double)part_l1[(size_t)(p + 48) * n + e];
    }
    for (; p < nparts; p += 16) a0 += (double)part_l1[(size_t)p * n + e];
    s_lane[sidx][l] = (a0 + a1) + (a2 + a3);
  }
  __syncthreads();
  if (tid < 12) {
    double a = 0.0;
    for (int i = 0; i < 16; ++i) a += s_lane[tid][i];
    s_sum[tid] = a;
  }
  __syncthreads();
  if (tid < ldw) {
    const double g = coef[c * 4 + 0], k0 = coef[c * 4 + 1], k1 = coef[c * 4 + 2];
    dW1[c * ldw + tid] = (float)(g * s_sum[tid] + k0 * s_sum[8 + tid] - k1 * s_sum[4 + tid]);
  }
}
}  // namespace
extern "C" int spacap_sa_l1_dw_f32(const float *part_l1, int nparts, const float *coef, int C1, int ldw, float *dW1,
                                   spacap_stream_t stream) {
  const char *what = "spacap_sa_l1_dw_f32";
  SPACAP_REQUIRE(part_l1 && coef && dW1 && nparts >= 1 && C1 >= 1 && C1 <= 512 && ldw >= 1 && ldw <= 4, "%s: bad arguments", what);
  hipLaunchKernelGGL(sa_l1_dw_kernel, dim3(C1), dim3(256), 0, spacap::as_stream(stream), part_l1, nparts, coef, C1, ldw, dW1);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// partW: [spacap_sa_wgrad_slabs(R,CK,CP,pooled)][CK][CP] partial weight gradients, summed by the caller in slab order
extern "C" int spacap_sa_wgrad_f32(const float *dy, const uint8_t *arg, int S, const float *zk, const float *coef,
                                   const float *zp, const float *st_p, long R, int CK, int CP, float *partW,
                                   spacap_stream_t stream) {
  const char *what = "spacap_sa_wgrad_f32";
  SPACAP_REQUIRE(dy && zk && coef && zp && st_p && partW && R >= 1, "%s: bad arguments", what);
  SPACAP_REQUIRE(!arg || (S >= 1 && R % S == 0), "%s: bad S", what);
  hipStream_t s = spacap::as_stream(stream);
  const int nslab = spacap_sa_wgrad_slabs(R, CK, CP, arg ? 1 : 0);
#define WG(CKB, CPV, PV) \
  hipLaunchKernelGGL((sa_wgrad_kernel<CKB, CPV, PV>), dim3(nslab, CK / CKB), dim3(256), 0, s, dy, arg, S, zk, coef, CK, zp, st_p, R, partW)
  if (arg && CK % 128 == 0 && CP == 64) WG(128, 64, true);
  else if (arg && CK % 128 == 0 && CP == 128) WG(128, 128, true);
  else if (!arg && CK == 64 && CP == 64) WG(64, 64, false);
  else if (!arg && CK == 128 && CP == 128) WG(128, 128, false);
  else SPACAP_REQUIRE(false, "%s: (CK=%d, CP=%d, pooled=%d) unsupported", what, CK, CP, arg ? 1 : 0);
#undef WG
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// dy1 is overwritten with dz1 when write_dz != 0 (only the rows -> source points scatter of the feature gradient
// needs it); partW [spacap_sa_nparts()][C1][4] (columns: rel x, y, z, inline feature)
extern "C" int spacap_sa_l1_bwd_f32(float *dy1, const float *z1, const float *coef, const float *feat, const float *xyz,
                                    const float *new_xyz, const int32_t *idx, const float *W1, int ldw, float rdiv, int B,
                                    int Np, int N, int S, int C1, float *partW, float *drel, int write_dz,
                                    spacap_stream_t stream) {
  const char *what = "spacap_sa_l1_bwd_f32";
  SPACAP_REQUIRE(dy1 && z1 && coef && xyz && new_xyz && idx && W1 && partW && rdiv > 0.f, "%s: bad arguments", what);
  SPACAP_REQUIRE(C1 == 64 || C1 == 128, "%s: C1=%d unsupported", what, C1);
  const long R = (long)B * N * S;
  hipStream_t s = spacap::as_stream(stream);
  if (C1 == 64)
    hipLaunchKernelGGL((sa_l1_bwd_kernel<64>), dim3(NPART), dim3(256), 0, s, dy1, z1, coef, feat, xyz, new_xyz, idx, W1, ldw, rdiv, Np, N, S, R, partW, drel, write_dz);
  else
    hipLaunchKernelGGL((sa_l1_bwd_kernel<128>), dim3(NPART), dim3(256), 0, s, dy1, z1, coef, feat, xyz, new_xyz, idx, W1, ldw, rdiv, Np, N, S, R, partW, drel, write_dz);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// dW1 f32 [C1, 3 + Cf] from pw1 f32 [n1][C1][4] (spacap_sa_l1_bwd_f32) and pf f32 [nf][C1 * Cf] (spacap_linear_wgrad_f32 of the
// feature product): columns 0..2 and 3.. in one launch, the values of spacap_sum_slabs_f32 on each + a concatenation
extern "C" int spacap_sa_dw1_assemble_f32(const float *pw1, int n1, const float *pf, int nf, int C1, int Cf, float *dW1,
                                          spacap_stream_t stream) {
  const char *what = "spacap_sa_dw1_assemble_f32";
  SPACAP_REQUIRE(pw1 && pf && dW1 && n1 >= 1 && nf >= 1 && C1 >= 1 && Cf >= 1, "%s: bad arguments", what);
  hipLaunchKernelGGL(sa_dw1_assemble_kernel, dim3(nblocks((long)C1 * (3 + Cf), 64)), dim3(256), 0, spacap::as_stream(stream), pw1, n1, pf,
                     nf, C1, Cf, dW1);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
