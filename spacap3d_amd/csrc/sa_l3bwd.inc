// Weight gradient of the POOLED last layer of a shared MLP from its INPUT pre-activation z2 alone; included by sa_bwd.hip (uses
// ld4, st4, f32x4, MFMA16 of mfma.hpp and NPART).
//
// Reference: the autograd backward of  Conv2d 1x1 -> BatchNorm2d -> ReLU -> max_pool2d  (lib/pointnet2/pytorch_utils.py:11-36,
// lib/pointnet2/pointnet2_modules.py:256-259).  With a2 = relu(bn(z2)) [R, C2] the layer's input, z3 = a2 W3^T its
// pre-activation and d [R, C3] the pooled gradient routed to the arg-max rows (ONE non-zero per group and channel), the
// BatchNorm backward is  dz3 = g d + k0 - k1 z3  with per-channel constants (sa_bwd_finalize_kernel), and because z3 is a
// linear function of a2 the weight gradient does not need z3:
//     dW3 = dz3^T a2          = (g d)^T a2  +  k0 (x) colsum(a2)  -  diag(k1) W3 (a2^T a2)
// (The DATA gradient has the same property, dy2 = (g d) W3 + k0 W3 - a2 W3^T diag(k1) W3; a kernel for it was built in round 4,
// measured 2x slower than the stored-z3 data-gradient kernel and moved to tools/lab/sa_l3bwd_data_half/ in round 5.)
// Partials per workgroup: [C3][C2] (g d)^T a2 | [C2][C2] Gram | [C2] colsum(a2); summed and combined by sa_l3_sum_kernel / sa_l3_dw_kernel.

// sums[e] = sum over the workgroups' partials, in double (e over [C3][C2] | [C2][C2] | [C2], a multiple of 4 elements).  Block =
// 64 elements x 16 lanes over the partials: a lane reads 16 bytes of every 16th partial, eight loads in flight (256 contiguous
// bytes per partial and 16 threads), its sums in order; the 16 lanes are combined in order.
__global__ __launch_bounds__(256) void sa_l3_sum_kernel(const float *__restrict__ partW, int nparts, long n, double *__restrict__ sums) {
  __shared__ double s_l[16][65];
  const int q = threadIdx.x & 15, l = threadIdx.x >> 4;
  const long e0 = (long)blockIdx.x * 64 + q * 4;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  if (e0 < n) {
    const float *pp = partW + e0;
    int p = l;
    for (; p + 7 * 16 < nparts; p += 8 * 16) {
      f32x4 t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = ld4(pp + (size_t)(p + 16 * u) * n);
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] += (double)t[u][k];
    }
    for (; p < nparts; p += 16) {
      const f32x4 t = ld4(pp + (size_t)p * n);
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] += (double)t[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) s_l[l][q * 4 + k] = a[k];
  __syncthreads();
  if (threadIdx.x < 64 && (long)blockIdx.x * 64 + threadIdx.x < n) {
    double v = 0.0;
    for (int i = 0; i < 16; ++i) v += s_l[i][threadIdx.x];
    sums[(long)blockIdx.x * 64 + threadIdx.x] = v;
  }
}

// dW3[c][k] = Sgd[c][k] + k0[c] colsum[k] - k1[c] sum_j W3[c][j] Gram[j][k]   (block c; threads = k x slices of j)
__global__ __launch_bounds__(1024) void sa_l3_dw_kernel(const double *__restrict__ sums, const float *__restrict__ coef3,
                                                        const float *__restrict__ W3, int C3, int C2, float *__restrict__ dW3) {
  __shared__ double s_p[1024];
  const int c = blockIdx.x, k = threadIdx.x % C2, sl = threadIdx.x / C2, nsl = 1024 / C2;
  const double *gram = sums + (size_t)C3 * C2, *cs = gram + (size_t)C2 * C2;
  double acc = 0.0;
  for (int j0 = sl * 8; j0 < C2; j0 += nsl * 8) {
    double gv[8];
    float wv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = j0 + u < C2 ? j0 + u : C2 - 1;
      gv[u] = gram[(size_t)j * C2 + k];
      wv[u] = W3[(size_t)c * C2 + j];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (j0 + u < C2) acc += (double)wv[u] * gv[u];
  }
  s_p[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < C2) {
    double v = 0.0;
    for (int i = 0; i < nsl; ++i) v += s_p[i * C2 + threadIdx.x];
    const double k0 = coef3[c * 4 + 1], k1 = coef3[c * 4 + 2];
    dW3[(size_t)c * C2 + threadIdx.x] = (float)(sums[(size_t)c * C2 + threadIdx.x] + k0 * cs[threadIdx.x] - k1 * v);
  }
}

// ---- weight gradient of the pooled layer from z2 alone (the stored-z3 path's replacement for sa_wgrad_kernel<.., POOLED>) --------
// dW3 = (g d)^T a2 + k0 (x) colsum(a2) - diag(k1) W3 (a2^T a2): one pass over z2 (C2 floats per row) where the dense kernel
// streams z3 AND z2 (C3 + C2 floats per row) and multiplies a [C3 x rows] operand that is zero but for one row per group and
// channel.  Per tile (= one group of S rows; two tiles of rows ahead in registers, the a2 tile double-buffered in LDS, one
// barrier per tile):
//   * Gram += a2^T a2, fp32 MFMA 16x16x4, operands 16 bytes at a time along the columns ("column classes", see above); the
//     matrix is symmetric: wave w computes class w against the classes w, w + 1, .., w + NCL / 2 (mod NCL) and both triangles
//     are written at the end -- 5 / 8 (C2 = 128) or 3 / 4 (C2 = 64) of the full product's matrix instructions
//   * the sparse term: wave w owns the NI consecutive channels c3 = w NI ..; their (d, arg-max row offset) of the group travel
//     with the tile (requested two tiles ahead, staged into LDS next to a2) and are read back as 16-byte broadcasts (the same
//     address in every lane); the lane reads its one / two columns of the chosen a2 row and the sum lives in registers; the
//     iterations sit between the matrix instructions of the k steps (they issue while the MFMA pipe works).  g is applied
//     once at the end.
// Measured at SA1 (1 048 576 rows, 64 -> 128; tools/lab/wgrad_pool_bench.py): this form 92 us against 249 us of the dense
// kernel.  Tried and slower: scalar loads of (d, arg) at the start of each tile (every tile waits a memory latency: 120 us);
// (d, row) per lane + v_readlane instead of the LDS broadcasts (108 us: 130 more VALU instructions per tile and wave); three or
// four tiles of rows in flight instead of two, 64-row tiles at C2 = 128, three workgroups per CU (all 98 - 110 us: the pass is
// not short of bytes in flight -- a bare 16-KB-tile skeleton streams 268 MB in 38 us, tools/lab/hbm_stream.hip -- but of
// issue slots: per tile and wave 40 matrix instructions, ~250 VALU, ~50 LDS instructions behind one barrier, two waves per
// SIMD; rocprofv3 counters (tools/lab/pmc_passes.sh): matrix pipe busy 31 %, VALU 31 %, not overlapped).
// Partials per workgroup as for sa_l3bwd_kernel: [C3][C2] | [C2][C2] | [C2]; summed and combined by sa_l3_sum_kernel / sa_l3_dw_kernel.
struct WPArgs {
  const float *dym;       // [G][C3] masked pooled gradient
  const uint8_t *arg;     // [G][C3] arg-max row within the group
  const float *coef3;     // [C3][4] (g, k0, k1, -)
  const float *z2;        // [R][C2]
  const float *st2;       // [C2][4]
  long R;
  float *partW;           // [gridDim.x][C3 * C2 + C2 * C2 + C2]
};

template <int W, int C2, int C3, int TMT, int S>
__device__ __forceinline__ void wp_tile(const float *sa, const float *sv, const int *sr, f32x4 (&accG)[C2 / 32 + 1],
                                        float (&sacc)[C3 / (C2 / 16)][C2 / 64], int lane) {
  constexpr int NCL = C2 / 16, CH = C2 / 64, CPL = C2 / 64, NI = C3 / NCL, ND = NCL / 2 + 1, NDW = W < NCL / 2 ? ND : ND - 1;
  constexpr int LDA = C2 + 20, KS = TMT / 4, NG = TMT / S, IPK = NG * NI / KS;
  static_assert((NG * NI) % KS == 0 && NI % 4 == 0 && (IPK % 4 == 0 || 4 % IPK == 0), "sparse items per k step");
  using i32x4 = int __attribute__((ext_vector_type(4)));
  const int l15 = lane & 15, lg = lane >> 4;
  const float *pb = sa + lg * LDA + 4 * l15;
  const float *psp = sa + CPL * lane;
  // this wave's channels W NI .. of the tile's groups: (d, row offset) out of LDS, the same address in every lane
  const f32x4 *qv = reinterpret_cast<const f32x4 *>(sv) + W * (NI / 4);
  const i32x4 *qr = reinterpret_cast<const i32x4 *>(sr) + W * (NI / 4);
  f32x4 vn[CH], vc[CH], dv;
  i32x4 dr;
#pragma unroll
  for (int hh = 0; hh < CH; ++hh) vn[hh] = ld4(pb + 64 * hh);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
    for (int hh = 0; hh < CH; ++hh) vc[hh] = vn[hh];
    if (ks + 1 < KS) {
#pragma unroll
      for (int hh = 0; hh < CH; ++hh) vn[hh] = ld4(pb + (ks + 1) * 4 * LDA + 64 * hh);
    }
    const float ac = vc[W / 4][W % 4];
#pragma unroll
    for (int d = 0; d < NDW; ++d) {
      const int n = (W + d) % NCL;
      accG[d] = MFMA16(ac, vc[n / 4][n % 4], accG[d]);
    }
#pragma unroll
    for (int j = 0; j < IPK; ++j) {
      const int e = ks * IPK + j, gi = e / NI, i = e % NI;
      if (e % 4 == 0) dv = qv[gi * (C3 / 4) + i / 4], dr = qr[gi * (C3 / 4) + i / 4];
      const float *p = psp + dr[e % 4];
      if (CPL == 1) {
        sacc[i][0] = __builtin_fmaf(dv[e % 4], p[0], sacc[i][0]);
      } else {
        const float2 x = *reinterpret_cast<const float2 *>(p);
        sacc[i][0] = __builtin_fmaf(dv[e % 4], x.x, sacc[i][0]);
        sacc[i][CPL - 1] = __builtin_fmaf(dv[e % 4], x.y, sacc[i][CPL - 1]);
      }
    }
  }
}

template <int C2, int C3, int TMT, int S>
__global__ __launch_bounds__(C2 * 4) void sa_wgrad_pool_kernel(const WPArgs a) {
  constexpr int NT = C2 * 4, NW = NT / 64, NCL = C2 / 16, CPL = C2 / 64, NI = C3 / NW, ND = NCL / 2 + 1, NG = TMT / S;
  constexpr int LDA = C2 + 20, C4 = C2 / 4, RSTEP = NT / C4, NV = TMT / RSTEP, NGL = NG * C3 / 4, TILE = TMT * LDA + 2 * NG * C3;
  static_assert(NCL == NW && RSTEP == 16 && TMT % S == 0 && (C2 == 64 || C2 == 128) && NGL <= NT, "thread maps");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *s_c = smem;                       // [3][C2]   mean, gamma / std, beta of layer 2
  float *s_a = s_c + 4 * C2;               // [2]{[TMT][LDA] a2 | [NG][C3] d | [NG][C3] row offset}: the tile being multiplied, the next one
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c4 = tid % C4, r0 = tid / C4;
  const long ntiles = a.R / TMT;           // (R is a multiple of the tile)
  for (int c = tid; c < C2; c += NT) {
    const float *s = a.st2 + (size_t)c * 4;
    s_c[c] = s[0], s_c[C2 + c] = s[2], s_c[2 * C2 + c] = s[3];
  }
  __syncthreads();
  const f32x4 pm = ld4(&s_c[c4 * 4]), ps = ld4(&s_c[C2 + c4 * 4]), pb = ld4(&s_c[2 * C2 + c4 * 4]);
  float sacc[NI][CPL];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int e = 0; e < CPL; ++e) sacc[i][e] = 0.f;
  f32x4 accG[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) accG[d] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 csum = {0.f, 0.f, 0.f, 0.f};
  struct Rows {
    f32x4 z[NV];      // this thread's pieces of the tile's rows of z2
    f32x4 d;          // threads < NGL: four channels of a group's pooled gradient ...
    uint32_t r;       // ... and their arg-max rows
  };
  Rows pA, pB;
  auto request = [&](Rows &p, long t) {
    const long row0 = t * TMT;
#pragma unroll
    for (int i = 0; i < NV; ++i) p.z[i] = ld4(a.z2 + (size_t)(row0 + r0 + i * RSTEP) * C2 + c4 * 4);
    if (tid < NGL) {
      const size_t o = (size_t)(row0 / S) * C3 + tid * 4;   // (the tile's groups are consecutive: [NG][C3])
      p.d = ld4(a.dym + o);
      p.r = *reinterpret_cast<const uint32_t *>(a.arg + o);
    }
  };
  auto stage = [&](const Rows &p, float *sa) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      f32x4 av;
#pragma unroll
      for (int u = 0; u < 4; ++u) av[u] = fmaxf((p.z[i][u] - pm[u]) * ps[u] + pb[u], 0.f);
      csum += av;
      st4(&sa[(r0 + i * RSTEP) * LDA + c4 * 4], av);
    }
    if (tid < NGL) {
      using i32x4 = int __attribute__((ext_vector_type(4)));
      const int gi = tid / (C3 / 4);
      i32x4 ro;
#pragma unroll
      for (int u = 0; u < 4; ++u) ro[u] = ((int)((p.r >> (8 * u)) & 255u) + gi * S) * LDA;
      st4(&sa[TMT * LDA + tid * 4], p.d);
      *reinterpret_cast<i32x4 *>(&sa[TMT * LDA + NG * C3 + tid * 4]) = ro;
    }
  };
  auto compute = [&](const float *sa) {
    const float *sv = sa + TMT * LDA;
    const int *sr = reinterpret_cast<const int *>(sv + NG * C3);
    switch (w) {
#define WP_CASE(WV)                                                                              \
  case WV:                                                                                       \
    if (WV < NW) wp_tile<(WV < NW ? WV : 0), C2, C3, TMT, S>(sa, sv, sr, accG, sacc, lane);      \
    break;
      WP_CASE(0) WP_CASE(1) WP_CASE(2) WP_CASE(3) WP_CASE(4) WP_CASE(5) WP_CASE(6) WP_CASE(7)
#undef WP_CASE
      default: break;
    }
  };
  long t = blockIdx.x;
  const long g = gridDim.x;
  if (t < ntiles) request(pA, t);
  if (t + g < ntiles) request(pB, t + g);
  while (t < ntiles) {
    stage(pA, s_a);
    if (t + 2 * g < ntiles) request(pA, t + 2 * g);
    __syncthreads();
    compute(s_a);
    t += g;
    if (t >= ntiles) break;
    stage(pB, s_a + TILE);
    if (t + 2 * g < ntiles) request(pB, t + 2 * g);
    __syncthreads();
    compute(s_a + TILE);
    t += g;
  }

  // ---- partial results of this workgroup ----
  const int l15 = lane & 15, lg = lane >> 4;
  float *pw = a.partW + (size_t)blockIdx.x * ((size_t)C3 * C2 + C2 * C2 + C2);
  float *pg = pw + (size_t)C3 * C2;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int c = w * NI + i;
    const float gc = a.coef3[(size_t)c * 4];
#pragma unroll
    for (int e = 0; e < CPL; ++e) pw[(size_t)c * C2 + CPL * lane + e] = gc * sacc[i][e];
  }
  // accG[d][u] = Gram[c_i][c_j]: c_i = 64 (w / 4) + 4 (4 lg + u) + w % 4 (class w), c_j = 64 (n / 4) + 4 l15 + n % 4, n = (w + d) % NCL
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    if (d == ND - 1 && w >= NCL / 2) continue;   // the class pair (w, w + NCL / 2) belongs to the lower wave
    const int n = (w + d) % NCL;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ci = 64 * (w / 4) + 4 * (4 * lg + u) + (w % 4), cj = 64 * (n / 4) + 4 * l15 + (n % 4);
      pg[(size_t)ci * C2 + cj] = accG[d][u];
      if (d > 0) pg[(size_t)cj * C2 + ci] = accG[d][u];
    }
  }
  __syncthreads();
  float *s_red = s_a;   // [RSTEP][C2]
  st4(&s_red[r0 * C2 + c4 * 4], csum);
  __syncthreads();
  if (tid < C2) {
    float vsum = 0.f;
    for (int i = 0; i < RSTEP; ++i) vsum += s_red[i * C2 + tid];
    pg[(size_t)C2 * C2 + tid] = vsum;
  }
}

inline size_t wgrad_pool_lds_bytes(int C2, int C3, int TMT, int S) {
  return ((size_t)4 * C2 + (size_t)2 * (TMT * (C2 + 20) + 2 * (TMT / S) * C3)) * sizeof(float);
}
inline bool wgrad_pool_shape(int C2, int C3, int S) {
  return (C2 == 64 && C3 == 128 && S == 64) || (C2 == 128 && (C3 == 128 || C3 == 256) && S == 32);
}
