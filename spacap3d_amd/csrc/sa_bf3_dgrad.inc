// Streaming split-bf16 data-gradient kernel of the shared MLP; included by sa_bwd.hip (uses ld4, f32x4, bf16x8, bf16x4, split3 of
// mfma.hpp and f32x16, MFMA_BF16, NPART, dpp_xor1 / dpp_xor2 of sa_common.hpp).
//
//   dz_k[r, c]   = g[c] d[r, c] + k0[c] - k1[c] z_k[r, c]          BatchNorm backward of layer k (coef from sa_bwd_finalize)
//                  d = dy[r, c] (dense) or (arg[r / S, c] == r % S ? dy[r / S, c] : 0) (the max-pool's gradient)
//   dy_prev[r, o] = [relu(bn(z_prev[r, o])) > 0] * sum_c dz_k[r, c] W_k[c, o],   and the BN sums of dy_prev
//   (sum dy_prev, sum dy_prev * xhat(z_prev)) per output channel -- the backward of one Conv2d(1x1) -> BatchNorm2d -> ReLU link
//   of the reference's SharedMLP (lib/pointnet2/pytorch_utils.py), evaluated as in sa_dgrad_kernel.
//
// Organisation: that of sa_mid_fwd_bf3s_kernel (sa_bf3.inc) -- W_k^T for one block of 64 output channels resident in LDS as
// three bf16 images [64][CK + 8], waves own 32-row tiles end to end, slices of 32 channels of z_k (and of dy, or of the
// group's pooled dy + arg) land in AGPRs one slice ahead, dz is formed and split in registers, 6 MFMAs per product.  The
// epilogue transposes every 4 x 4 quad block, so that a lane holds 4 consecutive channels of one row: z_prev is read and
// dy_prev written as 16-byte pieces of whole lines, the sums are per-lane and reduced over the 8 lanes of a channel
// quartet once, at the end.
#define SPACAP_ACLOB_D                                                                                                 \
  "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17",  \
      "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", "a32", "a33",  \
      "a34", "a35", "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", "a48", "a49",  \
      "a50", "a51", "a52", "a53", "a54", "a55", "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", "a64", "a65",  \
      "a66", "a67", "a68", "a69", "a70", "a71"
#define SPACAP_LANDING_FENCE_D() asm volatile("" ::: SPACAP_ACLOB_D)

template <int CK, bool POOLED>
__global__ __launch_bounds__(512) void sa_dgrad_bf3s_kernel(const float *__restrict__ dy, const uint8_t *__restrict__ arg, int S,
                                                            const float *__restrict__ zk, const float *__restrict__ coef,
                                                            const float *__restrict__ Wk, int CP, const float *__restrict__ zp,
                                                            const float *__restrict__ st_p, long R, float *__restrict__ dyp,
                                                            double *__restrict__ part) {
  constexpr int LDW = CK + 8, NH = CK / 32, KP = 2, NJ = 4, NBUF = 2, COB = 64, WIMG = COB * LDW, NCQ = COB / 32, NW = 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __bf16 *wimg = reinterpret_cast<__bf16 *>(smem_raw);                         // [3][COB][LDW]   W_k^T, K-permuted
  f32x4 *s_co = reinterpret_cast<f32x4 *>(smem_raw + (size_t)3 * WIMG * 2);    // [CK / 4][3]     (g, k0, k1) of layer k
  f32x4 *s_pp = s_co + 3 * (CK / 4);                                           // [COB / 4][4]    (mean, istd, scale, shift) of z_prev
  float *s_red = reinterpret_cast<float *>(s_pp + 4 * (COB / 4));              // [NW][2][COB]
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, kk = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cbb = blockIdx.y * COB;
  // W_k is [CK][CP]: thread (c, o4) takes 4 consecutive output channels of input channel c and scatters them over the images'
  // rows o .. o + 3 at the permuted position of c (chunk q = c / 4 = 4 s + 2 half + g -> 16 s + 8 g + 4 half, + c % 4)
  for (int i = tid; i < CK * (COB / 4); i += 512) {
    const int c = i / (COB / 4), o4 = i % (COB / 4);
    const f32x4 v = ld4(Wk + (size_t)c * CP + cbb + 4 * o4);
    const int q = c >> 2, pos = 16 * (q >> 2) + 8 * (q & 1) + 4 * ((q >> 1) & 1) + (c & 3);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      __bf16 h, m, l;
      split3(v[u], h, m, l);
      __bf16 *dst = wimg + (4 * o4 + u) * LDW + pos;
      dst[0] = h, dst[WIMG] = m, dst[2 * WIMG] = l;
    }
  }
  for (int i = tid; i < CK; i += 512) {
    float *p = reinterpret_cast<float *>(s_co + 3 * (i / 4));
    p[i % 4] = coef[(size_t)i * 4], p[4 + i % 4] = coef[(size_t)i * 4 + 1], p[8 + i % 4] = coef[(size_t)i * 4 + 2];
  }
  for (int i = tid; i < COB; i += 512) {
    float *p = reinterpret_cast<float *>(s_pp + 4 * (i / 4));
#pragma unroll
    for (int k = 0; k < 4; ++k) p[4 * k + i % 4] = st_p[(size_t)(cbb + i) * 4 + k];
  }
  __syncthreads();

  const long ntiles = (R + 31) / 32, nfull = R / 32;
  const long gw = (long)blockIdx.x * NW + w, GW = (long)gridDim.x * NW;
  const int q4 = l31 & 3, a8 = l31 >> 2;
  const bool odd = q4 & 1, hi = q4 & 2;
  const unsigned lane_off = (unsigned)((4 * kk + q4) * CP + 4 * a8);   // row 4 kk + q4, channels 4 a8 ..
  const int lgS = (POOLED && (S & (S - 1)) == 0) ? __builtin_ctz((unsigned)S) : -1;
  f32x4 s1[NCQ], s2[NCQ];
#pragma unroll
  for (int c = 0; c < NCQ; ++c) s1[c] = s2[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x16 acc[NCQ];

  // landing registers (named literally, see sa_bf3.inc): buffer B = a[36 B .. 36 B + 35]: 16 of z_k, 16 of dy, 4 of arg
#define SPACAP_FETCH_D(NAME, Z0, Z1, Z2, Z3, D0, D1, D2, D3, G0, G1, G2, G3)                                            \
  auto NAME = [&](long t, int h) {                                                                                     \
    const long left = R - t * 32;                                                                                      \
    const int r = l31 < left ? l31 : (int)left - 1;                                                                    \
    const long grow = t * 32 + r;                                                                                      \
    const float *sz = zk + (size_t)grow * CK + 32 * h + 4 * kk;                                                        \
    if (POOLED) {                                                                                                      \
      const long grp = lgS >= 0 ? (grow >> lgS) : grow / S;                                                            \
      const float *sd = dy + (size_t)grp * CK + 32 * h + 4 * kk;                                                       \
      const uint8_t *sa = arg + (size_t)grp * CK + 32 * h + 4 * kk;                                                    \
      asm volatile("global_load_dwordx4 " Z0 ", %0, off\n\tglobal_load_dwordx4 " Z1 ", %0, off offset:32\n\t"         \
                   "global_load_dwordx4 " Z2 ", %0, off offset:64\n\tglobal_load_dwordx4 " Z3 ", %0, off offset:96\n\t" \
                   "global_load_dwordx4 " D0 ", %1, off\n\tglobal_load_dwordx4 " D1 ", %1, off offset:32\n\t"         \
                   "global_load_dwordx4 " D2 ", %1, off offset:64\n\tglobal_load_dwordx4 " D3 ", %1, off offset:96\n\t" \
                   "global_load_dword " G0 ", %2, off\n\tglobal_load_dword " G1 ", %2, off offset:8\n\t"              \
                   "global_load_dword " G2 ", %2, off offset:16\n\tglobal_load_dword " G3 ", %2, off offset:24"       \
                   :                                                                                                   \
                   : "v"(sz), "v"(sd), "v"(sa)                                                                         \
                   : "memory", SPACAP_ACLOB_D);                                                                        \
    } else {                                                                                                           \
      const float *sd = dy + (size_t)grow * CK + 32 * h + 4 * kk;                                                      \
      asm volatile("global_load_dwordx4 " Z0 ", %0, off\n\tglobal_load_dwordx4 " Z1 ", %0, off offset:32\n\t"         \
                   "global_load_dwordx4 " Z2 ", %0, off offset:64\n\tglobal_load_dwordx4 " Z3 ", %0, off offset:96\n\t" \
                   "global_load_dwordx4 " D0 ", %1, off\n\tglobal_load_dwordx4 " D1 ", %1, off offset:32\n\t"         \
                   "global_load_dwordx4 " D2 ", %1, off offset:64\n\tglobal_load_dwordx4 " D3 ", %1, off offset:96"    \
                   :                                                                                                   \
                   : "v"(sz), "v"(sd)                                                                                  \
                   : "memory", SPACAP_ACLOB_D);                                                                        \
    }                                                                                                                  \
  };
  SPACAP_FETCH_D(fetch0, "a[0:3]", "a[4:7]", "a[8:11]", "a[12:15]", "a[16:19]", "a[20:23]", "a[24:27]", "a[28:31]", "a32", "a33",
                 "a34", "a35")
  SPACAP_FETCH_D(fetch1, "a[36:39]", "a[40:43]", "a[44:47]", "a[48:51]", "a[52:55]", "a[56:59]", "a[60:63]", "a[64:67]", "a68",
                 "a69", "a70", "a71")
#undef SPACAP_FETCH_D
  auto fetch = [&](long pq) {
    const long t = gw + (pq / NH) * GW;
    const int h = (int)(pq % NH);
    if (pq % NBUF == 0) fetch0(t, h);
    else fetch1(t, h);
  };
  constexpr int NLD = POOLED ? 12 : 8;   // loads per slice

  auto phase = [&](long t, auto hc, auto bc, auto full, bool steady, long pnext) {
    constexpr int H = decltype(hc)::value, BUF = decltype(bc)::value;
    constexpr bool FULL = decltype(full)::value;
    const long row0 = t * 32;
    constexpr int STEADY = NLD * (NBUF - 1);   // loads retire in order among themselves (see sa_bf3.inc)
    float x[16], dd[16];
    unsigned am[4];
    {
#define SPACAP_RD16(DST, BASE)                                                                                         \
  asm volatile("v_accvgpr_read_b32 %0, a[" #BASE "+0]\n\tv_accvgpr_read_b32 %1, a[" #BASE "+1]\n\t"                    \
               "v_accvgpr_read_b32 %2, a[" #BASE "+2]\n\tv_accvgpr_read_b32 %3, a[" #BASE "+3]\n\t"                    \
               "v_accvgpr_read_b32 %4, a[" #BASE "+4]\n\tv_accvgpr_read_b32 %5, a[" #BASE "+5]\n\t"                    \
               "v_accvgpr_read_b32 %6, a[" #BASE "+6]\n\tv_accvgpr_read_b32 %7, a[" #BASE "+7]\n\t"                    \
               "v_accvgpr_read_b32 %8, a[" #BASE "+8]\n\tv_accvgpr_read_b32 %9, a[" #BASE "+9]\n\t"                    \
               "v_accvgpr_read_b32 %10, a[" #BASE "+10]\n\tv_accvgpr_read_b32 %11, a[" #BASE "+11]\n\t"                \
               "v_accvgpr_read_b32 %12, a[" #BASE "+12]\n\tv_accvgpr_read_b32 %13, a[" #BASE "+13]\n\t"                \
               "v_accvgpr_read_b32 %14, a[" #BASE "+14]\n\tv_accvgpr_read_b32 %15, a[" #BASE "+15]"                    \
               : "=v"(DST[0]), "=v"(DST[1]), "=v"(DST[2]), "=v"(DST[3]), "=v"(DST[4]), "=v"(DST[5]), "=v"(DST[6]),      \
                 "=v"(DST[7]), "=v"(DST[8]), "=v"(DST[9]), "=v"(DST[10]), "=v"(DST[11]), "=v"(DST[12]), "=v"(DST[13]),  \
                 "=v"(DST[14]), "=v"(DST[15])                                                                          \
               :                                                                                                       \
               : "memory", SPACAP_ACLOB_D)
#define SPACAP_RD4(DST, BASE)                                                                                          \
  asm volatile("v_accvgpr_read_b32 %0, a[" #BASE "+0]\n\tv_accvgpr_read_b32 %1, a[" #BASE "+1]\n\t"                    \
               "v_accvgpr_read_b32 %2, a[" #BASE "+2]\n\tv_accvgpr_read_b32 %3, a[" #BASE "+3]"                        \
               : "=v"(DST[0]), "=v"(DST[1]), "=v"(DST[2]), "=v"(DST[3])                                                \
               :                                                                                                       \
               : "memory", SPACAP_ACLOB_D)
      if (steady) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(STEADY) : "memory", SPACAP_ACLOB_D);
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory", SPACAP_ACLOB_D);
      if constexpr (BUF == 0) {
        SPACAP_RD16(x, 0);
        SPACAP_RD16(dd, 16);
        if (POOLED) SPACAP_RD4(am, 32);
      } else {
        SPACAP_RD16(x, 36);
        SPACAP_RD16(dd, 52);
        if (POOLED) SPACAP_RD4(am, 68);
      }
#undef SPACAP_RD16
#undef SPACAP_RD4
    }
    // dz = g d + k0 - k1 z, split into three bf16 images (x[4 j + u], dd[4 j + u]: channel 32 H + 8 j + 4 kk + u)
    int sidx = 0;
    if (POOLED) {
      const long left = R - row0;
      const long grow = row0 + (l31 < left ? l31 : (int)left - 1);
      sidx = (int)(lgS >= 0 ? (grow & (S - 1)) : grow % S);
    }
    bf16x8 asp[3][KP];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      __builtin_amdgcn_sched_barrier(0);
      const int g4 = 8 * H + 2 * j + kk;
      const f32x4 g = s_co[3 * g4], k0 = s_co[3 * g4 + 1], k1 = s_co[3 * g4 + 2];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float d = dd[4 * j + u];
        if (POOLED) d = (int)((am[j] >> (8 * u)) & 0xffu) == sidx ? d : 0.f;
        float a = __builtin_fmaf(g[u], d, k0[u]) - k1[u] * x[4 * j + u];
        if (!FULL && row0 + l31 >= R) a = 0.f;
        __bf16 h, m, l;
        split3(a, h, m, l);
        asp[0][j >> 1][4 * (j & 1) + u] = h, asp[1][j >> 1][4 * (j & 1) + u] = m, asp[2][j >> 1][4 * (j & 1) + u] = l;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (decltype(full)::value) {
      const long tn = gw + (pnext / NH) * GW;
      const int hn = (int)(pnext % NH);
      if constexpr (BUF == 0) fetch0(tn, hn);
      else fetch1(tn, hn);
    }
    if (H == 0) {
#pragma unroll
      for (int c = 0; c < NCQ; ++c)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[c][v] = 0.f;
    }
    constexpr int NSTEP = KP * NCQ;
    const __bf16 *wsrc = wimg + l31 * LDW + 32 * H + 8 * kk;
    bf16x8 wq[2][3];
    auto wload = [&](int c) {
      const int s = c / NCQ, cq = c % NCQ;
#pragma unroll
      for (int pz = 0; pz < 3; ++pz)
        wq[c & 1][pz] = *reinterpret_cast<const bf16x8 *>(wsrc + pz * WIMG + cq * 32 * LDW + 16 * s);
    };
    wload(0);
    wload(1);
#pragma unroll
    for (int c = 0; c < NSTEP; ++c) {
      const int s = c / NCQ, cq = c % NCQ;
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int p = 0; p < 6; ++p) acc[cq] = MFMA_BF16(asp[PA[p]][s], wq[c & 1][PB[p]], acc[cq]);   // smallest terms first (mfma.hpp)
      __builtin_amdgcn_sched_barrier(0);
      if (c + 2 < NSTEP) wload(c + 2);
    }
    if (H == NH - 1) {
      // acc[cq][4 b + u] = da[row 8 b + 4 kk + u][channel cbb + 32 cq + lane % 32]; after the quad transposition lane (a8, q4)
      // holds channels 4 a8 .. 4 a8 + 3 of row 8 b + 4 kk + q4: mask by relu'(bn(z_prev)), BN sums, 16-byte store
#pragma unroll
      for (int cq = 0; cq < NCQ; ++cq) {
        SPACAP_LANDING_FENCE_D();
        const size_t base = (size_t)row0 * CP + cbb + 32 * cq;
        const f32x4 pm = s_pp[4 * (8 * cq + a8)], pi = s_pp[4 * (8 * cq + a8) + 1], ps = s_pp[4 * (8 * cq + a8) + 2],
                    pb = s_pp[4 * (8 * cq + a8) + 3];
        f32x4 z[4];
#pragma unroll
        for (int b = 0; b < 4; ++b)
          z[b] = (FULL || row0 + 8 * b + 4 * kk + q4 < R) ? ld4(zp + base + (size_t)(8 * b) * CP + lane_off) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          SPACAP_LANDING_FENCE_D();
          const float r0 = acc[cq][4 * b], r1 = acc[cq][4 * b + 1], r2 = acc[cq][4 * b + 2], r3 = acc[cq][4 * b + 3];
          const float x0 = dpp_xor1(r0), x1 = dpp_xor1(r1), x2 = dpp_xor1(r2), x3 = dpp_xor1(r3);
          const float n0 = odd ? x1 : r0, n1 = odd ? r1 : x0, n2 = odd ? x3 : r2, n3 = odd ? r3 : x2;
          const float y0 = dpp_xor2(n0), y1 = dpp_xor2(n1), y2 = dpp_xor2(n2), y3 = dpp_xor2(n3);
          const f32x4 da = {hi ? y2 : n0, hi ? y3 : n1, hi ? n2 : y0, hi ? n3 : y1};
          const bool live = FULL || row0 + 8 * b + 4 * kk + q4 < R;
          f32x4 d;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float zc = z[b][u] - pm[u];
            const float pre = __builtin_fmaf(zc, ps[u], pb[u]);
            d[u] = (live && pre > 0.f) ? da[u] : 0.f;
            s1[cq][u] += d[u];
            s2[cq][u] = __builtin_fmaf(d[u], zc * pi[u], s2[cq][u]);
          }
          if (live) *reinterpret_cast<f32x4 *>(dyp + base + (size_t)(8 * b) * CP + lane_off) = d;
        }
      }
    }
  };
  const long ntw = gw < nfull ? (nfull - gw + GW - 1) / GW : 0;
  const long NP = ntw * NH;
#pragma unroll
  for (int k = 0; k < NBUF; ++k)
    if (k < NP) fetch(k);
  for (long p = 0; p < NP; p += NH) {
#define SPACAP_PH(K)                                                                                                   \
  {                                                                                                                    \
    const long pp = p + (K);                                                                                           \
    phase(gw + (pp / NH) * GW, std::integral_constant<int, (K)>{}, std::integral_constant<int, (K) % NBUF>{},          \
          std::true_type{}, pp + NBUF - 1 < NP, pp + NBUF < NP ? pp + NBUF : NP - 1);                                  \
  }
    SPACAP_PH(0) SPACAP_PH(1) SPACAP_PH(2) SPACAP_PH(3)
    if constexpr (NH == 8) { SPACAP_PH(4) SPACAP_PH(5) SPACAP_PH(6) SPACAP_PH(7) }
#undef SPACAP_PH
  }
  if (nfull < ntiles && gw == nfull % GW) {   // ragged last tile, one slice at a time through buffer 0
#define SPACAP_RG(K)                                                                                                   \
  fetch0(nfull, (K));                                                                                                  \
  phase(nfull, std::integral_constant<int, (K)>{}, std::integral_constant<int, 0>{}, std::false_type{}, false, 0);
    SPACAP_RG(0) SPACAP_RG(1) SPACAP_RG(2) SPACAP_RG(3)
    if constexpr (NH == 8) { SPACAP_RG(4) SPACAP_RG(5) SPACAP_RG(6) SPACAP_RG(7) }
#undef SPACAP_RG
  }
  // sums: a lane owns channels 4 a8 .. 4 a8 + 3 of column block cq for the rows (q4, kk) it saw: reduce over q4 and kk
#pragma unroll
  for (int cq = 0; cq < NCQ; ++cq)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float a = s1[cq][u], b = s2[cq][u];
      a += __shfl_xor(a, 1), b += __shfl_xor(b, 1);
      a += __shfl_xor(a, 2), b += __shfl_xor(b, 2);
      a += __shfl_xor(a, 32), b += __shfl_xor(b, 32);
      if (q4 == 0 && kk == 0) s_red[(w * 2 + 0) * COB + 32 * cq + 4 * a8 + u] = a, s_red[(w * 2 + 1) * COB + 32 * cq + 4 * a8 + u] = b;
    }
  __syncthreads();
  if (tid < 2 * COB) {
    const int which = tid / COB, c = tid % COB;
    double a = 0.0;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) a += (double)s_red[(ww * 2 + which) * COB + c];
    part[((size_t)blockIdx.x * 2 + which) * CP + cbb + c] = a;
    for (int pr = blockIdx.x + gridDim.x; pr < NPART; pr += gridDim.x)  // partial rows without a workgroup
      part[((size_t)pr * 2 + which) * CP + cbb + c] = 0.0;
  }
}

inline size_t bf3s_dgrad_lds_bytes(int CK) {
  return (size_t)3 * 64 * (CK + 8) * 2 + (size_t)3 * CK * 4 + (size_t)4 * 64 * 4 + (size_t)8 * 2 * 64 * 4;
}
