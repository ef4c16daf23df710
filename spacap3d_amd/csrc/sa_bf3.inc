// Streaming split-bf16 ("bf16 x 3") shared-MLP kernels; included by sa_fwd.hip (uses MFMA_BF16, NPART and
// dpp_xor1 / dpp_xor2 of sa_common.hpp, and ld4, f32x4, split3 and the product order PA / PB of mfma.hpp).
//
// Layer:  z_out[r, :] = relu(bn(z_in[r, :])) W^T  + per-channel sum / sum of squares of z_out (pointnet2/pytorch_utils.py:
// Conv2d -> BatchNorm2d -> ReLU chains built by SharedMLP, lib/pointnet2/pointnet2_modules.py:142-152).
//
// The 6-product split (see sa_mid_fwd_bf3_kernel) needs 6/16 of the fp32-MFMA time, which leaves these layers HBM bound:
// 4 (cin + cout) bytes per row against 12 cin cout bf16 flops.  So the kernel is organised as a stream:
//   * the WEIGHTS of one 128-column block live in LDS for the whole launch, as three bf16 images [128][CIN + 8] (row stride
//     == 4 words mod 64: conflict-free ds_read_b128), K-permuted to the order the activations arrive in;
//   * every WAVE owns 32-row tiles end to end, with no workgroup barrier in the steady state: each lane loads its 32-byte
//     pieces of row (lane % 32) straight into the MFMA operand layout (lane (r, g) holds floats [16 s + 4 g, +4) and
//     [16 s + 8 + 4 g, +4) of k-step s: the two lanes of a row cover 32 contiguous bytes per load instruction), applies BN +
//     ReLU, splits into three bf16 register images, issues the NEXT tile's loads, and then runs 4 column blocks x CIN/16
//     k-steps x 6 MFMAs (v_mfma_f32_32x32x16_bf16; A = activations, B = weights from LDS);
//   * the accumulator layout (lane = channel, 16 rows per lane) makes the statistics per-lane sums and the stores full
//     128-byte lines (32 consecutive channels of one row per half wave);
//   * 8 waves per workgroup, one workgroup per CU (two waves per SIMD alternate between their load / split and MFMA phases).
#define SPACAP_ACLOB                                                                                                   \
  "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17",  \
      "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31"
// nothing of the compiler's may live in the landing registers across this point
#define SPACAP_LANDING_FENCE() asm volatile("" ::: SPACAP_ACLOB)

// POOL: the kernel also emits, per sub-group of min(S, 32) consecutive rows and per output channel, the two best candidates for
// the max-pool that follows this layer (pointnet2_modules.py:259 F.max_pool2d over the nsample axis of relu(bn(z))):
// relu(bn(.)) is monotone in z with the sign of gamma, which is known before the layer's batch statistics are, so the row with
// the largest t = sign(gamma) z carries the largest activation.  Two DISTINCT largest t values with their first row indices
// are kept: when both round to the same activation the reference's first-maximum rule picks the smaller index, which
// spacap_sa_pool_finalize_f32 can then still do.  The pooling pass no longer reads z_out (537 MB at SA1).
// running top-2 of (value, first index) pairs arriving in increasing index order: distinct values m1 > m2
__device__ __forceinline__ void top2(float t, int ri, float &m1, int &i1, float &m2, int &i2) {
  const bool gt1 = t > m1, mid = (t < m1) & (t > m2);
  m2 = gt1 ? m1 : (mid ? t : m2);
  i2 = gt1 ? i1 : (mid ? ri : i2);
  m1 = gt1 ? t : m1;
  i1 = gt1 ? ri : i1;
}
// merge this lane's list with the one of lane ^ 32 (interleaved rows of the same channel); ties go to the smaller index
__device__ __forceinline__ void merge2(float m1, int i1, float m2, int i2, float &w1, int &wi, float &c2, int &ci) {
  const float o1 = __shfl_xor(m1, 32), o2 = __shfl_xor(m2, 32);
  const int j1 = __shfl_xor(i1, 32), j2 = __shfl_xor(i2, 32);
  const bool mine = (m1 > o1) | ((m1 == o1) & (i1 < j1));   // winner of the first place
  w1 = mine ? m1 : o1;
  wi = mine ? i1 : j1;
  const float l1 = mine ? o1 : m1;                            // the loser's best: a candidate for second place if smaller
  const int li = mine ? j1 : i1;
  c2 = l1 < w1 ? l1 : -INFINITY;
  ci = li;
  // (each list's second is strictly below its first, hence below w1)
  const bool ta = (m2 > c2) | ((m2 == c2) & (i2 < ci));
  c2 = ta ? m2 : c2;
  ci = ta ? i2 : ci;
  const bool tb = (o2 > c2) | ((o2 == c2) & (j2 < ci));
  c2 = tb ? o2 : c2;
  ci = tb ? j2 : ci;
}

struct PoolArgs {
  const float *gamma;   // [Cout] BatchNorm weight of THIS layer's output
  int S;                // rows per group: 16, 32 or 64
  float *cand_v;        // [R / min(S, 32)][Cout][2]  t1 >= t2 (t = sign(gamma) z; t2 = -inf: no second value)
  uint8_t *cand_i;      // [R / min(S, 32)][Cout][2]  their first row indices within the sub-group
};

// RAW: the plain product z_out = z_in W^T (no BatchNorm / ReLU on the way in, no statistics): spacap_gemm_rows_f32
template <int CIN, int INTER, bool POOL = false, bool RAW = false>
__global__ __launch_bounds__(512) void sa_mid_fwd_bf3s_kernel(const float *__restrict__ zin, const float *__restrict__ st_in,
                                                              const float *__restrict__ W, int Cout, long R,
                                                              float *__restrict__ zout, double *__restrict__ part,
                                                              const PoolArgs pa = PoolArgs{}) {
  // a tile is worked through in NH phases of 32 input channels (KP = 2 k-steps, one 128-byte line per row): the operand
  // registers hold one phase, the accumulators (4 column blocks x 16) live across the phases of a tile, the raw rows of
  // NBUF = 2 slices are in flight (deeper queues bought nothing: the kernel is not latency bound, DESIGN.md section 4a)
  constexpr int LDW = CIN + 8, NH = CIN / 32, KP = 2, NJ = 4, NBUF = 2, COB = 128, WIMG = COB * LDW, NCQ = COB / 32, NW = 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __bf16 *wimg = reinterpret_cast<__bf16 *>(smem_raw);                    // [3][COB][LDW]
  f32x4 *s_par = reinterpret_cast<f32x4 *>(smem_raw + (size_t)3 * WIMG * 2);   // [CIN / 4][3] (mean, scale, shift)
  float *s_red = reinterpret_cast<float *>(s_par + 3 * (CIN / 4));        // [NW][2][COB]
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, kk = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform on purpose: tile indices and bases stay scalar
  const int cbb = blockIdx.y * COB;
  constexpr int NWL = COB * (CIN / 4) / 512;   // weight chunks per thread: all loads first, then the splits
  f32x4 wv[NWL];
#pragma unroll
  for (int k = 0; k < NWL; ++k) {
    const int i = tid + 512 * k;
    wv[k] = ld4(W + (size_t)(cbb + i / (CIN / 4)) * CIN + 4 * (i % (CIN / 4)));
  }
#pragma unroll
  for (int k = 0; k < NWL; ++k) {
    const int i = tid + 512 * k;
    const int c = i / (CIN / 4), q = i % (CIN / 4);
    const f32x4 v = wv[k];
    bf16x4 p0, p1, p2;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      __bf16 h, m, l;
      split3(v[u], h, m, l);
      p0[u] = h, p1[u] = m, p2[u] = l;
    }
    // chunk q = 4 s + 2 half + g  ->  position 16 s + 8 g + 4 half of the permuted row
    __bf16 *dst = wimg + c * LDW + 16 * (q >> 2) + 8 * (q & 1) + 4 * ((q >> 1) & 1);
    *reinterpret_cast<bf16x4 *>(dst) = p0;
    *reinterpret_cast<bf16x4 *>(dst + WIMG) = p1;
    *reinterpret_cast<bf16x4 *>(dst + 2 * WIMG) = p2;
  }
  if (!RAW) {
    for (int i = tid; i < CIN; i += 512) {
      float *p = reinterpret_cast<float *>(s_par + 3 * (i / 4));
      p[i % 4] = st_in[(size_t)i * 4], p[4 + i % 4] = st_in[(size_t)i * 4 + 2], p[8 + i % 4] = st_in[(size_t)i * 4 + 3];
    }
  }
  __syncthreads();

  float ssum[NCQ], ssq[NCQ];
#pragma unroll
  for (int c = 0; c < NCQ; ++c) ssum[c] = ssq[c] = 0.f;
  float sgn[POOL ? NCQ : 1];
  if (POOL) {
#pragma unroll
    for (int c = 0; c < NCQ; ++c) sgn[c] = pa.gamma[cbb + 32 * c + l31] >= 0.f ? 1.f : -1.f;
  }
  const long ntiles = (R + 31) / 32, nfull = R / 32;
  const long gw = (long)blockIdx.x * NW + w, GW = (long)gridDim.x * NW;
  const int q4 = l31 & 3;
  const bool odd = q4 & 1, hi = q4 & 2;
  const bool s16 = POOL && pa.S == 16;
  const unsigned lane_off = (unsigned)((4 * kk + q4) * Cout + (l31 & ~3));   // row 4 kk + q4, channels 4 (l31 / 4) ..
  f32x16 acc[NCQ];
  // The raw rows of the NBUF slices in flight land in AGPR variables (L0 / L1: 4 x 16 bytes per lane each).  They are
  // written by inline-asm loads and become visible to the C++ code only through the hand-counted s_waitcnt below, whose "+a"
  // operands tie the two together: the register allocator sees values that are live from the load to the wait (it cannot
  // hand their registers to anything else), while the compiler's own wait-count pass -- which would drain the whole queue,
  // stores included, at every loop head -- does not know the loads exist.  tools/check_landing_regs.py verifies on the
  // generated assembly that no compiler instruction touches a landing register other than the copy-out after the wait.
  // The raw rows of the NBUF = 2 slices in flight land in AGPRs a[16 B .. 16 B + 15] (B = 0, 1), named literally in the asm and
  // therefore invisible to the register allocator: loads into ordinary variables would let it copy a register whose data is
  // still on its way (seen: v_accvgpr_mov of in-flight registers at the loop head), and plain C++ loads make the compiler's
  // wait-count pass drain the whole queue, stores included, at every loop head.  Every asm block that touches them, and the
  // fences sprinkled through the epilogue, declare a0..a31 clobbered, so nothing of the compiler's can live there across
  // them; tools/check_landing_regs.py verifies on the generated assembly that no compiler instruction uses a0..a31 at all.
#define SPACAP_FETCH(NAME, A0, A1, A2, A3)                                                                             \
  auto NAME = [&](long t, int h) {                                                                                     \
    const long left = R - t * 32; /* rows of this tile that exist (scalar) */                                          \
    const int r = l31 < left ? l31 : (int)left - 1;                                                                    \
    const float *src = zin + (size_t)t * 32 * CIN + 32 * h + (unsigned)(r * CIN + 4 * kk);                             \
    asm volatile("global_load_dwordx4 " A0 ", %0, off\n\tglobal_load_dwordx4 " A1 ", %0, off offset:32\n\t"           \
                 "global_load_dwordx4 " A2 ", %0, off offset:64\n\tglobal_load_dwordx4 " A3 ", %0, off offset:96"      \
                 :                                                                                                     \
                 : "v"(src)                                                                                            \
                 : "memory", SPACAP_ACLOB);                                                                            \
  };
  SPACAP_FETCH(fetch0, "a[0:3]", "a[4:7]", "a[8:11]", "a[12:15]")
  SPACAP_FETCH(fetch1, "a[16:19]", "a[20:23]", "a[24:27]", "a[28:31]")
#undef SPACAP_FETCH
  auto fetch = [&](long pq) {   // loads of phase pq into its buffer
    const long t = gw + (pq / NH) * GW;
    const int h = (int)(pq % NH);
    if (pq % NBUF == 0) fetch0(t, h);
    else fetch1(t, h);
  };
#undef SPACAP_FETCH
  // Phase p of this wave's stream (tile t, 32-channel slice H, raw rows in landing buffer BUF).  Issue order of the stream:
  //   phase p:  wait loads(p) | BN + ReLU + split | issue loads(p + NBUF) into the freed buffer | MFMAs | stores (last slice)
  // Loads retire in order among themselves, so "at most NJ (NBUF - 1) operations outstanding" means loads(p) have landed
  // whatever the stores do (counting the stores of the tile that ended in between as "younger and still outstanding" was
  // seen to fault on long streams: stores and loads are not retired in one common order).  `steady` false (stream end, ragged
  // tile): wait for everything.
  auto phase = [&](long t, auto hc, auto bc, auto full, bool steady, long pnext) {
    // FULL phases always prefetch; the ragged tile (outside the stream) never does
    constexpr int H = decltype(hc)::value, BUF = decltype(bc)::value;
    constexpr bool FULL = decltype(full)::value;
    const long row0 = t * 32;
    constexpr int STEADY = NJ * (NBUF - 1);
    f32x4 pre[NJ];
    {
      float x[16];
#define SPACAP_RD(WAIT, BASE)                                                                                          \
  asm volatile(WAIT "\n\t"                                                                                             \
               "v_accvgpr_read_b32 %0, a[" #BASE "+0]\n\tv_accvgpr_read_b32 %1, a[" #BASE "+1]\n\t"                    \
               "v_accvgpr_read_b32 %2, a[" #BASE "+2]\n\tv_accvgpr_read_b32 %3, a[" #BASE "+3]\n\t"                    \
               "v_accvgpr_read_b32 %4, a[" #BASE "+4]\n\tv_accvgpr_read_b32 %5, a[" #BASE "+5]\n\t"                    \
               "v_accvgpr_read_b32 %6, a[" #BASE "+6]\n\tv_accvgpr_read_b32 %7, a[" #BASE "+7]\n\t"                    \
               "v_accvgpr_read_b32 %8, a[" #BASE "+8]\n\tv_accvgpr_read_b32 %9, a[" #BASE "+9]\n\t"                    \
               "v_accvgpr_read_b32 %10, a[" #BASE "+10]\n\tv_accvgpr_read_b32 %11, a[" #BASE "+11]\n\t"                \
               "v_accvgpr_read_b32 %12, a[" #BASE "+12]\n\tv_accvgpr_read_b32 %13, a[" #BASE "+13]\n\t"                \
               "v_accvgpr_read_b32 %14, a[" #BASE "+14]\n\tv_accvgpr_read_b32 %15, a[" #BASE "+15]"                    \
               : "=v"(x[0]), "=v"(x[1]), "=v"(x[2]), "=v"(x[3]), "=v"(x[4]), "=v"(x[5]), "=v"(x[6]), "=v"(x[7]),        \
                 "=v"(x[8]), "=v"(x[9]), "=v"(x[10]), "=v"(x[11]), "=v"(x[12]), "=v"(x[13]), "=v"(x[14]), "=v"(x[15])   \
               : "n"(STEADY)                                                                                           \
               : "memory", SPACAP_ACLOB)
#define SPACAP_RDB(BASE)                                                                                               \
  if (steady) SPACAP_RD("s_waitcnt vmcnt(%16)", BASE);                                                                 \
  else SPACAP_RD("s_waitcnt vmcnt(0)", BASE)
      if constexpr (BUF == 0) { SPACAP_RDB(0); }
      else { SPACAP_RDB(16); }
#undef SPACAP_RDB
#undef SPACAP_RD
#pragma unroll
      for (int j = 0; j < NJ; ++j) pre[j] = f32x4{x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]};
    }
    bf16x8 asp[3][KP];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      __builtin_amdgcn_sched_barrier(0);
      f32x4 mean = {0.f, 0.f, 0.f, 0.f}, sc = mean, be = mean;
      if (!RAW) mean = s_par[3 * (8 * H + 2 * j + kk)], sc = s_par[3 * (8 * H + 2 * j + kk) + 1], be = s_par[3 * (8 * H + 2 * j + kk) + 2];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        // (the fused multiply-add is spelled out: every instantiation rounds alike)
        const float a = RAW ? pre[j][u] : fmaxf(__builtin_fmaf(pre[j][u] - mean[u], sc[u], be[u]), 0.f);
        __bf16 h, m, l;
        split3(a, h, m, l);
        asp[0][j >> 1][4 * (j & 1) + u] = h, asp[1][j >> 1][4 * (j & 1) + u] = m, asp[2][j >> 1][4 * (j & 1) + u] = l;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (decltype(full)::value) {
      // unconditional (the stream's last phases re-load the last phase): no control flow around registers in flight
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
    // steps: (s, group of INTER column blocks); weights of a step: INTER x 3 ds_read_b128, read two steps ahead
    constexpr int NG = NCQ / INTER, NSTEP = KP * NG;
    const __bf16 *wsrc = wimg + l31 * LDW + 32 * H + 8 * kk;
    bf16x8 wq[2][INTER][3];
    auto wload = [&](int c) {
      const int s = c / NG, g = c % NG;
#pragma unroll
      for (int i = 0; i < INTER; ++i)
#pragma unroll
        for (int pz = 0; pz < 3; ++pz)
          wq[c & 1][i][pz] = *reinterpret_cast<const bf16x8 *>(wsrc + pz * WIMG + (g * INTER + i) * 32 * LDW + 16 * s);
    };
    wload(0);
    wload(1);
#pragma unroll
    for (int c = 0; c < NSTEP; ++c) {
      const int s = c / NG, g = c % NG;
      __builtin_amdgcn_sched_barrier(0);
      // smallest terms first (PA, PB: mfma.hpp); the INTER accumulators alternate
#pragma unroll
      for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int i = 0; i < INTER; ++i)
          acc[g * INTER + i] = MFMA_BF16(asp[PA[p]][s], wq[c & 1][i][PB[p]], acc[g * INTER + i]);
      __builtin_amdgcn_sched_barrier(0);
      if (c + 2 < NSTEP) wload(c + 2);
    }
    if (H == NH - 1) {
      // acc[cq][4 b + u] = z[row 8 b + 4 kk + u][channel 32 cq + lane % 32]: statistics are per-lane sums; for the stores
      // every quad of lanes transposes its 4 x 4 block (two select + DPP rounds), after which lane (a, q) holds channels
      // 4 a .. 4 a + 3 of row 8 b + 4 kk + q: one 16-byte store, full 128-byte lines per wave instruction
#pragma unroll
      for (int cq = 0; cq < NCQ; ++cq) {
        float *dst = zout + (size_t)row0 * Cout + cbb + 32 * cq;   // scalar bases, ONE 32-bit lane offset
        SPACAP_LANDING_FENCE();
        float ma1 = -INFINITY, ma2 = -INFINITY, mb1 = -INFINITY, mb2 = -INFINITY;   // candidates of the tile's sub-groups
        int ia1 = 0, ia2 = 0, ib1 = 0, ib2 = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          SPACAP_LANDING_FENCE();
          float r[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            r[u] = acc[cq][4 * b + u];
            if (FULL || row0 + 8 * b + 4 * kk + u < R) {
              ssum[cq] += r[u];
              ssq[cq] = __builtin_fmaf(r[u], r[u], ssq[cq]);
              if (POOL) {   // this lane's rows arrive in increasing order: strict comparisons keep first indices
                // (branch-free on purpose: selects only, the quad transposition below needs every lane)
                const int ri = (s16 ? 8 * (b & 1) : 8 * b) + 4 * kk + u;
                const float t = sgn[cq] * r[u];
                if (b < 2 || !s16) top2(t, ri, ma1, ia1, ma2, ia2);     // sub-group 0 (the whole tile unless S == 16)
                else top2(t, ri, mb1, ib1, mb2, ib2);                    // sub-group 1 (rows 16 .. 31, S == 16 only)
              }
            }
          }
          // (every DPP read is executed by all lanes; only the selects depend on the lane)
          const float x0 = dpp_xor1(r[0]), x1 = dpp_xor1(r[1]), x2 = dpp_xor1(r[2]), x3 = dpp_xor1(r[3]);
          const float n0 = odd ? x1 : r[0], n1 = odd ? r[1] : x0, n2 = odd ? x3 : r[2], n3 = odd ? r[3] : x2;
          const float y0 = dpp_xor2(n0), y1 = dpp_xor2(n1), y2 = dpp_xor2(n2), y3 = dpp_xor2(n3);
          const f32x4 m = {hi ? y2 : n0, hi ? y3 : n1, hi ? n2 : y0, hi ? n3 : y1};
          if (zout && (FULL || row0 + 8 * b + 4 * kk + q4 < R))   // (zout == NULL: a pooled last layer whose backward needs no z)
            *reinterpret_cast<f32x4 *>(dst + (size_t)(8 * b) * Cout + lane_off) = m;
        }
        if (POOL) {
          SPACAP_LANDING_FENCE();
          // the other half wave holds the rows 4..7 mod 8 of the same channel: merge the two candidate lists
          const size_t oc = (size_t)(cbb + 32 * cq + l31) * 2;
          {
            float w1, c2;
            int wi, ci;
            merge2(ma1, ia1, ma2, ia2, w1, wi, c2, ci);
            const long sub = s16 ? row0 / 16 : row0 / 32;
            {   // (both half waves hold the merged result and store it: no divergent branch)
              const size_t o = (size_t)sub * Cout * 2 + oc;
              *reinterpret_cast<float2 *>(pa.cand_v + o) = make_float2(w1, c2);
              *reinterpret_cast<uchar2 *>(pa.cand_i + o) = make_uchar2((unsigned char)wi, (unsigned char)ci);
            }
          }
          if (s16) {
            float w1, c2;
            int wi, ci;
            merge2(mb1, ib1, mb2, ib2, w1, wi, c2, ci);
            if (FULL || row0 + 16 < R) {
              const size_t o = (size_t)(row0 / 16 + 1) * Cout * 2 + oc;
              *reinterpret_cast<float2 *>(pa.cand_v + o) = make_float2(w1, c2);
              *reinterpret_cast<uchar2 *>(pa.cand_i + o) = make_uchar2((unsigned char)wi, (unsigned char)ci);
            }
          }
        }
      }
    }
  };
  // this wave's full tiles: t_i = gw + i GW, i < ntw; phases p = i NH + H
  const long ntw = gw < nfull ? (nfull - gw + GW - 1) / GW : 0;
  const long NP = ntw * NH;
#pragma unroll
  for (int k = 0; k < NBUF; ++k)
    if (k < NP) fetch(k);
  for (long p = 0; p < NP; p += NH) {   // one tile per iteration: slice K of the tile uses landing buffer K % NBUF
    // steady state: NBUF phases behind (their stores were issued) and the loads of the next NBUF - 1 phases in flight
#define SPACAP_PH(K)                                                                                                   \
  if ((K) < NH || p + (K) < NP) { /* NP is a multiple of NH: whole tiles need no test */                               \
    const long pp = p + (K);                                                                                           \
    phase(gw + (pp / NH) * GW, std::integral_constant<int, (K) % NH>{}, std::integral_constant<int, (K) % NBUF>{},            \
          std::true_type{}, pp + NBUF - 1 < NP, pp + NBUF < NP ? pp + NBUF : NP - 1);            \
  }
    SPACAP_PH(0) SPACAP_PH(1)
    if constexpr (NH == 4) { SPACAP_PH(2) SPACAP_PH(3) }
#undef SPACAP_PH
  }
  if (nfull < ntiles && gw == nfull % GW) {   // ragged last tile, outside the stream
    // one slice at a time through buffer 0 (nothing else is in flight here)
    fetch0(nfull, 0);
    phase(nfull, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, std::false_type{}, false, 0);
    fetch0(nfull, 1);
    phase(nfull, std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{}, std::false_type{}, false, 0);
    if constexpr (NH == 4) {
      fetch0(nfull, 2);
      phase(nfull, std::integral_constant<int, 2>{}, std::integral_constant<int, 0>{}, std::false_type{}, false, 0);
      fetch0(nfull, 3);
      phase(nfull, std::integral_constant<int, 3>{}, std::integral_constant<int, 0>{}, std::false_type{}, false, 0);
    }
  }
#pragma unroll
  for (int cq = 0; cq < NCQ; ++cq) {
    const float a = ssum[cq] + __shfl_xor(ssum[cq], 32), q = ssq[cq] + __shfl_xor(ssq[cq], 32);
    if (kk == 0) s_red[(w * 2 + 0) * COB + 32 * cq + l31] = a, s_red[(w * 2 + 1) * COB + 32 * cq + l31] = q;
  }
  __syncthreads();
  if (!RAW && tid < 2 * COB) {
    const int which = tid / COB, c = tid % COB;
    double a = 0.0;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) a += (double)s_red[(ww * 2 + which) * COB + c];
    part[((size_t)blockIdx.x * 2 + which) * Cout + cbb + c] = a;
    for (int pr = blockIdx.x + gridDim.x; pr < NPART; pr += gridDim.x)  // partial rows without a workgroup
      part[((size_t)pr * 2 + which) * Cout + cbb + c] = 0.0;
  }
}

inline size_t bf3s_lds_bytes(int Cin) {
  return (size_t)3 * 128 * (Cin + 8) * 2 + (size_t)3 * Cin * 4 + (size_t)8 * 2 * 128 * 4;
}
