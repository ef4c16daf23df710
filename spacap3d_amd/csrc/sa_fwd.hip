// Forward kernels of the set-abstraction shared MLP (data flow: sa_common.hpp) and their entry points: the first layer and its
// statistics, the statistics finalisation, the middle layers (fp32-MFMA: sa_mid_fwd_kernel; streaming split-bf16: sa_bf3.inc)
// and the pooling.
//
// Two entry points that are not set abstraction live here because of the kernels they launch: spacap_gemm_rows_* (plain row
// products on sa_mid_fwd_bf3s_kernel, one of the streaming kernels under the landing-register check of csrc/Makefile) and
// spacap_rel_tail_fwd_f32 (the relation head's layers 2 and 3: the TAIL = true instantiation of sa_mid_fwd_kernel; its
// backward is rel_tail.hip).
#include "sa_common.hpp"

namespace {

// ---- layer 1 forward --------------------------------------------------------------------------------------
// z1[r, :] = Y[b, idx[r], :] + W1[:, 0:3] rel(r) + W1[:, 3] feat[b, idx[r]]      (Y and feat optional)
// rel(r) = (xyz[b, idx[r]] - new_xyz[b, n]) / rdiv
template <int C1, int UR = 4>
__global__ __launch_bounds__(256) void sa_l1_fwd_kernel(const float *__restrict__ Y, const float *__restrict__ feat,
                                                        const float *__restrict__ xyz, const float *__restrict__ new_xyz,
                                                        const int32_t *__restrict__ idx, const float *__restrict__ W1,
                                                        int ldw, float rdiv, int Np, int N, int S, long R,
                                                        float *__restrict__ z1, double *__restrict__ part,
                                                        float *__restrict__ rel4 = nullptr) {
  constexpr int C4 = C1 / 4, RP = 256 / C4;
  __shared__ float s_red[2][RP][C1];
  const int tid = threadIdx.x, c4 = tid % C4, rs = tid / C4;
  f32x4 wx, wy, wz, wf = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float *w = W1 + (size_t)(c4 * 4 + u) * ldw;
    wx[u] = w[0], wy[u] = w[1], wz[u] = w[2];
    if (feat) wf[u] = w[3];
  }
  f32x4 sum = {0.f, 0.f, 0.f, 0.f}, sq = {0.f, 0.f, 0.f, 0.f};
  const long NS = (long)N * S;
  // The row's inputs hang off a dependent chain (idx -> point -> coordinates): four rows per iteration keep four chains in
  // flight (one row at a time the kernel sat at the chain's latency, 119 us for SA1 against an HBM time of 55 us; 8 or 16 rows
  // measured slower at every SA shape: 45.7 -> 65.6 us at SA2, tools/lab/l1_fwd_time.py).  The
  // statistics are accumulated in the same row order as before.
  const long G = (long)gridDim.x * RP;
  long r = (long)blockIdx.x * RP + rs;
  auto row_in = [&](long rr, int &p, long &b) {
    b = row_div(rr, NS);
    p = idx[rr];
  };
  auto row_z = [&](long rr, int p, long b) {
    const long g = row_div(rr, S);
    const float *q = xyz + ((size_t)b * Np + p) * 3, *c = new_xyz + (size_t)g * 3;
    const f32x4 in = {(q[0] - c[0]) / rdiv, (q[1] - c[1]) / rdiv, (q[2] - c[2]) / rdiv, feat ? feat[(size_t)b * Np + p] : 0.f};
    if (rel4 && c4 == 0) st4(rel4 + (size_t)rr * 4, in);   // the row's four inputs: what the later passes rebuild z1 from
    f32x4 z = l1_row(wx, wy, wz, wf, in, feat != nullptr);
    if (Y) z += ld4(Y + ((size_t)b * Np + p) * C1 + c4 * 4);
    return z;
  };
  for (; r + (UR - 1) * G < R; r += UR * G) {
    int p[UR];
    long b[UR];
#pragma unroll
    for (int k = 0; k < UR; ++k) row_in(r + k * G, p[k], b[k]);
    f32x4 z[UR];
#pragma unroll
    for (int k = 0; k < UR; ++k) z[k] = row_z(r + k * G, p[k], b[k]);
#pragma unroll
    for (int k = 0; k < UR; ++k) {
      if (z1) st4(z1 + (size_t)(r + k * G) * C1 + c4 * 4, z[k]);
      sum += z[k];
      sq += z[k] * z[k];
    }
  }
  for (; r < R; r += G) {
    int p;
    long b;
    row_in(r, p, b);
    const f32x4 z = row_z(r, p, b);
    if (z1) st4(z1 + (size_t)r * C1 + c4 * 4, z);
    sum += z;
    sq += z * z;
  }
  st4(&s_red[0][rs][c4 * 4], sum);
  st4(&s_red[1][rs][c4 * 4], sq);
  __syncthreads();
  if (tid < 2 * C1) {
    const int k = tid / C1, c = tid % C1;
    double a = 0.0;
    for (int i = 0; i < RP; ++i) a += (double)s_red[k][i][c];
    part[((size_t)blockIdx.x * 2 + k) * C1 + c] = a;
  }
}

// ---- first layer without point features (SA1): BatchNorm statistics in closed form -------------------------------------------
// z1[r][c] = W1[c] . in[r] is LINEAR in the row's four inputs in = (rel x, rel y, rel z, inline feature), so the layer's batch
// statistics need only the first and second moments of `in` over all rows:
//     sum_r z1[r][c] = W1[c] . S,   sum_r z1[r][c]^2 = W1[c]^T Mom W1[c],   S = sum_r in[r] (4),  Mom = sum_r in[r] in[r]^T (10 distinct)
// 14 sums per row instead of 2 x 64 -- and one THREAD per row instead of 16 (the 64-channel form repeated the row's dependent
// chain idx -> point -> coordinates and its three divisions in the 16 threads that shared a row: 87 us at SA1).  The pass still
// leaves rel4 [R][4], from which every later pass rebuilds z1.  Reference: lib/pointnet2/pointnet2_utils.py:350-355 (grouping),
// lib/pointnet2/pytorch_utils.py:11-36 (Conv2d -> BatchNorm2d: statistics over all rows).
// part [gridDim.x][16] doubles: S0..S3 | M00 M01 M02 M03 M11 M12 M13 M22 M23 M33 | 0 0
__global__ __launch_bounds__(256) void sa_l1_moments_kernel(const float *__restrict__ feat, const float *__restrict__ xyz,
                                                            const float *__restrict__ new_xyz, const int32_t *__restrict__ idx,
                                                            float rdiv, int Np, int N, int S, long R, float *__restrict__ rel4,
                                                            double *__restrict__ part) {
  __shared__ float s_m[14][256 + 1];
  const int tid = threadIdx.x;
  const long NS = (long)N * S, G = (long)gridDim.x * 256;
  float a[14];
#pragma unroll
  for (int i = 0; i < 14; ++i) a[i] = 0.f;
  auto row = [&](long r, int p) {
    const long b = row_div(r, NS), g = row_div(r, S);
    const float *q = xyz + ((size_t)b * Np + p) * 3, *c = new_xyz + (size_t)g * 3;
    const f32x4 in = {(q[0] - c[0]) / rdiv, (q[1] - c[1]) / rdiv, (q[2] - c[2]) / rdiv, feat ? feat[(size_t)b * Np + p] : 0.f};
    st4(rel4 + (size_t)r * 4, in);
    return in;
  };
  auto add = [&](f32x4 in) {
    a[0] += in[0], a[1] += in[1], a[2] += in[2], a[3] += in[3];
    a[4] += in[0] * in[0], a[5] += in[0] * in[1], a[6] += in[0] * in[2], a[7] += in[0] * in[3];
    a[8] += in[1] * in[1], a[9] += in[1] * in[2], a[10] += in[1] * in[3];
    a[11] += in[2] * in[2], a[12] += in[2] * in[3], a[13] += in[3] * in[3];
  };
  constexpr int UR = 4;   // four rows' chains (idx -> point -> coordinates) in flight per thread
  long r = (long)blockIdx.x * 256 + tid;
  for (; r + (UR - 1) * G < R; r += UR * G) {
    int p[UR];
#pragma unroll
    for (int k = 0; k < UR; ++k) p[k] = idx[r + k * G];
    f32x4 in[UR];
#pragma unroll
    for (int k = 0; k < UR; ++k) in[k] = row(r + k * G, p[k]);
#pragma unroll
    for (int k = 0; k < UR; ++k) add(in[k]);
  }
  for (; r < R; r += G) add(row(r, idx[r]));
#pragma unroll
  for (int i = 0; i < 14; ++i) s_m[i][tid] = a[i];
  __syncthreads();
  if (tid < 16) {
    double v = 0.0;
    if (tid < 14)
      for (int t = 0; t < 256; ++t) v += (double)s_m[tid][t];
    part[(size_t)blockIdx.x * 16 + tid] = v;
  }
}

// moments [nparts][16] -> stats [C1][4] of the first layer (mean, 1 / std, gamma / std, beta) + running statistics (torch semantics)
__global__ __launch_bounds__(1024) void sa_l1_moments_finalize_kernel(const double *__restrict__ part, int nparts, const float *__restrict__ W1,
                                                                     int ldw, int has_feat, int C1, double M, float eps, float momentum,
                                                                     const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                     float *__restrict__ running_mean, float *__restrict__ running_var,
                                                                     float *__restrict__ stats) {
  __shared__ double s_mom[16];
  const int tid = threadIdx.x, m = tid >> 6, lane = tid & 63;
  if (m < 14) {   // wave m adds moment m over the partial rows: lane l takes rows l, l + 64, .. in order, then a fixed tree
    double v = 0.0;
    for (int p = lane; p < nparts; p += 64) v += part[(size_t)p * 16 + m];
    v = spacap::wave_sum(v);
    if (lane == 0) s_mom[m] = v;
  }
  __syncthreads();
  if (tid < C1) {
    const float *wr = W1 + (size_t)tid * ldw;
    const double w[4] = {wr[0], wr[1], wr[2], has_feat ? wr[3] : 0.0};
    const double *Sm = s_mom, *Q = s_mom + 4;   // Q: 00 01 02 03 11 12 13 22 23 33
    const double sm = w[0] * Sm[0] + w[1] * Sm[1] + w[2] * Sm[2] + w[3] * Sm[3];
    const double q = w[0] * w[0] * Q[0] + w[1] * w[1] * Q[4] + w[2] * w[2] * Q[7] + w[3] * w[3] * Q[9] +
                     2.0 * (w[0] * w[1] * Q[1] + w[0] * w[2] * Q[2] + w[0] * w[3] * Q[3] + w[1] * w[2] * Q[5] + w[1] * w[3] * Q[6] +
                            w[2] * w[3] * Q[8]);
    const spacap::BnChannel bn = spacap::bn_channel(sm, q, M, eps);
    stats[tid * 4 + 0] = (float)bn.mean;
    stats[tid * 4 + 1] = bn.istd;
    stats[tid * 4 + 2] = gamma[tid] * bn.istd;
    stats[tid * 4 + 3] = beta[tid];
    if (running_mean) spacap::bn_update_running(bn, M, momentum, running_mean, running_var, tid);
  }
}

// ---- statistics finalisation --------------------------------------------------------------------------------
// part [NPART][2][C] (sum, sum of squares) -> stats [C][4]; optional running-statistics update (torch semantics)
__global__ __launch_bounds__(1024) void sa_bn_finalize_kernel(const double *__restrict__ part, int nparts, int C,
                                                             double M, float eps, float momentum,
                                                             const float *__restrict__ gamma, const float *__restrict__ beta,
                                                             float *__restrict__ running_mean,
                                                             float *__restrict__ running_var, float *__restrict__ stats) {
  // workgroup = 8 channels x {sum, sq} x 64 slabs of partial rows
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
    double sm = 0.0, q = 0.0;
    for (int i = 0; i < 64; ++i) sm += s[i][tid], q += s[i][tid + 8];
    const spacap::BnChannel bn = spacap::bn_channel(sm, q, M, eps);
    stats[c * 4 + 0] = (float)bn.mean;
    stats[c * 4 + 1] = bn.istd;
    stats[c * 4 + 2] = gamma[c] * bn.istd;
    stats[c * 4 + 3] = beta[c];
    if (running_mean) spacap::bn_update_running(bn, M, momentum, running_mean, running_var, c);
  }
}

// ---- middle layers forward: zout = relu(bn(zin)) W^T, statistics of zout -------------------------------------
// Per 64-row tile: [prefetched registers -> BN+ReLU -> LDS] | sync | issue the next tile's loads | MFMA |
// accumulators -> LDS (transposed staging) | sync | full-row 16-byte stores.  The loads of tile t+1 and the stores
// of tile t are in flight while the matrix cores work on tile t.
// TAIL = true turns the same pipeline into the relation head's last two layers
// (models/transformer_captioner.py:319-326, 392-397: Linear(128,128) -> ReLU -> Linear(128,9) on B*K*K pair rows):
// rows are staged as they are (the first layer's ReLU output), the epilogue adds the bias and applies the ReLU, the
// tile is stored (the backward needs it) and multiplied by the 9 x 128 output weights (padded to one 16-row MFMA
// operand) while it is still in LDS.  No statistics.
struct TailArgs {
  const float *bias;   // [Cout]
  const float *W3;     // [NO3][Cout]
  const float *b3;     // [NO3]
  float *pred;         // [R][NO3]
  int NO3;             // <= 16
};
template <int CIN, int NT, bool TAIL = false, int TMT = 64>
__global__ __launch_bounds__(256) void sa_mid_fwd_kernel(const float *__restrict__ zin, const float *__restrict__ st_in,
                                                         const float *__restrict__ W, int Cout, long R,
                                                         float *__restrict__ zout, double *__restrict__ part, TailArgs ta,
                                                         L1In li = L1In{nullptr, 0, 0}) {
  // LD = CIN + 8 (== 8 mod 64 words) together with the K order below makes every ds_read_b128 of the B operand
  // conflict-free: MFMA step s of lane group lg (= lane / 16) uses channel kperm(s, lg); the four steps 4q..4q+3 of
  // a lane are 4 consecutive words, lg 0/1 (and 2/3) interleave in 4-word chunks, lg 0,1 own the first half of the
  // row and lg 2,3 the second (ds_read_b128 is served in the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ...:
  // each holds all 16 rows with lg in {0,1} or {2,3}, and 8*row + 4*(lg&1) tiles the 64 banks exactly once).
  constexpr int LD = CIN + 8, KS = CIN / 4, KQ = KS / 4, C4 = CIN / 4, NV = TMT * C4 / 256, RSTEP = 256 / C4;
  constexpr int COB = 64 * NT, LDO = COB + 4, O4 = COB / 4, NO = TMT * O4 / 256, OSTEP = 256 / O4;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *s_a = smem;             // [TMT][LD]   activations (MFMA B operand)
  float *s_o = smem + TMT * LD;   // [TMT][LDO]  output tile, row-major
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int cbb = blockIdx.y * COB, wc = w * 16 * NT, cb = cbb + wc;
  float wf[NT][KS];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int q = 0; q < KQ; ++q) {   // steps 4q .. 4q+3 of a lane are 4 consecutive channels: one 16-byte load
      const f32x4 w4 = ld4(W + (size_t)(cb + 16 * j + l15) * CIN + (lg >> 1) * (CIN / 2) + q * 8 + (lg & 1) * 4);
#pragma unroll
      for (int u = 0; u < 4; ++u) wf[j][q * 4 + u] = w4[u];
    }
  const int c4 = tid % C4, r0 = tid / C4, o4 = tid % O4, or0 = tid / O4;
  f32x4 mean = {0.f, 0.f, 0.f, 0.f}, sc = mean, be = mean;
  if (!TAIL) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float *s = st_in + (size_t)(c4 * 4 + u) * 4;
      mean[u] = s[0], sc[u] = s[2], be[u] = s[3];
    }
  }
  float wf3[TAIL ? COB / 4 : 1];
  f32x4 bv[NT];
  if (TAIL) {
#pragma unroll
    for (int ks = 0; ks < COB / 4; ++ks) wf3[TAIL ? ks : 0] = l15 < ta.NO3 ? ta.W3[(size_t)l15 * Cout + ks * 4 + lg] : 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) bv[j] = ld4(ta.bias + cb + 16 * j + 4 * lg);
  }
  f32x4 ssum[NT], ssq[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) ssum[j] = ssq[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const long ntiles = (R + TMT - 1) / TMT;
  f32x4 pre[NV];
  // Prefetch with hand-issued loads: the compiler's wait-count insertion would drain the previous tile's stores
  // too (vmcnt is one in-order counter for loads and stores on gfx9); here the wait before staging is
  // vmcnt(#stores of one tile), which leaves those stores in flight.  Row index clamped: rows past the end are
  // zeroed when staged.
  auto fetch = [&](long t) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      long grow = t * TMT + r0 + i * RSTEP;
      grow = grow < R ? grow : R - 1;
      const float *src = li.W1 ? zin + (size_t)grow * 4 : zin + (size_t)grow * CIN + c4 * 4;
      asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(pre[i]) : "v"(src) : "memory");
    }
  };
  f32x4 l1x = {0.f, 0.f, 0.f, 0.f}, l1y = l1x, l1z = l1x, l1f = l1x;
  if (li.W1) l1_weights(li, c4 * 4, l1x, l1y, l1z, l1f);
  auto wait_prefetch = [&](bool stores_pending) {
    if (stores_pending) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NO) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < NV; ++i) asm volatile("" : "+v"(pre[i]));  // uses of pre[] stay below the wait
  };
  // one tile; FULL = all TMT rows exist (no bounds checks: the stores are then straight-line code too)
  auto tile = [&](long t, auto full, bool stores_pending) {
    constexpr bool FULL = decltype(full)::value;
    const long row0 = t * TMT;
    {
      wait_prefetch(stores_pending);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int row = r0 + i * RSTEP;
        f32x4 a;
        const f32x4 zv = li.W1 ? l1_row(l1x, l1y, l1z, l1f, pre[i], li.has_feat != 0) : pre[i];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = TAIL ? zv[u] : fmaxf((zv[u] - mean[u]) * sc[u] + be[u], 0.f);
        if (!FULL && row0 + row >= R) a = f32x4{0.f, 0.f, 0.f, 0.f};
        st4(&s_a[row * LD + c4 * 4], a);
      }
      __syncthreads();
      if (FULL) fetch(t + gridDim.x);  // (the ragged tile is the last one: nothing to prefetch)
    }
    f32x4 acc[TMT / 16][NT];
#pragma unroll
    for (int mt = 0; mt < TMT / 16; ++mt)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
      // B operand by ds_read_b128, software-pipelined in chunks of (16 rows x half of K): two register buffers; the
      // reads of chunk c + 2 are issued right after the MFMAs of chunk c, i.e. one chunk of MFMA time (16 * NT
      // instructions) before their first use.  sched_barriers pin that order (the scheduler otherwise sinks every
      // read to just before its use, exposing the LDS latency once per chunk).
      constexpr int KH = KQ / 2 > 0 ? KQ / 2 : 1, NCH = (TMT / 16) * (KQ / KH);
      const float *bsrc = s_a + l15 * LD + (lg >> 1) * (CIN / 2) + (lg & 1) * 4;
      f32x4 bq[2][KH];
      auto bload = [&](int c) {
        const int mt = c / (KQ / KH), h = c % (KQ / KH);
#pragma unroll
        for (int q = 0; q < KH; ++q) bq[c & 1][q] = ld4(bsrc + mt * 16 * LD + (h * KH + q) * 8);
      };
      bload(0);
      if (NCH > 1) bload(1);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int mt = c / (KQ / KH), h = c % (KQ / KH);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < KH; ++q)
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < NT; ++j)
              acc[mt][j] = MFMA16(wf[j][(h * KH + q) * 4 + u], bq[c & 1][q][u], acc[mt][j]);
        __builtin_amdgcn_sched_barrier(0);
        if (c + 2 < NCH) bload(c + 2);
      }
    }
#pragma unroll
    for (int mt = 0; mt < TMT / 16; ++mt)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        if (TAIL) {
          f32x4 v = acc[mt][j] + bv[j];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = fmaxf(v[u], 0.f);
          st4(&s_o[(mt * 16 + l15) * LDO + wc + 16 * j + 4 * lg], v);
        } else {
          st4(&s_o[(mt * 16 + l15) * LDO + wc + 16 * j + 4 * lg], acc[mt][j]);
          if (FULL || row0 + mt * 16 + l15 < R) {
            ssum[j] += acc[mt][j];
            ssq[j] += acc[mt][j] * acc[mt][j];
          }
        }
      }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NO; ++i) {
      const int row = or0 + i * OSTEP;
      if (FULL || row0 + row < R) st4(zout + (size_t)(row0 + row) * Cout + cbb + o4 * 4, ld4(&s_o[row * LDO + o4 * 4]));
    }
    if (TAIL) {   // wave w: rows 16 w .. 16 w + 15 of the tile times the padded output weights
      f32x4 a3 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < COB / 4; ++ks) a3 = MFMA16(wf3[TAIL ? ks : 0], s_o[(w * 16 + l15) * LDO + ks * 4 + lg], a3);
      const long row = row0 + w * 16 + l15;
      if (FULL || row < R) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (4 * lg + u < ta.NO3) ta.pred[(size_t)row * ta.NO3 + 4 * lg + u] = a3[u] + ta.b3[4 * lg + u];
      }
    }
  };
  const long nfull = R / TMT;
  bool pending = false;
  if ((long)blockIdx.x < nfull) fetch(blockIdx.x);
  for (long t = blockIdx.x; t < nfull; t += gridDim.x) {
    tile(t, std::true_type{}, pending);
    pending = true;
  }
  // the last prefetch is unused, but its destination registers must stay reserved until it has landed
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int i = 0; i < NV; ++i) asm volatile("" ::"v"(pre[i]));
  if (nfull < ntiles && (long)blockIdx.x == nfull % gridDim.x) {  // ragged last tile
    fetch(nfull);
    tile(nfull, std::false_type{}, false);
  }
  if (TAIL) return;
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float a = ssum[j][u], q = ssq[j][u];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) a += __shfl_xor(a, o), q += __shfl_xor(q, o);
      if (l15 == 0) {
        const int c = cb + 16 * j + 4 * lg + u;
        part[((size_t)blockIdx.x * 2 + 0) * Cout + c] = (double)a;
        part[((size_t)blockIdx.x * 2 + 1) * Cout + c] = (double)q;
        for (int pr = blockIdx.x + gridDim.x; pr < NPART; pr += gridDim.x)  // partial rows without a workgroup
          part[((size_t)pr * 2 + 0) * Cout + c] = 0.0, part[((size_t)pr * 2 + 1) * Cout + c] = 0.0;
      }
    }
}

#include "sa_bf3.inc"

// ---- pooling forward: out[g, c] = max_s relu(bn(z[g*S+s, c])), first maximum ------------------------------------
__global__ __launch_bounds__(256) void sa_pool_fwd_kernel(const float *__restrict__ z, const float *__restrict__ st,
                                                          long G, int S, int C, float *__restrict__ out,
                                                          uint8_t *__restrict__ arg) {
  const int C4 = C / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= G * C4) return;
  const long g = i / C4;
  const int c4 = (int)(i % C4);
  f32x4 mean, sc, be;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float *s = st + (size_t)(c4 * 4 + u) * 4;
    mean[u] = s[0], sc[u] = s[2], be[u] = s[3];
  }
  f32x4 best = {-1.f, -1.f, -1.f, -1.f};
  int bi[4] = {0, 0, 0, 0};
  const float *p = z + ((size_t)g * S) * C + c4 * 4;
#pragma unroll 4
  for (int s = 0; s < S; ++s, p += C) {
    const f32x4 v = ld4(p);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float a = fmaxf((v[u] - mean[u]) * sc[u] + be[u], 0.f);
      if (a > best[u]) best[u] = a, bi[u] = s;
    }
  }
  st4(out + (size_t)g * C + c4 * 4, best);
  *reinterpret_cast<uchar4 *>(arg + (size_t)g * C + c4 * 4) =
      make_uchar4((unsigned char)bi[0], (unsigned char)bi[1], (unsigned char)bi[2], (unsigned char)bi[3]);
}

}  // namespace

// ===========================================================================================================
extern "C" int spacap_sa_nparts(void) { return NPART; }

extern "C" int spacap_sa_mlp_supported(int C1, int C2, int C3) {
  const bool sa1 = (C1 == 64 && C2 == 64 && C3 == 128);
  const bool big = (C1 == 128 && C2 == 128 && (C3 == 128 || C3 == 256));
  return (sa1 || big) ? 1 : 0;
}

extern "C" int spacap_sa_l1_fwd_f32(const float *Y, const float *feat, const float *xyz, const float *new_xyz,
                                    const int32_t *idx, const float *W1, int ldw, float rdiv, int B, int Np, int N,
                                    int S, int C1, float *z1, double *part, spacap_stream_t stream) {
  const char *what = "spacap_sa_l1_fwd_f32";
  SPACAP_REQUIRE(B >= 1 && Np >= 1 && N >= 1 && S >= 1 && S <= 255, "%s: bad sizes", what);
  SPACAP_REQUIRE(C1 == 64 || C1 == 128, "%s: C1=%d unsupported", what, C1);
  SPACAP_REQUIRE(xyz && new_xyz && idx && W1 && z1 && part && ldw >= (feat ? 4 : 3) && rdiv > 0.f, "%s: bad arguments", what);
  const long R = (long)B * N * S;
  hipStream_t s = spacap::as_stream(stream);
  if (C1 == 64)
    hipLaunchKernelGGL((sa_l1_fwd_kernel<64>), dim3(NPART), dim3(256), 0, s, Y, feat, xyz, new_xyz, idx, W1, ldw, rdiv, Np, N, S, R, z1, part);
  else
    hipLaunchKernelGGL((sa_l1_fwd_kernel<128>), dim3(NPART), dim3(256), 0, s, Y, feat, xyz, new_xyz, idx, W1, ldw, rdiv, Np, N, S, R, z1, part);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// The same pass WITHOUT the z1 store: the BatchNorm sums of the first layer and rel4 [R][4] = each grouped row's four inputs
// (relative x, y, z / rdiv, inline feature or 0).  The later passes rebuild z1 from rel4 and W1 (spacap_sa_*_l1in_f32): 16 bytes
// per row instead of 4 C1 written once and read three times.  Modules whose first layer also has point features (Y) keep z1.
extern "C" int spacap_sa_l1_stats_f32(const float *feat, const float *xyz, const float *new_xyz, const int32_t *idx, const float *W1,
                                      int ldw, float rdiv, int B, int Np, int N, int S, int C1, float *rel4, double *part,
                                      spacap_stream_t stream) {
  const char *what = "spacap_sa_l1_stats_f32";
  SPACAP_REQUIRE(B >= 1 && Np >= 1 && N >= 1 && S >= 1 && S <= 255, "%s: bad sizes", what);
  SPACAP_REQUIRE(C1 == 64, "%s: C1=%d unsupported", what, C1);
  SPACAP_REQUIRE(xyz && new_xyz && idx && W1 && rel4 && part && ldw >= (feat ? 4 : 3) && rdiv > 0.f, "%s: bad arguments", what);
  const long R = (long)B * N * S;
  hipLaunchKernelGGL((sa_l1_fwd_kernel<64>), dim3(NPART), dim3(256), 0, spacap::as_stream(stream), (const float *)nullptr, feat, xyz,
                     new_xyz, idx, W1, ldw, rdiv, Np, N, S, R, (float *)nullptr, part, rel4);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// The same pass in closed form (sa_l1_moments_kernel): rel4 f32 [B*N*S, 4] and the moments of the rows' four inputs,
// mom f64 [spacap_sa_nparts()][16]; spacap_sa_l1_moments_finalize_f32 turns them into the first layer's statistics.
extern "C" int spacap_sa_l1_moments_f32(const float *feat, const float *xyz, const float *new_xyz, const int32_t *idx, float rdiv, int B,
                                        int Np, int N, int S, float *rel4, double *mom, spacap_stream_t stream) {
  const char *what = "spacap_sa_l1_moments_f32";
  SPACAP_REQUIRE(B >= 1 && Np >= 1 && N >= 1 && S >= 1 && S <= 255, "%s: bad sizes", what);
  SPACAP_REQUIRE(xyz && new_xyz && idx && rel4 && mom && rdiv > 0.f && spacap::aligned16(rel4), "%s: bad arguments", what);
  const long R = (long)B * N * S;
  hipLaunchKernelGGL(sa_l1_moments_kernel, dim3(NPART), dim3(256), 0, spacap::as_stream(stream), feat, xyz, new_xyz, idx, rdiv, Np, N, S, R,
                     rel4, mom);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_sa_l1_moments_finalize_f32(const double *mom, const float *W1, int ldw, int has_feat, int C1, long count, float eps,
                                                 float momentum, const float *gamma, const float *beta, float *running_mean,
                                                 float *running_var, float *stats, spacap_stream_t stream) {
  const char *what = "spacap_sa_l1_moments_finalize_f32";
  SPACAP_REQUIRE(mom && W1 && gamma && beta && stats && C1 >= 1 && C1 <= 1024 && count >= 1 && ldw >= (has_feat ? 4 : 3), "%s: bad arguments", what);
  hipLaunchKernelGGL(sa_l1_moments_finalize_kernel, dim3(1), dim3(1024), 0, spacap::as_stream(stream), mom, NPART, W1, ldw, has_feat, C1,
                     (double)count, eps, momentum, gamma, beta, running_mean, running_var, stats);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// Second layer (64 -> 64) reading rel4 instead of z1: z2 = relu(bn1(W1 in)) W2^T, BatchNorm sums of z2 in `part`
extern "C" int spacap_sa_mid_fwd_l1in_f32(const float *rel4, const float *W1, int ldw, int has_feat, const float *st_in, const float *W,
                                          long R, float *zout, double *part, spacap_stream_t stream) {
  const char *what = "spacap_sa_mid_fwd_l1in_f32";
  SPACAP_REQUIRE(rel4 && W1 && st_in && W && zout && part && R >= 1 && ldw >= (has_feat ? 4 : 3), "%s: bad arguments", what);
  const size_t lds = (size_t)TM * ((64 + 8) + (64 + 4)) * sizeof(float);
  const long tiles = (R + TM - 1) / TM;
  static const int res = resident_blocks(sa_mid_fwd_kernel<64, 1, false>, lds);
  hipLaunchKernelGGL((sa_mid_fwd_kernel<64, 1, false>), dim3(grid_rows(res, 1, tiles), 1), dim3(256), lds, spacap::as_stream(stream),
                     rel4, st_in, W, 64, R, zout, part, TailArgs{}, L1In{W1, ldw, has_feat});
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_sa_bn_finalize_f32(const double *part, int C, long count, float eps, float momentum,
                                         const float *gamma, const float *beta, float *running_mean,
                                         float *running_var, float *stats, spacap_stream_t stream) {
  const char *what = "spacap_sa_bn_finalize_f32";
  SPACAP_REQUIRE(part && gamma && beta && stats && C >= 1 && count >= 1, "%s: bad arguments", what);
  hipLaunchKernelGGL(sa_bn_finalize_kernel, dim3((C + 7) / 8), dim3(1024), 0, spacap::as_stream(stream), part, NPART, C,
                     (double)count, eps, momentum, gamma, beta, running_mean, running_var, stats);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_sa_mid_fwd_f32(const float *zin, const float *st_in, const float *W, long R, int Cin, int Cout,
                                     float *zout, double *part, spacap_stream_t stream) {
  const char *what = "spacap_sa_mid_fwd_f32";
  SPACAP_REQUIRE(zin && st_in && W && zout && part && R >= 1, "%s: bad arguments", what);
  hipStream_t s = spacap::as_stream(stream);
  const int nt = (Cin == 64 && Cout == 64) ? 1 : 2;
  // default: the streaming split-bf16 kernel (fp32-equivalent products); SPACAP_SA_F32MFMA=1 (the
  // library's one switch) keeps every shared-MLP product on the fp32-MFMA kernels
  if (!spacap::sa_f32_mfma_only() && (Cin == 64 || Cin == 128) && Cout % 128 == 0) {
    const size_t ldss = bf3s_lds_bytes(Cin);
    const int gy = Cout / 128;
    const unsigned gx = stream_grid(fwd_cus(), gy, R);
    if (Cin == 64)
      hipLaunchKernelGGL((sa_mid_fwd_bf3s_kernel<64, 1>), dim3(gx, gy), dim3(512), ldss, s, zin, st_in, W, Cout, R, zout,
                         part, PoolArgs{});
    else
      hipLaunchKernelGGL((sa_mid_fwd_bf3s_kernel<128, 1>), dim3(gx, gy), dim3(512), ldss, s, zin, st_in, W, Cout, R, zout,
                         part, PoolArgs{});
    SPACAP_CHECK_LAUNCH(what);
    return SPACAP_OK;
  }
  const size_t lds = (size_t)TM * ((Cin + 8) + (64 * nt + 4)) * sizeof(float);
  const long tiles = (R + TM - 1) / TM;
#define MF(CI, NTV, GY)                                                                                              \
  {                                                                                                                  \
    static const int res = resident_blocks(sa_mid_fwd_kernel<CI, NTV, false>, lds);                                  \
    hipLaunchKernelGGL((sa_mid_fwd_kernel<CI, NTV, false>), dim3(grid_rows(res, GY, tiles), GY), dim3(256), lds, s,  \
                       zin, st_in, W, Cout, R, zout, part, TailArgs{});                                              \
  }
  if (Cin == 64 && Cout == 64) MF(64, 1, 1)
  else if (Cin == 64 && Cout % 128 == 0) MF(64, 2, Cout / 128)
  else if (Cin == 128 && Cout % 128 == 0) MF(128, 2, Cout / 128)
  else
    SPACAP_REQUIRE(false, "%s: (Cin=%d, Cout=%d) unsupported", what, Cin, Cout);
#undef MF
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// ---- pooling from the candidates the streaming layer kernel left (PoolArgs in sa_bf3.inc) -----------------------------
// per (group, channel): merge the sub-groups' candidate lists (S = 64: two halves, the second with indices + 32), evaluate the
// activation of the best and of the runner-up, and keep the reference's first maximum:
//   equal activations -> smaller row index;  activation 0 (or a constant channel) -> row 0, as a strict ">" scan from -1 does.
__global__ __launch_bounds__(256) void sa_pool_finalize_kernel(const float *__restrict__ cand_v, const uint8_t *__restrict__ cand_i,
                                                               const float *__restrict__ st, const float *__restrict__ gamma,
                                                               long G, int S, int C, float *__restrict__ out,
                                                               uint8_t *__restrict__ arg, float *__restrict__ zmax) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= G * C) return;
  const long g = i / C;
  const int c = (int)(i % C);
  const int nsub = S > 32 ? S / 32 : 1;
  size_t o = ((size_t)(g * nsub) * C + c) * 2;
  float t1 = cand_v[o], t2 = cand_v[o + 1];
  int i1 = cand_i[o], i2 = cand_i[o + 1];
  for (int h = 1; h < nsub; ++h) {   // later sub-groups: all their indices are larger, ties go to what we have
    o = ((size_t)(g * nsub + h) * C + c) * 2;
    const float u1 = cand_v[o], u2 = cand_v[o + 1];
    const int j1 = cand_i[o] + 32 * h, j2 = cand_i[o + 1] + 32 * h;
    const bool mine = !(u1 > t1);
    const float w1 = mine ? t1 : u1, l1 = mine ? u1 : t1;
    const int wi = mine ? i1 : j1, li = mine ? j1 : i1;
    float c2 = l1 < w1 ? l1 : -INFINITY;
    int ci = li;
    if (t2 > c2 || (t2 == c2 && i2 < ci)) c2 = t2, ci = i2;
    if (u2 > c2 || (u2 == c2 && j2 < ci)) c2 = u2, ci = j2;
    t1 = w1, i1 = wi, t2 = c2, i2 = ci;
  }
  const float *s = st + (size_t)c * 4;
  const float mean = s[0], sc = s[2], be = s[3], sg = gamma[c] >= 0.f ? 1.f : -1.f;
  const float v1 = fmaxf((sg * t1 - mean) * sc + be, 0.f);
  int a = i1;
  float za = sg * t1;     // the pre-activation of the chosen row
  if (t2 > -INFINITY) {
    const float v2 = fmaxf((sg * t2 - mean) * sc + be, 0.f);
    if (v2 == v1 && i2 < i1) a = i2, za = sg * t2;
  }
  if (!(v1 > 0.f) || sc == 0.f) a = 0;
  out[i] = v1;
  arg[i] = (uint8_t)a;
  // what the pooled layer's BatchNorm backward needs of z (xhat at the arg-max row) when z itself is not stored.  Where the
  // choice fell back to row 0 -- the activation is 0: no gradient; or gamma == 0 exactly: a constant channel -- this is the
  // best row's value, not row 0's (only d gamma of an exactly-zero gamma could tell the difference).
  if (zmax) zmax[i] = za;
}

/* 1 when spacap_sa_mid_fwd_pool_f32 has a kernel for this layer (the streaming split-bf16 kernel is the active one). */
/* out[R][Cout] = x[R][Cin] W[Cout][Cin]^T, fp32 in / out / accumulate, on the streaming split-bf16 kernel (every fp32 product as
   six bf16 matrix products): the relation head's dhid1 = dz2 W2 (models/transformer_captioner.py:319-326 backward), 524 288
   rows.  _supported: 1 for Cin in {64, 128}, Cout a multiple of 128 (and the split kernels not switched off). */
extern "C" int spacap_gemm_rows_supported(int Cin, int Cout) {
  return !spacap::sa_f32_mfma_only() && (Cin == 64 || Cin == 128) && Cout % 128 == 0;
}
extern "C" int spacap_gemm_rows_f32(const float *x, const float *W, long R, int Cin, int Cout, float *out,
                                    spacap_stream_t stream) {
  const char *what = "spacap_gemm_rows_f32";
  SPACAP_REQUIRE(x && W && out && R >= 1, "%s: bad arguments", what);
  SPACAP_REQUIRE(spacap_gemm_rows_supported(Cin, Cout), "%s: (Cin=%d, Cout=%d) unsupported", what, Cin, Cout);
  hipStream_t s = spacap::as_stream(stream);
  const size_t ldss = bf3s_lds_bytes(Cin);
  const int gy = Cout / 128;
  const unsigned gx = stream_grid(bwd_cus(), gy, R);
  if (Cin == 64)
    hipLaunchKernelGGL((sa_mid_fwd_bf3s_kernel<64, 1, false, true>), dim3(gx, gy), dim3(512), ldss, s, x,
                       (const float *)nullptr, W, Cout, R, out, (double *)nullptr, PoolArgs{});
  else
    hipLaunchKernelGGL((sa_mid_fwd_bf3s_kernel<128, 1, false, true>), dim3(gx, gy), dim3(512), ldss, s, x,
                       (const float *)nullptr, W, Cout, R, out, (double *)nullptr, PoolArgs{});
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_sa_mid_fwd_pool_supported(int Cin, int Cout, int S) {
  return !spacap::sa_f32_mfma_only() && (Cin == 64 || Cin == 128) && Cout % 128 == 0 && (S == 16 || S == 32 || S == 64);
}

/* spacap_sa_mid_fwd_f32 for the LAST layer of a shared MLP whose output is max-pooled over groups of S consecutive rows:
   also leaves the pooling candidates (cand_v f32 / cand_i u8, [R / min(S,32)][Cout][2]) for spacap_sa_pool_finalize_f32.
   gamma_out: BatchNorm weight of this layer's output (its sign orders the activations). */
extern "C" int spacap_sa_mid_fwd_pool_f32(const float *zin, const float *st_in, const float *W, const float *gamma_out, long R,
                                          int Cin, int Cout, int S, float *zout, double *part, float *cand_v,
                                          uint8_t *cand_i, spacap_stream_t stream) {
  const char *what = "spacap_sa_mid_fwd_pool_f32";
  SPACAP_REQUIRE(zin && st_in && W && gamma_out && part && cand_v && cand_i && R >= 1, "%s: bad arguments", what);   // (zout may be NULL)
  SPACAP_REQUIRE(spacap_sa_mid_fwd_pool_supported(Cin, Cout, S) && R % S == 0, "%s: (Cin=%d, Cout=%d, S=%d) unsupported", what,
                 Cin, Cout, S);
  hipStream_t s = spacap::as_stream(stream);
  const size_t ldss = bf3s_lds_bytes(Cin);
  const int gy = Cout / 128;
  const unsigned gx = stream_grid(fwd_cus(), gy, R);
  const PoolArgs pa{gamma_out, S, cand_v, cand_i};
  if (Cin == 64)
    hipLaunchKernelGGL((sa_mid_fwd_bf3s_kernel<64, 1, true>), dim3(gx, gy), dim3(512), ldss, s, zin, st_in, W, Cout,
                       R, zout, part, pa);
  else
    hipLaunchKernelGGL((sa_mid_fwd_bf3s_kernel<128, 1, true>), dim3(gx, gy), dim3(512), ldss, s, zin, st_in, W, Cout,
                       R, zout, part, pa);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

/* out[g,c] = max_s relu(bn(z[g*S+s,c])) (first maximum) and its arg, from the candidates of spacap_sa_mid_fwd_pool_f32. */
extern "C" int spacap_sa_pool_finalize_f32(const float *cand_v, const uint8_t *cand_i, const float *stats, const float *gamma,
                                           long G, int S, int C, float *out, uint8_t *arg, float *zmax, spacap_stream_t stream) {
  const char *what = "spacap_sa_pool_finalize_f32";
  SPACAP_REQUIRE(cand_v && cand_i && stats && gamma && out && arg && G >= 1 && C >= 1, "%s: bad arguments", what);
  SPACAP_REQUIRE(S == 16 || S == 32 || S == 64, "%s: S=%d unsupported", what, S);
  hipLaunchKernelGGL(sa_pool_finalize_kernel, dim3(nblocks(G * C, 256)), dim3(256), 0, spacap::as_stream(stream), cand_v, cand_i,
                     stats, gamma, G, S, C, out, arg, zmax);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_sa_pool_fwd_f32(const float *z, const float *stats, long G, int S, int C, float *out,
                                      uint8_t *arg, spacap_stream_t stream) {
  const char *what = "spacap_sa_pool_fwd_f32";
  SPACAP_REQUIRE(z && stats && out && arg && G >= 1 && S >= 1 && S <= 255 && C % 4 == 0, "%s: bad arguments", what);
  hipLaunchKernelGGL(sa_pool_fwd_kernel, dim3(nblocks(G * (C / 4), 256)), dim3(256), 0, spacap::as_stream(stream), z, stats,
                     G, S, C, out, arg);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// ---- relation head, layers 2 and 3, forward (backward: rel_tail.hip) -----------------------------------------------------------
// hid2 = relu(hid1 W2^T + b2) [R,128],  pred = hid2 W3^T + b3 [R,9] on R = B*K*K pair rows in one pass of sa_mid_fwd_kernel's
// TAIL = true form (read hid1, write hid2 and pred).  Its persistent grid leaves the reserved CUs out (fwd_resident).
// hid1 f32 [R,128], W2 f32 [128,128], b2 f32 [128], W3 f32 [9,128], b3 f32 [9] -> hid2 f32 [R,128], pred f32 [R,9]
extern "C" int spacap_rel_tail_fwd_f32(const float *hid1, const float *W2, const float *b2, const float *W3, const float *b3,
                                       long R, float *hid2, float *pred, spacap_stream_t stream) {
  const char *what = "spacap_rel_tail_fwd_f32";
  SPACAP_REQUIRE(hid1 && W2 && b2 && W3 && b3 && hid2 && pred && R >= 1, "%s: bad arguments", what);
  const size_t lds = (size_t)TM * ((128 + 8) + (128 + 4)) * sizeof(float);
  const long tiles = (R + TM - 1) / TM;
  static const int res = resident_blocks(sa_mid_fwd_kernel<128, 2, true>, lds);
  hipLaunchKernelGGL((sa_mid_fwd_kernel<128, 2, true>), dim3(grid_rows(fwd_resident(res), 1, tiles), 1), dim3(256), lds,
                     spacap::as_stream(stream), hid1, (const float *)nullptr, W2, 128, R, hid2, (double *)nullptr,
                     TailArgs{b2, W3, b3, pred, 9});
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
