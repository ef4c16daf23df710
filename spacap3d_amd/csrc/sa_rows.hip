// The inverted index of a grouping -- which grouped rows reference each source point, ascending -- and everything that reads it:
// the sums of row gradients over the rows of a source point (the feature gradient of a set-abstraction module's first layer, the
// gradient of the relative coordinates).  A function of idx alone, i.e. of the input coordinates: a trainer can build it ahead of
// the step.  Built in one launch (rows_index_kernel) at the model's shapes, by a radix sort otherwise: this is the only file that
// includes hipcub.
#include <hipcub/hipcub.hpp>

#include "common.hpp"
#include "launch.hpp"
#include "mfma.hpp"

namespace {
using namespace spacap::mfma;
using namespace spacap::launch;

// ---- rows -> source points: dY[b, p, :] = sum over the rows r with idx[r] = p of dz1[r, :] --------------------
__global__ __launch_bounds__(256) void rows_keys_kernel(const int32_t *__restrict__ idx, int Np, long E, long total,
                                                        unsigned *__restrict__ keys, int *__restrict__ vals) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  keys[i] = (unsigned)((i / E) * Np + idx[i]);
  vals[i] = (int)i;
}

__global__ __launch_bounds__(256) void rows_offsets_kernel(const unsigned *__restrict__ sorted, long total, long K,
                                                           int *__restrict__ off) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k > K) return;
  long lo = 0, hi = total;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if ((long)sorted[mid] < k) lo = mid + 1; else hi = mid;
  }
  off[k] = (int)lo;
}

// The same index without a sort, one launch: a workgroup of 16 waves per scene.  Wave w owns the w-th stretch of the scene's
// rows.  (1) per-wave histograms h[w][p] (16-bit counters, two per LDS word), (2) per point: counts -> exclusive prefix over the
// waves, totals -> exclusive scan over the points = off, (3) every wave walks its stretch in order, 64 rows at a time; a row's
// slot is off[p] + rows of p in earlier waves + in earlier iterations of this wave + in lower lanes of this iteration (one
// ballot per distinct point among the 64 rows).  Ascending row order within a point by construction: the result equals the
// stable sort's.  Np <= 4096, E <= 65535 (LDS, 16-bit counters); other shapes take the radix sort below.
constexpr int RI_WAVES = 16;
__global__ __launch_bounds__(1024) void rows_index_kernel(const int32_t *__restrict__ idx, int Np, int E, int B,
                                                          int *__restrict__ off, int *__restrict__ order) {
  extern __shared__ unsigned s_ri[];
  const int NpW = (Np + 1) / 2;
  unsigned *h = s_ri;                                        // [16][NpW]
  int *start = reinterpret_cast<int *>(h + RI_WAVES * NpW);  // [2 NpW]
  int *wsum = start + 2 * NpW;                               // [1024]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, b = blockIdx.x;
  const int32_t *ib = idx + (size_t)b * E;
  const int seg = ((E + RI_WAVES * 64 - 1) / (RI_WAVES * 64)) * 64, e_beg = w * seg, e_end = min(E, e_beg + seg);
  for (int i = tid; i < RI_WAVES * NpW; i += 1024) h[i] = 0u;
  __syncthreads();
  for (int e = e_beg + lane; e < e_end; e += 64) {
    const int p = ib[e];
    atomicAdd(&h[w * NpW + (p >> 1)], 1u << (16 * (p & 1)));
  }
  __syncthreads();
  for (int q = tid; q < NpW; q += 1024) {   // one word = two points: counts -> prefix over the waves, totals -> start
    unsigned a0 = 0, a1 = 0;
    for (int v = 0; v < RI_WAVES; ++v) {
      const unsigned c = h[v * NpW + q];
      h[v * NpW + q] = a0 | (a1 << 16);
      a0 += c & 0xffffu, a1 += c >> 16;
    }
    start[2 * q] = (int)a0, start[2 * q + 1] = (int)a1;
  }
  __syncthreads();
  {   // exclusive scan of start[0 .. 2 NpW): CH consecutive entries per thread, then the 1024 partial sums
    const int CH = (2 * NpW + 1023) / 1024, lo = min(tid * CH, 2 * NpW), hi = min(lo + CH, 2 * NpW);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += start[i];
    wsum[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const int v = tid >= d ? wsum[tid - d] : 0;
      __syncthreads();
      wsum[tid] += v;
      __syncthreads();
    }
    int run = wsum[tid] - sum;
    for (int i = lo; i < hi; ++i) {
      const int c = start[i];
      start[i] = run;
      if (i < Np) off[(size_t)b * Np + i] = b * E + run;
      run += c;
    }
    if (b == B - 1 && tid == 0) off[(size_t)B * Np] = B * E;
  }
  __syncthreads();
  for (int e0 = e_beg; e0 < e_end; e0 += 64) {
    const int e = e0 + lane;
    const bool active = e < e_end;
    const int p = active ? ib[e] : -1;
    unsigned long long todo = __ballot(active);
    int rank = 0, n = 0;
    bool lead = false;
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int k = __builtin_amdgcn_readlane(p, leader);
      const unsigned long long m = __ballot(p == k);
      if (p == k) rank = __popcll(m & ((1ull << lane) - 1ull)), n = __popcll(m), lead = lane == leader;
      todo &= ~m;
    }
    if (active) {
      const unsigned word = h[w * NpW + (p >> 1)];
      const int pos = start[p] + (int)((word >> (16 * (p & 1))) & 0xffffu) + rank;
      order[(size_t)b * E + pos] = b * E + e;
    }
    if (lead) atomicAdd(&h[w * NpW + (p >> 1)], (unsigned)n << (16 * (p & 1)));
  }
}

__global__ __launch_bounds__(256) void rows_gather_sum_kernel(const float *__restrict__ dz, const int *__restrict__ off,
                                                              const int *__restrict__ order, long K, int C,
                                                              float *__restrict__ out) {
  const int C4 = C / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= K * C4) return;
  const long k = i / C4;
  const int c4 = (int)(i % C4);
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  const int beg = off[k], end = off[k + 1];
  // (order[p] -> row is a dependent chain: four of them in flight per iteration; the sum keeps its order)
  int p = beg;
  for (; p + 3 < end; p += 4) {
    const int o0 = order[p], o1 = order[p + 1], o2 = order[p + 2], o3 = order[p + 3];
    const f32x4 r0 = ld4(dz + (size_t)o0 * C + c4 * 4), r1 = ld4(dz + (size_t)o1 * C + c4 * 4),
                r2 = ld4(dz + (size_t)o2 * C + c4 * 4), r3 = ld4(dz + (size_t)o3 * C + c4 * 4);
    a += r0;
    a += r1;
    a += r2;
    a += r3;
  }
  for (; p < end; ++p) a += ld4(dz + (size_t)order[p] * C + c4 * 4);
  st4(out + (size_t)k * C + c4 * 4, a);
}

// Gradient of the relative coordinates (rel = (xyz[idx] - new_xyz) / r, drel [B * E][3], E = N S rows per scene) routed to
// both of its sources in one launch, fixed summation orders (the autograd composition is a zero-fill + an int64 copy of idx +
// an atomic scatter_add_ + a sum + a neg):
//   threads 0 .. K-1 (K = B Np):   dxyz[k][:] = sum of drel[r][:] over the rows r that reference source point k, ascending r
//   threads K .. K + B N - 1:      dnew[g][:] = - sum_s drel[g S + s][:]
__global__ __launch_bounds__(256) void sa_drel_sums_kernel(const float *__restrict__ drel, const int *__restrict__ off,
                                                           const int *__restrict__ order, long K, long G, int S,
                                                           float *__restrict__ dxyz, float *__restrict__ dnew) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < K) {
    if (!dxyz) return;
    float ax = 0.f, ay = 0.f, az = 0.f;
    const int beg = off[i], end = off[i + 1];
    int p = beg;
    for (; p + 3 < end; p += 4) {   // (order[p] -> row is a dependent chain: four in flight, the sum keeps its order)
      const float *r0 = drel + (size_t)order[p] * 3, *r1 = drel + (size_t)order[p + 1] * 3, *r2 = drel + (size_t)order[p + 2] * 3,
                  *r3 = drel + (size_t)order[p + 3] * 3;
      const float x0 = r0[0], y0 = r0[1], z0 = r0[2], x1 = r1[0], y1 = r1[1], z1 = r1[2];
      const float x2 = r2[0], y2 = r2[1], z2 = r2[2], x3 = r3[0], y3 = r3[1], z3 = r3[2];
      ax += x0, ay += y0, az += z0;
      ax += x1, ay += y1, az += z1;
      ax += x2, ay += y2, az += z2;
      ax += x3, ay += y3, az += z3;
    }
    for (; p < end; ++p) {
      const float *r = drel + (size_t)order[p] * 3;
      ax += r[0], ay += r[1], az += r[2];
    }
    dxyz[i * 3] = ax, dxyz[i * 3 + 1] = ay, dxyz[i * 3 + 2] = az;
  } else if (i < K + G && dnew) {
    const long g = i - K;
    const float *r = drel + (size_t)g * S * 3;
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int sidx = 0; sidx < S; ++sidx) ax += r[sidx * 3], ay += r[sidx * 3 + 1], az += r[sidx * 3 + 2];
    dnew[g * 3] = -ax, dnew[g * 3 + 1] = -ay, dnew[g * 3 + 2] = -az;
  }
}

struct RowsLayout {
  size_t total, K, keys_in, keys_out, vals_in, vals_out, off, cub, cub_bytes, bytes;
  int bits;
};
bool rows_layout(int B, int Np, long E, RowsLayout &L) {
  if (B <= 0 || Np <= 0 || E <= 0) return false;
  L.total = (size_t)B * E;
  L.K = (size_t)B * Np;
  if (L.K >= (1ull << 31) || L.total >= (1ull << 31)) return false;
  L.bits = 1;
  while ((1ull << L.bits) < L.K) ++L.bits;
  size_t cub = 0;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, cub, (const unsigned *)nullptr, (unsigned *)nullptr,
                                         (const int *)nullptr, (int *)nullptr, (int)L.total, 0, L.bits,
                                         (hipStream_t)0) != hipSuccess)
    cub = 0;
  (void)hipGetLastError();
  if (cub == 0) cub = 16 * L.total + (1 << 20);
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  size_t o = 0;
  L.keys_in = o; o += up(4 * L.total);
  L.keys_out = o; o += up(4 * L.total);
  L.vals_in = o; o += up(4 * L.total);
  L.vals_out = o; o += up(4 * L.total);
  L.off = o; o += up(4 * (L.K + 1));
  L.cub = o; L.cub_bytes = cub; o += up(cub);
  L.bytes = o;
  return true;
}

}  // namespace

// ===========================================================================================================
extern "C" size_t spacap_sa_rows_scatter_workspace_bytes(int B, int Np, long E) {
  RowsLayout L;
  return rows_layout(B, Np, E, L) ? L.bytes : 0;
}

// The inverted index of a grouping (which rows reference each source point, ascending): a function of idx alone, i.e.
// of the input coordinates -- a trainer can build it ahead of the step (detector.geometry_pyramid) and the backward
// then only gathers.  `workspace` (spacap_sa_rows_scatter_workspace_bytes) holds the index afterwards.
extern "C" int spacap_sa_rows_index_f32(const int32_t *idx, int B, int Np, long E, void *workspace, spacap_stream_t stream) {
  const char *what = "spacap_sa_rows_index_f32";
  RowsLayout L;
  SPACAP_REQUIRE(idx && workspace && rows_layout(B, Np, E, L), "%s: bad arguments", what);
  hipStream_t s = spacap::as_stream(stream);
  char *ws = reinterpret_cast<char *>(workspace);
  unsigned *keys_in = reinterpret_cast<unsigned *>(ws + L.keys_in), *keys_out = reinterpret_cast<unsigned *>(ws + L.keys_out);
  int *vals_in = reinterpret_cast<int *>(ws + L.vals_in), *vals_out = reinterpret_cast<int *>(ws + L.vals_out);
  int *off = reinterpret_cast<int *>(ws + L.off);
  if (Np <= 4096 && E <= 65535 && B <= 65535) {   // one launch, no sort
    const size_t lds = (size_t)(RI_WAVES * ((Np + 1) / 2) + 2 * ((Np + 1) / 2) + 1024) * 4;
    static unsigned long long lds_ok = 0;
    SPACAP_CHECK_HIP(spacap::allow_dynamic_lds(reinterpret_cast<const void *>(&rows_index_kernel), 160 * 1024, lds_ok), what);
    hipLaunchKernelGGL(rows_index_kernel, dim3(B), dim3(1024), lds, s, idx, Np, (int)E, B, off, vals_out);
    SPACAP_CHECK_LAUNCH(what);
    return SPACAP_OK;
  }
  hipLaunchKernelGGL(rows_keys_kernel, dim3(nblocks((long)L.total, 256)), dim3(256), 0, s, idx, Np, E, (long)L.total, keys_in, vals_in);
  size_t cub_bytes = L.cub_bytes;
  SPACAP_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(ws + L.cub, cub_bytes, keys_in, keys_out, vals_in, vals_out,
                                                      (int)L.total, 0, L.bits, s), what);
  hipLaunchKernelGGL(rows_offsets_kernel, dim3(nblocks((long)L.K + 1, 256)), dim3(256), 0, s, keys_out, (long)L.total, (long)L.K, off);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// out[b, p, :] = sum of dz[r, :] over the rows r = (b, e) with idx[b, e] = p, ascending r, from the index
// spacap_sa_rows_index_f32 left in `workspace` (same B, Np, E)
extern "C" int spacap_sa_rows_gather_f32(const float *dz, int B, int Np, long E, int C, const void *workspace, float *out,
                                         spacap_stream_t stream) {
  const char *what = "spacap_sa_rows_gather_f32";
  RowsLayout L;
  SPACAP_REQUIRE(dz && out && workspace && C % 4 == 0 && rows_layout(B, Np, E, L), "%s: bad arguments", what);
  const char *ws = reinterpret_cast<const char *>(workspace);
  hipLaunchKernelGGL(rows_gather_sum_kernel, dim3(nblocks((long)L.K * (C / 4), 256)), dim3(256), 0, spacap::as_stream(stream), dz,
                     reinterpret_cast<const int *>(ws + L.off), reinterpret_cast<const int *>(ws + L.vals_out), (long)L.K, C, out);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// drel f32 [B, N S, 3] -> dxyz f32 [B, Np, 3] (sum over the rows that reference each source point, ascending, from the index
// spacap_sa_rows_index_f32 left in `workspace`; may be NULL) and dnew f32 [B, N, 3] = - sum over each group's S rows (may be NULL)
extern "C" int spacap_sa_drel_sums_f32(const float *drel, int B, int Np, int N, int S, const void *workspace, float *dxyz, float *dnew,
                                       spacap_stream_t stream) {
  const char *what = "spacap_sa_drel_sums_f32";
  RowsLayout L;
  SPACAP_REQUIRE(drel && (dxyz || dnew) && N >= 1 && S >= 1 && rows_layout(B, Np, (long)N * S, L) && (!dxyz || workspace),
                 "%s: bad arguments", what);
  const char *ws = reinterpret_cast<const char *>(workspace);
  const long K = (long)L.K, G = (long)B * N;
  hipLaunchKernelGGL(sa_drel_sums_kernel, dim3(nblocks(K + G, 256)), dim3(256), 0, spacap::as_stream(stream), drel,
                     ws ? reinterpret_cast<const int *>(ws + L.off) : nullptr, ws ? reinterpret_cast<const int *>(ws + L.vals_out) : nullptr,
                     K, G, S, dxyz, dnew);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

// out[b, p, :] = sum of dz[r, :] over the rows r = (b, e) with idx[b, e] = p, ascending r (E = rows per scene)
extern "C" int spacap_sa_rows_scatter_f32(const float *dz, const int32_t *idx, int B, int Np, long E, int C, float *out,
                                          void *workspace, spacap_stream_t stream) {
  SPACAP_REQUIRE(dz && out && C % 4 == 0, "spacap_sa_rows_scatter_f32: bad arguments");
  const int rc = spacap_sa_rows_index_f32(idx, B, Np, E, workspace, stream);
  return rc ? rc : spacap_sa_rows_gather_f32(dz, B, Np, E, C, workspace, out, stream);
}
