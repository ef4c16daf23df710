// Caption decoding over the kept proposals only, for gfx950 (MI355X): the decoders of caption_decode.hip take any number of
// independent rows, and every reader of lang_cap reads it only where post-processing kept the box.  This unit makes the rows
// sparse: pack the flagged (scene, proposal) pairs into a dense row list, read the decoder's indicator rows through that list,
// and put the captions, scores and lengths back where the readers expect them.
//
//  decode_select_kernel   ONE workgroup of 256 threads: the ordered compaction of n <= 65 536 flags.  Thread t owns the
//                         contiguous chunk [t c, (t + 1) c), c = ceil(n / 256): it counts its set flags, a block scan over the
//                         256 counts in LDS ranks the chunks, and a second walk over the chunk writes slot[] and rows[].  The
//                         tail of rows[] behind the last kept flag is filled with -1 by all threads.
//  decode_gather_kernel   out[i] = obj[rows[i]] (+ memory[rows[i]]), one thread per 16-byte piece of a row: consecutive lanes
//                         read and write consecutive 16 bytes (d = 128: 32 lanes a row, a wave moves 1 KiB).  rows[i] < 0: +0.0.
//  decode_scatter_kernel  out[j] = slot[j] >= 0 ? vals[slot[j]] : the fill, one thread per element, consecutive lanes
//                         consecutive elements.  For words the fill is the empty caption: eos at l % L == 0, else 0.
// Every element of every output is written on every call; no atomics, no allocation, no state between calls, no host
// synchronisation; plain vector loads and stores only.
#include "common.hpp"

namespace {

constexpr int DS_THREADS = 256;
constexpr long DS_MAX_N = 65536;
constexpr long DS_MAX_INNER = 1 << 20;

__global__ __launch_bounds__(DS_THREADS) void decode_select_kernel(const uint8_t *__restrict__ mask, int n, int capacity,
                                                                   int32_t *__restrict__ rows, int32_t *__restrict__ slot,
                                                                   int32_t *__restrict__ count) {
  __shared__ int s_scan[2][DS_THREADS];
  const int t = threadIdx.x;
  const int chunk = (n + DS_THREADS - 1) / DS_THREADS;
  const int lo = min(t * chunk, n), hi = min(lo + chunk, n);
  int mine = 0;
  for (int j = lo; j < hi; ++j) mine += mask[j] != 0 ? 1 : 0;
  // inclusive scan over the 256 chunk counts (Hillis-Steele, double-buffered)
  int cur = 0;
  s_scan[0][t] = mine;
  __syncthreads();
  for (int o = 1; o < DS_THREADS; o <<= 1) {
    const int v = s_scan[cur][t] + (t >= o ? s_scan[cur][t - o] : 0);
    s_scan[cur ^ 1][t] = v;
    cur ^= 1;
    __syncthreads();
  }
  const int total = s_scan[cur][DS_THREADS - 1];
  const int held = min(total, capacity);
  int pos = s_scan[cur][t] - mine;                  // the set flags ahead of this chunk
  for (int j = lo; j < hi; ++j) {
    int s = -1;
    if (mask[j] != 0) {
      if (pos < capacity) {
        s = pos;
        rows[pos] = j;
      }
      ++pos;
    }
    slot[j] = s;
  }
  for (int i = held + t; i < capacity; i += DS_THREADS) rows[i] = -1;
  if (t == 0) {
    count[0] = total;
    count[1] = held;
  }
}

__global__ __launch_bounds__(256) void decode_gather_kernel(const float4 *__restrict__ obj, const float4 *__restrict__ memory,
                                                            const int32_t *__restrict__ rows, long pieces, int d4,
                                                            float4 *__restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= pieces) return;
  const long r = i / d4;
  const int c = (int)(i - r * d4);
  const int src = rows[r];
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (src >= 0) {
    v = obj[(size_t)src * d4 + c];
    if (memory != nullptr) {
      const float4 m = memory[(size_t)src * d4 + c];
      v.x += m.x, v.y += m.y, v.z += m.z, v.w += m.w;
    }
  }
  out[i] = v;
}

// FILL_WORDS: the empty caption (fill at l % L == 0, zero elsewhere); otherwise the scalar fill everywhere
template <typename T, bool FILL_WORDS>
__global__ __launch_bounds__(256) void decode_scatter_kernel(const T *__restrict__ vals, const int32_t *__restrict__ slot, long total,
                                                             int inner, int L, T fill, T *__restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long j = i / inner;
  const int l = (int)(i - j * inner);
  const int s = slot[j];
  T v = fill;
  if (FILL_WORDS && l % L != 0) v = T(0);
  if (s >= 0) v = vals[(size_t)s * inner + l];
  out[i] = v;
}

template <typename T, bool FILL_WORDS>
int scatter(const char *what, const T *vals, const int32_t *slot, long n, int inner, int L, T fill, T *out, spacap_stream_t stream) {
  SPACAP_REQUIRE(n >= 0 && n <= DS_MAX_N && inner >= 1 && inner <= DS_MAX_INNER && L >= 1 && inner % L == 0,
                 "%s: bad sizes (n=%ld inner=%d L=%d; 0 <= n <= %ld, 1 <= inner <= %ld, inner a multiple of L >= 1)", what, n, inner, L,
                 DS_MAX_N, DS_MAX_INNER);
  if (n == 0) return SPACAP_OK;
  SPACAP_REQUIRE(vals && slot && out, "%s: null pointer", what);
  const long total = n * inner;
  hipLaunchKernelGGL((decode_scatter_kernel<T, FILL_WORDS>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     spacap::as_stream(stream), vals, slot, total, inner, L, fill, out);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

}  // namespace

extern "C" int spacap_decode_select_i32(const uint8_t *mask, long n, long capacity, int32_t *rows, int32_t *slot, int32_t *count,
                                        spacap_stream_t stream) {
  const char *what = "spacap_decode_select_i32";
  SPACAP_REQUIRE(n >= 0 && n <= DS_MAX_N, "%s: bad sizes (n=%ld; 0 <= n <= %ld)", what, n, DS_MAX_N);
  if (n == 0) return SPACAP_OK;
  SPACAP_REQUIRE(capacity >= 1 && capacity <= n, "%s: bad sizes (capacity=%ld; 1 <= capacity <= n = %ld)", what, capacity, n);
  SPACAP_REQUIRE(mask && rows && slot && count, "%s: null pointer", what);
  hipLaunchKernelGGL(decode_select_kernel, dim3(1), dim3(DS_THREADS), 0, spacap::as_stream(stream), mask, (int)n, (int)capacity, rows,
                     slot, count);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_decode_gather_f32(const float *obj, const float *memory, const int32_t *rows, long capacity, int d, float *out,
                                        spacap_stream_t stream) {
  const char *what = "spacap_decode_gather_f32";
  SPACAP_REQUIRE(capacity >= 0 && capacity <= DS_MAX_N && d >= 4 && d <= DS_MAX_INNER && d % 4 == 0,
                 "%s: bad sizes (capacity=%ld d=%d; 0 <= capacity <= %ld, d a multiple of 4 in 4..%ld)", what, capacity, d, DS_MAX_N,
                 DS_MAX_INNER);
  if (capacity == 0) return SPACAP_OK;
  SPACAP_REQUIRE(obj && rows && out, "%s: null pointer", what);
  SPACAP_REQUIRE(spacap::aligned16(obj, memory, out), "%s: obj, memory and out must be 16-byte aligned", what);
  const int d4 = d / 4;
  const long pieces = capacity * d4;
  hipLaunchKernelGGL(decode_gather_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, spacap::as_stream(stream),
                     reinterpret_cast<const float4 *>(obj), reinterpret_cast<const float4 *>(memory), rows, pieces, d4,
                     reinterpret_cast<float4 *>(out));
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_decode_scatter_i64(const int64_t *ys, const int32_t *slot, long n, int inner, int L, int64_t eos, int64_t *out,
                                         spacap_stream_t stream) {
  return scatter<int64_t, true>("spacap_decode_scatter_i64", ys, slot, n, inner, L, eos, out, stream);
}

extern "C" int spacap_decode_scatter_f32(const float *vals, const int32_t *slot, long n, int inner, float fill, float *out,
                                         spacap_stream_t stream) {
  return scatter<float, false>("spacap_decode_scatter_f32", vals, slot, n, inner, 1, fill, out, stream);
}

extern "C" int spacap_decode_scatter_i32(const int32_t *vals, const int32_t *slot, long n, int inner, int32_t fill, int32_t *out,
                                         spacap_stream_t stream) {
  return scatter<int32_t, false>("spacap_decode_scatter_i32", vals, slot, n, inner, 1, fill, out, stream);
}
