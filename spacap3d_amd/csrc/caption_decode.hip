// Caption decoding for gfx950 (MI355X), one token per row and step over pre-allocated key / value caches: the greedy decoder
// (models/transformer_captioner.py:402-453) and the beam search (the semantics are the project's own,
// restated by tests/beam_search_restated.py: each of R sequences keeps W <= 8 hypotheses).  The layers between two attention
// calls are the row / feed-forward kernels of tf_layer.hip; this unit holds what only decoding needs.  Per word:
//   decode_attn_kernel / decode_attn_beam_kernel : attention of the newest token over the caches; the beam one reads position
//       p < t of hypothesis (r, w) from cache slot (r, anc[r][w][p], p), so that the caches are never reordered
//   vocab_argmax_kernel + decode_next_kernel : greedy word = arg-max of the vocabulary projection, into the caption and the next input row
//   beam_topw_kernel<WB> + beam_topw_merge_kernel : the W best (log-probability, word) of each of the R W rows -- the greedy
//       kernel's workgroup shape and logit tile with a sorted top-W list and an online (max, sum exp) per lane
//   beam_step_kernel : one wave per sequence ranks the <= W W candidates by counting (score descending, then the smaller parent
//       beam, then the smaller word) and writes the W survivors: state, ancestor table, trace, next input rows
// and beam_finish_kernel backtracks the trace once at the end.  Sampled decoding (restated by
// tests/sampling_restated.py) draws a word per row and step by the Gumbel-max rule:
//   vocab_gumbel_kernel + sample_next_kernel : word = arg-max of logit / tau + Gumbel noise (the greedy kernel's workgroup shape
//       and logit tile; the noise is a hash of (row, step, word)), its log-probability from an online (max, sum exp), the row's
//       score / length / finished flag and the next input row; with top_k the candidates are beam_topw_kernel's k best
//   vocab_logits_kernel + nucleus_next_kernel : nucleus (top-p) sampling -- the same draw restricted to the words whose strictly
//       more probable words hold less than p of softmax(logit / tau); the set needs a whole row, so this mode alone writes
//       the logits to HBM (one image in the workspace) and a workgroup per row reads them back
// Otherwise no logits reach HBM; no step reads a value back on the host.  Constrained decoding (restated by
// tests/decode_constraints_restated.py) -- a minimum length, a no-repeat n-gram rule, bad words, a repetition penalty -- sits at
// the end of the device code:
//   decode_constraint_kernel : per step, a row's banned and seen words as two bit images over the vocabulary
//   vocab_argmax_constrained_kernel, beam_topw_constrained_kernel<WB>, vocab_gumbel_constrained_kernel : the word kernels with two
//       bit tests per logit; logits_constrain_kernel patches the nucleus mode's image
//
// The logit tile -- row split, weight staging, the same six piece products in the same order on the same two accumulators -- the
// first-maximum compare and the slicing of the vocabulary over workgroups are defined ONCE below: that is what makes a beam of
// width 1 choose the greedy decoder's words bit for bit.  The device pieces are MACROS, not functions: vocab_argmax_kernel must
// keep the instruction stream it was measured with, and hipcc allocates its registers differently (and emits another loop) as
// soon as one of these blocks goes through a __forceinline__ function with array-reference parameters -- even the three-term
// compare.  A macro hands the compiler the token stream the kernel had before; each names the kernel's variables as listed with it.
#include <math.h>

#include "common.hpp"
#include "dropout.hpp"
#include "launch.hpp"
#include "mfma.hpp"

namespace {

using namespace spacap;
using namespace spacap::mfma;

constexpr int VA_D = 128;                                       // d_model: the contraction length of a logit
constexpr int VA_CHUNK = 64, VA_LDB = VA_D + 8, VA_ROWS = 16;   // words per LDS chunk, LDS row stride (bf16), sequences per workgroup
constexpr int VA_IMGW = VA_CHUNK * VA_LDB;                      // one piece image of a chunk in LDS (bf16 elements)
constexpr int VA_STAGE_ELEMS = 3 * VA_CHUNK * VA_LDB;           // the staging buffer: three piece images (bf16 elements)

// vocabulary slices of a launch over R rows: ~4 workgroups per CU, whole chunks per slice
inline int va_slices(long R, int V) {
  const long tiles = (R + VA_ROWS - 1) / VA_ROWS;
  long ns = (4L * device_cus() + tiles - 1) / tiles;   // ~4 workgroups per CU
  const long most = (V + VA_CHUNK - 1) / VA_CHUNK;
  if (ns > most) ns = most;
  if (ns > 64) ns = 64;
  return (int)(ns < 1 ? 1 : ns);
}
inline int va_per_slice(int V, int ns) { return ((V + ns - 1) / ns + VA_CHUNK - 1) / VA_CHUNK * VA_CHUNK; }

constexpr int BEAM_MAX = 8;           // widest beam: W W candidates sit one per lane of a wave
constexpr int NO_WORD = 0x7fffffff;   // the word of an empty list entry (value -inf): behind every real entry

// (value, index) is ahead of (m, mi): the larger value, among equal values the SMALLER index (torch.max: first maximum)
#define SPACAP_FIRST_MAX(val, idx, m, mi) ((val) > (m) || ((val) == (m) && (idx) < (mi)))

// The sequences' rows as the A operand, split once: a[kc][piece] = pieces of x[row0 + l15][32 kc + 8 lg .. + 7].
// Declares `bf16x8 a[VA_D / 32][3]`; reads x (f32 [R][128]), row0, R, l15 = lane % 16, lg = lane / 16.
// (split8 of mfma.hpp, spelled out element by element: through the function the kernel's registers are allocated differently)
#define SPACAP_VA_SPLIT_ROWS()                                                           \
  bf16x8 a[VA_D / 32][3];                                                                \
  {                                                                                      \
    const float *xr = x + (size_t)min(row0 + l15, R - 1) * VA_D + 8 * lg;                \
    _Pragma("unroll") for (int kc = 0; kc < VA_D / 32; ++kc) {                           \
      const f32x4 lo = ld4(xr + 32 * kc), hi = ld4(xr + 32 * kc + 4);                    \
      _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                    \
        const float v = e < 4 ? lo[e] : hi[e - 4];                                       \
        const __bf16 h = (__bf16)v;                                                      \
        const float r1 = v - (float)h;                                                   \
        const __bf16 m = (__bf16)r1;                                                     \
        a[kc][0][e] = h, a[kc][1][e] = m, a[kc][2][e] = (__bf16)(r1 - (float)m);         \
      }                                                                                  \
    }                                                                                    \
  }

// Staging of the weight pieces Wp bf16 [3][V][128], one chunk of 64 words at a time: per piece 64 rows x 16 sixteen-byte pieces
// = 1 024 loads: 4 per thread and piece.  Declares c8, r0, wimg, `bf16x8 stg[3][4]` and the lambda fetch(v0) (chunk v0 .. v0 + 63
// into stg; rows behind V - 1 repeat the last row); reads tid (0..255), Wp, V.
#define SPACAP_VA_STAGING()                                                                                             \
  const int c8 = tid & 15, r0 = tid >> 4;                                                                               \
  const size_t wimg = (size_t)V * VA_D;                                                                                 \
  bf16x8 stg[3][4];                                                                                                     \
  auto fetch = [&](int v0) {                                                                                            \
    _Pragma("unroll") for (int p = 0; p < 3; ++p) _Pragma("unroll") for (int i = 0; i < 4; ++i) {                       \
      const int v = v0 + r0 + 16 * i;                                                                                   \
      stg[p][i] = *reinterpret_cast<const bf16x8 *>(Wp + p * wimg + (size_t)min(v, V - 1) * VA_D + 8 * c8);             \
    }                                                                                                                   \
  }
// stg -> the LDS staging buffer s_w (bf16 [VA_STAGE_ELEMS], 16-byte aligned); a barrier on both sides is the caller's
#define SPACAP_VA_STORE_STAGE()                               \
  _Pragma("unroll") for (int p = 0; p < 3; ++p) _Pragma("unroll") for (int i = 0; i < 4; ++i) \
      *reinterpret_cast<bf16x8 *>(s_w + p * VA_IMGW + (r0 + 16 * i) * VA_LDB + 8 * c8) = stg[p][i]

// The 16 x 16 logit tile of wave w: sequences row0 .. row0 + 15 against words 16 w .. 16 w + 15 of the staged chunk.  Declares
// the accumulators acc, acc2: the logit of sequence row0 + 4 lg + u and word 16 w + l15 of the chunk is (acc[u] + acc2[u]) + bias.
#define SPACAP_VA_TILE()                                                                                                       \
  f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};                                                               \
  _Pragma("unroll") for (int kc = 0; kc < VA_D / 32; ++kc) {                                                                   \
    bf16x8 b[3];                                                                                                               \
    _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                                              \
        b[p] = *reinterpret_cast<const bf16x8 *>(s_w + p * VA_IMGW + (16 * w + l15) * VA_LDB + 32 * kc + 8 * lg);              \
    _Pragma("unroll") for (int q = 0; q < 6; ++q) {                                                                            \
      if (kc & 1) acc2 = MFMA_B(a[kc][PA[q]], b[PB[q]], acc2);                                                                 \
      else acc = MFMA_B(a[kc][PA[q]], b[PB[q]], acc);                                                                          \
    }                                                                                                                          \
  }

// ---- attention of the newest token over the key / value caches ----------------------------------------------------------------
// One decoding step of self-attention (models/transformer_captioner.py:402-453: the reference re-runs the whole decoder prefix
// for every new word; with pre-norm layers and a causal mask the newest row of that recomputation equals this incremental
// step).  One workgroup per row: the new token's k, v (from its packed q|k|v row) are appended at position t of the row's cache
// slot [rows][T][h*16], thread (head, key) forms one logit, a 32-lane softmax per head, then thread (head, d) accumulates
// sum_key p[key] v[key][d] over coalesced 64-byte reads.  h = 8, d_k = 16, T <= 32.
//
// TWO kernels side by side: the beam one is the greedy one with one indirection (same thread roles, same arithmetic in the same
// order; bit-equal with anc[row][p] = w, tests/test_beam_search_gpu.py) -- change them together.  One `template <bool BEAM>
// __forceinline__` body behind two wrappers gave the beam kernel's instruction stream below but the greedy instance on 40 instead
// of 44 VGPRs (or one merged cache store), and a kernel here keeps the code object it was measured with (as the macros above).
__global__ __launch_bounds__(256) void decode_attn_kernel(const float *__restrict__ qkv, float *__restrict__ kc,
                                                          float *__restrict__ vc, int T, int t, float scale,
                                                          float *__restrict__ out) {
  constexpr int HD = 128;
  __shared__ float s_p[8][32];
  const int tid = threadIdx.x, hh = tid >> 5, tk = tid & 31;
  const size_t row = blockIdx.x;
  const float *me = qkv + row * 3 * HD;
  float *kr = kc + row * (size_t)T * HD, *vr = vc + row * (size_t)T * HD;
  if (tid < 32) st4(kr + (size_t)t * HD + tid * 4, ld4(me + HD + tid * 4));
  else if (tid < 64) st4(vr + (size_t)t * HD + (tid - 32) * 4, ld4(me + 2 * HD + (tid - 32) * 4));
  float logit = -INFINITY;
  if (tk <= t) {
    const float *kp = tk == t ? me + HD + hh * 16 : kr + (size_t)tk * HD + hh * 16;   // (position t: straight from the row)
    float a = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 kv = ld4(kp + 4 * q), qv = ld4(me + hh * 16 + 4 * q);
      a += qv[0] * kv[0] + qv[1] * kv[1] + qv[2] * kv[2] + qv[3] * kv[3];
    }
    logit = a * scale;
  }
  const float mx = wave_max<32>(logit);   // a head's 32 key lanes
  const float e = tk <= t ? __expf(logit - mx) : 0.f;
  s_p[hh][tk] = e / wave_sum<32>(e);
  __syncthreads();
  // thread (head, half, d): keys of its parity
  const int d = tk & 15, par = tk >> 4;
  float acc = 0.f;
  for (int k2 = par; k2 <= t; k2 += 2) {
    const float v = k2 == t ? me[2 * HD + hh * 16 + d] : vr[(size_t)k2 * HD + hh * 16 + d];
    acc += s_p[hh][k2] * v;
  }
  acc += __shfl_xor(acc, 16);
  if (par == 0) out[row * HD + hh * 16 + d] = acc;
}

// The same for row = r W + w of a beam: the new k, v go to the row's own cache slot at position t; position p < t is read from
// slot r W + anc[row][p].  An entry outside 0..W-1 reads the row's own slot (never out of bounds).
__global__ __launch_bounds__(256) void decode_attn_beam_kernel(const float *__restrict__ qkv, float *__restrict__ kc, float *__restrict__ vc,
                                                               const signed char *__restrict__ anc, int W, int T, int t, float scale,
                                                               float *__restrict__ out) {
  constexpr int HD = 128;
  __shared__ float s_p[8][32];
  __shared__ int s_slot[32];
  const int tid = threadIdx.x, hh = tid >> 5, tk = tid & 31;
  const size_t row = blockIdx.x;
  const int w = (int)(row % (size_t)W);
  const size_t seq0 = row - w;                        // the sequence's first cache slot
  const float *me = qkv + row * 3 * HD;
  float *kr = kc + row * (size_t)T * HD, *vr = vc + row * (size_t)T * HD;
  if (tid < 32) st4(kr + (size_t)t * HD + tid * 4, ld4(me + HD + tid * 4));
  else if (tid < 64) st4(vr + (size_t)t * HD + (tid - 32) * 4, ld4(me + 2 * HD + (tid - 32) * 4));
  int slot = w;
  if (tk < t) {
    const int s = anc[row * (size_t)T + tk];
    slot = (unsigned)s < (unsigned)W ? s : w;
  }
  if (tid < 32) s_slot[tid] = slot;
  float logit = -INFINITY;
  if (tk <= t) {
    const float *kp = tk == t ? me + HD + hh * 16 : kc + ((seq0 + slot) * (size_t)T + tk) * HD + hh * 16;
    float a = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 kv = ld4(kp + 4 * q), qv = ld4(me + hh * 16 + 4 * q);
      a += qv[0] * kv[0] + qv[1] * kv[1] + qv[2] * kv[2] + qv[3] * kv[3];
    }
    logit = a * scale;
  }
  const float mx = wave_max<32>(logit);   // a head's 32 key lanes
  const float e = tk <= t ? __expf(logit - mx) : 0.f;
  s_p[hh][tk] = e / wave_sum<32>(e);
  __syncthreads();
  const int d = tk & 15, par = tk >> 4;
  float acc = 0.f;
  for (int k2 = par; k2 <= t; k2 += 2) {
    const float v = k2 == t ? me[2 * HD + hh * 16 + d] : vc[((seq0 + s_slot[k2]) * (size_t)T + k2) * HD + hh * 16 + d];
    acc += s_p[hh][k2] * v;
  }
  acc += __shfl_xor(acc, 16);
  if (par == 0) out[row * HD + hh * 16 + d] = acc;
}

// ---- greedy decoding: vocabulary projection + arg-max without the logits, and the next token's embedding ---------------------
// (models/transformer_captioner.py:93-100 Generator: log_softmax(proj(x)) and :441-447: `_, next_word = torch.max(prob, dim=1)`;
// the arg-max of the log-softmax is the arg-max of the logits.)  Round 4 ran F.linear on 2 048 x 3 001 logits + torch.argmax for
// each of the 31 words.  Here a workgroup owns 16 sequences and one slice of the vocabulary: the slice's weight rows go through
// LDS 64 at a time (next chunk's loads in flight), logits come out of v_mfma_f32_16x16x4_f32 (exact fp32 products) 16 words per
// wave, and every lane keeps the running (best logit, first index) of its rows; the slices' winners [R][NS] are merged by
// decode_next_kernel, which also writes the word into the caption and forms the next input row lut[word] sqrt(d) + pe[t].
// Arithmetic: split-bf16 (three bf16 pieces per operand, the six piece products above 2^-24 on v_mfma_f32_16x16x32_bf16:
// fp32-equivalent logits at 6/16 of the fp32-MFMA time -- 1.6 GFLOP per word on the fp32 pipe alone is 10 us).  The weight's
// pieces Wp bf16 [3][V][128] are made once per decoding call (spacap_gemm_bf3_split_w_f32).
// (the logit tile -- row split, weight staging, the six piece products -- and the compare are the macros above: shared with beam_topw_kernel)
__global__ __launch_bounds__(256) void vocab_argmax_kernel(const float *__restrict__ x, const __bf16 *__restrict__ Wp, const float *__restrict__ bias,
                                                           long R, int V, int per_slice, float *__restrict__ best_v, int *__restrict__ best_i) {
  __shared__ __attribute__((aligned(16))) __bf16 s_w[VA_STAGE_ELEMS];
  __shared__ float s_bv[4][VA_ROWS][17];
  __shared__ int s_bi[4][VA_ROWS][17];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const long row0 = (long)blockIdx.x * VA_ROWS;
  const int ns = gridDim.y, sl = blockIdx.y;
  const int v_beg = sl * per_slice, v_end = min(V, v_beg + per_slice);
  SPACAP_VA_SPLIT_ROWS();   // bf16x8 a[kc][piece]: the sequences' rows as the A operand, split once
  float bv[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int bi[4] = {v_beg, v_beg, v_beg, v_beg};
  SPACAP_VA_STAGING();      // stg, fetch(v0): the next chunk of the weight pieces in registers
  fetch(v_beg < V ? v_beg : 0);
  for (int v0 = v_beg; v0 < v_end; v0 += VA_CHUNK) {
    __syncthreads();
    SPACAP_VA_STORE_STAGE();
    __syncthreads();
    if (v0 + VA_CHUNK < v_end) fetch(v0 + VA_CHUNK);
    const int v = v0 + 16 * w + l15;                    // this lane's word of the chunk
    SPACAP_VA_TILE();                                   // acc, acc2: the 16 x 16 logits of this wave's words
    if (v < v_end) {
      const float bsv = bias[v];
#pragma unroll
      for (int u = 0; u < 4; ++u) {      // logit of sequence row0 + 4 lg + u, word v; words arrive in increasing order
        const float val = (acc[u] + acc2[u]) + bsv;
        if (val > bv[u]) bv[u] = val, bi[u] = v;
      }
    }
  }
  // merge across the 16 lanes and the 4 waves; ties go to the smaller word index (torch.max: first maximum)
#pragma unroll
  for (int u = 0; u < 4; ++u) s_bv[w][4 * lg + u][l15] = bv[u], s_bi[w][4 * lg + u][l15] = bi[u];
  __syncthreads();
  if (tid < 64) {
    const int row = tid >> 2, ww = tid & 3;          // four threads per sequence, one wave's 16 candidates each
    float m = -INFINITY;
    int mi = 0x7fffffff;
#pragma unroll
    for (int l = 0; l < 16; ++l) {
      const float val = s_bv[ww][row][l];
      const int idx = s_bi[ww][row][l];
      if (SPACAP_FIRST_MAX(val, idx, m, mi)) m = val, mi = idx;
    }
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
      const float om = __shfl_xor(m, o);
      const int oi = __shfl_xor(mi, o);
      if (SPACAP_FIRST_MAX(om, oi, m, mi)) m = om, mi = oi;
    }
    if (ww == 0 && row0 + row < R) {
      best_v[(size_t)(row0 + row) * ns + sl] = m;
      best_i[(size_t)(row0 + row) * ns + sl] = mi;
    }
  }
}

// word[r] = the best of the NS slice winners (first maximum); ys[r][t_out] = word; x[r, :] = lut[word] * scale + pe_row
__global__ __launch_bounds__(256) void decode_next_kernel(const float *__restrict__ best_v, const int *__restrict__ best_i, int ns, long R,
                                                          const float *__restrict__ lut, float scale, const float *__restrict__ pe_row,
                                                          long long *__restrict__ ys, int ys_ld, int t_out, float *__restrict__ x) {
  const long r = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
  const int c4 = threadIdx.x & 31;
  if (r >= R) return;
  float m = -INFINITY;
  int mi = 0x7fffffff;
  for (int s = 0; s < ns; ++s) {
    const float val = best_v[(size_t)r * ns + s];
    const int idx = best_i[(size_t)r * ns + s];
    if (SPACAP_FIRST_MAX(val, idx, m, mi)) m = val, mi = idx;
  }
  if (c4 == 0) ys[(size_t)r * ys_ld + t_out] = mi;
  const f32x4 e = ld4(lut + (size_t)mi * VA_D + 4 * c4), p = ld4(pe_row + 4 * c4);
  st4(x + (size_t)r * VA_D + 4 * c4, f32x4{e[0] * scale + p[0], e[1] * scale + p[1], e[2] * scale + p[2], e[3] * scale + p[3]});
}

// ---- the W best words of every row -----------------------------------------------------------------------------------------
// Grid (rows / 16, vocabulary slices), 256 threads: as vocab_argmax_kernel.  Lane (l15, lg) of wave w sees, per chunk of 64
// words, the logits of sequences row0 + 4 lg + u (u < 4) for word 16 w + l15: its words arrive in increasing order, so its
// list stays sorted by (logit descending, word ascending) under a plain insertion, which is entered only when the logit beats
// the list's last entry.  WB = compile-time list length (>= W).  After the last chunk the staging buffer is dead and the
// merge aliases it: LDS stays at the 51 KB of the staging buffer (room for three workgroups per CU; the 174 / 206 VGPRs of the
// two instantiations make it two, as many as vocab_argmax_kernel's 60 KB of LDS allow it).
template <int WB>
__global__ __launch_bounds__(256) void beam_topw_kernel(const float *__restrict__ x, const __bf16 *__restrict__ Wp, const float *__restrict__ bias,
                                                        long R, int V, int per_slice, int W, float *__restrict__ part_v,
                                                        int *__restrict__ part_i, float *__restrict__ part_ms) {
  __shared__ __attribute__((aligned(16))) __bf16 s_w[VA_STAGE_ELEMS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const long row0 = (long)blockIdx.x * VA_ROWS;
  const int ns = gridDim.y, sl = blockIdx.y;
  const int v_beg = sl * per_slice, v_end = min(V, v_beg + per_slice);
  SPACAP_VA_SPLIT_ROWS();   // bf16x8 a[kc][piece]
  float tv[4][WB], mx[4], sm[4];
  int ti[4][WB];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    mx[u] = -INFINITY, sm[u] = 0.f;
#pragma unroll
    for (int k = 0; k < WB; ++k) tv[u][k] = -INFINITY, ti[u][k] = NO_WORD;
  }
  SPACAP_VA_STAGING();      // stg, fetch(v0)
  fetch(v_beg < V ? v_beg : 0);
  for (int v0 = v_beg; v0 < v_end; v0 += VA_CHUNK) {
    __syncthreads();
    SPACAP_VA_STORE_STAGE();
    __syncthreads();
    if (v0 + VA_CHUNK < v_end) fetch(v0 + VA_CHUNK);
    const int v = v0 + 16 * w + l15;                    // this lane's word of the chunk
    SPACAP_VA_TILE();                                   // acc, acc2
    if (v < v_end) {
      const float bsv = bias[v];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float val = (acc[u] + acc2[u]) + bsv;     // (the greedy kernel's logit, bit for bit)
        if (val > mx[u]) sm[u] = sm[u] * expf(mx[u] - val) + 1.f, mx[u] = val;
        else sm[u] += expf(val - mx[u]);
        if (val > tv[u][WB - 1]) {
          float cv = val;
          int ci = v;
#pragma unroll
          for (int k = 0; k < WB; ++k)
            if (SPACAP_FIRST_MAX(cv, ci, tv[u][k], ti[u][k])) {
              const float ov = tv[u][k];
              const int oi = ti[u][k];
              tv[u][k] = cv, ti[u][k] = ci, cv = ov, ci = oi;
            }
        }
      }
    }
  }
  __syncthreads();   // every wave is done with the last chunk: the staging buffer becomes the merge area
  float *s_mv = reinterpret_cast<float *>(s_w);               // [4 waves][16 rows][WB]
  int *s_mi = reinterpret_cast<int *>(s_mv + 4 * VA_ROWS * WB);
  float *s_ms = reinterpret_cast<float *>(s_mi + 4 * VA_ROWS * WB);   // [4][16][2]
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int row = 4 * lg + u;
    // the 16 lanes that hold this sequence's words: (max, sum exp), then W rounds of "best head, its owner pops"
    float M = mx[u];
#pragma unroll
    for (int o = 1; o <= 8; o <<= 1) M = fmaxf(M, __shfl_xor(M, o));
    float S = mx[u] == -INFINITY ? 0.f : sm[u] * expf(mx[u] - M);
#pragma unroll
    for (int o = 1; o <= 8; o <<= 1) S += __shfl_xor(S, o);
    if (l15 == 0) s_ms[(w * VA_ROWS + row) * 2] = M, s_ms[(w * VA_ROWS + row) * 2 + 1] = S;
#pragma unroll
    for (int k = 0; k < WB; ++k) {
      if (k >= W) break;
      float bvv = tv[u][0];
      int bii = ti[u][0];
#pragma unroll
      for (int o = 1; o <= 8; o <<= 1) {
        const float ov = __shfl_xor(bvv, o);
        const int oi = __shfl_xor(bii, o);
        if (SPACAP_FIRST_MAX(ov, oi, bvv, bii)) bvv = ov, bii = oi;
      }
      if (ti[u][0] == bii) {   // (a word sits in one lane only; empty heads all pop, which changes nothing)
#pragma unroll
        for (int q = 0; q + 1 < WB; ++q) tv[u][q] = tv[u][q + 1], ti[u][q] = ti[u][q + 1];
        tv[u][WB - 1] = -INFINITY, ti[u][WB - 1] = NO_WORD;
      }
      if (l15 == 0) s_mv[(w * VA_ROWS + row) * WB + k] = bvv, s_mi[(w * VA_ROWS + row) * WB + k] = bii;
    }
  }
  __syncthreads();
  if (tid < VA_ROWS && row0 + tid < R) {   // one thread per sequence: the four waves' sorted lists, merged
    const int row = tid;
    const size_t o = ((size_t)(row0 + row) * ns + sl);
    int hd[4] = {0, 0, 0, 0};
    for (int k = 0; k < W; ++k) {
      float bvv = -INFINITY;
      int bii = NO_WORD, bw = 0;
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) {
        const bool has = hd[ww] < W;
        const float cv = has ? s_mv[(ww * VA_ROWS + row) * WB + hd[ww]] : -INFINITY;
        const int ci = has ? s_mi[(ww * VA_ROWS + row) * WB + hd[ww]] : NO_WORD;
        if (SPACAP_FIRST_MAX(cv, ci, bvv, bii)) bvv = cv, bii = ci, bw = ww;
      }
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) hd[ww] += ww == bw ? 1 : 0;
      part_v[o * W + k] = bvv, part_i[o * W + k] = bii;
    }
    float M = -INFINITY, S = 0.f;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) M = fmaxf(M, s_ms[(ww * VA_ROWS + row) * 2]);
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
      const float m = s_ms[(ww * VA_ROWS + row) * 2];
      S += m == -INFINITY ? 0.f : s_ms[(ww * VA_ROWS + row) * 2 + 1] * expf(m - M);
    }
    part_ms[o * 2] = M, part_ms[o * 2 + 1] = S;
  }
}

// One thread per row: the slices' lists [rows][ns][W] and (max, sum exp) pairs -> the row's W (log-probability, word) pairs,
// log-probability descending, equal ones the smaller word first.  Round k takes the best entry behind round k - 1's: no heads
// to keep, and ns W entries are a few hundred at most.
__global__ __launch_bounds__(256) void beam_topw_merge_kernel(const float *__restrict__ part_v, const int *__restrict__ part_i,
                                                              const float *__restrict__ part_ms, int ns, long rows, int W,
                                                              float *__restrict__ top_logp, int *__restrict__ top_word) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  float M = -INFINITY, S = 0.f;
  for (int s = 0; s < ns; ++s) M = fmaxf(M, part_ms[((size_t)r * ns + s) * 2]);
  for (int s = 0; s < ns; ++s) {
    const float m = part_ms[((size_t)r * ns + s) * 2];
    S += m == -INFINITY ? 0.f : part_ms[((size_t)r * ns + s) * 2 + 1] * expf(m - M);
  }
  const float log_s = logf(S);   // lse = M + log S; logp = (logit - M) - log S keeps the small difference exact
  const float *pv = part_v + (size_t)r * ns * W;
  const int *pi = part_i + (size_t)r * ns * W;
  float lv = INFINITY;   // the previous round's entry: ahead of everything at first
  int li = -1;
  for (int k = 0; k < W; ++k) {
    float bvv = -INFINITY;
    int bii = NO_WORD;
    for (int e = 0; e < ns * W; ++e) {
      const float cv = pv[e];
      const int ci = pi[e];
      if (SPACAP_FIRST_MAX(lv, li, cv, ci) && SPACAP_FIRST_MAX(cv, ci, bvv, bii)) bvv = cv, bii = ci;
    }
    top_logp[(size_t)r * W + k] = (bvv - M) - log_s, top_word[(size_t)r * W + k] = bii;
    lv = bvv, li = bii;
  }
}

// ---- one selection ---------------------------------------------------------------------------------------------------------
// One wave per sequence, lane c = j W + i: candidate i of hypothesis j.  A dead hypothesis (score -inf) offers nothing, a
// finished one its own (score, eos) once, a live one score + logp of its i-th best word.  Rank = the number of candidates
// ahead: score descending, then the smaller j, then the smaller word.  Survivor w (rank w) becomes hypothesis w.
// State is read from *_in and written to *_out, the ancestor table from anc_old to anc_new: nothing is updated in place.
__global__ __launch_bounds__(256) void beam_step_kernel(const float *__restrict__ top_logp, const int *__restrict__ top_word, long R, int W, int V,
                                                        int T, int t, int eos, const float *__restrict__ score_in,
                                                        const int *__restrict__ fin_in, const int *__restrict__ len_in,
                                                        float *__restrict__ score_out, int *__restrict__ fin_out, int *__restrict__ len_out,
                                                        const signed char *__restrict__ anc_old, signed char *__restrict__ anc_new,
                                                        signed char *__restrict__ tr_parent, int *__restrict__ tr_word,
                                                        const float *__restrict__ lut, float scale, const float *__restrict__ pe_row,
                                                        float *__restrict__ x_next) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;   // (wave-uniform)
  const int j = lane / W, i = lane - j * W;
  const bool in = lane < W * W;
  const size_t hj = (size_t)r * W + (in ? j : 0);
  const float sj = in ? score_in[hj] : -INFINITY;
  const int fj = in ? fin_in[hj] : 0, lj = in ? len_in[hj] : 0;
  const bool valid = in && sj != -INFINITY && (fj == 0 || i == 0);
  float cs = -INFINITY;
  int cw = eos;
  if (valid) {
    if (fj) cs = sj;
    else cs = sj + top_logp[hj * W + i], cw = top_word[hj * W + i];
  }
  int rank = 0;
  for (int c = 0; c < W * W; ++c) {
    const float os = __shfl(cs, c);
    const int ow = __shfl(cw, c), ov = __shfl((int)valid, c), oj = c / W;
    rank += (ov && (os > cs || (os == cs && (oj < j || (oj == j && ow < cw))))) ? 1 : 0;
  }
  if (!valid) rank = 64;
  const size_t step = (size_t)(t - 1);
  for (int w = 0; w < W; ++w) {
    const unsigned long long hit = __ballot(rank == w);
    const int src = hit ? __ffsll((long long)hit) - 1 : 0;   // (V >= W: there always is one; otherwise a dead hypothesis)
    const int parent = hit ? __shfl(j, src) : 0, word = hit ? __shfl(cw, src) : eos;
    const float ns_ = hit ? __shfl(cs, src) : -INFINITY;
    const int pf = hit ? __shfl(fj, src) : 1, pl = hit ? __shfl(lj, src) : 0;
    const size_t hw = (size_t)r * W + w;
    if (lane == 0) {
      score_out[hw] = ns_;
      fin_out[hw] = (pf || word == eos) ? 1 : 0;
      len_out[hw] = pl + (pf ? 0 : 1);
      tr_parent[(step * R + r) * W + w] = (signed char)parent;
      tr_word[(step * R + r) * W + w] = word;
    }
    if (lane < T) {
      const signed char av = lane < t ? anc_old[((size_t)r * W + parent) * T + lane] : (signed char)(lane == t ? parent : w);
      anc_new[hw * T + lane] = av;
    }
    if (x_next != nullptr && lane < 32) {   // the next input row, as decode_next_kernel forms it
      const int wd = min(max(word, 0), V - 1);
      const f32x4 e = ld4(lut + (size_t)wd * VA_D + 4 * lane), p = ld4(pe_row + 4 * lane);
      st4(x_next + hw * VA_D + 4 * lane, f32x4{e[0] * scale + p[0], e[1] * scale + p[1], e[2] * scale + p[2], e[3] * scale + p[3]});
    }
  }
}

// ---- the end: winner and backtracking -----------------------------------------------------------------------------------------
// One thread per hypothesis.  The winner of a sequence maximises score / length^alpha (alpha = 0: the score), the smaller slot
// on ties; its tokens go to ys, its score to best_score.  With all_tokens every hypothesis writes its own tokens, score, length.
__global__ __launch_bounds__(256) void beam_finish_kernel(const float *__restrict__ score, const int *__restrict__ len,
                                                          const signed char *__restrict__ tr_parent, const int *__restrict__ tr_word, long R, int W,
                                                          int n_words, double alpha, long long *__restrict__ ys, float *__restrict__ best_score,
                                                          long long *__restrict__ all_tokens, float *__restrict__ all_scores, int *__restrict__ all_len) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= R * W) return;
  const long r = idx / W;
  const int w = (int)(idx - r * W);
  int best = 0;
  double bn = 0.0;
  for (int k = 0; k < W; ++k) {
    const double s = (double)score[r * W + k];
    const int l = len[r * W + k];
    const double n = alpha == 0.0 ? s : s / pow((double)(l > 1 ? l : 1), alpha);
    if (k == 0 || n > bn) best = k, bn = n;
  }
  const bool win = w == best;
  if (all_tokens != nullptr) all_scores[idx] = score[idx], all_len[idx] = len[idx];
  if (win) best_score[r] = score[idx];
  if (!win && all_tokens == nullptr) return;
  int slot = w;
  for (int s = n_words - 1; s >= 0; --s) {
    const size_t e = ((size_t)s * R + r) * W + slot;
    const long long tok = tr_word[e];
    if (all_tokens != nullptr) all_tokens[(size_t)idx * n_words + s] = tok;
    if (win) ys[(size_t)r * n_words + s] = tok;
    const int p = tr_parent[e];
    slot = (unsigned)p < (unsigned)W ? p : slot;
  }
}

// ---- sampled decoding: a word drawn per row and step ---------------------------------------------------------------------------
// row rho draws word i as arg-max_v z_v, z_v = logit_v * (1 / tau) + g_v with Gumbel noise
// g_v = -log(-log u), u = ((hash >> 9) + 0.5) 2^-23 in [2^-24, 1 - 2^-24] (exact in fp32), hash = the keep mask's hash32
// (dropout.hpp) of the flat index (rho n_words + i) V + v: the arg-max is distributed as softmax(logit / tau).  Full-precision
// logf: tests/sampling_restated.py restates g in numpy float32.
__device__ __forceinline__ float gumbel_noise(unsigned long long idx, DropSeed sd) {
  const float u = ((float)(hash32(idx, sd) >> 9) + 0.5f) * 1.1920928955078125e-07f;   // 2^-23
  return -logf(-logf(u));
}

// vocab_argmax_kernel's grid, row split, staging and logit tile (the macros above).  Per lane and row: the running best
// (z, word) under the first-maximum compare -- the lane's words arrive in increasing order --, the raw logit of that best, and
// the online (max, sum exp) of the raw logits, as beam_topw_kernel keeps it.  After the last chunk the staging buffer is dead
// and the merge aliases it (LDS stays at its 51 KB).  Per row and slice one partial (z, word, logit, max, sum); an empty slice
// writes (-inf, NO_WORD, -inf, -inf, 0).  Words behind V - 1 (the staging repeats the last row) never pass `v < v_end`.
__global__ __launch_bounds__(256) void vocab_gumbel_kernel(const float *__restrict__ x, const __bf16 *__restrict__ Wp, const float *__restrict__ bias,
                                                           long R, int V, int per_slice, float inv_tau, unsigned long long seed,
                                                           const unsigned long long *__restrict__ seed_dev, int n_words, int step,
                                                           float *__restrict__ part_z, int *__restrict__ part_w, float *__restrict__ part_l,
                                                           float *__restrict__ part_ms) {
  __shared__ __attribute__((aligned(16))) __bf16 s_w[VA_STAGE_ELEMS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const long row0 = (long)blockIdx.x * VA_ROWS;
  const int ns = gridDim.y, sl = blockIdx.y;
  const int v_beg = sl * per_slice, v_end = min(V, v_beg + per_slice);
  const DropSeed sd = make_seed(seed, seed_dev);
  SPACAP_VA_SPLIT_ROWS();   // bf16x8 a[kc][piece]
  float bz[4], bl[4], mx[4], sm[4];
  int bi[4];
  unsigned long long nbase[4];   // the noise index of word 0 of row row0 + 4 lg + u at this step
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    bz[u] = -INFINITY, bl[u] = -INFINITY, bi[u] = NO_WORD, mx[u] = -INFINITY, sm[u] = 0.f;
    nbase[u] = ((unsigned long long)(row0 + 4 * lg + u) * (unsigned long long)n_words + (unsigned long long)step) * (unsigned long long)V;
  }
  SPACAP_VA_STAGING();      // stg, fetch(v0)
  fetch(v_beg < V ? v_beg : 0);
  for (int v0 = v_beg; v0 < v_end; v0 += VA_CHUNK) {
    __syncthreads();
    SPACAP_VA_STORE_STAGE();
    __syncthreads();
    if (v0 + VA_CHUNK < v_end) fetch(v0 + VA_CHUNK);
    const int v = v0 + 16 * w + l15;                    // this lane's word of the chunk
    SPACAP_VA_TILE();                                   // acc, acc2
    if (v < v_end) {
      const float bsv = bias[v];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float val = (acc[u] + acc2[u]) + bsv;     // (the greedy kernel's logit, bit for bit)
        if (val > mx[u]) sm[u] = sm[u] * expf(mx[u] - val) + 1.f, mx[u] = val;
        else sm[u] += expf(val - mx[u]);
        const float z = val * inv_tau + gumbel_noise(nbase[u] + (unsigned long long)v, sd);
        if (z > bz[u]) bz[u] = z, bi[u] = v, bl[u] = val;
      }
    }
  }
  __syncthreads();   // every wave is done with the last chunk: the staging buffer becomes the merge area
  constexpr int MA = 4 * VA_ROWS * 17;                        // [4 waves][16 rows][16 lanes + 1]
  float *s_z = reinterpret_cast<float *>(s_w);
  int *s_i = reinterpret_cast<int *>(s_z + MA);
  float *s_l = reinterpret_cast<float *>(s_i + MA), *s_m = s_l + MA, *s_s = s_m + MA;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int o = (w * VA_ROWS + 4 * lg + u) * 17 + l15;
    s_z[o] = bz[u], s_i[o] = bi[u], s_l[o] = bl[u], s_m[o] = mx[u], s_s[o] = sm[u];
  }
  __syncthreads();
  if (tid < 64) {
    const int row = tid >> 2, ww = tid & 3;          // four threads per sequence, one wave's 16 lanes each
    const int o = (ww * VA_ROWS + row) * 17;
    float m = -INFINITY, ml = -INFINITY, M = -INFINITY, S = 0.f;
    int mi = NO_WORD;
#pragma unroll
    for (int l = 0; l < 16; ++l) {
      const float val = s_z[o + l];
      const int idx = s_i[o + l];
      if (SPACAP_FIRST_MAX(val, idx, m, mi)) m = val, mi = idx, ml = s_l[o + l];
      M = fmaxf(M, s_m[o + l]);
    }
#pragma unroll
    for (int l = 0; l < 16; ++l) {
      const float lm = s_m[o + l];
      S += lm == -INFINITY ? 0.f : s_s[o + l] * expf(lm - M);
    }
#pragma unroll
    for (int q = 1; q <= 2; q <<= 1) {
      const float om = __shfl_xor(m, q), ol = __shfl_xor(ml, q), oM = __shfl_xor(M, q), oS = __shfl_xor(S, q);
      const int oi = __shfl_xor(mi, q);
      if (SPACAP_FIRST_MAX(om, oi, m, mi)) m = om, mi = oi, ml = ol;
      const float nM = fmaxf(M, oM);
      S = (M == -INFINITY ? 0.f : S * expf(M - nM)) + (oM == -INFINITY ? 0.f : oS * expf(oM - nM));
      M = nM;
    }
    if (ww == 0 && row0 + row < R) {
      const size_t e = (size_t)(row0 + row) * ns + sl;
      part_z[e] = m, part_w[e] = mi, part_l[e] = ml, part_ms[2 * e] = M, part_ms[2 * e + 1] = S;
    }
  }
}

// One row per 32 lanes, as decode_next_kernel.  top_k = 0: the slices' partials merged (first maximum of z; logp = (logit - M) -
// log S).  top_k >= 1: the candidates are the row's k entries of top_logp / top_word (spacap_beam_topw_f32), perturbed by the
// noise of their WORD: z = logp * (1 / tau) + g -- the log-probabilities are the logits minus one constant per row.  A finished
// row writes eos and keeps score and length; another adds logp to its score, sets length = step + 1 and becomes finished when
// it drew eos.  A row reads and writes its own state only.  xw[row] = lut[word] * scale + pe_row.
__global__ __launch_bounds__(256) void sample_next_kernel(const float *__restrict__ part_z, const int *__restrict__ part_w,
                                                          const float *__restrict__ part_l, const float *__restrict__ part_ms, int ns,
                                                          const float *__restrict__ top_logp, const int *__restrict__ top_word, int top_k,
                                                          float inv_tau, unsigned long long seed, const unsigned long long *__restrict__ seed_dev,
                                                          long R, int V, int n_words, int step, int eos, const float *__restrict__ lut,
                                                          float scale, const float *__restrict__ pe_row, long long *__restrict__ ys,
                                                          float *score, int *length, int *fin, float *__restrict__ xw) {
  const long r = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
  const int c4 = threadIdx.x & 31;
  if (r >= R) return;
  float m = -INFINITY, logp = 0.f;
  int mi = NO_WORD;
  if (top_k == 0) {
    float ml = -INFINITY, M = -INFINITY, S = 0.f;
    for (int s = 0; s < ns; ++s) {
      const size_t e = (size_t)r * ns + s;
      const float val = part_z[e];
      const int idx = part_w[e];
      if (SPACAP_FIRST_MAX(val, idx, m, mi)) m = val, mi = idx, ml = part_l[e];
      M = fmaxf(M, part_ms[2 * e]);
    }
    for (int s = 0; s < ns; ++s) {
      const float pm = part_ms[2 * ((size_t)r * ns + s)];
      S += pm == -INFINITY ? 0.f : part_ms[2 * ((size_t)r * ns + s) + 1] * expf(pm - M);
    }
    logp = (ml - M) - logf(S);
  } else {
    const DropSeed sd = make_seed(seed, seed_dev);
    const unsigned long long nbase = ((unsigned long long)r * (unsigned long long)n_words + (unsigned long long)step) * (unsigned long long)V;
    for (int k = 0; k < top_k; ++k) {
      const float lp = top_logp[(size_t)r * top_k + k];
      const int idx = top_word[(size_t)r * top_k + k];
      const float val = lp * inv_tau + gumbel_noise(nbase + (unsigned long long)idx, sd);
      if (SPACAP_FIRST_MAX(val, idx, m, mi)) m = val, mi = idx, logp = lp;
    }
  }
  const int f = fin[r];
  const int word = f ? eos : min(max(mi, 0), V - 1);
  if (c4 == 0) {
    ys[(size_t)r * n_words + step] = word;
    if (!f) {
      score[r] += logp;
      length[r] = step + 1;
      if (word == eos) fin[r] = 1;
    }
  }
  const f32x4 e = ld4(lut + (size_t)word * VA_D + 4 * c4), p = ld4(pe_row + 4 * c4);
  st4(xw + (size_t)r * VA_D + 4 * c4, f32x4{e[0] * scale + p[0], e[1] * scale + p[1], e[2] * scale + p[2], e[3] * scale + p[3]});
}

// ---- nucleus (top-p) sampling: the draw restricted to the words whose more probable words hold less than p ---------------------
// DESIGN.md section 7i, "Top-p", restated by tests/nucleus_restated.py: q = softmax(l / tau), A_v = the mass of the words with
// l_u > l_v, nucleus = { v : A_v < p }; the row draws the first maximum of z over the nucleus, z and its noise as above.  The
// set needs the whole row at once, so this mode alone writes the logits to HBM: vocab_logits_kernel stores the image
// f32 [rows][ld], ld = V rounded up to whole chunks, and nucleus_next_kernel reads each row back once.
constexpr int NUC_MAX_V = 16384;      // a row's (key, q) pairs sit in LDS: 8 bytes a word, 128 KB
inline int nuc_ld(int V) { return (V + VA_CHUNK - 1) / VA_CHUNK * VA_CHUNK; }

// vocab_argmax_kernel's grid, row split, staging and logit tile (the macros above).  The 16 x 64 logits of a chunk go through
// LDS so that a row's 64 words leave as 16 sixteen-byte stores of one 256-byte run: ld is a multiple of 64 floats, every run is
// whole lines.  Words V .. ld - 1 of the last chunk are written too (the repeated last weight row, no bias) and never read.
__global__ __launch_bounds__(256) void vocab_logits_kernel(const float *__restrict__ x, const __bf16 *__restrict__ Wp, const float *__restrict__ bias,
                                                           long R, int V, int per_slice, int ld, float *__restrict__ img) {
  __shared__ __attribute__((aligned(16))) __bf16 s_w[VA_STAGE_ELEMS];
  __shared__ __attribute__((aligned(16))) float s_o[VA_ROWS][VA_CHUNK + 4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const long row0 = (long)blockIdx.x * VA_ROWS;
  const int sl = blockIdx.y;
  const int v_beg = sl * per_slice, v_end = min(V, v_beg + per_slice);
  SPACAP_VA_SPLIT_ROWS();   // bf16x8 a[kc][piece]
  SPACAP_VA_STAGING();      // stg, fetch(v0)
  fetch(v_beg < V ? v_beg : 0);
  for (int v0 = v_beg; v0 < v_end; v0 += VA_CHUNK) {
    __syncthreads();        // (also: every thread is done reading s_o of the chunk before)
    SPACAP_VA_STORE_STAGE();
    __syncthreads();
    if (v0 + VA_CHUNK < v_end) fetch(v0 + VA_CHUNK);
    const int v = v0 + 16 * w + l15;                    // this lane's word of the chunk
    SPACAP_VA_TILE();                                   // acc, acc2
    const float bsv = v < V ? bias[v] : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) s_o[4 * lg + u][16 * w + l15] = (acc[u] + acc2[u]) + bsv;   // (the greedy kernel's logit, bit for bit)
    __syncthreads();
    const int row = tid >> 4, c = 4 * (tid & 15);
    if (row0 + row < R) st4(img + (size_t)(row0 + row) * ld + v0 + c, ld4(&s_o[row][c]));
  }
}

// a > b <=> key(a) > key(b) for floats that are not NaN; -0 counts as +0, as in the float compare
__device__ __forceinline__ unsigned nucleus_key(float l) {
  const unsigned u = __float_as_uint(l + 0.f);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float nucleus_unkey(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// The sum of the four waves' values in one fixed order.  s_red: 4 floats nobody else writes before the next barrier.
__device__ __forceinline__ float nucleus_block_sum(float v, float *s_red, int tid) {
  v = wave_sum(v);          // a butterfly: every lane holds the same bits
  if ((tid & 63) == 0) s_red[tid >> 6] = v;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// One workgroup per row; thread t owns words t, t + 256, ...  The row's logits are read once, into LDS as their keys (s_kq, V
// pairs of dynamic LDS; a thread reads back its own words only).  M = max l; T = sum exp((l - M) / tau) and S = sum exp(l - M),
// each in one fixed order (per thread by increasing word, a butterfly over the wave, then the four waves); the terms
// q = exp((l - M) / tau) are kept beside the keys.  The threshold key: the smallest 32-bit key k with
// mass(k) = sum_{key(l_u) > k} q_u < p T, found bit by bit from the top -- bit b stays 0 when mass(k | (2^b - 1)) < p T: 32
// passes over the pairs (with exp recomputed in every pass a word choice took 165 instead of 141 us at 2 048 x 3 001).  mass()
// adds the SAME floats in the same fixed order with 0 for the words outside the set, so it is monotone in k in float arithmetic
// and the bisection is valid.  The nucleus is { v : key(l_v) >= k }: words with equal logits share a key and enter together,
// and the largest logit is always in (mass = 0 < p T).  Then the first maximum of z over the nucleus and the row's state as
// sample_next_kernel.  No atomics; the same inputs give the same bits.
__global__ __launch_bounds__(256) void nucleus_next_kernel(const float *__restrict__ img, int ld, float top_p, float inv_tau, unsigned long long seed,
                                                           const unsigned long long *__restrict__ seed_dev, int V, int n_words, int step,
                                                           int eos, const float *__restrict__ lut, float scale, const float *__restrict__ pe_row,
                                                           long long *__restrict__ ys, float *score, int *length, int *fin,
                                                           float *__restrict__ xw) {
  extern __shared__ __attribute__((aligned(16))) uint2 s_kq[];   // (key of l, bits of q)
  __shared__ float s_red[2][4];
  __shared__ float s_z[4], s_wl[4];
  __shared__ int s_wi[4];
  const int tid = threadIdx.x;
  const size_t r = blockIdx.x;
  const float *row = img + r * (size_t)ld;
  float M = -INFINITY;
  for (int v = tid; v < V; v += 256) {
    const float l = row[v];
    s_kq[v].x = nucleus_key(l);
    M = fmaxf(M, l);
  }
  M = wave_max(M);
  if ((tid & 63) == 0) s_red[1][tid >> 6] = M;
  __syncthreads();
  M = fmaxf(fmaxf(s_red[1][0], s_red[1][1]), fmaxf(s_red[1][2], s_red[1][3]));
  float t = 0.f, s = 0.f;
  for (int v = tid; v < V; v += 256) {
    const float d = nucleus_unkey(s_kq[v].x) - M, q = expf(d * inv_tau);
    s_kq[v].y = __float_as_uint(q);
    t += q, s += expf(d);
  }
  // The two scratch rows alternate from here on: a row is written again only behind the barrier of the sum that followed its
  // last read (the maxima of row 1 were read before the barrier inside T's sum).
  const float T = nucleus_block_sum(t, s_red[0], tid);
  const float S = nucleus_block_sum(s, s_red[1], tid);
  const float bar = top_p * T;
  unsigned k = 0u;
  for (int b = 31; b >= 0; --b) {
    const unsigned cand = k | ((1u << b) - 1u);
    float m = 0.f;
    for (int v = tid; v < V; v += 256) {
      const uint2 e = s_kq[v];
      m += e.x > cand ? __uint_as_float(e.y) : 0.f;
    }
    if (!(nucleus_block_sum(m, s_red[(b & 1) ^ 1], tid) < bar)) k |= 1u << b;   // (b = 31 takes row 0: S sits in row 1)
  }
  const DropSeed sd = make_seed(seed, seed_dev);
  const unsigned long long nbase = ((unsigned long long)r * (unsigned long long)n_words + (unsigned long long)step) * (unsigned long long)V;
  float bz = -INFINITY, bl = -INFINITY;
  int bi = NO_WORD;
  for (int v = tid; v < V; v += 256) {
    const unsigned key = s_kq[v].x;
    if (key >= k) {
      const float l = nucleus_unkey(key);
      const float z = l * inv_tau + gumbel_noise(nbase + (unsigned long long)v, sd);
      if (z > bz) bz = z, bi = v, bl = l;       // (the thread's words arrive in increasing order)
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float oz = __shfl_xor(bz, o), ol = __shfl_xor(bl, o);
    const int oi = __shfl_xor(bi, o);
    if (SPACAP_FIRST_MAX(oz, oi, bz, bi)) bz = oz, bi = oi, bl = ol;
  }
  if ((tid & 63) == 0) s_z[tid >> 6] = bz, s_wi[tid >> 6] = bi, s_wl[tid >> 6] = bl;
  __syncthreads();
  if (tid >= 32) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float oz = s_z[q], ol = s_wl[q];
    const int oi = s_wi[q];
    if (q == 0 || SPACAP_FIRST_MAX(oz, oi, bz, bi)) bz = oz, bi = oi, bl = ol;
  }
  const float logp = (bl - M) - logf(S);
  const int f = fin[r];
  const int word = f ? eos : min(max(bi, 0), V - 1);
  if (tid == 0) {
    ys[r * (size_t)n_words + step] = word;
    if (!f) {
      score[r] += logp;
      length[r] = step + 1;
      if (word == eos) fin[r] = 1;
    }
  }
  const f32x4 e = ld4(lut + (size_t)word * VA_D + 4 * tid), p = ld4(pe_row + 4 * tid);
  st4(xw + r * VA_D + 4 * tid, f32x4{e[0] * scale + p[0], e[1] * scale + p[1], e[2] * scale + p[2], e[3] * scale + p[3]});
}

// ---- constrained decoding (restated by tests/decode_constraints_restated.py) ---------------------------
// Before a step's word choice looks at the logits z of a row they become z': every word of the row's history is penalised
// (z / theta when z > 0, else z theta: the CTRL rule), then the banned words -- bad_words, eos before min_length, and the words
// that would repeat an n-gram of the history -- go to -inf.  A constraint touches at most ~100 logits of a row, so the row's
// sets travel as two BIT IMAGES over the vocabulary, u32 [rows][2][nw]: plane 0 "banned", plane 1 "seen" (in the history),
// nw = 2 ceil(V / 64) words, so that a chunk of 64 words is two whole words of each plane.  decode_constraint_kernel builds
// them once per step; the word kernels below are the kernels above with two bit tests where a lane forms its logit.  The
// kernels above are not touched (they keep the instruction streams they were measured with); the copies use the same
// SPACAP_VA_* macros, so the tile arithmetic and the first-maximum rule are the same by construction.
inline int vc_words(int V) { return 2 * ((V + VA_CHUNK - 1) / VA_CHUNK); }
constexpr int VC_MAX_BAD = 64, VC_HIST = 31;   // bad words per call; history words of a row (T <= 32 positions)
struct VcBad { int w[VC_MAX_BAD]; };            // the bad words travel as a kernel argument: no device buffer, nothing to upload

// One wave per row.  The wave's candidates sit in LDS: entries 0..30 the history words y_0 .. y_{step-1} (-1: none), entry
// 31 eos while step < min_length, entries 32..95 the bad words.  History word y_j is banned by the n-gram rule when
// j >= n - 1 and (y_{j-n+1} .. y_{j-1}) = (y_{step-n+1} .. y_{step-1}); n = 1 bans every used word.  Then lane l forms image
// words l, l + 64, ... of both planes from the candidates and stores them: every image word is written once, by one lane,
// with a plain vector store -- no atomics, the same inputs give the same bits.
// The history: ys != nullptr: row's words ys[row][0 .. step); else row = r W + w is a beam hypothesis and word j is
// tr_word[j][r][slot], slot = the cache slot the hypothesis occupied at position j + 2 (where word j was the input):
// anc[row][j + 2] for j + 2 < t = step + 1, the row's own slot w at position t; an entry outside 0..W-1 reads w, as
// decode_attn_beam_kernel does.  A word outside 0..V-1 counts as no word: it sets no bit and matches nothing in an n-gram.
__global__ __launch_bounds__(256) void decode_constraint_kernel(const long long *__restrict__ ys, int ys_ld, const int *__restrict__ tr_word,
                                                                const signed char *__restrict__ anc, long R, int W, int T, long rows, int V,
                                                                int step, int eos, int min_length, int ngram, VcBad bad, int n_bad,
                                                                unsigned *__restrict__ bits, int nw) {
  __shared__ int s_c[4][VC_HIST + 1 + VC_MAX_BAD];
  __shared__ int s_f[4][VC_HIST + 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 4 + wv;
  const bool live = row < rows;
  int *c = s_c[wv], *f = s_f[wv];
  int word = -1;
  if (live && lane < step) {
    if (ys != nullptr) {
      const long long y = ys[(size_t)row * ys_ld + lane];
      word = y >= 0 && y < V ? (int)y : -1;
    } else {
      const long r = row / W;
      const int w = (int)(row - r * W), p = lane + 2;
      int slot = w;
      if (p < step + 1) {
        const int s = anc[(size_t)row * T + p];
        slot = (unsigned)s < (unsigned)W ? s : w;
      }
      const int y = tr_word[((size_t)lane * R + r) * W + slot];
      word = (unsigned)y < (unsigned)V ? y : -1;
    }
  }
  if (lane < VC_HIST) c[lane] = word;
  if (lane == VC_HIST) c[lane] = step < min_length ? eos : -1;
  c[VC_HIST + 1 + lane] = lane < n_bad ? bad.w[lane] : -1;
  __syncthreads();
  if (lane < VC_HIST) {
    bool hit = ngram >= 1 && lane < step && lane >= ngram - 1 && step >= ngram - 1;
    for (int k = 1; hit && k < ngram; ++k) hit = c[lane - k] == c[step - k] && c[lane - k] >= 0;   // (no word matches nothing)
    f[lane] = hit ? 1 : 0;
  }
  __syncthreads();
  if (!live) return;
  for (int j = lane; j < nw; j += 64) {
    unsigned ban = 0u, seen = 0u;
    for (int e = 0; e < step; ++e) {                       // (step <= VC_HIST)
      const int wd = c[e];
      if (wd >= 0 && (wd >> 5) == j) seen |= 1u << (wd & 31), ban |= f[e] ? 1u << (wd & 31) : 0u;
    }
    for (int e = VC_HIST; e < VC_HIST + 1 + n_bad; ++e) {
      const int wd = c[e];
      if (wd >= 0 && wd < V && (wd >> 5) == j) ban |= 1u << (wd & 31);
    }
    bits[((size_t)row * 2) * nw + j] = ban;
    bits[((size_t)row * 2 + 1) * nw + j] = seen;
  }
}

// The bits of a chunk of 64 words for the workgroup's 16 rows: 2 planes x 16 rows x 2 words, fetched by the first wave one
// chunk ahead (beside the weight staging) and handed over through LDS between the two barriers of the staging: one load
// per chunk and thread instead of one per compare.  Declares s_cb, cbit and the lambda fetch_bits(v0); reads tid, bits, nw,
// row0, R.  v0 is a multiple of 64 below V, so both words exist (nw = 2 ceil(V / 64)).
#define SPACAP_VC_BITS()                                                                                        \
  __shared__ unsigned s_cb[2][VA_ROWS][2];                                                                      \
  unsigned cbit = 0u;                                                                                           \
  auto fetch_bits = [&](int v0) {                                                                               \
    if (tid < 64) cbit = bits[((size_t)min(row0 + ((tid >> 1) & 15), R - 1) * 2 + (tid >> 5)) * nw + (v0 >> 5) + (tid & 1)]; \
  }
#define SPACAP_VC_STORE_BITS() \
  if (tid < 64) s_cb[tid >> 5][(tid >> 1) & 15][tid & 1] = cbit
// The lane's word is word 16 w + l15 of the chunk: bit 16 (w & 1) + l15 of word w >> 1.  Declares cban (banned) and applies
// the penalty to `val` (one fp32 operation) for row 4 lg + u; reads theta.
#define SPACAP_VC_APPLY(val, u)                                                              \
  const unsigned cbm = 1u << (16 * (w & 1) + l15);                                           \
  const unsigned cban = s_cb[0][4 * lg + (u)][w >> 1] & cbm;                                 \
  if (s_cb[1][4 * lg + (u)][w >> 1] & cbm) val = val > 0.f ? val / theta : val * theta

// vocab_argmax_kernel over z': a banned word never becomes a lane's best; a slice without an allowed word hands (-inf, v_beg)
// to decode_next_kernel, where every finite winner is ahead of it.
__global__ __launch_bounds__(256) void vocab_argmax_constrained_kernel(const float *__restrict__ x, const __bf16 *__restrict__ Wp,
                                                                       const float *__restrict__ bias, long R, int V, int per_slice,
                                                                       const unsigned *__restrict__ bits, int nw, float theta,
                                                                       float *__restrict__ best_v, int *__restrict__ best_i) {
  __shared__ __attribute__((aligned(16))) __bf16 s_w[VA_STAGE_ELEMS];
  __shared__ float s_bv[4][VA_ROWS][17];
  __shared__ int s_bi[4][VA_ROWS][17];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const long row0 = (long)blockIdx.x * VA_ROWS;
  const int ns = gridDim.y, sl = blockIdx.y;
  const int v_beg = sl * per_slice, v_end = min(V, v_beg + per_slice);
  SPACAP_VA_SPLIT_ROWS();   // bf16x8 a[kc][piece]
  float bv[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int bi[4] = {v_beg, v_beg, v_beg, v_beg};
  SPACAP_VC_BITS();         // s_cb, cbit, fetch_bits(v0)
  SPACAP_VA_STAGING();      // stg, fetch(v0)
  fetch(v_beg < V ? v_beg : 0);
  fetch_bits(v_beg < V ? v_beg : 0);
  for (int v0 = v_beg; v0 < v_end; v0 += VA_CHUNK) {
    __syncthreads();
    SPACAP_VA_STORE_STAGE();
    SPACAP_VC_STORE_BITS();
    __syncthreads();
    if (v0 + VA_CHUNK < v_end) fetch(v0 + VA_CHUNK), fetch_bits(v0 + VA_CHUNK);
    const int v = v0 + 16 * w + l15;                    // this lane's word of the chunk
    SPACAP_VA_TILE();                                   // acc, acc2
    if (v < v_end) {
      const float bsv = bias[v];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float val = (acc[u] + acc2[u]) + bsv;           // (the greedy kernel's logit, bit for bit)
        SPACAP_VC_APPLY(val, u);
        if (!cban && val > bv[u]) bv[u] = val, bi[u] = v;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) s_bv[w][4 * lg + u][l15] = bv[u], s_bi[w][4 * lg + u][l15] = bi[u];
  __syncthreads();
  if (tid < 64) {
    const int row = tid >> 2, ww = tid & 3;          // four threads per sequence, one wave's 16 candidates each
    float m = -INFINITY;
    int mi = 0x7fffffff;
#pragma unroll
    for (int l = 0; l < 16; ++l) {
      const float val = s_bv[ww][row][l];
      const int idx = s_bi[ww][row][l];
      if (SPACAP_FIRST_MAX(val, idx, m, mi)) m = val, mi = idx;
    }
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
      const float om = __shfl_xor(m, o);
      const int oi = __shfl_xor(mi, o);
      if (SPACAP_FIRST_MAX(om, oi, m, mi)) m = om, mi = oi;
    }
    if (ww == 0 && row0 + row < R) {
      best_v[(size_t)(row0 + row) * ns + sl] = m;
      best_i[(size_t)(row0 + row) * ns + sl] = mi;
    }
  }
}

// beam_topw_kernel over z': a banned word adds no term to the row's (max, sum exp) -- exp(-inf) = 0 -- and enters no list, so
// the merge kernel's log-probabilities are log_softmax(z').  A row with fewer than W allowed words ends its list with
// (-inf, NO_WORD) entries.
template <int WB>
__global__ __launch_bounds__(256) void beam_topw_constrained_kernel(const float *__restrict__ x, const __bf16 *__restrict__ Wp,
                                                                    const float *__restrict__ bias, long R, int V, int per_slice,
                                                                    const unsigned *__restrict__ bits, int nw, float theta, int W,
                                                                    float *__restrict__ part_v, int *__restrict__ part_i,
                                                                    float *__restrict__ part_ms) {
  __shared__ __attribute__((aligned(16))) __bf16 s_w[VA_STAGE_ELEMS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const long row0 = (long)blockIdx.x * VA_ROWS;
  const int ns = gridDim.y, sl = blockIdx.y;
  const int v_beg = sl * per_slice, v_end = min(V, v_beg + per_slice);
  SPACAP_VA_SPLIT_ROWS();   // bf16x8 a[kc][piece]
  float tv[4][WB], mx[4], sm[4];
  int ti[4][WB];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    mx[u] = -INFINITY, sm[u] = 0.f;
#pragma unroll
    for (int k = 0; k < WB; ++k) tv[u][k] = -INFINITY, ti[u][k] = NO_WORD;
  }
  SPACAP_VC_BITS();         // s_cb, cbit, fetch_bits(v0)
  SPACAP_VA_STAGING();      // stg, fetch(v0)
  fetch(v_beg < V ? v_beg : 0);
  fetch_bits(v_beg < V ? v_beg : 0);
  for (int v0 = v_beg; v0 < v_end; v0 += VA_CHUNK) {
    __syncthreads();
    SPACAP_VA_STORE_STAGE();
    SPACAP_VC_STORE_BITS();
    __syncthreads();
    if (v0 + VA_CHUNK < v_end) fetch(v0 + VA_CHUNK), fetch_bits(v0 + VA_CHUNK);
    const int v = v0 + 16 * w + l15;                    // this lane's word of the chunk
    SPACAP_VA_TILE();                                   // acc, acc2
    if (v < v_end) {
      const float bsv = bias[v];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float val = (acc[u] + acc2[u]) + bsv;           // (the greedy kernel's logit, bit for bit)
        SPACAP_VC_APPLY(val, u);
        if (!cban) {
          if (val > mx[u]) sm[u] = sm[u] * expf(mx[u] - val) + 1.f, mx[u] = val;
          else sm[u] += expf(val - mx[u]);
          if (val > tv[u][WB - 1]) {
            float cv = val;
            int ci = v;
#pragma unroll
            for (int k = 0; k < WB; ++k)
              if (SPACAP_FIRST_MAX(cv, ci, tv[u][k], ti[u][k])) {
                const float ov = tv[u][k];
                const int oi = ti[u][k];
                tv[u][k] = cv, ti[u][k] = ci, cv = ov, ci = oi;
              }
          }
        }
      }
    }
  }
  __syncthreads();   // every wave is done with the last chunk: the staging buffer becomes the merge area
  float *s_mv = reinterpret_cast<float *>(s_w);               // [4 waves][16 rows][WB]
  int *s_mi = reinterpret_cast<int *>(s_mv + 4 * VA_ROWS * WB);
  float *s_ms = reinterpret_cast<float *>(s_mi + 4 * VA_ROWS * WB);   // [4][16][2]
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int row = 4 * lg + u;
    float M = mx[u];
#pragma unroll
    for (int o = 1; o <= 8; o <<= 1) M = fmaxf(M, __shfl_xor(M, o));
    float S = mx[u] == -INFINITY ? 0.f : sm[u] * expf(mx[u] - M);
#pragma unroll
    for (int o = 1; o <= 8; o <<= 1) S += __shfl_xor(S, o);
    if (l15 == 0) s_ms[(w * VA_ROWS + row) * 2] = M, s_ms[(w * VA_ROWS + row) * 2 + 1] = S;
#pragma unroll
    for (int k = 0; k < WB; ++k) {
      if (k >= W) break;
      float bvv = tv[u][0];
      int bii = ti[u][0];
#pragma unroll
      for (int o = 1; o <= 8; o <<= 1) {
        const float ov = __shfl_xor(bvv, o);
        const int oi = __shfl_xor(bii, o);
        if (SPACAP_FIRST_MAX(ov, oi, bvv, bii)) bvv = ov, bii = oi;
      }
      if (ti[u][0] == bii) {   // (a word sits in one lane only; empty heads all pop, which changes nothing)
#pragma unroll
        for (int q = 0; q + 1 < WB; ++q) tv[u][q] = tv[u][q + 1], ti[u][q] = ti[u][q + 1];
        tv[u][WB - 1] = -INFINITY, ti[u][WB - 1] = NO_WORD;
      }
      if (l15 == 0) s_mv[(w * VA_ROWS + row) * WB + k] = bvv, s_mi[(w * VA_ROWS + row) * WB + k] = bii;
    }
  }
  __syncthreads();
  if (tid < VA_ROWS && row0 + tid < R) {   // one thread per sequence: the four waves' sorted lists, merged
    const int row = tid;
    const size_t o = ((size_t)(row0 + row) * ns + sl);
    int hd[4] = {0, 0, 0, 0};
    for (int k = 0; k < W; ++k) {
      float bvv = -INFINITY;
      int bii = NO_WORD, bw = 0;
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) {
        const bool has = hd[ww] < W;
        const float cv = has ? s_mv[(ww * VA_ROWS + row) * WB + hd[ww]] : -INFINITY;
        const int ci = has ? s_mi[(ww * VA_ROWS + row) * WB + hd[ww]] : NO_WORD;
        if (SPACAP_FIRST_MAX(cv, ci, bvv, bii)) bvv = cv, bii = ci, bw = ww;
      }
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) hd[ww] += ww == bw ? 1 : 0;
      part_v[o * W + k] = bvv, part_i[o * W + k] = bii;
    }
    float M = -INFINITY, S = 0.f;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) M = fmaxf(M, s_ms[(ww * VA_ROWS + row) * 2]);
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
      const float m = s_ms[(ww * VA_ROWS + row) * 2];
      S += m == -INFINITY ? 0.f : s_ms[(ww * VA_ROWS + row) * 2 + 1] * expf(m - M);
    }
    part_ms[o * 2] = M, part_ms[o * 2 + 1] = S;
  }
}

// vocab_gumbel_kernel over z': z_v = z'_v / tau + g_v; a banned word is never drawn and adds nothing to (max, sum exp), so
// sample_next_kernel's log-probability is log_softmax(z')[word].
__global__ __launch_bounds__(256) void vocab_gumbel_constrained_kernel(const float *__restrict__ x, const __bf16 *__restrict__ Wp,
                                                                       const float *__restrict__ bias, long R, int V, int per_slice,
                                                                       const unsigned *__restrict__ bits, int nw, float theta, float inv_tau,
                                                                       unsigned long long seed, const unsigned long long *__restrict__ seed_dev,
                                                                       int n_words, int step, float *__restrict__ part_z,
                                                                       int *__restrict__ part_w, float *__restrict__ part_l,
                                                                       float *__restrict__ part_ms) {
  __shared__ __attribute__((aligned(16))) __bf16 s_w[VA_STAGE_ELEMS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const long row0 = (long)blockIdx.x * VA_ROWS;
  const int ns = gridDim.y, sl = blockIdx.y;
  const int v_beg = sl * per_slice, v_end = min(V, v_beg + per_slice);
  const DropSeed sd = make_seed(seed, seed_dev);
  SPACAP_VA_SPLIT_ROWS();   // bf16x8 a[kc][piece]
  float bz[4], bl[4], mx[4], sm[4];
  int bi[4];
  unsigned long long nbase[4];   // the noise index of word 0 of row row0 + 4 lg + u at this step
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    bz[u] = -INFINITY, bl[u] = -INFINITY, bi[u] = NO_WORD, mx[u] = -INFINITY, sm[u] = 0.f;
    nbase[u] = ((unsigned long long)(row0 + 4 * lg + u) * (unsigned long long)n_words + (unsigned long long)step) * (unsigned long long)V;
  }
  SPACAP_VC_BITS();         // s_cb, cbit, fetch_bits(v0)
  SPACAP_VA_STAGING();      // stg, fetch(v0)
  fetch(v_beg < V ? v_beg : 0);
  fetch_bits(v_beg < V ? v_beg : 0);
  for (int v0 = v_beg; v0 < v_end; v0 += VA_CHUNK) {
    __syncthreads();
    SPACAP_VA_STORE_STAGE();
    SPACAP_VC_STORE_BITS();
    __syncthreads();
    if (v0 + VA_CHUNK < v_end) fetch(v0 + VA_CHUNK), fetch_bits(v0 + VA_CHUNK);
    const int v = v0 + 16 * w + l15;                    // this lane's word of the chunk
    SPACAP_VA_TILE();                                   // acc, acc2
    if (v < v_end) {
      const float bsv = bias[v];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float val = (acc[u] + acc2[u]) + bsv;           // (the greedy kernel's logit, bit for bit)
        SPACAP_VC_APPLY(val, u);
        if (!cban) {
          if (val > mx[u]) sm[u] = sm[u] * expf(mx[u] - val) + 1.f, mx[u] = val;
          else sm[u] += expf(val - mx[u]);
          const float z = val * inv_tau + gumbel_noise(nbase[u] + (unsigned long long)v, sd);
          if (z > bz[u]) bz[u] = z, bi[u] = v, bl[u] = val;
        }
      }
    }
  }
  __syncthreads();   // every wave is done with the last chunk: the staging buffer becomes the merge area
  constexpr int MA = 4 * VA_ROWS * 17;                        // [4 waves][16 rows][16 lanes + 1]
  float *s_z = reinterpret_cast<float *>(s_w);
  int *s_i = reinterpret_cast<int *>(s_z + MA);
  float *s_l = reinterpret_cast<float *>(s_i + MA), *s_m = s_l + MA, *s_s = s_m + MA;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int o = (w * VA_ROWS + 4 * lg + u) * 17 + l15;
    s_z[o] = bz[u], s_i[o] = bi[u], s_l[o] = bl[u], s_m[o] = mx[u], s_s[o] = sm[u];
  }
  __syncthreads();
  if (tid < 64) {
    const int row = tid >> 2, ww = tid & 3;          // four threads per sequence, one wave's 16 lanes each
    const int o = (ww * VA_ROWS + row) * 17;
    float m = -INFINITY, ml = -INFINITY, M = -INFINITY, S = 0.f;
    int mi = NO_WORD;
#pragma unroll
    for (int l = 0; l < 16; ++l) {
      const float val = s_z[o + l];
      const int idx = s_i[o + l];
      if (SPACAP_FIRST_MAX(val, idx, m, mi)) m = val, mi = idx, ml = s_l[o + l];
      M = fmaxf(M, s_m[o + l]);
    }
#pragma unroll
    for (int l = 0; l < 16; ++l) {
      const float lm = s_m[o + l];
      S += lm == -INFINITY ? 0.f : s_s[o + l] * expf(lm - M);
    }
#pragma unroll
    for (int q = 1; q <= 2; q <<= 1) {
      const float om = __shfl_xor(m, q), ol = __shfl_xor(ml, q), oM = __shfl_xor(M, q), oS = __shfl_xor(S, q);
      const int oi = __shfl_xor(mi, q);
      if (SPACAP_FIRST_MAX(om, oi, m, mi)) m = om, mi = oi, ml = ol;
      const float nM = fmaxf(M, oM);
      S = (M == -INFINITY ? 0.f : S * expf(M - nM)) + (oM == -INFINITY ? 0.f : oS * expf(oM - nM));
      M = nM;
    }
    if (ww == 0 && row0 + row < R) {
      const size_t e = (size_t)(row0 + row) * ns + sl;
      part_z[e] = m, part_w[e] = mi, part_l[e] = ml, part_ms[2 * e] = M, part_ms[2 * e + 1] = S;
    }
  }
}

// Nucleus sampling keeps the step's logits in HBM between its two launches anyway: z' is made by patching the image.  One
// thread per (row, image word): the set bits of "seen" and "banned" name the <= ~100 logits of the row that change.
__global__ __launch_bounds__(256) void logits_constrain_kernel(float *__restrict__ img, int ld, const unsigned *__restrict__ bits, int nw,
                                                               long rows, int V, float theta) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * nw) return;
  const long r = idx / nw;
  const int j = (int)(idx - r * nw);
  const unsigned ban = bits[((size_t)r * 2) * nw + j], seen = bits[((size_t)r * 2 + 1) * nw + j];
  for (unsigned any = ban | seen; any; any &= any - 1) {
    const int b = __ffs((int)any) - 1, v = 32 * j + b;
    if (v >= V) break;
    float *p = img + (size_t)r * ld + v;
    float val = *p;
    if ((seen >> b) & 1u) val = val > 0.f ? val / theta : val * theta;
    if ((ban >> b) & 1u) val = -INFINITY;
    *p = val;
  }
}

// the arguments every constrained word choice shares: the images of decode_constraint_kernel and the penalty
inline bool vc_ok(const void *bits, float theta) { return bits != nullptr && isfinite(theta) && theta >= 1.f; }

}  // namespace

extern "C" int spacap_decode_attn_f32(const float *qkv, float *kcache, float *vcache, long R, int h, int d_k, int T, int t, float scale,
                                      float *out, spacap_stream_t stream) {
  const char *what = "spacap_decode_attn_f32";
  SPACAP_REQUIRE(R >= 0 && h == 8 && d_k == 16 && T >= 1 && T <= 32 && t >= 0 && t < T, "%s: (R=%ld, h=%d, d_k=%d, T=%d, t=%d) unsupported",
                 what, R, h, d_k, T, t);
  if (R == 0) return SPACAP_OK;
  SPACAP_REQUIRE(qkv && kcache && vcache && out && aligned16(qkv, kcache, vcache, out), "%s: null or unaligned pointer", what);
  SPACAP_REQUIRE(R <= 2147483647L, "%s: too many sequences", what);
  hipLaunchKernelGGL(decode_attn_kernel, dim3((unsigned)R), dim3(256), 0, spacap::as_stream(stream), qkv, kcache, vcache, T, t, scale, out);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

/* One greedy-decoding step's word choice (models/transformer_captioner.py:441-447 with the Generator of :93-100): x f32 [R,128] the
   decoder's output rows, Wp bf16 [3][V][128] = the pieces of the projection weight (spacap_gemm_bf3_split_w_f32), bias f32 [V]
   -> ys i64 [R][ys_ld] column t_out = arg-max word (first maximum), and the next
   step's input rows x_next f32 [R,128] = lut[word] * scale + pe_row (lut f32 [V,128], pe_row f32 [128]).
   workspace: spacap_decode_word_workspace_bytes(R, V) bytes (the vocabulary slices' winners). */
extern "C" size_t spacap_decode_word_workspace_bytes(long R, int V) { return R > 0 && V > 0 ? (size_t)R * va_slices(R, V) * 8 : 0; }
extern "C" int spacap_decode_word_f32(const float *x, const void *W, const float *bias, long R, int V, const float *lut, float scale,
                                      const float *pe_row, int64_t *ys, int ys_ld, int t_out, float *x_next, void *workspace,
                                      spacap_stream_t stream) {
  const char *what = "spacap_decode_word_f32";
  SPACAP_REQUIRE(R >= 0 && V >= 1 && ys_ld >= 1 && t_out >= 0 && t_out < ys_ld, "%s: bad sizes", what);
  if (R == 0) return SPACAP_OK;
  SPACAP_REQUIRE(x && W && bias && lut && pe_row && ys && x_next && workspace && aligned16(x, W, lut, pe_row, x_next),
                 "%s: null or unaligned pointer", what);
  SPACAP_REQUIRE(R <= 16L * 2147483647L, "%s: too many sequences", what);
  const int ns = va_slices(R, V);
  const int per = va_per_slice(V, ns);   // whole chunks per slice
  float *bv = static_cast<float *>(workspace);
  int *bi = reinterpret_cast<int *>(bv + (size_t)R * ns);
  hipStream_t s = spacap::as_stream(stream);
  hipLaunchKernelGGL(vocab_argmax_kernel, dim3((unsigned)((R + VA_ROWS - 1) / VA_ROWS), ns), dim3(256), 0, s, x, static_cast<const __bf16 *>(W),
                     bias, R, V, per, bv, bi);
  hipLaunchKernelGGL(decode_next_kernel, dim3((unsigned)((R + 7) / 8)), dim3(256), 0, s, bv, bi, ns, R, lut, scale, pe_row,
                     reinterpret_cast<long long *>(ys), ys_ld, t_out, x_next);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" size_t spacap_beam_topw_workspace_bytes(long rows, int V, int W) {
  return rows > 0 && V > 0 && W >= 1 && W <= BEAM_MAX ? (size_t)rows * va_slices(rows, V) * (8 * (size_t)W + 8) : 0;
}

// bits == nullptr: the unconstrained kernels, as ever; else the constrained ones over the images `bits` with penalty theta
static int beam_topw_impl(const char *what, const float *x, const void *Wp, const float *bias, long rows, int V, int W, const uint32_t *bits,
                          float theta, float *top_logp, int32_t *top_word, void *workspace, spacap_stream_t stream) {
  SPACAP_REQUIRE(rows >= 0 && V >= 1 && W >= 1 && W <= BEAM_MAX && W <= V, "%s: (rows=%ld, V=%d, W=%d) unsupported: 1 <= W <= %d and W <= V",
                 what, rows, V, W, BEAM_MAX);
  if (rows == 0) return SPACAP_OK;
  SPACAP_REQUIRE(x && Wp && bias && top_logp && top_word && workspace && aligned16(x, Wp), "%s: null or unaligned pointer", what);
  SPACAP_REQUIRE(rows <= 16L * 2147483647L, "%s: too many rows", what);
  const int ns = va_slices(rows, V);
  const int per = va_per_slice(V, ns);
  float *pv = static_cast<float *>(workspace);
  int *pi = reinterpret_cast<int *>(pv + (size_t)rows * ns * W);
  float *pms = reinterpret_cast<float *>(pi + (size_t)rows * ns * W);
  hipStream_t s = spacap::as_stream(stream);
  const dim3 grid((unsigned)((rows + VA_ROWS - 1) / VA_ROWS), ns);
  const __bf16 *wp = static_cast<const __bf16 *>(Wp);
  const int nw = vc_words(V);
  if (bits == nullptr) {
    if (W <= 4) hipLaunchKernelGGL((beam_topw_kernel<4>), grid, dim3(256), 0, s, x, wp, bias, rows, V, per, W, pv, pi, pms);
    else hipLaunchKernelGGL((beam_topw_kernel<8>), grid, dim3(256), 0, s, x, wp, bias, rows, V, per, W, pv, pi, pms);
  } else if (W <= 4) {
    hipLaunchKernelGGL((beam_topw_constrained_kernel<4>), grid, dim3(256), 0, s, x, wp, bias, rows, V, per, bits, nw, theta, W, pv, pi, pms);
  } else {
    hipLaunchKernelGGL((beam_topw_constrained_kernel<8>), grid, dim3(256), 0, s, x, wp, bias, rows, V, per, bits, nw, theta, W, pv, pi, pms);
  }
  hipLaunchKernelGGL(beam_topw_merge_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, pv, pi, pms, ns, rows, W, top_logp,
                     reinterpret_cast<int *>(top_word));
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_beam_topw_f32(const float *x, const void *Wp, const float *bias, long rows, int V, int W, float *top_logp,
                                    int32_t *top_word, void *workspace, spacap_stream_t stream) {
  return beam_topw_impl("spacap_beam_topw_f32", x, Wp, bias, rows, V, W, nullptr, 1.f, top_logp, top_word, workspace, stream);
}

extern "C" int spacap_beam_topw_constrained_f32(const float *x, const void *Wp, const float *bias, long rows, int V, int W, const uint32_t *bits,
                                                float theta, float *top_logp, int32_t *top_word, void *workspace, spacap_stream_t stream) {
  const char *what = "spacap_beam_topw_constrained_f32";
  SPACAP_REQUIRE(vc_ok(bits, theta), "%s: bits must not be null and the repetition penalty %g must be finite and >= 1", what, (double)theta);
  return beam_topw_impl(what, x, Wp, bias, rows, V, W, bits, theta, top_logp, top_word, workspace, stream);
}

extern "C" int spacap_decode_attn_beam_f32(const float *qkv, float *kcache, float *vcache, const int8_t *anc, long R, int W, int h, int d_k,
                                           int T, int t, float scale, float *out, spacap_stream_t stream) {
  const char *what = "spacap_decode_attn_beam_f32";
  SPACAP_REQUIRE(R >= 0 && W >= 1 && W <= BEAM_MAX && h == 8 && d_k == 16 && T >= 1 && T <= 32 && t >= 0 && t < T,
                 "%s: (R=%ld, W=%d, h=%d, d_k=%d, T=%d, t=%d) unsupported", what, R, W, h, d_k, T, t);
  if (R == 0) return SPACAP_OK;
  SPACAP_REQUIRE(qkv && kcache && vcache && anc && out && aligned16(qkv, kcache, vcache, out), "%s: null or unaligned pointer", what);
  SPACAP_REQUIRE(R * W <= 2147483647L, "%s: too many sequences", what);
  hipLaunchKernelGGL(decode_attn_beam_kernel, dim3((unsigned)(R * W)), dim3(256), 0, spacap::as_stream(stream), qkv, kcache, vcache,
                     reinterpret_cast<const signed char *>(anc), W, T, t, scale, out);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_beam_step_f32(const float *top_logp, const int32_t *top_word, long R, int W, int V, int T, int t, int eos,
                                    const float *score_in, const int32_t *fin_in, const int32_t *len_in, float *score_out, int32_t *fin_out,
                                    int32_t *len_out, const int8_t *anc_old, int8_t *anc_new, int8_t *trace_parent, int32_t *trace_word,
                                    const float *lut, float scale, const float *pe_row, float *x_next, spacap_stream_t stream) {
  const char *what = "spacap_beam_step_f32";
  SPACAP_REQUIRE(R >= 0 && W >= 1 && W <= BEAM_MAX && V >= W && T >= 2 && T <= 64 && t >= 1 && t < T && eos >= 0 && eos < V,
                 "%s: (R=%ld, W=%d, V=%d, T=%d, t=%d, eos=%d) unsupported", what, R, W, V, T, t, eos);
  if (R == 0) return SPACAP_OK;
  SPACAP_REQUIRE(top_logp && top_word && score_in && fin_in && len_in && score_out && fin_out && len_out && anc_old && anc_new &&
                     trace_parent && trace_word, "%s: null pointer", what);
  SPACAP_REQUIRE(score_in != score_out && fin_in != fin_out && len_in != len_out && anc_old != anc_new,
                 "%s: state and ancestor table are double-buffered: in and out must differ", what);
  SPACAP_REQUIRE(x_next == nullptr || (lut && pe_row && aligned16(lut, pe_row, x_next)), "%s: x_next needs lut and pe_row, 16-byte aligned", what);
  SPACAP_REQUIRE((R + 3) / 4 <= 2147483647L, "%s: too many sequences", what);
  hipLaunchKernelGGL(beam_step_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, spacap::as_stream(stream), top_logp,
                     reinterpret_cast<const int *>(top_word), R, W, V, T, t, eos, score_in, reinterpret_cast<const int *>(fin_in),
                     reinterpret_cast<const int *>(len_in), score_out, reinterpret_cast<int *>(fin_out), reinterpret_cast<int *>(len_out),
                     reinterpret_cast<const signed char *>(anc_old), reinterpret_cast<signed char *>(anc_new),
                     reinterpret_cast<signed char *>(trace_parent), reinterpret_cast<int *>(trace_word), lut, scale, pe_row, x_next);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_beam_finish_f32(const float *score, const int32_t *len, const int8_t *trace_parent, const int32_t *trace_word, long R,
                                      int W, int n_words, double alpha, int64_t *ys, float *best_score, int64_t *all_tokens,
                                      float *all_scores, int32_t *all_len, spacap_stream_t stream) {
  const char *what = "spacap_beam_finish_f32";
  SPACAP_REQUIRE(R >= 0 && W >= 1 && W <= BEAM_MAX && n_words >= 1, "%s: (R=%ld, W=%d, n_words=%d) unsupported", what, R, W, n_words);
  if (R == 0) return SPACAP_OK;
  SPACAP_REQUIRE(score && len && trace_parent && trace_word && ys && best_score, "%s: null pointer", what);
  SPACAP_REQUIRE(all_tokens == nullptr || (all_scores && all_len), "%s: all_tokens needs all_scores and all_len", what);
  SPACAP_REQUIRE((R * W + 255) / 256 <= 2147483647L, "%s: too many sequences", what);
  hipLaunchKernelGGL(beam_finish_kernel, dim3((unsigned)((R * W + 255) / 256)), dim3(256), 0, spacap::as_stream(stream), score,
                     reinterpret_cast<const int *>(len), reinterpret_cast<const signed char *>(trace_parent),
                     reinterpret_cast<const int *>(trace_word), R, W, n_words, alpha, reinterpret_cast<long long *>(ys), best_score,
                     reinterpret_cast<long long *>(all_tokens), all_scores, reinterpret_cast<int *>(all_len));
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

/* Sampled decoding: one step's word choice for `rows` rows.  top_k = 0 draws from the whole vocabulary
   (vocab_gumbel_kernel + sample_next_kernel); top_k >= 1 runs spacap_beam_topw_f32 into the workspace first and draws among its
   k entries.  workspace: top_k = 0: the slices' partials, 20 bytes each; else spacap_beam_topw_f32's own workspace, then the
   lists top_logp f32 [rows][k] and top_word i32 [rows][k]. */
extern "C" size_t spacap_sample_word_workspace_bytes(long rows, int V, int top_k) {
  if (rows <= 0 || V < 1 || top_k < 0 || top_k > BEAM_MAX || top_k > V) return 0;
  if (top_k == 0) return (size_t)rows * va_slices(rows, V) * 20;
  return spacap_beam_topw_workspace_bytes(rows, V, top_k) + (size_t)rows * top_k * 8;
}

static int sample_word_impl(const char *what, const float *x, const void *Wp, const float *bias, long rows, int V, int top_k, float inv_tau,
                            uint64_t seed, const uint64_t *seed_dev, int n_words, int step, int eos, const uint32_t *bits, float theta,
                            const float *lut, float scale, const float *pe_row, int64_t *ys, float *score, int32_t *length,
                            int32_t *finished, float *xw, void *workspace, spacap_stream_t stream) {
  SPACAP_REQUIRE(rows >= 0 && V >= 1, "%s: (rows=%ld, V=%d) unsupported: rows >= 0 and V >= 1", what, rows, V);
  SPACAP_REQUIRE(top_k >= 0 && top_k <= BEAM_MAX && top_k <= V, "%s: top_k=%d unsupported: 0 <= top_k <= min(%d, V=%d)", what, top_k,
                 BEAM_MAX, V);
  SPACAP_REQUIRE(isfinite(inv_tau) && inv_tau > 0.f, "%s: 1/temperature = %g must be finite and positive", what, (double)inv_tau);
  SPACAP_REQUIRE(n_words >= 1 && step >= 0 && step < n_words, "%s: (n_words=%d, step=%d) unsupported: 0 <= step < n_words", what, n_words, step);
  SPACAP_REQUIRE(eos >= 0 && eos < V, "%s: eos=%d outside the vocabulary (V=%d)", what, eos, V);
  if (rows == 0) return SPACAP_OK;
  SPACAP_REQUIRE(x && Wp && bias && lut && pe_row && ys && score && length && finished && xw && workspace, "%s: null pointer", what);
  SPACAP_REQUIRE(aligned16(x, Wp, lut, pe_row, xw), "%s: x, Wp, lut, pe_row and xw must be 16-byte aligned", what);
  SPACAP_REQUIRE(rows <= 2147483647L, "%s: too many rows", what);
  hipStream_t s = spacap::as_stream(stream);
  const unsigned long long *sdev = reinterpret_cast<const unsigned long long *>(seed_dev);
  const float *pz = nullptr, *pl = nullptr, *pms = nullptr, *top_lp = nullptr;
  const int *pw = nullptr, *top_wd = nullptr;
  int ns = 0;
  if (top_k == 0) {
    ns = va_slices(rows, V);
    const int per = va_per_slice(V, ns);
    float *wz = static_cast<float *>(workspace);
    int *ww = reinterpret_cast<int *>(wz + (size_t)rows * ns);
    float *wl = reinterpret_cast<float *>(ww + (size_t)rows * ns), *wms = wl + (size_t)rows * ns;
    if (bits == nullptr)
      hipLaunchKernelGGL(vocab_gumbel_kernel, dim3((unsigned)((rows + VA_ROWS - 1) / VA_ROWS), ns), dim3(256), 0, s, x,
                         static_cast<const __bf16 *>(Wp), bias, rows, V, per, inv_tau, (unsigned long long)seed, sdev, n_words, step, wz, ww, wl,
                         wms);
    else
      hipLaunchKernelGGL(vocab_gumbel_constrained_kernel, dim3((unsigned)((rows + VA_ROWS - 1) / VA_ROWS), ns), dim3(256), 0, s, x,
                         static_cast<const __bf16 *>(Wp), bias, rows, V, per, bits, vc_words(V), theta, inv_tau, (unsigned long long)seed, sdev,
                         n_words, step, wz, ww, wl, wms);
    pz = wz, pw = ww, pl = wl, pms = wms;
  } else {
    char *base = static_cast<char *>(workspace);
    float *lp = reinterpret_cast<float *>(base + spacap_beam_topw_workspace_bytes(rows, V, top_k));
    int32_t *wd = reinterpret_cast<int32_t *>(lp + (size_t)rows * top_k);
    // (unconstrained: the top-W entry reports its refusals under its own name, as it always did)
    const int rc = beam_topw_impl(bits == nullptr ? "spacap_beam_topw_f32" : what, x, Wp, bias, rows, V, top_k, bits, theta, lp, wd, workspace,
                                  stream);
    if (rc != SPACAP_OK) return rc;
    top_lp = lp, top_wd = reinterpret_cast<const int *>(wd);
  }
  hipLaunchKernelGGL(sample_next_kernel, dim3((unsigned)((rows + 7) / 8)), dim3(256), 0, s, pz, pw, pl, pms, ns, top_lp, top_wd, top_k, inv_tau,
                     (unsigned long long)seed, sdev, rows, V, n_words, step, eos, lut, scale, pe_row, reinterpret_cast<long long *>(ys), score,
                     reinterpret_cast<int *>(length), reinterpret_cast<int *>(finished), xw);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_sample_word_f32(const float *x, const void *Wp, const float *bias, long rows, int V, int top_k, float inv_tau,
                                      uint64_t seed, const uint64_t *seed_dev, int n_words, int step, int eos, const float *lut, float scale,
                                      const float *pe_row, int64_t *ys, float *score, int32_t *length, int32_t *finished, float *xw,
                                      void *workspace, spacap_stream_t stream) {
  return sample_word_impl("spacap_sample_word_f32", x, Wp, bias, rows, V, top_k, inv_tau, seed, seed_dev, n_words, step, eos, nullptr, 1.f, lut,
                          scale, pe_row, ys, score, length, finished, xw, workspace, stream);
}

extern "C" int spacap_sample_word_constrained_f32(const float *x, const void *Wp, const float *bias, long rows, int V, int top_k, float inv_tau,
                                                  uint64_t seed, const uint64_t *seed_dev, int n_words, int step, int eos, const uint32_t *bits,
                                                  float theta, const float *lut, float scale, const float *pe_row, int64_t *ys, float *score,
                                                  int32_t *length, int32_t *finished, float *xw, void *workspace, spacap_stream_t stream) {
  const char *what = "spacap_sample_word_constrained_f32";
  SPACAP_REQUIRE(vc_ok(bits, theta), "%s: bits must not be null and the repetition penalty %g must be finite and >= 1", what, (double)theta);
  return sample_word_impl(what, x, Wp, bias, rows, V, top_k, inv_tau, seed, seed_dev, n_words, step, eos, bits, theta, lut, scale, pe_row, ys,
                          score, length, finished, xw, workspace, stream);
}

/* Nucleus (top-p) sampling ("Top-p"): spacap_sample_word_f32's step with the draw restricted to the
   words v whose strictly more probable words hold less than top_p of softmax(logits * inv_tau).  Two launches:
   vocab_logits_kernel writes the logits to the workspace -- f32 [rows][V rounded up to a multiple of 64], the whole
   workspace -- and nucleus_next_kernel, one workgroup per row, finds the threshold, draws and updates the row.  V <= 16 384:
   the row kernel keeps 8 bytes a word in LDS. */
extern "C" size_t spacap_sample_word_nucleus_workspace_bytes(long rows, int V) {
  return rows > 0 && V >= 1 && V <= NUC_MAX_V ? (size_t)rows * nuc_ld(V) * sizeof(float) : 0;
}

static int sample_word_nucleus_impl(const char *what, const float *x, const void *Wp, const float *bias, long rows, int V, float top_p,
                                    float inv_tau, uint64_t seed, const uint64_t *seed_dev, int n_words, int step, int eos,
                                    const uint32_t *bits, float theta, const float *lut, float scale, const float *pe_row, int64_t *ys,
                                    float *score, int32_t *length, int32_t *finished, float *xw, void *workspace, spacap_stream_t stream) {
  SPACAP_REQUIRE(rows >= 0 && V >= 1 && V <= NUC_MAX_V, "%s: (rows=%ld, V=%d) unsupported: rows >= 0 and 1 <= V <= %d", what, rows, V,
                 NUC_MAX_V);
  SPACAP_REQUIRE(isfinite(top_p) && top_p > 0.f && top_p <= 1.f, "%s: top_p = %g must lie in (0, 1]", what, (double)top_p);
  SPACAP_REQUIRE(isfinite(inv_tau) && inv_tau > 0.f, "%s: 1/temperature = %g must be finite and positive", what, (double)inv_tau);
  SPACAP_REQUIRE(n_words >= 1 && step >= 0 && step < n_words, "%s: (n_words=%d, step=%d) unsupported: 0 <= step < n_words", what, n_words, step);
  SPACAP_REQUIRE(eos >= 0 && eos < V, "%s: eos=%d outside the vocabulary (V=%d)", what, eos, V);
  if (rows == 0) return SPACAP_OK;
  SPACAP_REQUIRE(x && Wp && bias && lut && pe_row && ys && score && length && finished && xw && workspace, "%s: null pointer", what);
  SPACAP_REQUIRE(aligned16(x, Wp, lut, pe_row, xw, workspace), "%s: x, Wp, lut, pe_row, xw and workspace must be 16-byte aligned", what);
  SPACAP_REQUIRE(rows <= 2147483647L, "%s: too many rows", what);
  hipStream_t s = spacap::as_stream(stream);
  const int ns = va_slices(rows, V), per = va_per_slice(V, ns), ld = nuc_ld(V);
  float *img = static_cast<float *>(workspace);
  static unsigned long long lds_ok = 0;
  SPACAP_CHECK_HIP(spacap::allow_dynamic_lds(reinterpret_cast<const void *>(&nucleus_next_kernel), NUC_MAX_V * 8, lds_ok), what);
  hipLaunchKernelGGL(vocab_logits_kernel, dim3((unsigned)((rows + VA_ROWS - 1) / VA_ROWS), ns), dim3(256), 0, s, x,
                     static_cast<const __bf16 *>(Wp), bias, rows, V, per, ld, img);
  if (bits != nullptr) {   // z' in place: the image is this mode's own copy of the logits
    const int nw = vc_words(V);
    hipLaunchKernelGGL(logits_constrain_kernel, dim3((unsigned)((rows * nw + 255) / 256)), dim3(256), 0, s, img, ld, bits, nw, rows, V, theta);
  }
  hipLaunchKernelGGL(nucleus_next_kernel, dim3((unsigned)rows), dim3(256), (size_t)V * 8, s, img, ld, top_p, inv_tau,
                     (unsigned long long)seed, reinterpret_cast<const unsigned long long *>(seed_dev), V, n_words, step, eos, lut, scale,
                     pe_row, reinterpret_cast<long long *>(ys), score, reinterpret_cast<int *>(length), reinterpret_cast<int *>(finished), xw);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_sample_word_nucleus_f32(const float *x, const void *Wp, const float *bias, long rows, int V, float top_p, float inv_tau,
                                              uint64_t seed, const uint64_t *seed_dev, int n_words, int step, int eos, const float *lut,
                                              float scale, const float *pe_row, int64_t *ys, float *score, int32_t *length,
                                              int32_t *finished, float *xw, void *workspace, spacap_stream_t stream) {
  return sample_word_nucleus_impl("spacap_sample_word_nucleus_f32", x, Wp, bias, rows, V, top_p, inv_tau, seed, seed_dev, n_words, step, eos,
                                  nullptr, 1.f, lut, scale, pe_row, ys, score, length, finished, xw, workspace, stream);
}

extern "C" int spacap_sample_word_nucleus_constrained_f32(const float *x, const void *Wp, const float *bias, long rows, int V, float top_p,
                                                          float inv_tau, uint64_t seed, const uint64_t *seed_dev, int n_words, int step,
                                                          int eos, const uint32_t *bits, float theta, const float *lut, float scale,
                                                          const float *pe_row, int64_t *ys, float *score, int32_t *length, int32_t *finished,
                                                          float *xw, void *workspace, spacap_stream_t stream) {
  const char *what = "spacap_sample_word_nucleus_constrained_f32";
  SPACAP_REQUIRE(vc_ok(bits, theta), "%s: bits must not be null and the repetition penalty %g must be finite and >= 1", what, (double)theta);
  return sample_word_nucleus_impl(what, x, Wp, bias, rows, V, top_p, inv_tau, seed, seed_dev, n_words, step, eos, bits, theta, lut, scale,
                                  pe_row, ys, score, length, finished, xw, workspace, stream);
}

/* Constrained decoding: the two bit images of every row for step `step` -- bits u32 [rows][2][nw],
   nw = 2 ceil(V / 64): plane 0 the banned words (bad_words, eos while step < min_length, the no-repeat n-gram rule), plane 1
   the words of the row's history.  rows = R W.  The history is either ys i64 [rows][ys_ld] columns 0 .. step - 1 (greedy and
   sampled decoding, W = 1) or, with ys null, a beam's: trace_word i32 [n_words][R][W] read through anc i8 [R W][T], the
   ancestor table of position step + 1 (spacap_beam_step_f32).  bad_words i32 [n_bad] in HOST memory, n_bad <= 64, read during the call. */
extern "C" size_t spacap_decode_constraints_bytes(long rows, int V) { return rows > 0 && V >= 1 ? (size_t)rows * 2 * vc_words(V) * 4 : 0; }

extern "C" int spacap_decode_constraints(const int64_t *ys, int ys_ld, const int32_t *trace_word, const int8_t *anc, long R, int W, int T, int V,
                                         int step, int eos, int min_length, int no_repeat_ngram, const int32_t *bad_words, int n_bad,
                                         uint32_t *bits, spacap_stream_t stream) {
  const char *what = "spacap_decode_constraints";
  SPACAP_REQUIRE(R >= 0 && W >= 1 && W <= BEAM_MAX && V >= 1 && T >= 2 && T <= 32, "%s: (R=%ld, W=%d, V=%d, T=%d) unsupported", what, R, W, V, T);
  SPACAP_REQUIRE(step >= 0 && step <= VC_HIST && step + 1 < T, "%s: step=%d outside 0 .. T - 2 = %d", what, step, T - 2);
  SPACAP_REQUIRE(eos >= 0 && eos < V && min_length >= 0 && no_repeat_ngram >= 0, "%s: (eos=%d, min_length=%d, no_repeat_ngram=%d) unsupported",
                 what, eos, min_length, no_repeat_ngram);
  SPACAP_REQUIRE(n_bad >= 0 && n_bad <= VC_MAX_BAD && (n_bad == 0 || bad_words), "%s: n_bad=%d outside 0..%d, or bad_words null", what, n_bad,
                 VC_MAX_BAD);
  SPACAP_REQUIRE((long)n_bad + step + 1 < V, "%s: %d bad words + %d history words + eos could leave no word of V=%d allowed", what, n_bad, step, V);
  if (R == 0) return SPACAP_OK;
  SPACAP_REQUIRE(bits != nullptr, "%s: null bits", what);
  SPACAP_REQUIRE(ys != nullptr ? (W == 1 && ys_ld >= step && ys_ld >= 1) : (trace_word != nullptr && anc != nullptr),
                 "%s: the history is ys (W = 1, ys_ld >= step) or trace_word with anc", what);
  const long rows = R * W;
  SPACAP_REQUIRE((rows + 3) / 4 <= 2147483647L, "%s: too many rows", what);
  VcBad bad;
  for (int i = 0; i < VC_MAX_BAD; ++i) bad.w[i] = i < n_bad ? bad_words[i] : -1;
  hipLaunchKernelGGL(decode_constraint_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, spacap::as_stream(stream),
                     reinterpret_cast<const long long *>(ys), ys_ld, reinterpret_cast<const int *>(trace_word),
                     reinterpret_cast<const signed char *>(anc), R, W, T, rows, V, step, eos, min_length, no_repeat_ngram,
                     bad, n_bad, reinterpret_cast<unsigned *>(bits), vc_words(V));
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

/* spacap_decode_word_f32 over the constrained logits: the same workspace, the same outputs. */
extern "C" int spacap_decode_word_constrained_f32(const float *x, const void *W, const float *bias, long R, int V, const uint32_t *bits,
                                                  float theta, const float *lut, float scale, const float *pe_row, int64_t *ys, int ys_ld,
                                                  int t_out, float *x_next, void *workspace, spacap_stream_t stream) {
  const char *what = "spacap_decode_word_constrained_f32";
  SPACAP_REQUIRE(R >= 0 && V >= 1 && ys_ld >= 1 && t_out >= 0 && t_out < ys_ld, "%s: bad sizes", what);
  SPACAP_REQUIRE(vc_ok(bits, theta), "%s: bits must not be null and the repetition penalty %g must be finite and >= 1", what, (double)theta);
  if (R == 0) return SPACAP_OK;
  SPACAP_REQUIRE(x && W && bias && lut && pe_row && ys && x_next && workspace && aligned16(x, W, lut, pe_row, x_next),
                 "%s: null or unaligned pointer", what);
  SPACAP_REQUIRE(R <= 16L * 2147483647L, "%s: too many sequences", what);
  const int ns = va_slices(R, V);
  const int per = va_per_slice(V, ns);
  float *bv = static_cast<float *>(workspace);
  int *bi = reinterpret_cast<int *>(bv + (size_t)R * ns);
  hipStream_t s = spacap::as_stream(stream);
  hipLaunchKernelGGL(vocab_argmax_constrained_kernel, dim3((unsigned)((R + VA_ROWS - 1) / VA_ROWS), ns), dim3(256), 0, s, x,
                     static_cast<const __bf16 *>(W), bias, R, V, per, bits, vc_words(V), theta, bv, bi);
  hipLaunchKernelGGL(decode_next_kernel, dim3((unsigned)((R + 7) / 8)), dim3(256), 0, s, bv, bi, ns, R, lut, scale, pe_row,
                     reinterpret_cast<long long *>(ys), ys_ld, t_out, x_next);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
