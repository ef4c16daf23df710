// What the caption decoders share (tf_layer.hip: greedy, beam_search.hip: beam search): the split-bf16 logit tile of the
// vocabulary projection, the first-maximum compare and the slicing of the vocabulary over workgroups.  ONE definition of the
// logit arithmetic -- the same six piece products in the same order on the same two accumulators -- is what makes a beam of
// width 1 choose the greedy decoder's words bit for bit.
//
// The device pieces are MACROS, not functions: vocab_argmax_kernel must keep the instruction stream it was measured with, and
// hipcc allocates its registers differently (and emits another loop) as soon as one of these blocks goes through a
// __forceinline__ function with array-reference parameters -- even the three-term compare.  A macro hands the compiler the
// token stream the kernel had before the pieces moved here.  Users say `using namespace spacap::decode;` and
// `using namespace spacap::mfma;` inside their own namespace; the macros name the caller's variables as listed with each.
#pragma once
#include "common.hpp"
#include "launch.hpp"
#include "mfma.hpp"

namespace spacap::decode {

constexpr int VA_D = 128;                                       // d_model: the contraction length of a logit
constexpr int VA_CHUNK = 64, VA_LDB = VA_D + 8, VA_ROWS = 16;   // words per LDS chunk, LDS row stride (bf16), sequences per workgroup
constexpr int VA_IMGW = VA_CHUNK * VA_LDB;                      // one piece image of a chunk in LDS (bf16 elements)
constexpr int VA_STAGE_ELEMS = 3 * VA_CHUNK * VA_LDB;           // the staging buffer: three piece images (bf16 elements)

// vocabulary slices of a launch over R rows: ~4 workgroups per CU, whole chunks per slice
inline int va_slices(long R, int V) {
  const long tiles = (R + VA_ROWS - 1) / VA_ROWS;
  long ns = (4L * spacap::device_cus() + tiles - 1) / tiles;   // ~4 workgroups per CU
  const long most = (V + VA_CHUNK - 1) / VA_CHUNK;
  if (ns > most) ns = most;
  if (ns > 64) ns = 64;
  return (int)(ns < 1 ? 1 : ns);
}
inline int va_per_slice(int V, int ns) { return ((V + ns - 1) / ns + VA_CHUNK - 1) / VA_CHUNK * VA_CHUNK; }

}  // namespace spacap::decode

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
