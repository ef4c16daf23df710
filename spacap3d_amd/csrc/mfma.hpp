// Matrix-core primitives shared by the gfx950 kernels of libspacap_hip.so: the vector types, the two MFMA forms the library
// uses, 16-byte loads and stores, and the split-bf16 device -- ONE definition of the split and of the
// order of the six piece products, which is what the "fp32-equivalent products" claim rests on.
// The claim is held per kernel and per term by tests/test_split_bf16_terms_gpu.py: every kernel that runs this table (through
// mfma6 or a loop of its own over PA / PB, with its own piece images and fragment reads) is given inputs on which ONE of the three
// 2^-16 products (a0 b2, a2 b0, a1 b1) is positive in every summand, and must stay under a quarter of that term's share of
// sum |a| |b|.  On random operands a lost 2^-16 term averages out of a max-norm; there it cannot.  A kernel that gains a copy of
// the loop gains a probe there (tests/split_bf16_restated.py: CASES).
// Everything here is a type, a constant, a macro or a __device__ __forceinline__ function; users say
// `using namespace spacap::mfma;` inside their own namespace.
#pragma once
#include <hip/hip_runtime.h>

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)    // fp32 in, fp32 accumulate
#define MFMA_B(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)  // bf16 in, fp32 accumulate

namespace spacap {
namespace mfma {

using f32x4 = float __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// ---- split-bf16 operands: x = x0 + x1 + x2 exactly (x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1): 3 x 8 = 24
// significant bits; every conversion rounds to nearest even) ----------------------------------------------------------------
__device__ __forceinline__ void split3(float v, __bf16 &h, __bf16 &m, __bf16 &l) {
  h = (__bf16)v;
  const float r = v - (float)h;
  m = (__bf16)r;
  l = (__bf16)(r - (float)m);
}
__device__ __forceinline__ void split4(f32x4 v, bf16x4 &p0, bf16x4 &p1, bf16x4 &p2) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const __bf16 h = (__bf16)v[u];
    const float r = v[u] - (float)h;
    const __bf16 m = (__bf16)r;
    p0[u] = h, p1[u] = m, p2[u] = (__bf16)(r - (float)m);
  }
}
__device__ __forceinline__ void split8(f32x4 lo, f32x4 hi, bf16x8 *p) {
  bf16x4 a[3], c[3];
  split4(lo, a[0], a[1], a[2]);
  split4(hi, c[0], c[1], c[2]);
#pragma unroll
  for (int q = 0; q < 3; ++q) p[q] = bf16x8{a[q][0], a[q][1], a[q][2], a[q][3], c[q][0], c[q][1], c[q][2], c[q][3]};
}

// A product a * b = the six piece products whose weight is above 2^-24 (dropped: a1 b2, a2 b1, a2 b2), each exact in the fp32
// accumulator, added smallest terms first: product q takes piece PA[q] of a and piece PB[q] of b (piece 0 = the leading bf16).
// Kernels that interleave the six with other work or alternate accumulators run their own loop over this table.
constexpr int PA[6] = {0, 2, 1, 0, 1, 0}, PB[6] = {2, 0, 1, 1, 0, 0};
__device__ __forceinline__ f32x4 mfma6(const bf16x8 *a, const bf16x8 *b, f32x4 acc) {
#pragma unroll
  for (int q = 0; q < 6; ++q) acc = MFMA_B(a[PA[q]], b[PB[q]], acc);
  return acc;
}

// 16x16x32 operand fragment out of a row-major bf16 LDS image [contraction index][LD columns] through ds_read_b64_tr_b16, the
// transposing LDS read of gfx950: the 16 outer indices are the image columns c0 .. c0 + 15, the contraction index the image's
// 32 rows.  Lane (g = lane >> 4, i = lane & 15) gets rows 8 g .. 8 g + 7 of column c0 + i (two reads of 4 rows each; lane
// 4 q + p of a group supplies the address of row q, columns 4 p .. 4 p + 3 of the 4 x 16 block).
template <int LD>
__device__ __forceinline__ bf16x8 tr_frag(const __bf16 *img, int c0, int lane) {
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const __bf16 *a = img + (8 * g + q) * LD + c0 + 4 * p;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(a));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(a + 4 * LD));
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

}  // namespace mfma
}  // namespace spacap
