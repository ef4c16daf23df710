// Shared helpers for the gfx950 kernels of libspacap_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/spacap_hip.h"

namespace spacap {

// thread-local last-error text (defined in capi.hip)
void set_error(const char *fmt, ...);

inline hipStream_t as_stream(spacap_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Raises a kernel's dynamic-LDS limit on the CURRENT device.  `done` is the call site's own bit mask of devices that already
// have it (a function attribute is per device: a process that moves to another GPU must set it there too).
inline hipError_t allow_dynamic_lds(const void *fn, int bytes, unsigned long long &done) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const unsigned long long bit = 1ull << (dev & 63);
  if (done & bit) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done |= bit;
  return e;
}

// true when every pointer is 16-byte aligned (a null pointer counts as aligned: callers test for null themselves)
template <typename... P>
inline bool aligned16(const P *...p) {
  return ((... | reinterpret_cast<uintptr_t>(p)) & 15) == 0;
}

#define SPACAP_REQUIRE(cond, ...)          \
  do {                                     \
    if (!(cond)) {                         \
      ::spacap::set_error(__VA_ARGS__);    \
      return SPACAP_E_INVALID;             \
    }                                      \
  } while (0)

#define SPACAP_CHECK_LAUNCH(what)                                              \
  do {                                                                         \
    hipError_t e__ = hipGetLastError();                                        \
    if (e__ != hipSuccess) {                                                   \
      ::spacap::set_error("%s: %s", what, hipGetErrorString(e__));             \
      return SPACAP_E_LAUNCH;                                                  \
    }                                                                          \
  } while (0)

#define SPACAP_CHECK_HIP(expr, what)                                           \
  do {                                                                         \
    hipError_t e__ = (expr);                                                   \
    if (e__ != hipSuccess) {                                                   \
      ::spacap::set_error("%s: %s", what, hipGetErrorString(e__));             \
      return SPACAP_E_LAUNCH;                                                  \
    }                                                                          \
  } while (0)

// ---- wave64 cross-lane helpers (DPP: no LDS round trip) ----------------------------------
// dpp_ctrl encodings (CDNA ISA): quad_perm = 0x00..0xFF, row_mirror 0x140, row_half_mirror 0x141.
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false);
}

// max over the 64 lanes of a signed 32-bit value; result is wave-uniform (SGPR).
__device__ __forceinline__ int wave_max_i32(int v) {
  v = max(v, dpp_i32<0xB1>(v));   // quad_perm [1,0,3,2]  : lane ^ 1
  v = max(v, dpp_i32<0x4E>(v));   // quad_perm [2,3,0,1]  : lane ^ 2
  v = max(v, dpp_i32<0x141>(v));  // row_half_mirror      : folds 4-groups inside 8
  v = max(v, dpp_i32<0x140>(v));  // row_mirror           : folds 8-groups inside 16
  int r0 = __builtin_amdgcn_readlane(v, 0);
  int r1 = __builtin_amdgcn_readlane(v, 16);
  int r2 = __builtin_amdgcn_readlane(v, 32);
  int r3 = __builtin_amdgcn_readlane(v, 48);
  return max(max(r0, r1), max(r2, r3));
}

__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
  v = min(v, (unsigned)dpp_i32<0xB1>((int)v));
  v = min(v, (unsigned)dpp_i32<0x4E>((int)v));
  v = min(v, (unsigned)dpp_i32<0x141>((int)v));
  v = min(v, (unsigned)dpp_i32<0x140>((int)v));
  unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)v, 0);
  unsigned r1 = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
  unsigned r2 = (unsigned)__builtin_amdgcn_readlane((int)v, 32);
  unsigned r3 = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
  return min(min(r0, r1), min(r2, r3));
}

// Wave reductions with the DPP modifier ON the max / min itself (the helpers of common.hpp go through a v_mov_dpp: four
// instructions per step) and the two row_bcast steps instead of four readlanes: 6 steps, result from lane 63.  These sit
// on the serial chain of every sampling round.
__device__ __forceinline__ int wave_max_i32_fast(int v) {
  asm volatile("s_nop 1\n\t"
               "v_max_i32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_max_i32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_max_i32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_max_i32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_max_i32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"
               "v_max_i32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1"
               : "+v"(v));
  return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ unsigned wave_min_u32_fast(unsigned v) {
  asm volatile("s_nop 1\n\t"
               "v_min_u32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_min_u32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_min_u32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_min_u32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_min_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"
               "v_min_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1"
               : "+v"(v));
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// Reductions over W adjacent lanes (W = 64: the whole wave) by the xor-shuffle ladder, offsets W/2 .. 1 in that order;
// every lane ends up with the result.  float / double / int.
template <int W = 64, typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
template <int W = 64, typename T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
template <int W = 64, typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// ---- furthest point sampling: the reference's tie-break and its fminf (fps.hip, fps_bucket.inc, tools/lab) ----------------
// v_min_f32 without the canonicalising v_max hipcc emits in front of fminf (operands are never sNaN there); in IEEE mode
// it returns the non-NaN operand, i.e. the reference's fminf (sampling_gpu.cu:106).
__device__ __forceinline__ float vmin_f32(float a, float b) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// key(k) orders candidates the way the reference's shared-memory tree does (the lower slot wins at every level): among
// equal maxima the winner minimises (bitreverse_lg(k mod 2^lg), k div 2^lg); smaller key wins.
__device__ __forceinline__ unsigned fps_key(int k, int lg) {
  const unsigned low = (unsigned)k & ((1u << lg) - 1u);
  const unsigned rev = lg ? (__brev(low) >> (32 - lg)) : 0u;
  return (rev << 20) | ((unsigned)k >> lg);
}
__device__ __forceinline__ int fps_unkey(unsigned key, int lg) {
  const unsigned rev = key >> 20;
  const unsigned low = lg ? (__brev(rev) >> (32 - lg)) : 0u;
  return (int)(((key & 0xFFFFFu) << lg) | low);
}

// ---- training-mode BatchNorm of one channel from its fp64 (sum, sum of squares) over M elements, torch semantics ----------
// Two steps, because every caller stores its own statistics record between them: the biased variance, clamped at 0,
// normalises; the UNBIASED one goes into running_var.  The running statistics are optional in every entry point: callers
// skip bn_update_running when running_mean is null.  Inline on purpose: both compile under the including file's
// -ffp-contract flag, as the code they replaced did.
struct BnChannel {
  double mean, var;
  float istd;
};
__device__ __forceinline__ BnChannel bn_channel(double sum, double sumsq, double M, float eps) {
  const double mean = sum / M;
  double var = sumsq / M - mean * mean;
  if (var < 0.0) var = 0.0;
  return BnChannel{mean, var, (float)(1.0 / sqrt(var + (double)eps))};
}
__device__ __forceinline__ void bn_update_running(BnChannel bn, double M, float momentum, float *running_mean,
                                                  float *running_var, int c) {
  const double unbiased = M > 1.0 ? bn.var * M / (M - 1.0) : bn.var;
  running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * bn.mean);
  running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * unbiased);
}

}  // namespace spacap
