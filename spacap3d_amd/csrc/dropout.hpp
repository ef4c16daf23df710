// The library's dropout keep mask: ONE definition for every kernel that draws it (elementwise.hip, tf_layer.hip,
// caption_prep.hip, mha.hip).  Every backward regenerates the mask instead of storing it, and the fused Transformer
// layer is tested against the composed operators at the same seed, so all of them must draw it bit for bit alike.
//
//   seed    = host word of the call + device-resident step counter * the 64-bit golden-ratio constant (mod 2^64; the
//             counter is optional: with it a replayed hipGraph draws new masks every step)
//   hash    = murmur3 fmix32 over the flat element index mixed with both halves of the seed
//   keep    iff thresh == 0 or hash >= thresh,  thresh = floor(p * 2^32);  kept values are scaled by 1 / (1 - p)
//             (torch.nn.Dropout semantics: keep with probability 1 - p)
#pragma once
#include <hip/hip_runtime.h>

namespace spacap {

struct DropSeed {
  unsigned lo, hi;
};

// formed once per kernel: a 64-bit finaliser per element would cost VALU time in every kernel that draws a mask
__device__ __forceinline__ DropSeed make_seed(unsigned long long seed, const unsigned long long *seed_dev) {
  const unsigned long long s = seed + (seed_dev ? *seed_dev * 0x9E3779B97F4A7C15ull : 0ull);
  return DropSeed{(unsigned)s, (unsigned)(s >> 32)};
}

__device__ __forceinline__ unsigned hash32(unsigned long long idx, DropSeed s) {
  unsigned h = (unsigned)idx ^ s.lo;
  h += ((unsigned)(idx >> 32) ^ s.hi) * 0x9E3779B1u;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// host side: false when p is outside [0, 1).  thresh == 0 means "no dropout"; the largest float p < 1, 1 - 2^-24, gives
// 2^32 - 256, so the conversion cannot overflow.
inline bool drop_params(float p, unsigned &thresh, float &scale) {
  if (!(p >= 0.f && p < 1.f)) return false;
  thresh = p > 0.f ? (unsigned)((double)p * 4294967296.0) : 0u;
  scale = 1.0f / (1.0f - p);
  return true;
}

}  // namespace spacap
