// What a NaN does in ReLU and in the max over a group: one definition for bn_relu.hip and group_max.hip, taken from the
// composition they replace (BatchNorm -> ReLU -> F.max_pool2d).  A diverged channel (one NaN or Inf makes its statistics, and
// with them every pre-activation, NaN) must come out as NaN, not as a clean 0: nothing downstream checks for finiteness.
// On finite inputs each of these returns, bit for bit, what fmaxf / a plain `>` would.
#pragma once

namespace spacap {

// relu(v) as torch's clamp_min(0): 0 for v <= 0 (either zero gives +0, as v_max_f32 does), v itself otherwise -- NaN included,
// which fmaxf(v, 0) would turn into 0.
__device__ __forceinline__ float relu_keep_nan(float v) { return !(v <= 0.f) ? v : 0.f; }

// whether the ReLU's gradient passes at pre-activation v: wherever the output is not <= 0 (threshold_backward), so also at NaN
__device__ __forceinline__ bool relu_passes(float v) { return !(v <= 0.f); }

// candidate (v, i) replaces (bv, bi) as the maximum of a group: larger value, NaN beats non-NaN, ties / NaN-NaN keep the lower index
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;
  if (vn) return i < bi;
  return v > bv || (v == bv && i < bi);
}

}  // namespace spacap
