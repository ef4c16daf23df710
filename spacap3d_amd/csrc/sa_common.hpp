// Shared MLP of a set-abstraction module in point-major ("rows") layout, training mode, for gfx950 (MI355X): the data flow,
// and the device code that the forward and the backward kernels both inline.
//
// Replaces, for the training step, the chain the reference runs per SA module
// (lib/pointnet2/pointnet2_modules.py:241-259: QueryAndGroup -> SharedMLP -> max_pool2d, with SharedMLP =
// [Conv2d 1x1 -> BatchNorm2d -> ReLU] x 3, lib/pointnet2/pytorch_utils.py:11-36) on (B, C, npoint, nsample)
// tensors.  Same mathematics (fp32, batch statistics over all B*npoint*nsample positions, biased variance,
// eps inside the square root, first-maximum pooling), different data flow:
//
//   * rows r = (b, centre, sample) are the slow index, channels the fast one: every pass over an activation is one
//     contiguous stream, the 1x1 convolutions are row-major GEMMs on the matrix cores (v_mfma_f32_16x16x4_f32,
//     fp32 in / fp32 accumulate), and no NCHW <-> NHWC transposes exist;
//   * the first layer commutes with the grouping gather:  W1 [rel_xyz ; f(idx)] = Wx rel_xyz + (Wf f)(idx), so
//     Wf f is computed once per SOURCE point (8..16x fewer rows than grouped positions) and layer 1 is a gather
//     of that product plus a 3-term update (sa_l1_fwd_kernel);
//   * only the pre-activation z_k of every layer is stored; BatchNorm + ReLU of layer k are applied while the
//     tile is staged into LDS for layer k+1 (and again in the backward), and each layer's batch statistics are
//     accumulated in the epilogue of the GEMM that produces it -- one write and one read per activation in the
//     forward pass instead of write + 3 reads + write;
//   * the backward of max-pool -> ReLU -> BN is evaluated on the fly from (masked pooled gradient, argmax, z_k)
//     while staging the GEMM operands: dz_k = g dy + k0 - k1 z_k with per-channel constants (sa_bwd_finalize).
//
// Weights stay in registers for the whole kernel (each wave owns 16*NT output channels); the activation tile
// (64 rows) goes through LDS with a 4-word row padding, which makes the MFMA operand reads conflict-free.
// All reductions (statistics, weight gradients) are two-stage with a fixed order: no float atomics.
//
// One unit per pass, which share nothing but this header: sa_fwd.hip (forward kernels, with sa_bf3.inc), sa_bwd.hip (backward
// kernels, with sa_bf3_dgrad.inc and sa_l3bwd.inc) and sa_rows.hip (the inverted index of a grouping and what reads it).
// Everything here is a type, a constant, a macro or a __device__ __forceinline__ function, in the unnamed namespace the units'
// kernels live in (so that a kernel's name does not depend on which unit instantiates it).
#pragma once
#include <type_traits>

#include "common.hpp"
#include "launch.hpp"
#include "mfma.hpp"

namespace {
using namespace spacap::mfma;
using namespace spacap::launch;

constexpr int TM = 64;      // rows per tile of the forward / data-gradient GEMMs
constexpr int TW = 32;      // rows per tile of the weight-gradient GEMM
// NPART (launch.hpp, which caps every persistent grid at it): partial-sum rows of every statistics reduction

// stats row of a layer: {mean, 1/sqrt(var+eps), gamma/sqrt(var+eps), beta}
// coef  row of a layer (backward): {g, k0, k1, -}:  dz = g*dy + k0 - k1*z

// r / d for row indices: a 64-bit division is ~200 instructions on this chip and the first-layer passes paid two of them per
// row and thread; row counts fit 32 bits on the model's path (one 32-bit division, ~30 instructions), the general case stays
__device__ __forceinline__ long row_div(long r, long d) {
  if (((unsigned long long)r | (unsigned long long)d) >> 32) return r / d;
  return (long)((unsigned)r / (unsigned)d);
}

// ---- first layer: z1 of one grouped row ------------------------------------------------------------------------------------
// First-layer pre-activation of one grouped row for four channels: z = wx rx + wy ry + wz rz (+ wf f).  ONE definition for the
// statistics pass and for every pass that rebuilds z1 from the row's four inputs instead of reading it back (L1In): the values
// must agree bit for bit.  Both units are compiled with -ffp-contract=fast, so the rounding is whatever fused form the compiler
// picks for this expression; it is kept as the plain vector expression the original first-layer kernel had (the values the
// golden fixtures were recorded against -- spelling it out as separately rounded operations, or as an explicit fma chain,
// both changed them), and tests/test_sa_mlp_gpu.py::test_first_layer_rebuilt_instead_of_stored fails if any of the kernels
// that inline it should ever contract it differently.
__device__ __forceinline__ f32x4 l1_row(f32x4 wx, f32x4 wy, f32x4 wz, f32x4 wf, f32x4 in, bool has_feat) {
  f32x4 z = wx * in[0] + wy * in[1] + wz * in[2];
  if (has_feat) z += wf * in[3];
  return z;
}
// z_prev = the first layer's pre-activation rebuilt from rel4 [R][4] (relative x, y, z, inline feature) and W1 [C][ldw]
struct L1In {
  const float *W1;
  int ldw, has_feat;
};
__device__ __forceinline__ void l1_weights(const L1In &li, int c0, f32x4 &wx, f32x4 &wy, f32x4 &wz, f32x4 &wf) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float *w = li.W1 + (size_t)(c0 + u) * li.ldw;
    wx[u] = w[0], wy[u] = w[1], wz[u] = w[2];
    wf[u] = li.has_feat ? w[3] : 0.f;
  }
}

// ---- the same layer on the bf16 matrix cores with fp32-equivalent accuracy ("bf16 x 3") ---------------------------------
// fp32 MFMA runs at 1/16 of the bf16 MFMA rate on gfx950, which makes these 128-wide layers matrix-core bound.  Every fp32
// operand is split exactly into three bf16 pieces, x = x1 + x2 + x3 (x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2):
// 3 x 8 = 24 significant bits), and the product a*w is evaluated as the six bf16 products with weight >= 2^-16
//     a1 w1 + a1 w2 + a2 w1 + a2 w2 + a1 w3 + a3 w1        (dropped: a2 w3, a3 w2, a3 w3 <= 2^-24 |a w|)
// each exact in the fp32 accumulator of v_mfma_f32_32x32x16_bf16: 6/16 of the fp32-MFMA time for the same fp32-level result.
// The kernels are in sa_bf3.inc (forward layers, sa_fwd.hip) and sa_bf3_dgrad.inc (data gradient, sa_bwd.hip).  Earlier variants of this layer (a
// 32x32x2 fp32-MFMA kernel, an LDS-staged split-bf16 kernel, a streaming fp32 kernel, timing builds) are in the
// history (round 2, `git log -- tools/lab/sa_variants`), not in the tree.
// (split3 and the order of the six products: mfma.hpp; these kernels use the 32x32x16 form of the instruction)
using f32x16 = float __attribute__((ext_vector_type(16)));
#define MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ float dpp_xor1(float v) {   // value of lane ^ 1 (quad_perm [1, 0, 3, 2])
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpp_xor2(float v) {   // value of lane ^ 2 (quad_perm [2, 3, 0, 1])
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
}

}  // namespace
