// The ENet image encoder for gfx950 (MI355X): colour frames to the pixel-major feature maps that csrc/multiview.hip projects
// onto scene points.  Forward only; the network is frozen in the reference (lib/enet.py: create_enet without its classifier,
// scripts/compute_multiview_features.py runs it in eval()).  DESIGN.md section 7g.
//
// The network, as a table (every BatchNorm with eps = 0.001 and running statistics; "drop p" is the reference's Dropout2d,
// which in eval() is a multiplication by 1 - p):
//   initial    conv 3 -> 13, 3x3, stride 2, pad 1, bias  ||  maxpool 2x2 of the 3 input channels  -> 16 channels, BN, PReLU
//   stage 1    down 16 -> 64, then 4 x regular (dilation 1); inner width 16, drop 0.01
//   stage 2    down 64 -> 128, then regular 1, dilated 2, asymmetric, dilated 4, regular 1, dilated 8, asymmetric, dilated 16;
//              inner width 32, drop 0.1
//   stage 3    the same eight, without the down-sampling one
// One bottleneck (C_in -> C_out, inner width M = C_out / 4):
//   reduce     regular: 1x1 conv C_in -> M, no bias; down: 2x2 stride-2 conv (the map halves, rounding down); BN, PReLU
//   middle     3x3 conv M -> M, dilation d, pad d, bias; asymmetric: a 1x5 conv (pad 0,2; no bias) and a 5x1 conv (pad 2,0;
//              bias) with nothing between them; BN, PReLU
//   expand     1x1 conv M -> C_out, no bias; BN; drop p
//   skip       regular: the input; down: maxpool 2x2 stride 2 of the input, channels >= C_in are zero
//   out        PReLU(expand + skip)
//
// What the kernels see: BN and the drop constant are folded into conv weights and a bias on the host, in float64 (enet.py);
// the asymmetric middle is the exactly equal 5x5 conv W[o,i,ky,kx] = sum_m W2[o,m,ky] W1[m,i,kx], composed on the host.
// So every layer is   y = PReLU_a(conv_w(x) + b [+ skip]).
//
// Activations are pixel-major f32 [B][h w][C].  Three kernels:
//   enet_initial_kernel  one thread per output pixel, 27 x 13 products on the vector pipe (1.5 % of the network's work); the
//                        u8 variant normalises x = (u8 / 255 - mean) / std on the way in;
//   enet_reduce_kernel   the bottleneck's reduce -> the inner-width map [B][h w][M] in the workspace;
//   enet_main_kernel     middle conv -> bias -> PReLU -> expand -> bias -> skip -> PReLU; the inner-width result of the middle
//                        conv stays in the accumulator registers.
// Both bottleneck kernels run v_mfma_f32_16x16x4_f32 (MFMA16: fp32 products, fp32 accumulation) with 16 output channels on
// the A side, 16 output pixels on the B side and taps x input channels as the contraction.  A wave owns 16 consecutive pixels;
// lane (i = lane & 15, g = lane >> 4) reads FOUR consecutive channels 16 q + 4 g .. + 3 of its pixel (one 16-byte load) and of
// its weight row, and feeds element u of both to the u-th of four MFMAs: MFMA (q, u) contracts the channels {16 q + 4 g + u}.
// The order of a contraction is free as long as both operands agree, and this one makes the accumulator layout
// (lane holds channels 4 g .. 4 g + 3 of pixel i) the B operand of the next product as it is: the expand reads the middle
// conv's result out of its own registers, no LDS round trip, and every global access is 16 bytes.
// A tap outside the map contributes zeros (the load is predicated, nothing is read out of bounds); a tap outside for all 16
// pixels of the wave is skipped -- with dilation 16 on a 41 x 32 map that is most of them.
// The kernels wait on memory, not on the matrix pipe, so a wave issues every load of a round before its first product: the
// reduce its pixel's whole contraction row (templated on C_in for that), the middle conv all nine taps of a 3x3 or one row of
// five of a 5x5, the expand its skip rows (measured, DESIGN 7g: 7.3 -> 6.7 ms for 256 frames; more pixel tiles per wave with
// shared weight fragments gave nothing, and neither did the next bottleneck's reduce fused into the epilogue).
// A workgroup (4 waves, 64 pixels per round) stages the layer's weights in LDS once and walks the tiles of ONE image
// (blockIdx.y) with stride gridDim.x.  Plain loads and stores; no atomics, no host synchronisation, nothing depends on the
// order of workgroups: a pixel's value is the same whatever the batch or the grid.
#include "common.hpp"
#include "mfma.hpp"

namespace {

using namespace spacap::mfma;

enum { EN_REGULAR = 0, EN_ASYM = 1, EN_DOWN = 2 };
constexpr int EN_INITIAL_FLOATS = 480;   // w[16][27] (rows 13..15 unused), b[16], pool scale[16] (13..15 used), slope[16]
constexpr int EN_W0 = 0, EN_B0 = 432, EN_S0 = 448, EN_A0 = 464;
constexpr int EN_NLAYERS = 22;
// Workgroups of a bottleneck's launches.  Every workgroup stages its layer's weights (up to 121 KB) before its first tile, so
// the grid is about what the chip holds at once: two workgroups of a 128-wide layer per CU (55 KB of LDS each), four of a
// 64-wide one.  Measured at B = 256: 2 048 groups for every layer took 6.64 ms, these 5.7.
constexpr int EN_GROUPS_64 = 1024, EN_GROUPS_128 = 512;

struct EnLayer {
  int kind, cin, cout, dil;
};
constexpr EnLayer EN_LAYERS[EN_NLAYERS] = {
    {EN_DOWN, 16, 64, 1},     {EN_REGULAR, 64, 64, 1},   {EN_REGULAR, 64, 64, 1},   {EN_REGULAR, 64, 64, 1},
    {EN_REGULAR, 64, 64, 1},  {EN_DOWN, 64, 128, 1},     {EN_REGULAR, 128, 128, 1}, {EN_REGULAR, 128, 128, 2},
    {EN_ASYM, 128, 128, 1},   {EN_REGULAR, 128, 128, 4}, {EN_REGULAR, 128, 128, 1}, {EN_REGULAR, 128, 128, 8},
    {EN_ASYM, 128, 128, 1},   {EN_REGULAR, 128, 128, 16}, {EN_REGULAR, 128, 128, 1}, {EN_REGULAR, 128, 128, 2},
    {EN_ASYM, 128, 128, 1},   {EN_REGULAR, 128, 128, 4}, {EN_REGULAR, 128, 128, 1}, {EN_REGULAR, 128, 128, 8},
    {EN_ASYM, 128, 128, 1},   {EN_REGULAR, 128, 128, 16}};

// floats of one bottleneck in the packed buffer: w1[M][T1 C_in], b1[M], a1[M], w2[M][T2 M], b2[M], a2[M], w3[C_out][M],
// b3[C_out], a3[C_out]; T1 = 4 (down) or 1, T2 = 25 (asymmetric) or 9; a tap-major, channel-minor contraction index
struct EnOffsets {
  int M, K1, K2;
  size_t w1, b1, a1, w2, b2, a2, w3, b3, a3, total;
};
EnOffsets en_offsets(int kind, int cin, int cout) {
  EnOffsets o;
  o.M = cout / 4;
  o.K1 = (kind == EN_DOWN ? 4 : 1) * cin;
  o.K2 = (kind == EN_ASYM ? 25 : 9) * o.M;
  o.w1 = 0;
  o.b1 = o.w1 + (size_t)o.M * o.K1;
  o.a1 = o.b1 + o.M;
  o.w2 = o.a1 + o.M;
  o.b2 = o.w2 + (size_t)o.M * o.K2;
  o.a2 = o.b2 + o.M;
  o.w3 = o.a2 + o.M;
  o.b3 = o.w3 + (size_t)cout * o.M;
  o.a3 = o.b3 + cout;
  o.total = o.a3 + cout;
  return o;
}

__device__ __forceinline__ f32x4 prelu4(f32x4 v, f32x4 a) {
#pragma unroll
  for (int u = 0; u < 4; ++u) v[u] = v[u] > 0.f ? v[u] : a[u] * v[u];
  return v;
}
__device__ __forceinline__ f32x4 max4(f32x4 a, f32x4 b) {
#pragma unroll
  for (int u = 0; u < 4; ++u) a[u] = a[u] >= b[u] ? a[u] : b[u];
  return a;
}

// rows x K floats, contiguous in global memory, into an LDS image with row stride K + 4 (16-byte pieces; K % 4 == 0)
__device__ __forceinline__ void stage_rows(float *dst, const float *__restrict__ src, int rows, int K) {
  const int k4 = K >> 2;
  for (int i = threadIdx.x; i < rows * k4; i += blockDim.x) {
    const int r = i / k4, c = i - r * k4;
    st4(dst + r * (K + 4) + 4 * c, ld4(src + (size_t)i * 4));
  }
}

// ---- initial block ----------------------------------------------------------------------------------------------------------
struct EnNorm {
  float mean[3], std[3];
};

template <bool U8>
__global__ __launch_bounds__(256) void enet_initial_kernel(const void *__restrict__ images, int H, int W, EnNorm nm,
                                                           const float *__restrict__ prm, float *__restrict__ out) {
  const int ho = H >> 1, wo = W >> 1;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= ho * wo) return;
  const int y = p / wo, x = p - y * wo;
  const size_t img = (size_t)blockIdx.y * H * W * 3;
  float v[27];   // (ky, kx, c) of the 3x3 window at (2 y - 1, 2 x - 1); zeros outside the image
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int sy = 2 * y - 1 + ky, sx = 2 * x - 1 + kx;
      const bool ok = sy >= 0 && sy < H && sx >= 0 && sx < W;
      const size_t at = img + ((size_t)(ok ? sy : 0) * W + (ok ? sx : 0)) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float t = 0.f;
        if (ok) {
          if (U8) {
            t = (float)static_cast<const uint8_t *>(images)[at + c];
            t = (t / 255.0f - nm.mean[c]) / nm.std[c];
          } else {
            t = static_cast<const float *>(images)[at + c];
          }
        }
        v[(ky * 3 + kx) * 3 + c] = t;
      }
    }
  float o[16];
#pragma unroll
  for (int oc = 0; oc < 13; ++oc) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 27; ++j) acc = __builtin_fmaf(prm[EN_W0 + oc * 27 + j], v[j], acc);
    o[oc] = acc + prm[EN_B0 + oc];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {   // the pool's window is (2 y, 2 x) .. (2 y + 1, 2 x + 1): always inside (H, W even)
    const float m = fmaxf(fmaxf(v[12 + c], v[15 + c]), fmaxf(v[21 + c], v[24 + c]));
    o[13 + c] = m * prm[EN_S0 + 13 + c] + prm[EN_B0 + 13 + c];
  }
  float *dst = out + ((size_t)blockIdx.y * ho * wo + p) * 16;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f32x4 r;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float t = o[4 * q + u];
      r[u] = t > 0.f ? t : prm[EN_A0 + 4 * q + u] * t;
    }
    st4(dst + 4 * q, r);
  }
}

// ---- reduce: mid[b][p][M] = PReLU(conv(in)[p] + b1), 1x1 (stride 1) or 2x2 stride 2 ----------------------------------------------
struct EnReduceArgs {
  const float *in;    // [B][hin win][cin]
  float *mid;         // [B][ho wo][M]
  const float *w1, *b1, *a1;
  int win, cin, down, ho, wo;
  size_t in_image, mid_image;   // floats per image
};

template <int NT, int CIN, bool DOWN>   // M = 16 NT
__global__ __launch_bounds__(256) void enet_reduce_kernel(const EnReduceArgs a) {
  constexpr int M = 16 * NT, TAPS = DOWN ? 4 : 1, K1 = TAPS * CIN, LD = K1 + 4, Q = CIN / 16;
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  stage_rows(s_mem, a.w1, M, K1);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, lg = lane >> 4;
  const int hw = a.ho * a.wo, tiles = (hw + 63) >> 6, step = DOWN ? 2 : 1;
  const float *in = a.in + (size_t)blockIdx.y * a.in_image;
  float *mid = a.mid + (size_t)blockIdx.y * a.mid_image;
  f32x4 bias[NT], slope[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) bias[nt] = ld4(a.b1 + nt * 16 + 4 * lg), slope[nt] = ld4(a.a1 + nt * 16 + 4 * lg);
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int p = tile * 64 + wave * 16 + l15;
    const bool have = p < hw;
    const int y = have ? p / a.wo : 0, x = have ? p - y * a.wo : 0;
    // (the 2x2 window of a down-sampling reduce is inside the input: ho = floor(hin / 2))
    const float *src = in + ((size_t)(y * step) * a.win + x * step) * CIN + 4 * lg;
    f32x4 b[TAPS][Q];   // the pixel's whole contraction row: every load is in flight before the first product
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
      for (int q = 0; q < Q; ++q)
        b[t][q] = have ? ld4(src + ((size_t)(t >> 1) * a.win + (t & 1)) * CIN + 16 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
      for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const f32x4 w = ld4(s_mem + (nt * 16 + l15) * LD + t * CIN + 16 * q + 4 * lg);
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[nt] = MFMA16(w[u], b[t][q][u], acc[nt]);
        }
    if (have) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) st4(mid + (size_t)p * M + nt * 16 + 4 * lg, prelu4(acc[nt] + bias[nt], slope[nt]));
    }
  }
}

// ---- middle conv + expand + skip ------------------------------------------------------------------------------------------------
struct EnMainArgs {
  const float *mid;   // [B][h w][M]
  const float *in;    // the bottleneck's input: [B][h w][cout], or (down) [B][hin win][cin]
  float *out;         // [B][h w][cout]
  const float *w2, *b2, *a2, *w3, *b3, *a3;
  int h, w, dil, down, win, cin;
  size_t mid_image, in_image, out_image;
};

template <int NT, int KK>   // M = 16 NT, C_out = 64 NT; KK x KK taps
__global__ __launch_bounds__(256) void enet_main_kernel(const EnMainArgs a) {
  constexpr int M = 16 * NT, CO = 4 * M, K2 = KK * KK * M, LD2 = K2 + 4, LD3 = M + 4, OT = CO / 16;
  constexpr int GR = KK == 3 ? 3 : 1;   // kernel rows whose loads are issued together (3x3: all nine taps; 5x5: one row of five)
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  float *s_w2 = s_mem, *s_w3 = s_mem + M * LD2;
  stage_rows(s_w2, a.w2, M, K2);
  stage_rows(s_w3, a.w3, CO, M);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, lg = lane >> 4;
  const int hw = a.h * a.w, tiles = (hw + 63) >> 6;
  const float *mid = a.mid + (size_t)blockIdx.y * a.mid_image;
  const float *in = a.in + (size_t)blockIdx.y * a.in_image;
  float *out = a.out + (size_t)blockIdx.y * a.out_image;
  f32x4 bias2[NT], slope2[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) bias2[nt] = ld4(a.b2 + nt * 16 + 4 * lg), slope2[nt] = ld4(a.a2 + nt * 16 + 4 * lg);
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int p = tile * 64 + wave * 16 + l15;
    const bool have = p < hw;
    const int y = have ? p / a.w : 0, x = have ? p - y * a.w : 0;
    f32x4 t[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) t[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ky0 = 0; ky0 < KK; ky0 += GR) {
      f32x4 b[GR * KK][NT];
      bool ok[GR * KK];
#pragma unroll
      for (int j = 0; j < GR * KK; ++j) {
        const int sy = y + (ky0 + j / KK - KK / 2) * a.dil, sx = x + (j % KK - KK / 2) * a.dil;
        ok[j] = have && sy >= 0 && sy < a.h && sx >= 0 && sx < a.w;
        const float *src = mid + ((size_t)(ok[j] ? sy : 0) * a.w + (ok[j] ? sx : 0)) * M + 4 * lg;
#pragma unroll
        for (int q = 0; q < NT; ++q) b[j][q] = ok[j] ? ld4(src + 16 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < GR * KK; ++j) {
        if (__ballot(ok[j]) == 0ull) continue;   // outside for the whole wave (wave-uniform: the MFMAs below stay converged)
        const float *wr = s_w2 + l15 * LD2 + (ky0 * KK + j) * M + 4 * lg;
#pragma unroll
        for (int q = 0; q < NT; ++q)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const f32x4 w = ld4(wr + nt * 16 * LD2 + 16 * q);
#pragma unroll
            for (int u = 0; u < 4; ++u) t[nt] = MFMA16(w[u], b[j][q][u], t[nt]);
          }
      }
    }
    // t[nt][u] = channel 16 nt + 4 lg + u of pixel l15: the B operand of the expand as it stands
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) t[nt] = prelu4(t[nt] + bias2[nt], slope2[nt]);
    // the skip branch's loads go out before the expand's products
    f32x4 skip[OT];
#pragma unroll
    for (int ot = 0; ot < OT; ++ot) {
      const int c0 = ot * 16 + 4 * lg;
      skip[ot] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (have) {
        if (!a.down) {
          skip[ot] = ld4(in + (size_t)p * CO + c0);
        } else if (c0 < a.cin) {   // maxpool 2x2 stride 2 of the input; channels from cin on have no skip
          const float *s = in + ((size_t)(2 * y) * a.win + 2 * x) * a.cin + c0;
          skip[ot] = max4(max4(ld4(s), ld4(s + a.cin)), max4(ld4(s + (size_t)a.win * a.cin), ld4(s + (size_t)(a.win + 1) * a.cin)));
        }
      }
    }
#pragma unroll
    for (int ot = 0; ot < OT; ++ot) {
      const int c0 = ot * 16 + 4 * lg;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const f32x4 w = ld4(s_w3 + (ot * 16 + l15) * LD3 + nt * 16 + 4 * lg);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = MFMA16(w[u], t[nt][u], acc);
      }
      if (have) st4(out + (size_t)p * CO + c0, prelu4(acc + ld4(a.b3 + c0) + skip[ot], ld4(a.a3 + c0)));
    }
  }
}

constexpr int en_main_lds(int NT, int KK) { return (16 * NT * (KK * KK * 16 * NT + 4) + 64 * NT * (16 * NT + 4)) * (int)sizeof(float); }

int en_grid_x(int hw, int B, int target) {
  const int tiles = (hw + 63) / 64, want = (target + B - 1) / B;
  return tiles < want ? tiles : want;
}

template <int NT, int KK>
int en_launch_main(const char *what, const EnMainArgs &g, int B, int gx, hipStream_t stream) {
  static unsigned long long done = 0;
  constexpr int lds = en_main_lds(NT, KK);
  SPACAP_CHECK_HIP(spacap::allow_dynamic_lds(reinterpret_cast<const void *>(&enet_main_kernel<NT, KK>), lds, done), what);
  hipLaunchKernelGGL((enet_main_kernel<NT, KK>), dim3(gx, B), dim3(256), lds, stream, g);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

bool en_shape_ok(int kind, int cin, int cout) {
  if (kind == EN_REGULAR) return cin == cout && (cout == 64 || cout == 128);
  if (kind == EN_ASYM) return cin == cout && cout == 128;
  if (kind == EN_DOWN) return (cin == 16 && cout == 64) || (cin == 64 && cout == 128);
  return false;
}

// one bottleneck; every argument has been checked.  mid: B * ho * wo * (cout / 4) floats of workspace.
int en_bottleneck(const char *what, const float *in, int B, int h, int w, int cin, int cout, int kind, int dil,
                  const float *prm, float *mid, float *out, hipStream_t stream) {
  const EnOffsets o = en_offsets(kind, cin, cout);
  const int down = kind == EN_DOWN, ho = down ? h / 2 : h, wo = down ? w / 2 : w;
  EnReduceArgs r;
  r.in = in, r.mid = mid, r.w1 = prm + o.w1, r.b1 = prm + o.b1, r.a1 = prm + o.a1;
  r.win = w, r.cin = cin, r.down = down, r.ho = ho, r.wo = wo;
  r.in_image = (size_t)h * w * cin, r.mid_image = (size_t)ho * wo * o.M;
  const dim3 grid(en_grid_x(ho * wo, B, o.M == 16 ? EN_GROUPS_64 : EN_GROUPS_128), B);
  const int lds1 = o.M * (o.K1 + 4) * (int)sizeof(float);   // at most 32 x 260 floats
  if (cin == 16) hipLaunchKernelGGL((enet_reduce_kernel<1, 16, true>), grid, dim3(256), lds1, stream, r);
  else if (cin == 64 && down) hipLaunchKernelGGL((enet_reduce_kernel<2, 64, true>), grid, dim3(256), lds1, stream, r);
  else if (cin == 64) hipLaunchKernelGGL((enet_reduce_kernel<1, 64, false>), grid, dim3(256), lds1, stream, r);
  else hipLaunchKernelGGL((enet_reduce_kernel<2, 128, false>), grid, dim3(256), lds1, stream, r);
  SPACAP_CHECK_LAUNCH(what);
  EnMainArgs g;
  g.mid = mid, g.in = in, g.out = out;
  g.w2 = prm + o.w2, g.b2 = prm + o.b2, g.a2 = prm + o.a2, g.w3 = prm + o.w3, g.b3 = prm + o.b3, g.a3 = prm + o.a3;
  g.h = ho, g.w = wo, g.dil = kind == EN_ASYM ? 1 : dil, g.down = down, g.win = w, g.cin = cin;
  g.mid_image = r.mid_image, g.in_image = r.in_image, g.out_image = (size_t)ho * wo * cout;
  if (kind == EN_ASYM) return en_launch_main<2, 5>(what, g, B, grid.x, stream);
  if (o.M == 16) return en_launch_main<1, 3>(what, g, B, grid.x, stream);
  return en_launch_main<2, 3>(what, g, B, grid.x, stream);
}

int en_initial(const char *what, const void *images, bool u8, int B, int H, int W, EnNorm nm, const float *prm, float *out,
               hipStream_t stream) {
  const dim3 grid((unsigned)(((H / 2) * (W / 2) + 255) / 256), B);
  if (u8) hipLaunchKernelGGL(enet_initial_kernel<true>, grid, dim3(256), 0, stream, images, H, W, nm, prm, out);
  else hipLaunchKernelGGL(enet_initial_kernel<false>, grid, dim3(256), 0, stream, images, H, W, nm, prm, out);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

size_t en_params_total() {
  size_t n = EN_INITIAL_FLOATS;
  for (int i = 0; i < EN_NLAYERS; ++i) n += en_offsets(EN_LAYERS[i].kind, EN_LAYERS[i].cin, EN_LAYERS[i].cout).total;
  return n;
}

// the two activation buffers and the inner-width map of the whole encoder, in floats per image
void en_workspace_floats(int H, int W, size_t &act, size_t &mid) {
  const size_t h0 = H / 2, w0 = W / 2, h1 = h0 / 2, w1 = w0 / 2, h2 = h1 / 2, w2 = w1 / 2;
  act = h0 * w0 * 16;
  if (h1 * w1 * 64 > act) act = h1 * w1 * 64;
  if (h2 * w2 * 128 > act) act = h2 * w2 * 128;
  mid = h1 * w1 * 16 > h2 * w2 * 32 ? h1 * w1 * 16 : h2 * w2 * 32;
}

bool en_image_ok(int B, int H, int W) {
  return B >= 0 && B <= 65535 && H >= 8 && W >= 8 && H % 2 == 0 && W % 2 == 0 && (long long)H * W <= (1ll << 24);
}

int en_encode(const char *what, const void *images, bool u8, EnNorm nm, int B, int H, int W, const float *params, size_t n_params,
              void *workspace, size_t workspace_bytes, float *out, hipStream_t stream) {
  SPACAP_REQUIRE(en_image_ok(B, H, W), "%s: bad sizes (B=%d H=%d W=%d; 0 <= B <= 65535, H and W even, >= 8, H * W <= 2^24)", what,
                 B, H, W);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(images && params && workspace && out, "%s: null pointer", what);
  SPACAP_REQUIRE(n_params == en_params_total(), "%s: %zu parameters, %zu expected", what, n_params, en_params_total());
  SPACAP_REQUIRE(workspace_bytes >= spacap_enet_workspace_bytes(B, H, W), "%s: workspace of %zu bytes, %zu needed", what,
                 workspace_bytes, spacap_enet_workspace_bytes(B, H, W));
  SPACAP_REQUIRE(spacap::aligned16(params, static_cast<const float *>(workspace), out),
                 "%s: params, workspace and out must be 16-byte aligned", what);
  size_t act, midf;
  en_workspace_floats(H, W, act, midf);
  float *bufa = static_cast<float *>(workspace), *bufb = bufa + act * B, *mid = bufb + act * B;
  int rc = en_initial(what, images, u8, B, H, W, nm, params, bufa, stream);
  if (rc) return rc;
  const float *prm = params + EN_INITIAL_FLOATS;
  float *cur = bufa, *nxt = bufb;
  int h = H / 2, w = W / 2;
  for (int i = 0; i < EN_NLAYERS; ++i) {
    const EnLayer &L = EN_LAYERS[i];
    float *dst = i == EN_NLAYERS - 1 ? out : nxt;
    rc = en_bottleneck(what, cur, B, h, w, L.cin, L.cout, L.kind, L.dil, prm, mid, dst, stream);
    if (rc) return rc;
    if (L.kind == EN_DOWN) h /= 2, w /= 2;
    prm += en_offsets(L.kind, L.cin, L.cout).total;
    nxt = cur, cur = dst;
  }
  return SPACAP_OK;
}

}  // namespace

extern "C" size_t spacap_enet_param_floats(void) { return en_params_total(); }

extern "C" size_t spacap_enet_bottleneck_param_floats(int kind, int cin, int cout) {
  return en_shape_ok(kind, cin, cout) ? en_offsets(kind, cin, cout).total : 0;
}

extern "C" size_t spacap_enet_workspace_bytes(int B, int H, int W) {
  if (!en_image_ok(B, H, W)) return 0;
  size_t act, mid;
  en_workspace_floats(H, W, act, mid);
  return (2 * act + mid) * (size_t)B * sizeof(float);
}

extern "C" int spacap_enet_initial_f32(const float *images, int B, int H, int W, const float *params, float *out,
                                       spacap_stream_t stream) {
  const char *what = "spacap_enet_initial_f32";
  SPACAP_REQUIRE(en_image_ok(B, H, W), "%s: bad sizes (B=%d H=%d W=%d; 0 <= B <= 65535, H and W even, >= 8, H * W <= 2^24)", what,
                 B, H, W);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(images && params && out, "%s: null pointer", what);
  SPACAP_REQUIRE(spacap::aligned16(out), "%s: out must be 16-byte aligned", what);
  return en_initial(what, images, false, B, H, W, EnNorm{}, params, out, spacap::as_stream(stream));
}

extern "C" int spacap_enet_bottleneck_f32(const float *in, int B, int h, int w, int cin, int cout, int kind, int dilation,
                                          const float *params, void *workspace, size_t workspace_bytes, float *out,
                                          spacap_stream_t stream) {
  const char *what = "spacap_enet_bottleneck_f32";
  SPACAP_REQUIRE(B >= 0 && B <= 65535 && h >= 1 && w >= 1 && (long long)h * w <= (1ll << 24) && (kind != EN_DOWN || (h >= 2 && w >= 2)),
                 "%s: bad sizes (B=%d h=%d w=%d)", what, B, h, w);
  SPACAP_REQUIRE(en_shape_ok(kind, cin, cout) && dilation >= 1 && dilation <= 64,
                 "%s: kind=%d cin=%d cout=%d dilation=%d unsupported (kind 0 regular: 64->64, 128->128; 1 asymmetric: 128->128; "
                 "2 down: 16->64, 64->128; 1 <= dilation <= 64)", what, kind, cin, cout, dilation);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(in && params && workspace && out && in != out, "%s: null pointer (or in == out)", what);
  const int ho = kind == EN_DOWN ? h / 2 : h, wo = kind == EN_DOWN ? w / 2 : w;
  const size_t need = (size_t)B * ho * wo * (cout / 4) * sizeof(float);
  SPACAP_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, need);
  SPACAP_REQUIRE(spacap::aligned16(in, params, static_cast<const float *>(workspace), out),
                 "%s: in, params, workspace and out must be 16-byte aligned", what);
  return en_bottleneck(what, in, B, h, w, cin, cout, kind, dilation, params, static_cast<float *>(workspace), out,
                       spacap::as_stream(stream));
}

extern "C" int spacap_enet_encode_f32(const float *images, int B, int H, int W, const float *params, size_t n_params,
                                      void *workspace, size_t workspace_bytes, float *out, spacap_stream_t stream) {
  return en_encode("spacap_enet_encode_f32", images, false, EnNorm{}, B, H, W, params, n_params, workspace, workspace_bytes, out,
                   spacap::as_stream(stream));
}

extern "C" int spacap_enet_encode_u8(const uint8_t *images, int B, int H, int W, float mean0, float mean1, float mean2, float std0,
                                     float std1, float std2, const float *params, size_t n_params, void *workspace,
                                     size_t workspace_bytes, float *out, spacap_stream_t stream) {
  const EnNorm nm = {{mean0, mean1, mean2}, {std0, std1, std2}};
  return en_encode("spacap_enet_encode_u8", images, true, nm, B, H, W, params, n_params, workspace, workspace_bytes, out,
                   spacap::as_stream(stream));
}
