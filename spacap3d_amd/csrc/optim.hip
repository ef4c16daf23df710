// Grouped, clipped Adam over the flat parameter buffer for gfx950 (MI355X): the optimizer's second mode.
//
//   grad_sqnorm_kernel       : per-group partial sums of g^2 over the flat gradient bucket, float64, one slot per
//                              (workgroup, group) -- no floating-point atomics, no order that depends on timing
//   optim_finish_kernel      : one workgroup: partials -> sq[G+1], the norms, the clip coefficient, the apply flag, the
//                              step counter (advanced only when the update is applied) and the skipped-update counter
//   adam_flat_kernel_groups  : adam_flat_kernel (elementwise.hip) with lr / weight_decay read per group from a device
//                              table and the gradient scale multiplied by the clip coefficient; same expression order, so
//                              with one group, equal hyper-parameters and coef == 1 the result is that kernel's, bit for bit
//
// torch.optim.Adam([{non-caption}, {caption, lr: transformer_lr}], lr, weight_decay) of the reference (scripts/train.py:226-236)
// + torch.nn.utils.clip_grad_norm_ in three launches inside the captured step, none of which reads the host.
//
// Work split of the two passes over the bucket: workgroup b owns the CONTIGUOUS 16-byte pieces [b*chunk, (b+1)*chunk), so it
// crosses few segments; every thread bisects the segment table once for its first piece and then only walks forward.  Every
// segment starts on a 16-byte boundary (FlatGradBucket), so a piece never straddles two groups; padding elements are zero
// and belong to the segment before them.
#include "common.hpp"
#include "mfma.hpp"

namespace {

using namespace spacap;
using spacap::mfma::f32x4;

constexpr int MAXG = SPACAP_OPTIM_MAX_GROUPS, MAXS = SPACAP_OPTIM_MAX_SEGMENTS;

inline long pieces_of(long n) { return (n + 3) >> 2; }
inline unsigned blocks_for(long n) {
  long g = (pieces_of(n) + 255) / 256;
  if (g < 1) g = 1;
  if (g > 4096) g = 4096;
  return (unsigned)g;
}
inline long chunk_for(long n) {
  const long b = blocks_for(n);
  return (pieces_of(n) + b - 1) / b;
}

// the segment that holds element e: the last s with seg_off[s] <= e (0 <= e < seg_off[S]); reads stay inside [0, S)
__device__ __forceinline__ int find_segment(const long long *__restrict__ seg_off, int S, long e) {
  int lo = 0, hi = S;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg_off[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int advance_segment(const long long *__restrict__ seg_off, int S, int s, long e) {
  while (s + 1 < S && seg_off[s + 1] <= e) ++s;
  return s;
}
__device__ __forceinline__ int group_of(const int *__restrict__ seg_group, int s, int G) {
  const int k = seg_group[s];
  return k < 0 ? 0 : (k >= G ? G - 1 : k);   // (the host checked the table: this only keeps a corrupted one inside the arrays)
}

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const float *__restrict__ g, long n, long chunk,
                                                          const long long *__restrict__ seg_off,
                                                          const int *__restrict__ seg_group, int S, int G,
                                                          double *__restrict__ partials) {
  __shared__ double red[4][MAXG];
  const long np = (n + 3) >> 2;
  const long lo = (long)blockIdx.x * chunk;
  long hi = lo + chunk;
  if (hi > np) hi = np;
  double acc[MAXG];
#pragma unroll
  for (int k = 0; k < MAXG; ++k) acc[k] = 0.0;
  double cur = 0.0;    // the running sum of the group this thread is in: flushed into acc[] when the group changes
  int curg = 0;
  long i = lo + threadIdx.x;
  if (i < hi) {
    int s = find_segment(seg_off, S, 4 * i);
    curg = group_of(seg_group, s, G);
    for (; i < hi; i += 256) {
      s = advance_segment(seg_off, S, s, 4 * i);
      const int grp = group_of(seg_group, s, G);
      if (grp != curg) {
#pragma unroll
        for (int k = 0; k < MAXG; ++k) acc[k] += k == curg ? cur : 0.0;
        cur = 0.0;
        curg = grp;
      }
      if (4 * i + 4 <= n) {
        const f32x4 gv = *reinterpret_cast<const f32x4 *>(g + 4 * i);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double d = (double)gv[u];
          cur += d * d;     // (the product of two floats is exact in double)
        }
      } else {
        for (long e = 4 * i; e < n; ++e) {
          const double d = (double)g[e];
          cur += d * d;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < MAXG; ++k) acc[k] += k == curg ? cur : 0.0;
  // lanes by the xor ladder, then the four waves in index order: one fixed order for every run
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < MAXG; ++k) {
    if (k < G) {
      const double w = wave_sum<64>(acc[k]);
      if (lane == 0) red[wave][k] = w;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < G) {
    const int k = threadIdx.x;
    partials[(long)blockIdx.x * G + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

__global__ __launch_bounds__(256) void optim_finish_kernel(const double *__restrict__ partials, int blocks, int G,
                                                           float grad_scale,
                                                           const long long *__restrict__ skip_if_nonzero,
                                                           double *__restrict__ sq, float *__restrict__ ctrl,
                                                           long long *__restrict__ skipped) {
  __shared__ double col[MAXG][256];
  __shared__ double tot[MAXG];
  const int t = threadIdx.x;
  // thread t sums the workgroups t, t + 256, ... in index order; thread k then sums the 256 columns of group k in index order
  for (int k = 0; k < G; ++k) {
    double a = 0.0;
    for (int b = t; b < blocks; b += 256) a += partials[(long)b * G + k];
    col[k][t] = a;
  }
  __syncthreads();
  if (t < G) {
    double a = 0.0;
    for (int j = 0; j < 256; ++j) a += col[t][j];
    tot[t] = a;
    sq[t] = a;
    ctrl[SPACAP_OPTIM_CTRL_GROUP_NORM + t] = (float)((double)grad_scale * sqrt(a));
  }
  __syncthreads();
  if (t == 0) {
    double total = 0.0;
    for (int k = 0; k < G; ++k) total += tot[k];
    sq[G] = total;
    const double norm = (double)grad_scale * sqrt(total);
    ctrl[SPACAP_OPTIM_CTRL_NORM] = (float)norm;
    const bool finite = total - total == 0.0;     // false for inf and NaN
    const double max_norm = (double)ctrl[SPACAP_OPTIM_CTRL_MAX_NORM];
    double coef = 1.0;
    if (finite && max_norm > 0.0) {               // torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6))
      coef = max_norm / (norm + 1e-6);
      if (coef > 1.0) coef = 1.0;
    }
    ctrl[SPACAP_OPTIM_CTRL_COEF] = (float)coef;
    const bool blocked =
        skip_if_nonzero && __hip_atomic_load(skip_if_nonzero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    const bool apply = finite && !blocked;
    ctrl[SPACAP_OPTIM_CTRL_APPLY] = apply ? 1.0f : 0.0f;
    if (apply)
      ctrl[SPACAP_OPTIM_CTRL_STEP] += 1.0f;       // a skipped update never reaches Adam's bias correction
    else
      skipped[0] += 1;
  }
}

__global__ __launch_bounds__(256) void adam_flat_kernel_groups(float *__restrict__ p, const float *__restrict__ g,
                                                               float *__restrict__ m, float *__restrict__ v, long n,
                                                               long chunk, const long long *__restrict__ seg_off,
                                                               const int *__restrict__ seg_group, int S, int G,
                                                               const float *__restrict__ hyper, float b1, float b2,
                                                               float eps, const float *__restrict__ ctrl,
                                                               float grad_scale) {
  if (ctrl[SPACAP_OPTIM_CTRL_APPLY] == 0.0f) return;
  const float t = ctrl[SPACAP_OPTIM_CTRL_STEP];
  const float s = grad_scale * ctrl[SPACAP_OPTIM_CTRL_COEF];   // coef == 1: s == grad_scale exactly
  const float c1 = 1.0f - powf(b1, t), c2 = 1.0f - powf(b2, t);
  const float rs2 = 1.0f / sqrtf(c2);
  const long np = n >> 2;     // (n is a multiple of 4: the bucket pads every tensor to 16 bytes; checked by the entry point)
  const long lo = (long)blockIdx.x * chunk;
  long hi = lo + chunk;
  if (hi > np) hi = np;
  long i = lo + threadIdx.x;
  if (i >= hi) return;
  int seg = find_segment(seg_off, S, 4 * i);
  int curg = -1;
  float step_size = 0.f, wd = 0.f;
  for (; i < hi; i += 256) {
    seg = advance_segment(seg_off, S, seg, 4 * i);
    const int grp = group_of(seg_group, seg, G);
    if (grp != curg) {
      curg = grp;
      step_size = hyper[2 * grp] / c1;
      wd = hyper[2 * grp + 1];
    }
    f32x4 pv = *reinterpret_cast<f32x4 *>(p + 4 * i), mv = *reinterpret_cast<f32x4 *>(m + 4 * i),
          vv = *reinterpret_cast<f32x4 *>(v + 4 * i);
    const f32x4 gv = *reinterpret_cast<const f32x4 *>(g + 4 * i);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float gg = gv[u] * s + wd * pv[u];
      mv[u] = b1 * mv[u] + (1.0f - b1) * gg;
      vv[u] = b2 * vv[u] + (1.0f - b2) * gg * gg;
      pv[u] -= step_size * (mv[u] / (sqrtf(vv[u]) * rs2 + eps));
    }
    *reinterpret_cast<f32x4 *>(p + 4 * i) = pv;
    *reinterpret_cast<f32x4 *>(m + 4 * i) = mv;
    *reinterpret_cast<f32x4 *>(v + 4 * i) = vv;
  }
}

// the host-side copy of the segment table, when the caller hands one over: sorted, starting at 0, ending at n, every
// boundary but the last a multiple of 4 (16 bytes), every group inside [0, G)
const char *check_segments(const int64_t *off, const int32_t *grp, int S, int G, long n) {
  if (off) {
    if (off[0] != 0 || off[S] != n) return "segment table does not span [0, n)";
    for (int s = 0; s < S; ++s) {
      if (off[s] > off[s + 1]) return "segment offsets are not sorted";
      if (off[s] & 3) return "a segment does not start on a 16-byte boundary";
    }
  }
  if (grp)
    for (int s = 0; s < S; ++s)
      if (grp[s] < 0 || grp[s] >= G) return "a segment's group is outside [0, G)";
  return nullptr;
}

}  // namespace

#define OPTIM_TABLE_CHECKS(NAME)                                                                                     \
  SPACAP_REQUIRE(n >= 0, NAME ": bad size");                                                                         \
  SPACAP_REQUIRE(G >= 1 && G <= MAXG, NAME ": G=%d outside [1, %d]", G, MAXG);                                       \
  SPACAP_REQUIRE(S >= 1 && S <= MAXS, NAME ": S=%d outside [1, %d]", S, MAXS);                                       \
  {                                                                                                                  \
    const char *bad = check_segments(seg_off_host, seg_group_host, S, G, n);                                         \
    SPACAP_REQUIRE(!bad, NAME ": %s", bad);                                                                          \
  }

extern "C" int spacap_optim_blocks(long n) { return n < 0 ? 0 : (int)blocks_for(n); }

// g f32 [n] (16-byte aligned); seg_off i64 [S+1] / seg_group i32 [S] on the device (the *_host copies, nullable, are
// checked here); partials f64 [spacap_optim_blocks(n)][G]: every slot is written.
extern "C" int spacap_grad_sqnorm_f32(const float *g, long n, const int64_t *seg_off, const int32_t *seg_group, int S,
                                      int G, const int64_t *seg_off_host, const int32_t *seg_group_host,
                                      double *partials, spacap_stream_t stream) {
  OPTIM_TABLE_CHECKS("spacap_grad_sqnorm_f32")
  SPACAP_REQUIRE(seg_off && seg_group && partials && (g || n == 0), "spacap_grad_sqnorm_f32: null pointer");
  SPACAP_REQUIRE(aligned16(g), "spacap_grad_sqnorm_f32: unaligned pointer");
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(blocks_for(n)), dim3(256), 0, spacap::as_stream(stream), g, n, chunk_for(n),
                     reinterpret_cast<const long long *>(seg_off), seg_group, S, G, partials);
  SPACAP_CHECK_LAUNCH("spacap_grad_sqnorm_f32");
  return SPACAP_OK;
}

extern "C" int spacap_optim_finish_f64(const double *partials, int blocks, int G, float grad_scale,
                                       const int64_t *skip_if_nonzero, double *sq, float *ctrl, int64_t *skipped,
                                       spacap_stream_t stream) {
  SPACAP_REQUIRE(G >= 1 && G <= MAXG, "spacap_optim_finish_f64: G=%d outside [1, %d]", G, MAXG);
  SPACAP_REQUIRE(blocks >= 1 && blocks <= 4096, "spacap_optim_finish_f64: blocks=%d outside [1, 4096]", blocks);
  SPACAP_REQUIRE(partials && sq && ctrl && skipped, "spacap_optim_finish_f64: null pointer");
  hipLaunchKernelGGL(optim_finish_kernel, dim3(1), dim3(256), 0, spacap::as_stream(stream), partials, blocks, G, grad_scale,
                     reinterpret_cast<const long long *>(skip_if_nonzero), sq, ctrl, reinterpret_cast<long long *>(skipped));
  SPACAP_CHECK_LAUNCH("spacap_optim_finish_f64");
  return SPACAP_OK;
}

extern "C" int spacap_adam_flat_groups_f32(float *p, const float *g, float *m, float *v, long n, const int64_t *seg_off,
                                           const int32_t *seg_group, int S, int G, const int64_t *seg_off_host,
                                           const int32_t *seg_group_host, const float *hyper, float beta1, float beta2,
                                           float eps, const float *ctrl, float grad_scale, spacap_stream_t stream) {
  OPTIM_TABLE_CHECKS("spacap_adam_flat_groups_f32")
  SPACAP_REQUIRE((n & 3) == 0, "spacap_adam_flat_groups_f32: n=%ld is not a multiple of 4", n);
  if (n == 0) return SPACAP_OK;
  SPACAP_REQUIRE(p && g && m && v && seg_off && seg_group && hyper && ctrl, "spacap_adam_flat_groups_f32: null pointer");
  SPACAP_REQUIRE(aligned16(p, g, m, v), "spacap_adam_flat_groups_f32: unaligned pointer");
  hipLaunchKernelGGL(adam_flat_kernel_groups, dim3(blocks_for(n)), dim3(256), 0, spacap::as_stream(stream), p, g, m, v, n,
                     chunk_for(n), reinterpret_cast<const long long *>(seg_off), seg_group, S, G, hyper, beta1, beta2, eps,
                     ctrl, grad_scale);
  SPACAP_CHECK_LAUNCH("spacap_adam_flat_groups_f32");
  return SPACAP_OK;
}
