// The (proposal, object) pairs of a scene that self-critical training rewards, chosen on the device in one launch, for gfx950
// (MI355X).  DESIGN.md section 7k; the reference has no self-critical training, these semantics are the project's own and
// tests/scene_scst_restated.py restates them.
//
// One workgroup of four waves per scene.  Object slot j of scene b is a candidate when box_label_mask[b,j] > 0 and its key row
// key_table[dataset_idx[b]][scene_object_ids[b,j]] exists (an index outside the table, or an entry outside 0..nkeys-1: no row
// -- caption_row's rule, caption_eval.hip).  A wave takes a candidate, its lanes the proposals:
//   k_j = argmin_k d(b,k,j), first minimum;  d = ((x - cx)^2 + (z - cz)^2) + (y - cy)^2 in fp32, un-contracted (this unit is
//   compiled without contraction): cap_prep_fwd_kernel's expression, so a scene's referred object finds the proposal it finds
//   there.  A NaN distance is never a minimum; an object without a finite minimum does not qualify.
// The object qualifies when d_j < near2, strictly.  The qualifying objects are ranked by (d_j, j) ascending: the rank of an
// object is the number of qualifying objects in front of it (G^2 comparisons at most, G <= 256: no sort), the first M fill the
// slots 0 .. M-1, the rest of the slots are written empty.  Two objects may share a proposal.  No atomics, no state: a captured
// call replays.
#include <math.h>

#include "common.hpp"

namespace {

using namespace spacap;

constexpr int SEL_THREADS = 256, SEL_WAVES = SEL_THREADS / 64, SEL_GMAX = 256;

struct SelectArgs {
  const float *xyz, *center, *label_mask;
  const long long *object_ids, *dataset_idx;
  const int *key_table;
  int B, K, G, M, n_items, n_obj, nkeys;
  float near2;
  long long *prop, *obj;
  int *slot_of, *key;
  float *dist;
  int *n_sel;
};

__global__ __launch_bounds__(SEL_THREADS) void scst_select_kernel(SelectArgs a) {
  __shared__ float s_d[SEL_GMAX];
  __shared__ int s_k[SEL_GMAX], s_key[SEL_GMAX];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, G = a.G, M = a.M;
  const long long item = a.dataset_idx[b];
  // ---- per object slot, all at once: the key row (s_key < 0: no candidate) ----
  if (tid < G) {
    int row = -1;
    if (a.label_mask[(size_t)b * G + tid] > 0.f && item >= 0 && item < a.n_items) {
      const long long oid = a.object_ids[(size_t)b * G + tid];
      if (oid >= 0 && oid < a.n_obj) {
        row = a.key_table[(size_t)item * a.n_obj + oid];
        if (row < 0 || row >= a.nkeys) row = -1;
      }
    }
    s_key[tid] = row;
  }
  __syncthreads();
  // ---- per candidate, a wave each: the nearest proposal, whether it is near enough (s_key < 0 afterwards: does not qualify) ----
  for (int j = wave; j < G; j += SEL_WAVES) {   // (uniform over the wave)
    const int row = s_key[j];
    float best = INFINITY;
    int bk = 0x7fffffff;
    if (row >= 0) {
      const float *c = a.center + ((size_t)b * G + j) * 3;
      const float cx = c[0], cy = c[1], cz = c[2];
      for (int k = lane; k < a.K; k += 64) {
        const float *p = a.xyz + ((size_t)b * a.K + k) * 3;
        const float dx = p[0] - cx, dy = p[1] - cy, dz = p[2] - cz;
        const float d = (dx * dx + dz * dz) + dy * dy;
        if (d < best) best = d, bk = k;          // k ascends: the lane keeps its first minimum; NaN is never smaller
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const float d2 = __shfl_xor(best, o);
        const int k2 = __shfl_xor(bk, o);
        if (d2 < best || (d2 == best && k2 < bk)) best = d2, bk = k2;
      }
    }
    if (lane == 0) {
      const bool q = row >= 0 && bk != 0x7fffffff && best < a.near2;
      s_d[j] = best, s_k[j] = bk, s_key[j] = q ? row : -1;
    }
  }
  __syncthreads();
  // ---- ranks: thread j counts the qualifying objects in front of object j ----
  const bool mine = tid < G && s_key[tid] >= 0;
  int rank = 0;
  if (mine) {
    const float d = s_d[tid];
    for (int i = 0; i < G; ++i) {
      const float di = s_d[i];
      rank += (s_key[i] >= 0 && (di < d || (di == d && i < tid))) ? 1 : 0;
    }
  }
  const int n = min(__syncthreads_count(mine), M);
  if (mine && rank < M) {
    const size_t o = (size_t)b * M + rank;
    a.prop[o] = s_k[tid];
    a.obj[o] = a.object_ids[(size_t)b * G + tid];
    a.slot_of[o] = tid;
    a.key[o] = s_key[tid];
    a.dist[o] = s_d[tid];
  }
  if (tid >= n && tid < M) {   // (M <= G <= 256 threads: one empty slot each)
    const size_t o = (size_t)b * M + tid;
    a.prop[o] = -1, a.obj[o] = -1, a.slot_of[o] = -1, a.key[o] = -1, a.dist[o] = INFINITY;
  }
  if (tid == 0) a.n_sel[b] = n;
}

}  // namespace

extern "C" int spacap_scst_select_f32(const float *xyz, const float *center_label, const float *box_label_mask,
                                      const int64_t *scene_object_ids, const int64_t *dataset_idx, const int32_t *key_table,
                                      int B, int K, int G, int M, int n_items, int n_obj, int nkeys, float near2, int64_t *prop,
                                      int64_t *obj, int32_t *slot_of, int32_t *key, float *dist, int32_t *n_sel,
                                      spacap_stream_t stream) {
  const char *what = "spacap_scst_select_f32";
  SPACAP_REQUIRE(B >= 0 && K >= 1 && G >= 1 && G <= SEL_GMAX && M >= 1 && M <= G && n_items >= 0 && n_obj >= 0 && nkeys >= 0,
                 "%s: bad arguments (K=%d >= 1, 1 <= G=%d <= %d, 1 <= M=%d <= G)", what, K, G, SEL_GMAX, M);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(xyz && center_label && box_label_mask && scene_object_ids && dataset_idx && prop && obj && slot_of && key && dist &&
                     n_sel && (key_table || (size_t)n_items * n_obj == 0),
                 "%s: null pointer", what);
  SelectArgs a;
  a.xyz = xyz, a.center = center_label, a.label_mask = box_label_mask;
  a.object_ids = reinterpret_cast<const long long *>(scene_object_ids), a.dataset_idx = reinterpret_cast<const long long *>(dataset_idx);
  a.key_table = key_table;
  a.B = B, a.K = K, a.G = G, a.M = M, a.n_items = n_items, a.n_obj = n_obj, a.nkeys = nkeys, a.near2 = near2;
  a.prop = reinterpret_cast<long long *>(prop), a.obj = reinterpret_cast<long long *>(obj);
  a.slot_of = slot_of, a.key = key, a.dist = dist, a.n_sel = n_sel;
  hipLaunchKernelGGL(scst_select_kernel, dim3(B), dim3(SEL_THREADS), 0, spacap::as_stream(stream), a);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
