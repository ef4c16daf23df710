// Evaluation post-processing of the detector's proposals for gfx950 (MI355X): the per-batch host work of the reference's
// lib/ap_helper.py:45-160 (parse_predictions) and lib/eval_helper.py:146-177 (feed_scene_cap) on the device.
//
//  1. points_in_box_kernel: how many points of the scene lie in each proposal box (data/scannet/model_util_scannet.py:13-22,
//     a scipy Delaunay hull of the 8 corners tested against every point; "empty" = fewer than 5 points).  The boxes this
//     model decodes are axis-aligned (heading 0, NUM_HEADING_BIN = 1), so the hull IS the corners' axis-aligned bounding box
//     and the test is a closed-box test.  It is exact in f32: each f64 bound is rounded to the nearest float on the inside
//     (lo_f = smallest float >= lo, hi_f = largest float <= hi), so `p >= lo_f` is `(double)p >= lo` for every f32 p.
//     Grid (ceil(N / 1024), B), 256 threads, four points per thread in registers; the scene's K bounds in LDS (every lane
//     reads the same box: broadcast); per box one ballot + popcount per wave, a cross-wave sum in LDS and ONE plain store
//     per (workgroup, box) into a partial-count slab [B, nchunk, K].  No atomics, no memset: deterministic and capturable.
//  2. detection_nms_kernel: one workgroup of 512 threads per scene (one thread per proposal, K <= 512): sums the slab,
//     objectness softmax, class-aware 3D NMS (utils/nms.py:110-150 / 77-108) with the reference's arithmetic in f64, the
//     confidence table and the IoU against the assigned ground-truth box (utils/box_util.py:183-209).
//     Order: descending obj_prob by rank counting; equal probabilities put the HIGHER proposal index first (numpy's
//     quicksort leaves the order of ties unspecified), NaN ranks ahead of every number (np.argsort sorts NaN last).
//     Suppression: a K x K bit matrix in LDS in rank order (row r = what the r-th box suppresses among the boxes behind
//     it), then one wave runs the greedy scan, each of lanes 0..7 holding one 64-bit word of the "removed" set.
//
// Arithmetic: -ffp-contract=off (Makefile), plain IEEE f64 division in the overlap tests (no reciprocal, no rewrite as
// inter > thr * denom: the two differ at the boundary).  The two softmaxes use a correctly rounded exp (f64 exp rounded to
// f32) and numpy's summation order; numpy's own f32 exp is not correctly rounded, so probabilities agree with numpy's to a
// few ulp, not bit for bit.
#include <math.h>

#include "eval_common.hpp"

namespace {

using namespace spacap::eval;

constexpr int PIB_THREADS = 256;
constexpr int PIB_PPT = 4;                          // points per thread
constexpr int PIB_POINTS = PIB_THREADS * PIB_PPT;   // points per workgroup (one slab row)
constexpr int PP_MAXK = 512;
constexpr int PP_WORDS = PP_MAXK / 64;
constexpr int PP_MAXNC = 128;                       // numpy's pairwise-sum block: one block = its 8-accumulator order

__global__ __launch_bounds__(PIB_THREADS) void points_in_box_kernel(const float *__restrict__ pc, int N, int C,
                                                                      const double *__restrict__ corners, int K, int nchunk,
                                                                      int32_t *__restrict__ slab) {
  __shared__ float s_b[6][PP_MAXK];                     // lo x, y, z, hi x, y, z (rounded inwards)
  __shared__ int s_c[PIB_THREADS / 64][PP_MAXK];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
  for (int k = tid; k < K; k += PIB_THREADS) {
    double lo[3], hi[3];
    box_bounds(corners + ((size_t)b * K + k) * 24, lo, hi);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      float l = (float)lo[d], h = (float)hi[d];
      if ((double)l < lo[d]) l = nextafterf(l, INFINITY);
      if ((double)h > hi[d]) h = nextafterf(h, -INFINITY);
      s_b[d][k] = l;
      s_b[3 + d][k] = h;
    }
  }
  float px[PIB_PPT], py[PIB_PPT], pz[PIB_PPT];
  bool ok[PIB_PPT];
#pragma unroll
  for (int i = 0; i < PIB_PPT; ++i) {
    const int n = chunk * PIB_POINTS + i * PIB_THREADS + tid;
    ok[i] = n < N;
    const float *p = pc + ((size_t)b * N + (ok[i] ? n : 0)) * C;
    px[i] = p[0];
    py[i] = p[1];
    pz[i] = p[2];
  }
  __syncthreads();
  for (int k = 0; k < K; ++k) {
    const float lx = s_b[0][k], ly = s_b[1][k], lz = s_b[2][k], hx = s_b[3][k], hy = s_b[4][k], hz = s_b[5][k];
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < PIB_PPT; ++i) {
      const bool in = ok[i] && px[i] >= lx && px[i] <= hx && py[i] >= ly && py[i] <= hy && pz[i] >= lz && pz[i] <= hz;
      cnt += __popcll(__ballot(in));
    }
    if ((tid & 63) == 0) s_c[wave][k] = cnt;
  }
  __syncthreads();
  for (int k = tid; k < K; k += PIB_THREADS) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < PIB_THREADS / 64; ++w) s += s_c[w][k];
    slab[((size_t)b * nchunk + chunk) * K + k] = s;
  }
}

// correctly rounded f32 exp (see the file header)
__device__ __forceinline__ float exp_cr(float x) { return (float)exp((double)x); }

// does proposal j come before proposal k in the NMS order?  (descending probability, NaN first, ties: higher index first)
__device__ __forceinline__ bool ahead(float pj, int j, float pk, int k) {
  const bool nj = pj != pj, nk = pk != pk;
  if (nj != nk) return nj;
  if (!nj && pj != pk) return pj > pk;
  return j > k;
}

struct NmsArgs {
  const float *objectness;      // [B,K,2]
  const int64_t *sem_cls;       // [B,K]
  const float *sem_cls_scores;  // [B,K,NC] or null
  const double *corners;        // [B,K,8,3]
  const int32_t *slab;          // [B,nchunk,K]
  const double *gt_corners;     // [B,M,8,3] or null
  const int64_t *assignment;    // [B,K]
  int K, NC, nchunk, M, flags, min_points;
  double nms_iou, min_iou;
  float conf_thresh;
  float *obj_prob;
  int32_t *count;
  uint8_t *nonempty, *pred_mask, *valid;
  float *conf;
  double *iou;
  uint8_t *good;
};

__global__ __launch_bounds__(PP_MAXK) void detection_nms_kernel(NmsArgs a) {
  __shared__ double s_bnd[6][PP_MAXK];               // x1 y1 z1 x2 y2 z2 (f64, as utils/nms.py builds them)
  __shared__ uint64_t s_sup[PP_MAXK][PP_WORDS];      // rank-space suppression bits
  __shared__ long long s_cls[PP_MAXK];
  __shared__ float s_prob[PP_MAXK];
  __shared__ unsigned short s_order[PP_MAXK];        // rank -> proposal
  __shared__ uint8_t s_ne[PP_MAXK];
  __shared__ uint64_t s_removed[PP_WORDS];
  const int b = blockIdx.x, k = threadIdx.x, K = a.K;
  const bool act = k < K;
  const size_t p = (size_t)b * K + k;
  const bool cls_nms = a.flags & SPACAP_PP_CLS_NMS, old_type = a.flags & SPACAP_PP_OLD_TYPE;

  float prob = 0.f;
  bool ne = false;
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  if (act) {
    // lib/ap_helper.py:37-42 softmax(...)[:, :, 1]: exp(x - max) / sum
    const float x0 = a.objectness[p * 2], x1 = a.objectness[p * 2 + 1];
    const float m = x0 > x1 ? x0 : x1;
    const float e0 = exp_cr(x0 - m), e1 = exp_cr(x1 - m);
    prob = e1 / (e0 + e1);
    int cnt = 0;
    for (int c = 0; c < a.nchunk; ++c) cnt += a.slab[((size_t)b * a.nchunk + c) * K + k];
    ne = (a.flags & SPACAP_PP_REMOVE_EMPTY) ? cnt >= a.min_points : true;
    box_bounds(a.corners + p * 24, lo, hi);
    a.obj_prob[p] = prob;
    a.count[p] = cnt;
    a.nonempty[p] = ne ? 1 : 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      s_bnd[d][k] = lo[d];
      s_bnd[3 + d][k] = hi[d];
    }
    s_cls[k] = (long long)a.sem_cls[p];
    s_prob[k] = prob;
    s_ne[k] = ne ? 1 : 0;

    if (a.sem_cls_scores) {
      // softmax over the classes (f32, numpy's pairwise order for n <= 128: 8 accumulators, then the tail) times obj_prob
      const float *s = a.sem_cls_scores + p * a.NC;
      float *out = a.conf + p * a.NC;
      float mx = s[0];
      for (int j = 1; j < a.NC; ++j) mx = s[j] > mx ? s[j] : mx;
      float sum = 0.f;
      if (a.NC < 8) {
        for (int j = 0; j < a.NC; ++j) sum += exp_cr(s[j] - mx);
      } else {
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = exp_cr(s[j] - mx);
        int j = 8;
        for (; j < a.NC - (a.NC % 8); j += 8)
#pragma unroll
          for (int q = 0; q < 8; ++q) r[q] += exp_cr(s[j + q] - mx);
        sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; j < a.NC; ++j) sum += exp_cr(s[j] - mx);
      }
      for (int j = 0; j < a.NC; ++j) out[j] = (exp_cr(s[j] - mx) / sum) * prob;
    }

    if (a.gt_corners) {
      // utils/box_util.py:183-209 box3d_iou_batch_tensor(assigned gt corners, detected corners), same operation order
      const long long g = a.assignment[p];
      double iou = NAN;
      if (g >= 0 && g < a.M) {
        double glo[3], ghi[3];
        box_bounds(a.gt_corners + ((size_t)b * a.M + g) * 24, glo, ghi);
        double e[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const double A = glo[d] > lo[d] ? glo[d] : lo[d];
          const double B = ghi[d] < hi[d] ? ghi[d] : hi[d];
          const double w = B - A;
          e[d] = (w > 0.0 || w != w) ? w : 0.0;      // torch.max(., zeros) propagates NaN
        }
        const double inter = e[0] * e[1] * e[2];
        double vol1;
        if (a.flags & SPACAP_PP_GT_F32)   // the reference's dataset labels are f32: their volume is an f32 product
          vol1 = (double)(((float)ghi[0] - (float)glo[0]) * ((float)ghi[1] - (float)glo[1]) * ((float)ghi[2] - (float)glo[2]));
        else
          vol1 = (ghi[0] - glo[0]) * (ghi[1] - glo[1]) * (ghi[2] - glo[2]);
        const double vol2 = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]);
        iou = inter / (vol1 + vol2 - inter + 1e-8);
      }
      a.iou[p] = iou;
      a.good[p] = iou > a.min_iou ? 1 : 0;
    }
  }
  __syncthreads();

  // ranks among the non-empty proposals (empty ones take no part in the suppression, lib/ap_helper.py:128-132)
  int rank = 0;
  if (act && ne)
    for (int j = 0; j < K; ++j) rank += (s_ne[j] && ahead(s_prob[j], j, prob, k)) ? 1 : 0;
  const int Mne = __syncthreads_count(act && ne);
  if (act && ne) s_order[rank] = (unsigned short)k;
  __syncthreads();

  // suppression bits: row r, word w covers ranks 64w .. 64w+63; bit set when the r-th box suppresses a box behind it
  const double thr = a.nms_iou;
  for (int item = k; item < Mne * PP_WORDS; item += PP_MAXK) {
    const int r = item / PP_WORDS, w = item % PP_WORDS;
    const int c0 = max(w * 64, r + 1), c1 = min(w * 64 + 64, Mne);
    uint64_t bits = 0;
    if (c0 < c1) {
      const int i = s_order[r];
      const double ix1 = s_bnd[0][i], iy1 = s_bnd[1][i], iz1 = s_bnd[2][i];
      const double ix2 = s_bnd[3][i], iy2 = s_bnd[4][i], iz2 = s_bnd[5][i];
      const double area_i = (ix2 - ix1) * (iy2 - iy1) * (iz2 - iz1);
      const long long ci = s_cls[i];
      for (int c = c0; c < c1; ++c) {
        const int j = s_order[c];
        const double jx1 = s_bnd[0][j], jy1 = s_bnd[1][j], jz1 = s_bnd[2][j];
        const double jx2 = s_bnd[3][j], jy2 = s_bnd[4][j], jz2 = s_bnd[5][j];
        const double xx1 = ix1 > jx1 ? ix1 : jx1, yy1 = iy1 > jy1 ? iy1 : jy1, zz1 = iz1 > jz1 ? iz1 : jz1;
        const double xx2 = ix2 < jx2 ? ix2 : jx2, yy2 = iy2 < jy2 ? iy2 : jy2, zz2 = iz2 < jz2 ? iz2 : jz2;
        const double dl = xx2 - xx1, dw = yy2 - yy1, dh = zz2 - zz1;
        const double l = dl > 0.0 ? dl : 0.0, wd = dw > 0.0 ? dw : 0.0, h = dh > 0.0 ? dh : 0.0;   // np.maximum(0, .)
        const double inter = l * wd * h;
        const bool same = !cls_nms || s_cls[j] == ci;
        // a pair with no overlap or of different classes yields 0 (or NaN): never above a threshold >= 0
        if (thr >= 0.0 && !(inter > 0.0 && same)) continue;
        const double area_j = (jx2 - jx1) * (jy2 - jy1) * (jz2 - jz1);
        double o;
        if (old_type)
          o = inter / area_j;
        else if (cls_nms)
          o = inter / (area_i + area_j - inter + 1e-8);
        else
          o = inter / (area_i + area_j - inter);
        if (cls_nms) o = o * (same ? 1.0 : 0.0);
        if (o > thr) bits |= 1ull << (c - w * 64);
      }
    }
    s_sup[r][w] = bits;
  }
  __syncthreads();

  // greedy scan in rank order: one wave, lane w < 8 owns word w of the removed set
  if (k < 64) {
    const int lane = k & (PP_WORDS - 1);
    uint64_t removed = 0;
    for (int r = 0; r < Mne; ++r) {
      const uint64_t row = s_sup[r][lane];
      const int src = r >> 6;
      const unsigned lo32 = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)removed, src);
      const unsigned hi32 = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(removed >> 32), src);
      const uint64_t word = ((uint64_t)hi32 << 32) | lo32;
      if (!((word >> (r & 63)) & 1)) removed |= row;
    }
    if (k < PP_WORDS) s_removed[k] = removed;
  }
  __syncthreads();
  if (act) {
    const bool kept = ne && !((s_removed[rank >> 6] >> (rank & 63)) & 1);
    a.pred_mask[p] = kept ? 1 : 0;
    a.valid[p] = (kept && prob > a.conf_thresh) ? 1 : 0;
  }
}

}  // namespace

extern "C" size_t spacap_points_in_box_workspace_bytes(int B, int N, int K) {
  if (B < 0 || N < 1 || K < 1) return 0;
  return (size_t)B * ((N + PIB_POINTS - 1) / PIB_POINTS) * K * sizeof(int32_t);
}

extern "C" int spacap_points_in_box_f32(const float *point_clouds, int B, int N, int C, const double *bbox_corner, int K,
                                        void *workspace, size_t workspace_bytes, spacap_stream_t stream) {
  const char *what = "spacap_points_in_box_f32";
  SPACAP_REQUIRE(B >= 0 && B <= 65535 && N >= 1 && C >= 3 && K >= 1 && K <= PP_MAXK, "%s: bad sizes (B=%d N=%d C=%d K=%d)", what,
                 B, N, C, K);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(point_clouds && bbox_corner && workspace, "%s: null pointer", what);
  SPACAP_REQUIRE(workspace_bytes >= spacap_points_in_box_workspace_bytes(B, N, K), "%s: workspace too small", what);
  const int nchunk = (N + PIB_POINTS - 1) / PIB_POINTS;
  hipLaunchKernelGGL(points_in_box_kernel, dim3(nchunk, B), dim3(PIB_THREADS), 0, spacap::as_stream(stream), point_clouds, N, C,
                     bbox_corner, K, nchunk, static_cast<int32_t *>(workspace));
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_detection_nms_f32(const float *objectness, const int64_t *sem_cls, const float *sem_cls_scores, int NC,
                                        const double *bbox_corner, const void *workspace, int B, int N, int K,
                                        const double *gt_corner, int M, const int64_t *object_assignment, int flags,
                                        int min_points, double nms_iou, float conf_thresh, double min_iou, float *obj_prob,
                                        int32_t *count, uint8_t *nonempty, uint8_t *pred_mask, float *conf, uint8_t *valid,
                                        double *iou, uint8_t *good, spacap_stream_t stream) {
  const char *what = "spacap_detection_nms_f32";
  SPACAP_REQUIRE(B >= 0 && N >= 1 && K >= 1 && K <= PP_MAXK, "%s: bad sizes (B=%d N=%d K=%d; K <= %d)", what, B, N, K, PP_MAXK);
  SPACAP_REQUIRE(!sem_cls_scores || (NC >= 1 && NC <= PP_MAXNC), "%s: NC=%d outside 1..%d", what, NC, PP_MAXNC);
  SPACAP_REQUIRE(!gt_corner || M >= 1, "%s: M=%d", what, M);
  SPACAP_REQUIRE(!(flags & ~(SPACAP_PP_REMOVE_EMPTY | SPACAP_PP_CLS_NMS | SPACAP_PP_OLD_TYPE | SPACAP_PP_GT_F32)), "%s: unknown flags %d",
                 what, flags);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(objectness && sem_cls && bbox_corner && workspace && obj_prob && count && nonempty && pred_mask && valid,
                 "%s: null pointer", what);
  SPACAP_REQUIRE(!sem_cls_scores || conf, "%s: null pointer (conf)", what);
  SPACAP_REQUIRE(!gt_corner || (object_assignment && iou && good), "%s: null pointer (iou)", what);
  NmsArgs a;
  a.objectness = objectness;
  a.sem_cls = sem_cls;
  a.sem_cls_scores = sem_cls_scores;
  a.corners = bbox_corner;
  a.slab = static_cast<const int32_t *>(workspace);
  a.gt_corners = gt_corner;
  a.assignment = object_assignment;
  a.K = K;
  a.NC = NC;
  a.nchunk = (N + PIB_POINTS - 1) / PIB_POINTS;
  a.M = M;
  a.flags = flags;
  a.min_points = min_points;
  a.nms_iou = nms_iou;
  a.min_iou = min_iou;
  a.conf_thresh = conf_thresh;
  a.obj_prob = obj_prob;
  a.count = count;
  a.nonempty = nonempty;
  a.pred_mask = pred_mask;
  a.valid = valid;
  a.conf = conf;
  a.iou = iou;
  a.good = good;
  hipLaunchKernelGGL(detection_nms_kernel, dim3(B), dim3(PP_MAXK), 0, spacap::as_stream(stream), a);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
