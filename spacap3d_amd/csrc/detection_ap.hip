// Detection mAP / AR for gfx950 (MI355X): the reference's APCalculator (lib/ap_helper.py:195-250) with eval_det_cls and voc_ap
// (utils/eval_det.py:21-52, 74-158) on the device.
//
// The reference sorts all predictions of a class over the whole validation set and walks them once, calling box3d_iou
// (utils/box_util.py:122-133) per ground-truth box of the prediction's scene.  Whether a prediction is a true positive only
// depends on the better-ranked predictions of the same class IN THE SAME SCENE, so the flags are final per batch:
//
//  1. detection_match_kernel, one workgroup of 512 threads per (class, scene), one thread per proposal (K <= 512):
//     - the class's ground-truth boxes of the scene (box_label_mask == 1, sem_cls_label == class) are compacted in index
//       order into LDS as f64 bounds + volume;
//     - records of the (scene, class): per-class mode -- every valid box, scored conf[b,k,class]; single-class mode -- the
//       valid boxes whose sem_cls is the class, scored obj_prob[b,k];
//     - order: score descending compared as f32, equal scores LOWER proposal index first, NaN behind every number (the
//       reference's np.argsort(-confidence) is a quicksort: the order of ties is unspecified there), by rank counting over
//       one folded u32 key per proposal (rank_key / rank_count of eval_common.hpp, as predictions.hip ranks);
//     - per record ovmax / jmax over the class's boxes in index order with `iou > ovmax` from -inf (first strict maximum);
//       the IoU is box3d_iou in f64 in its operation order, IEEE division (a pair without overlap yields its exact +0
//       without dividing);
//     - per (ground-truth box, threshold) the minimum rank among the records that match it above the threshold (LDS
//       atomicMin): a record is a TP at threshold t when ovmax > t and it holds that minimum; everything else is an FP.
//     Output: a slab [B, NC, K] in rank order, every element written on every call: score f32 (-inf in the unused tail),
//     flag byte (bit t = TP at threshold t, bit 7 = the record exists), proposal index i16.  Workgroup (class, scene 0)
//     also counts the batch's ground-truth boxes of its class and ADDS them into npos[class] -- one thread, a plain
//     read-modify-write ordered by the stream; no atomics on global memory, no device state between calls.
//  2. ap_curve_kernel, one workgroup of 256 threads per (class, threshold), over the class's records of the whole run
//     sorted by score: a count of the TPs, then ONE walk over tiles of 1024 records from the END of the list (so that the
//     reverse running maximum of voc_ap is a forward scan): cumulative tp (fp = position + 1 - tp), rec = tp / (npos + 1e-8),
//     prec = tp / max(tp + fp, eps), the precision envelope, and the area summed over the points where recall changes.
//
// Arithmetic: -ffp-contract=off (Makefile default).  rec / prec are one IEEE division of exact integers each, so they are
// bit-equal to numpy's; the area is summed in a fixed order (per thread, then a tree) that is not numpy's pairwise order.
#include <math.h>

#include "eval_common.hpp"

namespace {

using namespace spacap::eval;

constexpr int AP_MAXK = 512;
constexpr int AP_MAXM = 256;
constexpr int AP_MAXNC = 128;
constexpr int AP_MAXT = 4;
constexpr int AP_EXISTS = 0x80;

constexpr int CURVE_THREADS = 256;
constexpr int CURVE_ITEMS = 4;
constexpr int CURVE_TILE = CURVE_THREADS * CURVE_ITEMS;

struct MatchArgs {
  const double *corners;        // [B,K,8,3]
  const uint8_t *valid;         // [B,K]
  const float *conf;            // [B,K,NC] or null (single-class mode)
  const float *obj_prob;        // [B,K]    single-class mode
  const int64_t *sem_cls;       // [B,K]    single-class mode
  const double *gt_corners;     // [B,M,8,3]
  const int64_t *gt_cls;        // [B,M]
  const uint8_t *gt_mask;       // [B,M]
  int B, K, NC, M, T;
  double thr[AP_MAXT];
  float *score;                 // [B,NC,K]
  uint8_t *flags;               // [B,NC,K]
  int16_t *index;               // [B,NC,K]
  int32_t *npos;                // [NC]
};

__global__ __launch_bounds__(AP_MAXK) void detection_match_kernel(MatchArgs a) {
  __shared__ double s_gb[6][AP_MAXM];               // bounds of the class's ground-truth boxes, compacted in index order
  __shared__ double s_gvol[AP_MAXM];
  __shared__ __attribute__((aligned(16))) unsigned s_key[AP_MAXK];   // rank_key of every proposal
  __shared__ uint8_t s_gsel[AP_MAXM];
  __shared__ unsigned s_min[AP_MAXT][AP_MAXM];      // per (threshold, box): lowest rank among the records matching it
  const int c = blockIdx.x, b = blockIdx.y, k = threadIdx.x, K = a.K, M = a.M;
  const bool act = k < K;
  const size_t p = (size_t)b * K + k;

  if (b == 0) {                                     // (uniform over the workgroup)
    int n = 0;
    const int all = a.B * M;                        // <= 65535 * 256
    for (int i0 = 0; i0 < all; i0 += AP_MAXK) {
      const int i = i0 + k;
      n += __syncthreads_count(i < all && a.gt_mask[i] == 1 && a.gt_cls[i] == (int64_t)c);
    }
    if (k == 0) a.npos[c] += n;
  }

  if (k < M) s_gsel[k] = (a.gt_mask[(size_t)b * M + k] == 1 && a.gt_cls[(size_t)b * M + k] == (int64_t)c) ? 1 : 0;
  float score = 0.f;
  bool ex = false;
  if (act) {
    ex = a.valid[p] != 0;
    if (a.conf) {
      score = a.conf[p * a.NC + c];
    } else {
      ex = ex && a.sem_cls[p] == (int64_t)c;
      score = a.obj_prob[p];
    }
  }
  const unsigned key = rank_key(ex, score);
  s_key[k] = key;                                   // (threads k >= K: 0, they pad the last group of four)
  __syncthreads();

  int G = 0;                                        // ground-truth boxes of the class (uniform over the workgroup)
  if (k < M) {
    int pos = 0;
    for (int m = 0; m < k; ++m) pos += s_gsel[m];
    if (s_gsel[k]) {
      double lo[3], hi[3];
      box_bounds(a.gt_corners + ((size_t)b * M + k) * 24, lo, hi);
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        s_gb[d][pos] = lo[d];
        s_gb[3 + d][pos] = hi[d];
      }
      s_gvol[pos] = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]);
    }
  }
  for (int m = 0; m < M; ++m) G += s_gsel[m];
  for (int i = k; i < AP_MAXT * AP_MAXM; i += AP_MAXK) s_min[i / AP_MAXM][i % AP_MAXM] = 0xFFFFFFFFu;

  // position in the slab: existing records by rank, then the others (key 0) by proposal index
  const int pos = act ? rank_count(s_key, K, key, k) : 0;
  __syncthreads();

  // box3d_iou(prediction, ground truth) over the class's boxes: first strict maximum
  double ovmax = -INFINITY;
  int jmax = 0;
  if (ex && G > 0) {
    double lo[3], hi[3];
    box_bounds(a.corners + p * 24, lo, hi);
    const double vol1 = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]);
    for (int g = 0; g < G; ++g) {
      double e[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const double g_lo = s_gb[d][g], g_hi = s_gb[3 + d][g];
        const double A = (lo[d] > g_lo || lo[d] != lo[d]) ? lo[d] : g_lo;     // np.maximum / np.minimum propagate NaN
        const double Bq = (hi[d] < g_hi || hi[d] != hi[d]) ? hi[d] : g_hi;
        const double w = Bq - A;
        e[d] = (w > 0.0 || w != w) ? w : 0.0;
      }
      const double inter = e[0] * e[1] * e[2];
      const double den = vol1 + s_gvol[g] - inter + 1e-8;
      // inter == 0: the quotient is an exact zero for every den but NaN (den > 0 here: volumes are max - min)
      const double iou = inter > 0.0 ? inter / den : (den != den || inter != inter ? NAN : 0.0);
      if (iou > ovmax) {
        ovmax = iou;
        jmax = g;
      }
    }
  }
  bool pass[AP_MAXT];
#pragma unroll
  for (int t = 0; t < AP_MAXT; ++t) {
    pass[t] = ex && G > 0 && t < a.T && ovmax > a.thr[t];
    if (pass[t]) atomicMin(&s_min[t][jmax], (unsigned)pos);
  }
  __syncthreads();
  if (act) {
    int f = ex ? AP_EXISTS : 0;
#pragma unroll
    for (int t = 0; t < AP_MAXT; ++t)
      if (pass[t] && s_min[t][jmax] == (unsigned)pos) f |= 1 << t;
    const size_t o = ((size_t)b * a.NC + c) * K + pos;
    a.score[o] = ex ? score : -INFINITY;
    a.flags[o] = (uint8_t)f;
    a.index[o] = (int16_t)k;
  }
}

// inclusive prefix over the workgroup's 256 threads in thread order: sums of an int and running maxima of a double
__device__ __forceinline__ void block_scan(int &s, double &m, int *s_ws, double *s_wm) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int so = __shfl_up(s, o);
    const double mo = __shfl_up(m, o);
    if (lane >= o) {
      s += so;
      m = mo > m ? mo : m;
    }
  }
  __syncthreads();                                  // the previous tile's readers are done with s_ws / s_wm
  if (lane == 63) {
    s_ws[wave] = s;
    s_wm[wave] = m;
  }
  __syncthreads();
  for (int w = 0; w < wave; ++w) {
    s += s_ws[w];
    m = s_wm[w] > m ? s_wm[w] : m;
  }
}

__global__ __launch_bounds__(CURVE_THREADS) void ap_curve_kernel(const uint8_t *__restrict__ flags, long long L,
                                                                  const int64_t *__restrict__ count,
                                                                  const int32_t *__restrict__ npos, int T,
                                                                  double *__restrict__ rec, double *__restrict__ prec,
                                                                  double *__restrict__ ap, double *__restrict__ last_rec) {
  __shared__ int s_ws[CURVE_THREADS / 64];
  __shared__ double s_wm[CURVE_THREADS / 64];
  __shared__ int s_red[CURVE_THREADS];
  __shared__ double s_sum[CURVE_THREADS];
  const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const uint8_t *f = flags + (size_t)c * L;
  long long n = count[c];
  n = n < 0 ? 0 : (n > L ? L : n);
  const uint8_t bit = (uint8_t)(1 << t);
  const double den = (double)npos[c] + 1e-8;         // float(npos + 1e-8)
  double *rec_o = rec ? rec + ((size_t)c * T + t) * L : nullptr;
  double *prec_o = prec ? prec + ((size_t)c * T + t) * L : nullptr;

  int cnt = 0;
  for (long long i = tid; i < n; i += CURVE_THREADS) cnt += (f[i] & bit) ? 1 : 0;
  s_red[tid] = cnt;
  __syncthreads();
  for (int o = CURVE_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) s_red[tid] += s_red[tid + o];
    __syncthreads();
  }
  const long long total = s_red[0];

  // Walk from the end: r counts records from the last one.  `after` = cumulative tp through the tile's last record,
  // `env` = maximum precision behind the tile (voc_ap's sentinel 0 behind the list).
  long long after = total;
  double env = 0.0, area = 0.0;
  for (long long r0 = 0; r0 < n; r0 += CURVE_TILE) {
    int tp[CURVE_ITEMS];
    bool in[CURVE_ITEMS];
    int s = 0;
#pragma unroll
    for (int q = 0; q < CURVE_ITEMS; ++q) {
      const long long r = r0 + tid * CURVE_ITEMS + q;
      in[q] = r < n;
      tp[q] = (in[q] && (f[n - 1 - r] & bit)) ? 1 : 0;
      s += tp[q];
    }
    // precision of this thread's records needs the tp counts first: scan the sums, then the maxima
    int incl = s;
    double none = 0.0;
    block_scan(incl, none, s_ws, s_wm);
    long long tp_cum = after - (incl - s);           // cumulative tp through this thread's FIRST record (the latest one)
    double pr[CURVE_ITEMS], rc[CURVE_ITEMS], rprev[CURVE_ITEMS];
    double m = 0.0;
#pragma unroll
    for (int q = 0; q < CURVE_ITEMS; ++q) {
      const long long i = n - 1 - (r0 + tid * CURVE_ITEMS + q);   // position in score order
      const double tpd = (double)tp_cum, all = (double)(i + 1);   // tp + fp = i + 1: every record is one or the other
      rc[q] = tpd / den;
      pr[q] = tpd / fmax(all, 2.220446049250313e-16);
      rprev[q] = (double)(tp_cum - tp[q]) / den;                  // mrec one place earlier (0 / den = voc_ap's sentinel)
      if (in[q]) {
        m = pr[q] > m ? pr[q] : m;
        if (rec_o) rec_o[i] = rc[q];
        if (prec_o) prec_o[i] = pr[q];
      }
      pr[q] = m;                                     // running maximum inside the thread, latest record first
      tp_cum -= tp[q];
    }
    int zero = 0;
    double mx = m;
    block_scan(zero, mx, s_ws, s_wm);                // inclusive over the threads
    // maximum over the threads before this one = behind these records in score order
    double before = __shfl_up(mx, 1);
    if ((tid & 63) == 0) {
      before = 0.0;
      for (int w = 0; w < (tid >> 6); ++w) before = s_wm[w] > before ? s_wm[w] : before;
    }
    before = env > before ? env : before;
#pragma unroll
    for (int q = 0; q < CURVE_ITEMS; ++q) {
      const double e = pr[q] > before ? pr[q] : before;
      if (in[q] && rc[q] != rprev[q]) area += (rc[q] - rprev[q]) * e;
    }
    // carry to the next (earlier) tile
    __syncthreads();
    if (tid == CURVE_THREADS - 1) {
      s_ws[0] = incl;
      s_wm[0] = mx > env ? mx : env;
    }
    __syncthreads();
    after -= s_ws[0];
    env = s_wm[0];
  }
  s_sum[tid] = area;
  __syncthreads();
  for (int o = CURVE_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) s_sum[tid] += s_sum[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    ap[c * T + t] = s_sum[0];
    last_rec[c * T + t] = (double)total / den;
  }
}

}  // namespace

extern "C" int spacap_detection_match_f32(const double *bbox_corner, const uint8_t *valid, const float *conf,
                                          const float *obj_prob, const int64_t *sem_cls, int B, int K, int NC,
                                          const double *gt_corner, const int64_t *sem_cls_label,
                                          const uint8_t *box_label_mask, int M, const double *thresholds, int T, float *score,
                                          uint8_t *flags, int16_t *index, int32_t *npos, spacap_stream_t stream) {
  const char *what = "spacap_detection_match_f32";
  SPACAP_REQUIRE(B >= 0 && B <= 65535 && K >= 1 && K <= AP_MAXK && M >= 1 && M <= AP_MAXM && NC >= 1 && NC <= AP_MAXNC && T >= 1 &&
                     T <= AP_MAXT,
                 "%s: bad sizes (B=%d K=%d M=%d NC=%d T=%d; K <= %d, M <= %d, NC <= %d, T <= %d)", what, B, K, M, NC, T, AP_MAXK,
                 AP_MAXM, AP_MAXNC, AP_MAXT);
  SPACAP_REQUIRE(thresholds, "%s: null pointer (thresholds)", what);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(bbox_corner && valid && gt_corner && sem_cls_label && box_label_mask && score && flags && index && npos,
                 "%s: null pointer", what);
  SPACAP_REQUIRE(conf || (obj_prob && sem_cls), "%s: null pointer (conf, or obj_prob and sem_cls)", what);
  MatchArgs a;
  a.corners = bbox_corner;
  a.valid = valid;
  a.conf = conf;
  a.obj_prob = obj_prob;
  a.sem_cls = sem_cls;
  a.gt_corners = gt_corner;
  a.gt_cls = sem_cls_label;
  a.gt_mask = box_label_mask;
  a.B = B;
  a.K = K;
  a.NC = NC;
  a.M = M;
  a.T = T;
  for (int t = 0; t < AP_MAXT; ++t) a.thr[t] = t < T ? thresholds[t] : 0.0;
  a.score = score;
  a.flags = flags;
  a.index = index;
  a.npos = npos;
  hipLaunchKernelGGL(detection_match_kernel, dim3(NC, B), dim3(AP_MAXK), 0, spacap::as_stream(stream), a);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_ap_curve_f64(const uint8_t *flags, int64_t L, const int64_t *count, const int32_t *npos, int NC, int T,
                                   double *rec, double *prec, double *ap, double *last_rec, spacap_stream_t stream) {
  const char *what = "spacap_ap_curve_f64";
  SPACAP_REQUIRE(L >= 1 && NC >= 1 && NC <= AP_MAXNC && T >= 1 && T <= AP_MAXT, "%s: bad sizes (L=%lld NC=%d T=%d; NC <= %d, T <= %d)",
                 what, (long long)L, NC, T, AP_MAXNC, AP_MAXT);
  SPACAP_REQUIRE(flags && count && npos && ap && last_rec, "%s: null pointer", what);
  SPACAP_REQUIRE((rec == nullptr) == (prec == nullptr), "%s: rec and prec go together", what);
  hipLaunchKernelGGL(ap_curve_kernel, dim3(NC, T), dim3(CURVE_THREADS), 0, spacap::as_stream(stream), flags, (long long)L, count,
                     npos, T, rec, prec, ap, last_rec);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
