// Dense-caption predictions for gfx950 (MI355X): per scene the proposals that survive post-processing, ranked, each with its
// class, score, box and caption -- what a caller of the reference assembles on the host from parse_predictions with
// per_class_proposal=False (lib/ap_helper.py:145-158) and decode_caption (lib/eval_helper.py:46-57) in a Python loop over
// (scene, proposal).  No ground truth is involved.
//
// dense_caption_select_kernel, one workgroup of 512 threads per scene, one thread per proposal (K <= 512):
//  1. every thread turns (valid, obj_prob) into ONE sortable u32 in LDS (rank_key of eval_common.hpp, the order
//     detection_ap.hip ranks by too): descending score compared as f32, equal scores lower proposal index first, NaN behind
//     every number, and a proposal that is not kept ahead of nobody.
//  2. rank counting (rank_count of eval_common.hpp): a kept thread counts the proposals ahead of it.  The rank of a kept
//     proposal counts kept proposals only: the kept rows are dense from 0.  s_src[rank] = proposal.
//  3. outputs by RANK, every element of every array on every call (rows behind the count: index -1, everything else zero):
//     count / index / score / cls / length one thread per row; the corners as 16-byte chunks (12 per 192-byte box, one per
//     thread-iteration: a wave stores 1 KiB contiguously); the captions one wave per row and one lane per position, by
//     decode_caption of eval_common.hpp -- sos, the tokens through the first eos inclusive, an eos appended when there was
//     none, zero padding (length counts sos and eos).
// No global atomics, no state between calls, no host synchronisation; plain vector loads and stores only.
#include "eval_common.hpp"

namespace {

using namespace spacap::eval;

constexpr int DP_MAXK = 512;
constexpr int DP_MAXL = 62;                         // L + 2 positions = the lanes of a wave
constexpr int DP_CHUNKS = 12;                       // 16-byte chunks of one box (8 x 3 f64 = 192 bytes)

struct PredArgs {
  const uint8_t *valid;         // [B,K]
  const float *obj_prob;        // [B,K]
  const int64_t *sem_cls;       // [B,K]
  const double2 *corners;       // [B,K,12]  (= f64 [B,K,8,3])
  const int64_t *tokens;        // [B,K,L]
  int K, L, sos, eos;
  int32_t *count;               // [B]
  int32_t *index;               // [B,K]
  float *score;                 // [B,K]
  int32_t *cls;                 // [B,K]
  double2 *out_corners;         // [B,K,12]
  int32_t *out_tokens;          // [B,K,L+2]
  int32_t *length;              // [B,K]
};

__global__ __launch_bounds__(DP_MAXK) void dense_caption_select_kernel(PredArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned s_key[DP_MAXK];
  __shared__ float s_score[DP_MAXK];
  __shared__ int s_src[DP_MAXK];                    // proposal at each rank
  const int b = blockIdx.x, k = threadIdx.x, K = a.K, L = a.L;
  const size_t row0 = (size_t)b * K;

  bool kept = false;
  float score = 0.f;
  if (k < K) {
    kept = a.valid[row0 + k] != 0;
    score = a.obj_prob[row0 + k];
  }
  const unsigned key = rank_key(kept, score);
  s_key[k] = key;                                   // (threads k >= K: 0 = not kept, they pad the last group of four)
  s_score[k] = score;
  const int count = __syncthreads_count(kept);      // (also the barrier behind the LDS writes)

  // pos < count <= K: the ranks of the kept proposals are a permutation of 0..count-1
  if (kept) s_src[rank_count(s_key, K, key, k)] = k;
  __syncthreads();

  if (k == 0) a.count[b] = count;
  if (k < K) {
    const int src = k < count ? s_src[k] : -1;
    a.index[row0 + k] = src;
    a.score[row0 + k] = src >= 0 ? s_score[src] : 0.f;
    a.cls[row0 + k] = src >= 0 ? (int32_t)a.sem_cls[row0 + src] : 0;
  }

  // boxes: chunk i of the scene = row i / 12, 16 bytes i % 12
  for (int i = k; i < K * DP_CHUNKS; i += DP_MAXK) {
    const int r = i / DP_CHUNKS, c = i - r * DP_CHUNKS;
    double2 v;
    v.x = v.y = 0.0;
    if (r < count) v = a.corners[(row0 + s_src[r]) * DP_CHUNKS + c];
    a.out_corners[row0 * DP_CHUNKS + i] = v;
  }

  // captions: one wave per row, one lane per position
  const int lane = k & 63, W = L + 2;
  for (int r = k >> 6; r < K; r += DP_MAXK / 64) {  // (uniform over the wave)
    int v = 0, len = 0;
    if (r < count) {
      const int64_t tok = lane < L ? a.tokens[(row0 + s_src[r]) * L + lane] : 0;
      v = decode_caption(tok, lane, L, a.sos, a.eos, len);
    }
    if (lane < W) a.out_tokens[(row0 + r) * W + lane] = v;
    if (lane == 0) a.length[row0 + r] = len;
  }
}

}  // namespace

extern "C" int spacap_dense_caption_select(const uint8_t *valid, const float *obj_prob, const int64_t *sem_cls,
                                           const double *bbox_corner, const int64_t *tokens, int B, int K, int L, int sos, int eos,
                                           int32_t *count, int32_t *index, float *score, int32_t *cls, double *corners,
                                           int32_t *out_tokens, int32_t *length, spacap_stream_t stream) {
  const char *what = "spacap_dense_caption_select";
  SPACAP_REQUIRE(B >= 0 && B <= 65535 && K >= 1 && K <= DP_MAXK && L >= 1 && L <= DP_MAXL && sos >= 0 && eos >= 0,
                 "%s: bad sizes (B=%d K=%d L=%d sos=%d eos=%d; K <= %d, L <= %d)", what, B, K, L, sos, eos, DP_MAXK, DP_MAXL);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(valid && obj_prob && sem_cls && bbox_corner && tokens && count && index && score && cls && corners && out_tokens &&
                     length,
                 "%s: null pointer", what);
  SPACAP_REQUIRE(spacap::aligned16(bbox_corner, corners),
                 "%s: bbox_corner and corners must be 16-byte aligned", what);
  PredArgs a;
  a.valid = valid;
  a.obj_prob = obj_prob;
  a.sem_cls = sem_cls;
  a.corners = reinterpret_cast<const double2 *>(bbox_corner);
  a.tokens = tokens;
  a.K = K;
  a.L = L;
  a.sos = sos;
  a.eos = eos;
  a.count = count;
  a.index = index;
  a.score = score;
  a.cls = cls;
  a.out_corners = reinterpret_cast<double2 *>(corners);
  a.out_tokens = out_tokens;
  a.length = length;
  hipLaunchKernelGGL(dense_caption_select_kernel, dim3(B), dim3(DP_MAXK), 0, spacap::as_stream(stream), a);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
