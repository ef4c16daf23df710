// What the evaluation kernels share (postprocess.hip, detection_ap.hip, caption_eval.hip, predictions.hip): the bounds of a
// box, the rank order of proposals by score, and decode_caption's rule.  The three IoU computations are NOT here: each restates
// another reference function (NaN through max / min / the clamp, the f32 ground-truth volume, the 1e-8 in the denominator),
// and neither is the NMS order of postprocess.hip (higher index first among ties, NaN first), which is another rule.
// The four files say `using namespace spacap::eval;` inside their own namespace.
#pragma once
#include "common.hpp"

namespace spacap::eval {

// axis-aligned bounds of the 8 corners c[8][3]
__device__ __forceinline__ void box_bounds(const double *__restrict__ c, double lo[3], double hi[3]) {
#pragma unroll
  for (int d = 0; d < 3; ++d) lo[d] = hi[d] = c[d];
#pragma unroll
  for (int v = 1; v < 8; ++v)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double x = c[v * 3 + d];
      lo[d] = x < lo[d] ? x : lo[d];
      hi[d] = x > hi[d] ? x : hi[d];
    }
}

// ---- rank order: descending score compared as f32, equal scores LOWER proposal index first, NaN behind every number, a
// proposal that does not exist behind all that do, in proposal order.
// One sortable u32 per proposal: 0 when it does not exist, 1 for a NaN, else the f32 bit pattern folded so that unsigned order
// = numeric order (-0 counts as +0; the smallest such key, that of -inf, is 0x007FFFFF).  Proposal j is ahead of proposal k
// when key[j] > key[k], or the keys are equal and j < k.
__device__ __forceinline__ unsigned rank_key(bool exists, float s) {
  if (!exists) return 0u;
  if (s != s) return 1u;
  const unsigned u = s == 0.f ? 0u : __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Rank counting: the number of proposals 0..K-1 ahead of proposal k, whose key is `key`.  s_key is 16-byte aligned LDS and
// holds a key for every index below K rounded up to a multiple of four -- 0 behind K, which is ahead of nobody.  All lanes
// read the same address, so the reads broadcast; they are 16 bytes wide (four keys per ds_read_b128).  Among the proposals
// that exist the ranks are dense from 0; those that do not exist follow in proposal order.
__device__ __forceinline__ int rank_count(const unsigned *s_key, int K, unsigned key, int k) {
  const uint4 *k4 = reinterpret_cast<const uint4 *>(s_key);
  int pos = 0;
  for (int j = 0; j < K; j += 4) {
    const uint4 q = k4[j >> 2];
    pos += (q.x > key || (q.x == key && j < k)) ? 1 : 0;
    pos += (q.y > key || (q.y == key && j + 1 < k)) ? 1 : 0;
    pos += (q.z > key || (q.z == key && j + 2 < k)) ? 1 : 0;
    pos += (q.w > key || (q.w == key && j + 3 < k)) ? 1 : 0;
  }
  return pos;
}

// ---- decode_caption (lib/eval_helper.py:46-57) by one wave, lane = position: sos, the L tokens through the first eos
// inclusive, an eos appended when there was none, zero padding.  `tok` is this lane's token (lanes >= L: anything).  Returns
// the word at this lane's position; len (wave-uniform) counts sos and eos, <= L + 2 <= 64.  Every lane of the wave calls it.
__device__ __forceinline__ int decode_caption(int64_t tok, int lane, int L, int sos, int eos, int &len) {
  const unsigned long long hit = __ballot(lane < L && tok == (int64_t)eos);
  const int first = hit ? __ffsll((long long)hit) - 1 : -1;        // position of the first eos
  const int body = first >= 0 ? first + 1 : L;                     // tokens kept (the eos included)
  len = 1 + body + (first >= 0 ? 0 : 1);
  const int prev = __shfl((int)tok, lane > 0 ? lane - 1 : 0);      // token lane-1 sits at position lane
  const int v = lane == 0 ? sos : (lane <= body ? prev : eos);
  return lane < len ? v : 0;
}

}  // namespace spacap::eval
