// The teacher-forcing rows of cross-entropy training over every matched object of a scene, chosen and built on the device in one
// launch, for gfx950 (MI355X).  DESIGN.md section 7o; tests/dense_xe_restated.py restates the semantics.
//
// One wave per group g = b M + m (the slots spacap_scst_select_f32 fills).  key[g] < 0 (an empty slot), a key outside 0..nkeys-1
// or a key with n = key_ref_off[key + 1] - key_ref_off[key] <= 0 references: every row of the group is empty.  Otherwise
//   h  = hash32(g, make_seed(seed, seed_dev))        -- dropout.hpp's, the library's one counter hash
//   j0 = (uint64(h) * n) >> 32                        -- uniform over 0..n-1 up to the 2^-32 rounding of the multiply-shift
//   row s < r takes reference key_ref_off[key] + (j0 + s) % n when s < n (a rotation: distinct references inside a group), and
//   is empty when s >= n.
// A sentence of len ids becomes T ids: len <= T -- its ids, then zeros; len > T -- its first T - 1 ids, then eos (the reference's
// dataset trims the words and closes the sentence).  An id outside 0..n_vocab-1 becomes unk (the corpus numbers the words outside
// the vocabulary upward from n_vocab).  An empty row is sos eos and zeros, good 0, length 0, ref -1.  tok = a leading 1 and the
// id row (lang_label's layout).  No atomics, no state: a captured call replays, and draws anew when *seed_dev moved.
#include "common.hpp"
#include "dropout.hpp"

namespace {

using namespace spacap;

constexpr int XE_THREADS = 64, XE_RMAX = 8;

struct DenseXeArgs {
  const int *key, *ref_tok, *ref_off, *ref_len, *key_ref_off;
  long long n_tok, n_refs;
  int groups, nkeys, n_vocab, unk, sos, eos, r, T;
  unsigned long long seed;
  const unsigned long long *seed_dev;
  long long *ids, *tok;
  int *ref;
  unsigned char *good;
  int *length;
};

__global__ __launch_bounds__(XE_THREADS) void dense_xe_targets_kernel(DenseXeArgs a) {
  const int g = blockIdx.x, lane = threadIdx.x, T = a.T;
  const int key = a.key[g];
  int n = 0, first = 0;
  if (key >= 0 && key < a.nkeys) {
    first = a.key_ref_off[key];
    n = a.key_ref_off[key + 1] - first;
  }
  unsigned j0 = 0;
  if (n > 0) {
    const unsigned h = hash32((unsigned long long)g, make_seed(a.seed, a.seed_dev));
    j0 = (unsigned)(((unsigned long long)h * (unsigned long long)n) >> 32);
  }
  for (int s = 0; s < a.r; ++s) {   // (uniform over the wave)
    const size_t row = (size_t)g * a.r + s;
    long long ref = -1, off = 0;
    int len = 0;
    if (s < n) {
      ref = (long long)first + (long long)((j0 + (unsigned)s) % (unsigned)n);
      if (ref < 0 || ref >= a.n_refs) {
        ref = -1;                     // (an offset table that does not fit its reference table: no row)
      } else {
        off = a.ref_off[ref], len = a.ref_len[ref];
        if (len < 0 || off < 0 || off + len > a.n_tok) ref = -1, len = 0;
      }
    }
    const bool live = ref >= 0;
    long long *ids = a.ids + row * T, *tok = a.tok + row * (T + 1);
    for (int c = lane; c < T; c += XE_THREADS) {
      long long w = 0;
      if (!live) {
        w = c == 0 ? a.sos : c == 1 ? a.eos : 0;
      } else if (len > T && c == T - 1) {
        w = a.eos;
      } else if (c < len) {
        const int t = a.ref_tok[off + c];
        w = (unsigned)t < (unsigned)a.n_vocab ? t : a.unk;
      }
      ids[c] = w, tok[c + 1] = w;
    }
    if (lane == 0) {
      tok[0] = 1;
      a.ref[row] = (int)ref;
      a.good[row] = live ? 1 : 0;
      a.length[row] = live ? max(min(len, T) - 1, 0) : 0;
    }
  }
}

}  // namespace

extern "C" int spacap_dense_xe_targets_i64(const int32_t *key, int B, int M, const int32_t *ref_tok, int64_t n_tok,
                                           const int32_t *ref_off, const int32_t *ref_len, int64_t n_refs,
                                           const int32_t *key_ref_off, int nkeys, int n_vocab, int unk, int sos, int eos, int r, int T,
                                           uint64_t seed, const uint64_t *seed_dev, int64_t *ids, int64_t *tok, int32_t *ref,
                                           uint8_t *good, int32_t *length, spacap_stream_t stream) {
  const char *what = "spacap_dense_xe_targets_i64";
  SPACAP_REQUIRE(B >= 0 && M >= 1 && (long long)B * M <= 0x7fffffffLL / XE_RMAX && r >= 1 && r <= XE_RMAX && T >= 2 && nkeys >= 0 &&
                     n_tok >= 0 && n_refs >= 0 && n_vocab >= 1 && unk >= 0 && sos >= 0 && eos >= 0,
                 "%s: bad arguments (B=%d >= 0, M=%d >= 1, 1 <= r=%d <= %d, T=%d >= 2, n_vocab=%d >= 1, ids >= 0)", what, B, M, r,
                 XE_RMAX, T, n_vocab);
  if (B == 0) return SPACAP_OK;
  SPACAP_REQUIRE(key && ids && tok && ref && good && length && (nkeys == 0 || key_ref_off) && (n_refs == 0 || (ref_off && ref_len)) &&
                     (n_tok == 0 || ref_tok),
                 "%s: null pointer", what);
  DenseXeArgs a;
  a.key = key, a.ref_tok = ref_tok, a.ref_off = ref_off, a.ref_len = ref_len, a.key_ref_off = key_ref_off;
  a.n_tok = n_tok, a.n_refs = n_refs;
  a.groups = B * M, a.nkeys = nkeys, a.n_vocab = n_vocab, a.unk = unk, a.sos = sos, a.eos = eos, a.r = r, a.T = T;
  a.seed = seed, a.seed_dev = reinterpret_cast<const unsigned long long *>(seed_dev);
  a.ids = reinterpret_cast<long long *>(ids), a.tok = reinterpret_cast<long long *>(tok);
  a.ref = ref, a.good = good, a.length = length;
  hipLaunchKernelGGL(dense_xe_targets_kernel, dim3(a.groups), dim3(XE_THREADS), 0, spacap::as_stream(stream), a);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}
