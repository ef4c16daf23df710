// ScanNet scene preparation for gfx950 (MI355X): decoded mesh arrays in, the per-scene arrays DeviceSceneDataset loads out
// (DESIGN.md section 7h).  Replaces data/scannet/load_scannet_data.py::export with scannet_utils.compute_normal, and the
// save_npy path of data/scannet/generate_spatiality_label.py.  Every result is a bit-exact restatement of what numpy computes
// there, so this unit is compiled with -ffp-contract=off; division and square root are the correctly rounded f32 ones.
//
// Normals (all f32).  Per face n = cross(v1 - v0, v2 - v0), a component = two rounded products and a rounded difference;
// len = sqrt((nx*nx + ny*ny) + nz*nz); n /= (len + 1e-8f).  The reference then adds n to its three corners with a fancy-indexed
// "+=", which numpy buffers: for a vertex that several faces use as corner c, only the LAST of them (file order) arrives.
// So normal[v] = ((0 + n[f_0]) + n[f_1]) + n[f_2], f_c = the largest face index with faces[f][c] == v (a missing corner adds
// nothing), normalised by the same formula.  Degenerate faces and isolated vertices give exact zeros.
//   se_init_kernel       the (3, N) last-face table to -1 and the box extrema to their neutral values: the workspace needs
//                        nothing from the caller and a repeated call starts clean;
//   se_last_face_kernel  one thread per face, atomicMax of the face index into the table: "the last write wins";
//   se_vertex_kernel     one thread per vertex: the up to three face normals recomputed from xyz, added in corner order and
//                        normalised; the alignment row r = ((x*A[r][0] + y*A[r][1]) + z*A[r][2]) + A[r][3] in f64, rounded to
//                        f32 (normals and colours are copied, the reference does not rotate them; without a matrix the
//                        aligned rows are the raw ones); ins = seg_ins[seg[v]], sem = seg_sem[seg[v]]; min / max of the raw
//                        and the aligned position into row ins - 1 of the extrema, by vector atomics on an order-preserving
//                        u32 image of the f32 (-0.0 sorts below +0.0; positions are finite) -- reduced over the wave first
//                        when all of its vertices belong to one instance, which mesh order makes the common case;
//   se_boxes_kernel      one thread per instance: centre (min + max) / 2 and size max - min in f32, widened into the f64 row
//                        [centre, size, label id, object id]; an instance without a vertex keeps an all-zero row;
//   se_relations_kernel  one thread per (i, j): the three relation classes from the f64 boxes, in the reference's expression
//                        order (see the functions below).
// min / max do not depend on the order of the atomics, so every output is deterministic.
// Indices are validated by the caller (spacap3d_amd/scene_export.py); the kernels still skip an index outside its table
// instead of following it.
#include "common.hpp"

namespace {

constexpr int SE_THREADS = 256;
constexpr int SE_MAX_INSTANCES = 1024;
constexpr int SE_MAX_VERTICES = 1 << 24;
constexpr int SE_EXT = 12;                 // per instance: raw min xyz, raw max xyz, aligned min xyz, aligned max xyz
constexpr uint32_t SE_MIN_NEUTRAL = 0xFFFFFFFFu, SE_MAX_NEUTRAL = 0u;

struct SeAlign {
  double a[12];     // rows 0..2 of the 4 x 4 matrix
  int on;
};

// order-preserving u32 image of a finite f32
__device__ __forceinline__ uint32_t se_encode(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float se_decode(uint32_t e) {
  return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e);
}

__global__ __launch_bounds__(SE_THREADS) void se_init_kernel(int32_t *__restrict__ table, long long n_table,
                                                             uint32_t *__restrict__ ext, int n_ext) {
  const long long stride = (long long)gridDim.x * SE_THREADS;
  for (long long i = (long long)blockIdx.x * SE_THREADS + threadIdx.x; i < n_table + n_ext; i += stride) {
    if (i < n_table) {
      table[i] = -1;
    } else {
      const int k = (int)(i - n_table);
      ext[k] = (k % 6) < 3 ? SE_MIN_NEUTRAL : SE_MAX_NEUTRAL;
    }
  }
}

__global__ __launch_bounds__(SE_THREADS) void se_last_face_kernel(const int32_t *__restrict__ faces, int F, int N,
                                                                  int32_t *__restrict__ table) {
  const long long f = (long long)blockIdx.x * SE_THREADS + threadIdx.x;
  if (f >= F) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int v = faces[f * 3 + c];
    if ((unsigned)v < (unsigned)N) atomicMax(&table[(size_t)c * N + v], (int)f);
  }
}

__device__ __forceinline__ void se_normalize(float *n) {
  const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
  const float d = len + 1e-8f;
  n[0] = n[0] / d;
  n[1] = n[1] / d;
  n[2] = n[2] / d;
}

__device__ __forceinline__ void se_face_normal(const float *__restrict__ xyz, const int32_t *__restrict__ faces, int N,
                                               int f, float *n) {
  float p[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int v = faces[(size_t)f * 3 + c];
    if ((unsigned)v >= (unsigned)N) v = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) p[c][k] = xyz[(size_t)v * 3 + k];
  }
  const float a0 = p[1][0] - p[0][0], a1 = p[1][1] - p[0][1], a2 = p[1][2] - p[0][2];
  const float b0 = p[2][0] - p[0][0], b1 = p[2][1] - p[0][1], b2 = p[2][2] - p[0][2];
  n[0] = a1 * b2 - a2 * b1;
  n[1] = a2 * b0 - a0 * b2;
  n[2] = a0 * b1 - a1 * b0;
  se_normalize(n);
}

struct SeVertexArgs {
  const float *xyz;        // [N,3]
  const float *rgb;        // [N,3]
  const int32_t *faces;    // [F,3]
  const int32_t *table;    // [3,N]
  const int32_t *seg;      // [N]
  const int32_t *seg_ins;  // [S]
  const int32_t *seg_sem;  // [S]
  int N, S, M;
  SeAlign align;
  uint32_t *ext;           // [M,12]
  float *normals;          // normals only: [N,3]
  float *vert;             // [N,9]
  float *aligned_vert;     // [N,9]
  int32_t *ins;            // [N]
  int32_t *sem;            // [N]
};

template <bool FULL>
__global__ __launch_bounds__(SE_THREADS) void se_vertex_kernel(SeVertexArgs a) {
  const long long v = (long long)blockIdx.x * SE_THREADS + threadIdx.x;
  const bool have = v < a.N;             // no early return: the wave reduction below needs every lane
  float n[3] = {0.f, 0.f, 0.f};
  float p[3] = {0.f, 0.f, 0.f}, q[3] = {0.f, 0.f, 0.f};
  int ins = 0;
  if (have) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int f = a.table[(size_t)c * a.N + v];
      if (f >= 0) {
        float fn[3];
        se_face_normal(a.xyz, a.faces, a.N, f, fn);
        n[0] = n[0] + fn[0];
        n[1] = n[1] + fn[1];
        n[2] = n[2] + fn[2];
      }
    }
    se_normalize(n);
    if (!FULL) {
#pragma unroll
      for (int k = 0; k < 3; ++k) a.normals[v * 3 + k] = n[k];
    }
  }
  if (!FULL) return;

  if (have) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = q[k] = a.xyz[v * 3 + k];
    if (a.align.on) {
      const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double *m = a.align.a + 4 * r;
        q[r] = (float)(((x * m[0] + y * m[1]) + z * m[2]) + m[3]);
      }
    }
    float *o = a.vert + v * 9, *oa = a.aligned_vert + v * 9;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float c = a.rgb[v * 3 + k];
      o[k] = p[k];
      oa[k] = q[k];
      o[3 + k] = oa[3 + k] = c;
      o[6 + k] = oa[6 + k] = n[k];
    }
    const int s = a.seg[v];
    int sem = 0;
    if ((unsigned)s < (unsigned)a.S) {
      ins = a.seg_ins[s];
      sem = a.seg_sem[s];
    }
    a.ins[v] = ins;
    a.sem[v] = sem;
  }

  // ---- box extrema, keyed by instance ----
  const int key = (have && ins >= 1 && ins <= a.M) ? ins : 0;
  uint32_t e[SE_EXT];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    e[k] = key ? se_encode(p[k]) : SE_MIN_NEUTRAL;
    e[3 + k] = key ? se_encode(p[k]) : SE_MAX_NEUTRAL;
    e[6 + k] = key ? se_encode(q[k]) : SE_MIN_NEUTRAL;
    e[9 + k] = key ? se_encode(q[k]) : SE_MAX_NEUTRAL;
  }
  const int k0 = __builtin_amdgcn_readfirstlane(key);
  if (__all(!have || key == k0)) {        // one instance for the whole wave (lanes past N hold the neutral values)
    if (k0 == 0) return;
#pragma unroll
    for (int k = 0; k < SE_EXT; ++k)
      e[k] = (k % 6) < 3 ? spacap::wave_min<64, uint32_t>(e[k]) : spacap::wave_max<64, uint32_t>(e[k]);
    if ((threadIdx.x & 63) == 0) {
      uint32_t *row = a.ext + (size_t)(k0 - 1) * SE_EXT;
#pragma unroll
      for (int k = 0; k < SE_EXT; ++k) {
        if ((k % 6) < 3) atomicMin(&row[k], e[k]);
        else atomicMax(&row[k], e[k]);
      }
    }
  } else if (key) {
    uint32_t *row = a.ext + (size_t)(key - 1) * SE_EXT;
#pragma unroll
    for (int k = 0; k < SE_EXT; ++k) {
      if ((k % 6) < 3) atomicMin(&row[k], e[k]);
      else atomicMax(&row[k], e[k]);
    }
  }
}

__global__ __launch_bounds__(SE_THREADS) void se_boxes_kernel(const uint32_t *__restrict__ ext,
                                                              const int32_t *__restrict__ box_label, int M,
                                                              double *__restrict__ bbox, double *__restrict__ aligned_bbox) {
  const int m = blockIdx.x * SE_THREADS + threadIdx.x;
  if (m >= M) return;
  const uint32_t *row = ext + (size_t)m * SE_EXT;
  const bool empty = row[0] == SE_MIN_NEUTRAL;     // no finite f32 encodes to the neutral value
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    double *o = (w ? aligned_bbox : bbox) + (size_t)m * 8;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float lo = se_decode(row[6 * w + k]), hi = se_decode(row[6 * w + 3 + k]);
      const float centre = (lo + hi) / 2.f, size = hi - lo;
      o[k] = empty ? 0.0 : (double)centre;
      o[3 + k] = empty ? 0.0 : (double)size;
    }
    o[6] = empty ? 0.0 : (double)box_label[m];
    o[7] = empty ? 0.0 : (double)m;
  }
}

// ---- relations: generate_spatiality_label.py:49-141 with save_npy=True, on [centre, size, ...] f64 rows ----
// Classes: 0 = forward / up, 1 = same, 2 = behind / below.  The reference's chain of transposed index assignments reduces to
//   class[i][j] = 1 if zero[i][j] or zero[j][i], else 2 if f1[j][i], else 0 if f1[i][j], else 1     (x and y)
//   class[i][j] = 2 if up[j][i], else 0 if up[i][j], else 1                                            (z)
struct SeSpan {
  double mn, mx, first, second, eps;
};
__device__ __forceinline__ SeSpan se_span(double c, double s) {
  SeSpan r;
  r.mn = c - s * 0.5;
  r.mx = c + s * 0.5;
  r.first = r.mn + s * 0.3;
  r.second = r.mn + s * 0.7;
  r.eps = s * 0.1;
  return r;
}
__device__ __forceinline__ bool se_zero(const SeSpan &a, const SeSpan &b) {
  return fabs(a.mx - b.mx) <= b.eps && fabs(a.mn - b.mn) <= b.eps;
}
__device__ __forceinline__ bool se_fwd0(const SeSpan &a, const SeSpan &b) {
  return (a.mx > b.mx && a.mn >= b.mn) || (a.mx <= b.mx && a.mx > b.second && a.mn > b.first);
}
__device__ __forceinline__ bool se_back(const SeSpan &a, const SeSpan &b) {
  return a.mx < b.second && a.mn > b.mn && a.mn < b.first;
}
__device__ __forceinline__ int se_class_xy(double ci, double si, double cj, double sj) {
  const SeSpan a = se_span(ci, si), b = se_span(cj, sj);
  if (se_zero(a, b) || se_zero(b, a)) return 1;
  if (se_fwd0(b, a) || se_back(a, b)) return 2;      // f1[j][i]
  if (se_fwd0(a, b) || se_back(b, a)) return 0;      // f1[i][j]
  return 1;
}
__device__ __forceinline__ int se_class_z(double ci, double si, double cj, double sj) {
  const double zi = ci - si * 0.5, zj = cj - sj * 0.5;
  if (zj - zi >= 0.3 * si) return 2;                  // up[j][i]
  if (zi - zj >= 0.3 * sj) return 0;                  // up[i][j]
  return 1;
}

__global__ __launch_bounds__(SE_THREADS) void se_relations_kernel(const double *__restrict__ bbox, int M,
                                                                  int32_t *__restrict__ rel) {
  const int t = blockIdx.x * SE_THREADS + threadIdx.x;     // M * M <= 2^20
  if (t >= M * M) return;
  const int i = t / M, j = t - i * M;
  const double *bi = bbox + (size_t)i * 8, *bj = bbox + (size_t)j * 8;
  rel[t] = se_class_xy(bi[0], bi[3], bj[0], bj[3]);
  rel[(size_t)M * M + t] = se_class_xy(bi[1], bi[4], bj[1], bj[4]);
  rel[(size_t)2 * M * M + t] = se_class_z(bi[2], bi[5], bj[2], bj[5]);
}

unsigned se_blocks(long long n) { return (unsigned)((n + SE_THREADS - 1) / SE_THREADS); }

size_t se_workspace_bytes(int N, int M) {
  const size_t words = (size_t)3 * (N > 0 ? N : 0) + (size_t)SE_EXT * (M > 0 ? M : 0);
  return (words * 4 + 15) & ~(size_t)15;
}

// the two launches of the last-face stage
int se_last_faces(const char *what, const int32_t *faces, int F, int N, int M, int32_t *table, uint32_t *ext,
                  hipStream_t stream) {
  const long long n_init = 3LL * N + (long long)SE_EXT * M;
  const unsigned init_blocks = se_blocks(n_init) < 4096u ? se_blocks(n_init) : 4096u;
  hipLaunchKernelGGL(se_init_kernel, dim3(init_blocks), dim3(SE_THREADS), 0, stream, table, 3LL * N, ext, SE_EXT * M);
  SPACAP_CHECK_LAUNCH(what);
  if (F > 0) {
    hipLaunchKernelGGL(se_last_face_kernel, dim3(se_blocks(F)), dim3(SE_THREADS), 0, stream, faces, F, N, table);
    SPACAP_CHECK_LAUNCH(what);
  }
  return SPACAP_OK;
}

int se_relations(const char *what, const double *bbox, int M, int32_t *rel, hipStream_t stream) {
  hipLaunchKernelGGL(se_relations_kernel, dim3(se_blocks((long long)M * M)), dim3(SE_THREADS), 0, stream, bbox, M, rel);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

}  // namespace

extern "C" size_t spacap_scene_export_workspace_bytes(int N, int M) { return se_workspace_bytes(N, M); }

extern "C" int spacap_scene_normals_f32(const float *xyz, int N, const int32_t *faces, int F, void *workspace,
                                        size_t workspace_bytes, float *normals, spacap_stream_t stream) {
  const char *what = "spacap_scene_normals_f32";
  SPACAP_REQUIRE(N >= 0 && N < SE_MAX_VERTICES && F >= 0, "%s: bad sizes (N=%d F=%d; N < %d)", what, N, F, SE_MAX_VERTICES);
  if (N == 0) return SPACAP_OK;
  SPACAP_REQUIRE(xyz && (faces || F == 0) && workspace && normals, "%s: null pointer", what);
  SPACAP_REQUIRE(workspace_bytes >= se_workspace_bytes(N, 0), "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes,
                 se_workspace_bytes(N, 0));
  hipStream_t st = spacap::as_stream(stream);
  int32_t *table = static_cast<int32_t *>(workspace);
  const int r = se_last_faces(what, faces, F, N, 0, table, nullptr, st);
  if (r) return r;
  SeVertexArgs a = {};
  a.xyz = xyz;
  a.faces = faces;
  a.table = table;
  a.N = N;
  a.normals = normals;
  hipLaunchKernelGGL(se_vertex_kernel<false>, dim3(se_blocks(N)), dim3(SE_THREADS), 0, st, a);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

extern "C" int spacap_scene_relations_f64(const double *bbox, int M, int32_t *rel, spacap_stream_t stream) {
  const char *what = "spacap_scene_relations_f64";
  SPACAP_REQUIRE(M >= 0 && M <= SE_MAX_INSTANCES, "%s: bad sizes (M=%d; M <= %d)", what, M, SE_MAX_INSTANCES);
  if (M == 0) return SPACAP_OK;
  SPACAP_REQUIRE(bbox && rel, "%s: null pointer", what);
  return se_relations(what, bbox, M, rel, spacap::as_stream(stream));
}

extern "C" int spacap_scene_export_f32(const float *xyz, const float *rgb, int N, const int32_t *faces, int F,
                                       const int32_t *seg, const int32_t *seg_ins, const int32_t *seg_sem, int S,
                                       const int32_t *box_label, int M, const double *axis_align, void *workspace,
                                       size_t workspace_bytes, float *vert, float *aligned_vert, int32_t *ins, int32_t *sem,
                                       double *bbox, double *aligned_bbox, int32_t *rel, spacap_stream_t stream) {
  const char *what = "spacap_scene_export_f32";
  SPACAP_REQUIRE(N >= 0 && N < SE_MAX_VERTICES && F >= 0 && S >= 1 && M >= 1 && M <= SE_MAX_INSTANCES,
                 "%s: bad sizes (N=%d F=%d S=%d M=%d; N < %d, S >= 1, 1 <= M <= %d)", what, N, F, S, M, SE_MAX_VERTICES,
                 SE_MAX_INSTANCES);
  if (N == 0) return SPACAP_OK;
  SPACAP_REQUIRE(xyz && rgb && (faces || F == 0) && seg && seg_ins && seg_sem && box_label && workspace && vert &&
                     aligned_vert && ins && sem && bbox && aligned_bbox && rel,
                 "%s: null pointer", what);
  SPACAP_REQUIRE(workspace_bytes >= se_workspace_bytes(N, M), "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes,
                 se_workspace_bytes(N, M));
  hipStream_t st = spacap::as_stream(stream);
  int32_t *table = static_cast<int32_t *>(workspace);
  uint32_t *ext = reinterpret_cast<uint32_t *>(table + (size_t)3 * N);
  int r = se_last_faces(what, faces, F, N, M, table, ext, st);
  if (r) return r;
  SeVertexArgs a = {};
  a.xyz = xyz;
  a.rgb = rgb;
  a.faces = faces;
  a.table = table;
  a.seg = seg;
  a.seg_ins = seg_ins;
  a.seg_sem = seg_sem;
  a.N = N;
  a.S = S;
  a.M = M;
  a.align.on = axis_align != nullptr;
  for (int i = 0; i < 12; ++i) a.align.a[i] = axis_align ? axis_align[i] : 0.0;
  a.ext = ext;
  a.vert = vert;
  a.aligned_vert = aligned_vert;
  a.ins = ins;
  a.sem = sem;
  hipLaunchKernelGGL(se_vertex_kernel<true>, dim3(se_blocks(N)), dim3(SE_THREADS), 0, st, a);
  SPACAP_CHECK_LAUNCH(what);
  hipLaunchKernelGGL(se_boxes_kernel, dim3(se_blocks(M)), dim3(SE_THREADS), 0, st, ext, box_label, M, bbox, aligned_bbox);
  SPACAP_CHECK_LAUNCH(what);
  return se_relations(what, aligned_bbox, M, rel, st);
}
