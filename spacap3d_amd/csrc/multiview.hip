// Multiview image features projected onto scene points for gfx950 (MI355X): what the reference does per frame with a few
// dozen torch ops over all vertices, three host reads, a torch.inverse and a masked (N, C) update (lib/projection.py:189-260
// under the loops of scripts/project_multiview_features.py:190-222 and scripts/project_multiview_labels.py:303-356).
//
// The pixel of one point in one frame, every step f32 and un-contracted (this unit is compiled with -ffp-contract=off):
//   1. frustum: the eight camera-space corners (computed in double on the host, rounded to f32) go to world space by
//      camera_to_world, row r = ((m[r][0]*x + m[r][1]*y) + m[r][2]*z) + m[r][3]; six UN-normalised plane normals by the cross
//      products of lib/projection.py:85-118 (cross(a, b) = (ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx));
//   2. inside when rint(dot(p - c, n_k) * 100) < 0 for all six planes, dot = ((dx*nx + dy*ny) + dz*nz), c = corner 2 for
//      k < 3 and corner 4 for k >= 3.  (The reference divides the rounded value by 100 before it compares with 0: the sign
//      of an integer-valued float does not change under that division, so it is left out.)
//   3. cam = world_to_camera * [p, 1] (rows as in 1), x = cam.x * fx / cam.z + cx, y likewise, u = rint(x), v = rint(y)
//      (half to even); kept when 0 <= u < W and 0 <= v < H (a NaN fails every comparison); pix = v * W + u;
//   4. d = depth[pix]; kept when d >= depth_min, d <= depth_max and |d - cam.z| <= accuracy.
// world_to_camera is the cofactor inverse of camera_to_world in f64, rounded to f32 (mv_setup_kernel, one thread per frame);
// a frame whose pose has a non-finite entry, or whose inverse has one, maps nothing.
//
// mv_project_kernel, 128 threads per workgroup, one lane per point for the tests.  The workgroup owns its 128 points for the
// whole launch and walks the frames in chunks: the depth maps and the 37 set-up floats of up to MV_MAXCHUNK frames are staged
// in LDS, every lane tests its point against the chunk's frames in order and leaves the pixel (u16) in LDS.  Then each WAVE
// takes its own 64 points one after the other, those with a hit in the chunk only: the point's accumulator row comes into
// registers (lane = channel, + 64 per register), the chunk's hits are applied in frame order -- one contiguous C-float row
// of the pixel-major features per hit -- and the row goes back.  One wave owns a row for the whole launch: no atomics, no
// order between waves to get wrong, and the result does not depend on how the frames are split over calls.
// The gather is a chain of dependent loads per wave, so the launch lives on waves in flight: 29 952 B of LDS per workgroup
// let five workgroups share a CU, and the small workgroup keeps the last round of the grid short (measured, DESIGN 7f: 256
// threads with ten-frame chunks, two workgroups per CU, took 1.8 times as long).
// Aggregation ("covers" = mapped and the pixel's vector is not all-zero, (proj_feat == 0).sum(1) != C):
//   max    accumulator all-zero -> the vector, otherwise the element-wise maximum (an accumulator that a maximum turns
//          all-zero counts as unfilled again: the reference's quirk);
//   first  accumulator all-zero -> the vector;
//   vote   C = 1, labels 1..63: per point a row of 64 u32, [0] = the number of distinct labels seen, [l] = 0 when label l was
//          never seen, else (count << 6) | (63 - order of first appearance): the largest entry is the most frequent label, ties
//          to the one seen first.  The lane that owns the point keeps the row itself.
// Plain vector loads and stores only; no global atomics, no state besides the in/out arguments, no host synchronisation.
#include "common.hpp"

namespace {

constexpr int MV_THREADS = 128;
constexpr int MV_MAXCHUNK = 8;             // frames per LDS chunk, at most
constexpr int MV_DEPTH_FLOATS = 6656;      // 26 KiB of depth maps per chunk (41 x 32: five frames)
constexpr int MV_PARAMS = 40;              // floats per frame in the workspace (37 used)
constexpr int MV_MAXC = 256;               // channels: four registers per lane
constexpr int MV_CPL = MV_MAXC / 64;
constexpr int MV_NLABEL = 64;
constexpr unsigned short MV_MISS = 0xFFFF;
// workspace floats of one frame
constexpr int P_W2C = 0, P_NORMAL = 12, P_C2 = 30, P_C4 = 33, P_VALID = 36;

enum { MODE_MAP = 0, MODE_MAX = 1, MODE_FIRST = 2, MODE_VOTE = 3 };

struct MvCam {
  float fx, fy, cx, cy, dmin, dmax, acc;
  int W, H;
};

struct MvCorners {
  float c[8][3];
};

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.4028234663852886e38f; }

__device__ __forceinline__ void cross3(const float *a, const float *b, float *o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

__global__ void mv_setup_kernel(const float *__restrict__ pose, int F, MvCorners cc, float *__restrict__ ws) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const float *m = pose + (size_t)f * 16;
  float *o = ws + (size_t)f * MV_PARAMS;
  bool ok = true;
  double a[4][4];
  for (int i = 0; i < 16; ++i) {
    ok = ok && finite_f(m[i]);
    a[i >> 2][i & 3] = (double)m[i];
  }
  // cofactor inverse from the 2x2 minors of the upper (s) and lower (c) row pairs; rows 0..2 are all the projection needs
  const double s0 = a[0][0] * a[1][1] - a[1][0] * a[0][1], s1 = a[0][0] * a[1][2] - a[1][0] * a[0][2];
  const double s2 = a[0][0] * a[1][3] - a[1][0] * a[0][3], s3 = a[0][1] * a[1][2] - a[1][1] * a[0][2];
  const double s4 = a[0][1] * a[1][3] - a[1][1] * a[0][3], s5 = a[0][2] * a[1][3] - a[1][2] * a[0][3];
  const double c5 = a[2][2] * a[3][3] - a[3][2] * a[2][3], c4 = a[2][1] * a[3][3] - a[3][1] * a[2][3];
  const double c3 = a[2][1] * a[3][2] - a[3][1] * a[2][2], c2 = a[2][0] * a[3][3] - a[3][0] * a[2][3];
  const double c1 = a[2][0] * a[3][2] - a[3][0] * a[2][2], c0 = a[2][0] * a[3][1] - a[3][0] * a[2][1];
  const double det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
  double b[12];
  b[0] = (a[1][1] * c5 - a[1][2] * c4 + a[1][3] * c3) / det;
  b[1] = (-a[0][1] * c5 + a[0][2] * c4 - a[0][3] * c3) / det;
  b[2] = (a[3][1] * s5 - a[3][2] * s4 + a[3][3] * s3) / det;
  b[3] = (-a[2][1] * s5 + a[2][2] * s4 - a[2][3] * s3) / det;
  b[4] = (-a[1][0] * c5 + a[1][2] * c2 - a[1][3] * c1) / det;
  b[5] = (a[0][0] * c5 - a[0][2] * c2 + a[0][3] * c1) / det;
  b[6] = (-a[3][0] * s5 + a[3][2] * s2 - a[3][3] * s1) / det;
  b[7] = (a[2][0] * s5 - a[2][2] * s2 + a[2][3] * s1) / det;
  b[8] = (a[1][0] * c4 - a[1][1] * c2 + a[1][3] * c0) / det;
  b[9] = (-a[0][0] * c4 + a[0][1] * c2 - a[0][3] * c0) / det;
  b[10] = (a[3][0] * s4 - a[3][1] * s2 + a[3][3] * s0) / det;
  b[11] = (-a[2][0] * s4 + a[2][1] * s2 - a[2][3] * s0) / det;
  for (int i = 0; i < 12; ++i) {
    const float v = (float)b[i];
    ok = ok && finite_f(v);
    o[P_W2C + i] = v;
  }
  float w[8][3];   // the frustum's corners in world space
  for (int k = 0; k < 8; ++k)
    for (int r = 0; r < 3; ++r)
      w[k][r] = ((m[r * 4 + 0] * cc.c[k][0] + m[r * 4 + 1] * cc.c[k][1]) + m[r * 4 + 2] * cc.c[k][2]) + m[r * 4 + 3];
  // (from, to) corner pairs of the two edge vectors of each plane: front, right, roof, left, bottom, back
  const int e[6][4] = {{0, 3, 0, 1}, {1, 2, 1, 5}, {2, 3, 2, 6}, {3, 0, 3, 7}, {0, 1, 0, 4}, {5, 6, 5, 4}};
  for (int k = 0; k < 6; ++k) {
    float v1[3], v2[3];
    for (int r = 0; r < 3; ++r) {
      v1[r] = w[e[k][1]][r] - w[e[k][0]][r];
      v2[r] = w[e[k][3]][r] - w[e[k][2]][r];
    }
    cross3(v1, v2, o + P_NORMAL + 3 * k);
  }
  for (int r = 0; r < 3; ++r) {
    o[P_C2 + r] = w[2][r];
    o[P_C4 + r] = w[4][r];
  }
  o[P_VALID] = ok ? 1.f : 0.f;
  o[37] = o[38] = o[39] = 0.f;
}

// the pixel of point (px, py, pz) in the frame whose set-up floats are P and whose depth map is `depth` (both LDS), or -1
__device__ __forceinline__ int mv_pixel(const float *P, const float *depth, float px, float py, float pz, const MvCam &cam) {
  if (P[P_VALID] == 0.f) return -1;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float *c = P + (k < 3 ? P_C2 : P_C4), *n = P + P_NORMAL + 3 * k;
    const float d = ((px - c[0]) * n[0] + (py - c[1]) * n[1]) + (pz - c[2]) * n[2];
    if (!(rintf(d * 100.f) < 0.f)) return -1;
  }
  const float *m = P + P_W2C;
  const float x = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3];
  const float y = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7];
  const float z = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11];
  const float u = rintf(x * cam.fx / z + cam.cx), v = rintf(y * cam.fy / z + cam.cy);
  if (!(u >= 0.f && u < (float)cam.W && v >= 0.f && v < (float)cam.H)) return -1;
  const int pix = (int)v * cam.W + (int)u;        // < W * H <= MV_DEPTH_FLOATS: inside the staged map
  const float d = depth[pix];
  if (!(d >= cam.dmin && d <= cam.dmax && fabsf(d - z) <= cam.acc)) return -1;
  return pix;
}

struct MvArgs {
  const float *points;   // [N,3]
  const float *depth;    // [F,H*W]
  const float *ws;       // [F,MV_PARAMS]
  int N, F, chunk, C;
  MvCam cam;
  int32_t *map;          // MODE_MAP: [F,N]
  const float *feats;    // MODE_MAX / MODE_FIRST: [F,H*W,C]
  float *acc;            //   [N,C] in/out
  const int32_t *labels; // MODE_VOTE: [F,H*W]
  uint32_t *state;       //   [N,64] in/out
  int32_t *voted;        //   [N]
};

template <int MODE>
__global__ __launch_bounds__(MV_THREADS) void mv_project_kernel(MvArgs a) {
  __shared__ float s_depth[MV_DEPTH_FLOATS];
  __shared__ float s_par[MV_MAXCHUNK * MV_PARAMS];
  __shared__ unsigned short s_pix[MV_MAXCHUNK][MV_THREADS];
  const int tid = threadIdx.x, lane = tid & 63, wave0 = tid & ~63;
  const int N = a.N, F = a.F, HW = a.cam.W * a.cam.H, C = a.C;
  const long long base = (long long)blockIdx.x * MV_THREADS;
  const long long p = base + tid;
  const bool have = p < N;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (have) {
    px = a.points[p * 3 + 0];
    py = a.points[p * 3 + 1];
    pz = a.points[p * 3 + 2];
  }
  uint32_t *row = MODE == MODE_VOTE && have ? a.state + p * MV_NLABEL : nullptr;

  for (int f0 = 0; f0 < F; f0 += a.chunk) {
    const int nf = min(a.chunk, F - f0);
    __syncthreads();                                   // the chunk before is done with
    for (int i = tid; i < nf * HW; i += MV_THREADS) s_depth[i] = a.depth[(size_t)f0 * HW + i];
    for (int i = tid; i < nf * MV_PARAMS; i += MV_THREADS) s_par[i] = a.ws[(size_t)f0 * MV_PARAMS + i];
    __syncthreads();

    bool any = false;
    for (int j = 0; j < nf; ++j) {
      const int pix = have ? mv_pixel(s_par + j * MV_PARAMS, s_depth + j * HW, px, py, pz, a.cam) : -1;
      if (MODE == MODE_MAP) {
        if (have) a.map[(size_t)(f0 + j) * N + p] = pix;
      } else if (MODE == MODE_VOTE) {
        if (pix >= 0) {
          const int lab = a.labels[(size_t)(f0 + j) * HW + pix];
          if (lab >= 1 && lab < MV_NLABEL) {
            uint32_t u = row[lab];
            if (u == 0) {
              const uint32_t order = row[0];
              row[0] = order + 1;
              u = 63u - order;
            }
            row[lab] = u + 64u;
          }
        }
      } else {
        s_pix[j][tid] = pix < 0 ? MV_MISS : (unsigned short)pix;
        any = any || pix >= 0;
      }
    }

    if (MODE == MODE_MAX || MODE == MODE_FIRST) {
      __syncthreads();                                 // s_pix is read across lanes
      unsigned long long todo = __ballot(any);         // this wave's points with a hit in the chunk
      while (todo) {
        const int q = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        float *arow = a.acc + (size_t)(base + wave0 + q) * C;
        float acc[MV_CPL];
#pragma unroll
        for (int i = 0; i < MV_CPL; ++i) acc[i] = lane + 64 * i < C ? arow[lane + 64 * i] : 0.f;
        bool changed = false;
        for (int j = 0; j < nf; ++j) {
          const unsigned short pix = s_pix[j][wave0 + q];   // one address for the wave: a broadcast
          if (pix == MV_MISS) continue;
          const float *frow = a.feats + ((size_t)(f0 + j) * HW + pix) * C;
          float v[MV_CPL];
          bool vnz = false, anz = false;
#pragma unroll
          for (int i = 0; i < MV_CPL; ++i) {
            v[i] = lane + 64 * i < C ? frow[lane + 64 * i] : 0.f;
            vnz = vnz || v[i] != 0.f;
            anz = anz || acc[i] != 0.f;
          }
          if (!__ballot(vnz)) continue;                // an all-zero vector does not cover the point
          const bool filled = __ballot(anz) != 0;
          if (filled && MODE == MODE_FIRST) continue;
#pragma unroll
          for (int i = 0; i < MV_CPL; ++i)             // torch.max: a NaN on either side stays
            acc[i] = filled ? ((acc[i] != acc[i] || acc[i] >= v[i]) ? acc[i] : v[i]) : v[i];
          changed = true;
        }
        if (changed) {
#pragma unroll
          for (int i = 0; i < MV_CPL; ++i)
            if (lane + 64 * i < C) arow[lane + 64 * i] = acc[i];
        }
      }
    }
  }

  if (MODE == MODE_VOTE && have) {
    uint32_t best = 0;
    int label = 0;
    for (int l = 1; l < MV_NLABEL; ++l) {
      const uint32_t u = row[l];
      if (u > best) {
        best = u;
        label = l;
      }
    }
    a.voted[p] = label;
  }
}

int mv_chunk(int H, int W) { return min(MV_MAXCHUNK, MV_DEPTH_FLOATS / (H * W)); }

// Argument checks shared by the three entry points, the set-up launch, and the fields of MvArgs they have in common.
// `others`: the entry point's own pointers are all there.  Returns 1 when there is nothing to do, 0 to go on, a negative code
// on an error.
int mv_prepare(const char *what, const float *points, int N, const float *depth, const float *pose, int F, int H, int W,
               float fx, float fy, float cx, float cy, float depth_min, float depth_max, float accuracy, const float *corners,
               void *workspace, size_t workspace_bytes, bool others, hipStream_t stream, MvArgs &a) {
  SPACAP_REQUIRE(N >= 0 && F >= 0 && H >= 1 && W >= 1 && (long long)H * W <= MV_DEPTH_FLOATS,
                 "%s: bad sizes (N=%d F=%d H=%d W=%d; H * W <= %d)", what, N, F, H, W, MV_DEPTH_FLOATS);
  if (N == 0 || F == 0) return 1;
  SPACAP_REQUIRE(points && depth && pose && corners && workspace && others, "%s: null pointer", what);
  SPACAP_REQUIRE(workspace_bytes >= spacap_multiview_workspace_bytes(F), "%s: workspace of %zu bytes, %zu needed", what,
                 workspace_bytes, spacap_multiview_workspace_bytes(F));
  MvCorners cc;
  for (int i = 0; i < 24; ++i) cc.c[i / 3][i % 3] = corners[i];
  float *ws = static_cast<float *>(workspace);
  hipLaunchKernelGGL(mv_setup_kernel, dim3((F + 63) / 64), dim3(64), 0, stream, pose, F, cc, ws);
  SPACAP_CHECK_LAUNCH(what);
  a.points = points;
  a.depth = depth;
  a.ws = ws;
  a.N = N;
  a.F = F;
  a.chunk = mv_chunk(H, W);
  a.C = 1;
  a.cam = MvCam{fx, fy, cx, cy, depth_min, depth_max, accuracy, W, H};
  a.map = nullptr;
  a.feats = nullptr;
  a.acc = nullptr;
  a.labels = nullptr;
  a.state = nullptr;
  a.voted = nullptr;
  return 0;
}

template <int MODE>
int mv_launch(const char *what, const MvArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(mv_project_kernel<MODE>, dim3((unsigned)(((long long)a.N + MV_THREADS - 1) / MV_THREADS)), dim3(MV_THREADS), 0, stream, a);
  SPACAP_CHECK_LAUNCH(what);
  return SPACAP_OK;
}

}  // namespace

extern "C" size_t spacap_multiview_workspace_bytes(int F) { return (size_t)(F > 0 ? F : 0) * MV_PARAMS * sizeof(float); }

extern "C" int spacap_multiview_map_f32(const float *points, int N, const float *depth, const float *pose, int F, int H, int W,
                                        float fx, float fy, float cx, float cy, float depth_min, float depth_max, float accuracy,
                                        const float *corners, void *workspace, size_t workspace_bytes, int32_t *map,
                                        spacap_stream_t stream) {
  const char *what = "spacap_multiview_map_f32";
  MvArgs a;
  const int r = mv_prepare(what, points, N, depth, pose, F, H, W, fx, fy, cx, cy, depth_min, depth_max, accuracy, corners,
                           workspace, workspace_bytes, map != nullptr, spacap::as_stream(stream), a);
  if (r) return r < 0 ? r : SPACAP_OK;
  a.map = map;
  return mv_launch<MODE_MAP>(what, a, spacap::as_stream(stream));
}

extern "C" int spacap_multiview_features_f32(const float *points, int N, const float *depth, const float *pose, int F, int H,
                                             int W, float fx, float fy, float cx, float cy, float depth_min, float depth_max,
                                             float accuracy, const float *corners, const float *feats, int C, int mode,
                                             void *workspace, size_t workspace_bytes, float *acc, spacap_stream_t stream) {
  const char *what = "spacap_multiview_features_f32";
  SPACAP_REQUIRE(C >= 1 && C <= MV_MAXC && (mode == 0 || mode == 1), "%s: bad sizes (C=%d mode=%d; C <= %d, mode 0 = max, 1 = first)",
                 what, C, mode, MV_MAXC);
  MvArgs a;
  const int r = mv_prepare(what, points, N, depth, pose, F, H, W, fx, fy, cx, cy, depth_min, depth_max, accuracy, corners,
                           workspace, workspace_bytes, feats && acc, spacap::as_stream(stream), a);
  if (r) return r < 0 ? r : SPACAP_OK;
  a.feats = feats;
  a.acc = acc;
  a.C = C;
  return mode == 0 ? mv_launch<MODE_MAX>(what, a, spacap::as_stream(stream))
                   : mv_launch<MODE_FIRST>(what, a, spacap::as_stream(stream));
}

extern "C" int spacap_multiview_vote_i32(const float *points, int N, const float *depth, const float *pose, int F, int H, int W,
                                         float fx, float fy, float cx, float cy, float depth_min, float depth_max, float accuracy,
                                         const float *corners, const int32_t *labels, void *workspace, size_t workspace_bytes,
                                         uint32_t *state, int32_t *voted, spacap_stream_t stream) {
  const char *what = "spacap_multiview_vote_i32";
  MvArgs a;
  const int r = mv_prepare(what, points, N, depth, pose, F, H, W, fx, fy, cx, cy, depth_min, depth_max, accuracy, corners,
                           workspace, workspace_bytes, labels && state && voted, spacap::as_stream(stream), a);
  if (r) return r < 0 ? r : SPACAP_OK;
  a.labels = labels;
  a.state = state;
  a.voted = voted;
  return mv_launch<MODE_VOTE>(what, a, spacap::as_stream(stream));
}
