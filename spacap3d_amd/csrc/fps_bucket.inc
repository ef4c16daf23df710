// Spatially bucketed furthest-point sampling with EXACT pruning -- the large-scene path of fps.hip.
// (Also included by tools/lab/fps_bucket_lab.hip, the stand-alone timing / verification harness.)
//
// Observation: after j samples the running minimum distance of almost every point is far smaller than its
// distance to the next sample, so the reference's O(N) update per round mostly rewrites values with themselves.
// If the points a wavefront owns are spatially compact, a whole 256-point bucket can be skipped when the squared
// distance from the new sample to the bucket's bounding box is >= the bucket's current maximum temp: every point
// then has d >= temp and fminf(d, temp) leaves temp untouched -- the result is bit-identical to the reference's.
//
// Prologue (once per launch, inside the one workgroup that owns the scene): counting sort of the scene by a
// 12-bit Morton cell (4096-bin LDS histogram, scan, scatter) into a structure-of-arrays copy in the caller's
// workspace; slot -> original index map kept in LDS (u16).  The order inside a cell depends on atomic arrival
// order, which is harmless: the layout only decides what can be skipped, never a result.
// Round: lanes 0..NB-1 of each wave test their wave's NB buckets (box distance vs bucket max), one ballot gives
// the wave-uniform to-do mask; touched buckets stream their coordinates from L2 (coalesced 16-byte loads), update
// temp in VGPRs and refresh the bucket max with a DPP reduction; the arg-max needs only the bucket maxima (SGPRs).
// The index of the maximum is recovered as in fps.hip: min over fps_key (common.hpp) of the points that hold the
// maximum, k being the ORIGINAL index.
// Each wave caches its own candidate (value, key, xyz) and recomputes it only when the bucket holding it was
// touched; one LDS exchange + ONE barrier per round decides the winner and hands its coordinates to everyone.
__device__ __forceinline__ unsigned fpsb_spread4(unsigned q) {  // bits 0..3 -> positions 0,3,6,9
  return (q & 1u) | ((q & 2u) << 2) | ((q & 4u) << 4) | ((q & 8u) << 6);
}

// The NB template instance launch_fps_bucket dispatches for N points: ceil(N / 4096) rounded UP to an instantiated
// value.  The kernel lays its planes out with NPAD = NB * 4096 slots per scene, so the workspace must be sized from
// THIS value, not from ceil(N / 4096) (they differ for nb = 7, 9, 11, 13-15, 17-19).
static inline int fps_bucket_nb(int N) {
  const int nb = (N + 4095) / 4096;
  if (N <= 65535) {
    const int inst[] = {3, 4, 5, 6, 8, 10, 12, 16};
    for (int v : inst)
      if (nb <= v) return v;
  }
  return nb <= 16 ? 16 : 20;
}
static inline size_t fps_bucket_workspace_floats(int N) {
  // x / y / z planes in bucket order (+ the 32-bit slot -> index map when it does not fit LDS as u16)
  return (size_t)(N <= 65535 ? 3 : 4) * fps_bucket_nb(N) * 4096;
}

// NB buckets of 256 points per wave (64 lanes x 4 consecutive slots), 16 waves: NPAD = NB * 4096 slots.
// Bucket g (Morton order) belongs to wave g % 16: the handful of spatially adjacent buckets a new sample touches
// are then updated by different waves in parallel instead of one wave paying their L2 round trips back to back.
// PERM_LDS: slot -> original index map as u16 in LDS (N <= 65 535); otherwise as u32 behind the planes in the
// workspace (read only when a wave recomputes its candidate).
template <int NB, bool PERM_LDS>
__global__ __launch_bounds__(1024) void fps_bucket_kernel(const float *__restrict__ xyz_all,
                                                          float *__restrict__ ws_all, int N, int m, int lg,
                                                          int32_t *__restrict__ idx_all) {
  constexpr int BLOCK = 1024, NW = 16, NPAD = NB * 4096, NCELL = 4096;
  __shared__ unsigned short s_perm[PERM_LDS ? NPAD : 2];  // slot -> original point index (0xFFFF = padding)
  __shared__ int s_hist[NCELL];
  __shared__ float s_box[6 * NW];
  __shared__ int s_wmax[NW];
  __shared__ int s_cand[2 * NW * 8];  // per round parity, per wave: {max temp bits, key}

  const float *__restrict__ xyz = xyz_all + (size_t)blockIdx.x * N * 3;
  float *__restrict__ planes = ws_all + (size_t)blockIdx.x * (PERM_LDS ? 3 : 4) * NPAD;
  unsigned *__restrict__ gperm = reinterpret_cast<unsigned *>(planes + (size_t)3 * NPAD);  // !PERM_LDS only
  int32_t *__restrict__ idxs = idx_all + (size_t)blockIdx.x * m;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

  // This kernel is a latency chain that usually runs on a side stream beside the dense kernels of a training
  // step.  Keep other workgroups' waves out of its SIMDs' issue slots: top wave priority, and a full VGPR
  // allocation (touching v127 rounds the allocation up to 128 x 4 waves = the whole register file of a SIMD,
  // so nothing else can become co-resident on this CU).
  __builtin_amdgcn_s_setprio(3);
  asm volatile("" ::: "v127");

  // ---- P1: bounding box of the points that take part (not skipped) --------------------------------
  float lox = INFINITY, loy = INFINITY, loz = INFINITY, hix = -INFINITY, hiy = -INFINITY, hiz = -INFINITY;
  for (int k = tid; k < N; k += BLOCK) {
    const float x = xyz[k * 3 + 0], y = xyz[k * 3 + 1], z = xyz[k * 3 + 2];
    const float mag = (x * x) + (y * y) + (z * z);
    if (!((double)mag <= 1e-3)) {
      lox = fminf(lox, x); loy = fminf(loy, y); loz = fminf(loz, z);
      hix = fmaxf(hix, x); hiy = fmaxf(hiy, y); hiz = fmaxf(hiz, z);
    }
  }
  for (int c = tid; c < NCELL; c += BLOCK) s_hist[c] = 0;
  lox = wave_min(lox); loy = wave_min(loy); loz = wave_min(loz);
  hix = wave_max(hix); hiy = wave_max(hiy); hiz = wave_max(hiz);
  if (lane == 0) {
    s_box[wid * 6 + 0] = lox; s_box[wid * 6 + 1] = loy; s_box[wid * 6 + 2] = loz;
    s_box[wid * 6 + 3] = hix; s_box[wid * 6 + 4] = hiy; s_box[wid * 6 + 5] = hiz;
  }
  __syncthreads();
  lox = s_box[0]; loy = s_box[1]; loz = s_box[2]; hix = s_box[3]; hiy = s_box[4]; hiz = s_box[5];
  for (int w = 1; w < NW; ++w) {
    lox = fminf(lox, s_box[w * 6 + 0]); loy = fminf(loy, s_box[w * 6 + 1]); loz = fminf(loz, s_box[w * 6 + 2]);
    hix = fmaxf(hix, s_box[w * 6 + 3]); hiy = fmaxf(hiy, s_box[w * 6 + 4]); hiz = fmaxf(hiz, s_box[w * 6 + 5]);
  }
  // cell = 4-bit quantisation per axis, Morton interleaved (any mapping is correct; locality is only speed)
  const float sx = 16.0f / fmaxf(hix - lox, 1e-20f), sy = 16.0f / fmaxf(hiy - loy, 1e-20f),
              sz = 16.0f / fmaxf(hiz - loz, 1e-20f);
  auto cell_of = [&](float x, float y, float z) -> unsigned {
    const unsigned qx = (unsigned)fminf(fmaxf((x - lox) * sx, 0.f), 15.f);
    const unsigned qy = (unsigned)fminf(fmaxf((y - loy) * sy, 0.f), 15.f);
    const unsigned qz = (unsigned)fminf(fmaxf((z - loz) * sz, 0.f), 15.f);
    return fpsb_spread4(qx) | (fpsb_spread4(qy) << 1) | (fpsb_spread4(qz) << 2);
  };
  // ---- P2: histogram over cells ---------------------------------------------------------------------
  for (int k = tid; k < N; k += BLOCK)
    atomicAdd(&s_hist[cell_of(xyz[k * 3 + 0], xyz[k * 3 + 1], xyz[k * 3 + 2])], 1);
  __syncthreads();
  // ---- P3: exclusive scan (4 cells per thread) --------------------------------------------------------
  {
    const int c0 = tid * 4;
    const int a0 = s_hist[c0], a1 = s_hist[c0 + 1], a2 = s_hist[c0 + 2], a3 = s_hist[c0 + 3];
    const int sum = a0 + a1 + a2 + a3;
    int incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane == 63) s_wmax[wid] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wid; ++w) base += s_wmax[w];
    const int excl = base + incl - sum;
    s_hist[c0] = excl; s_hist[c0 + 1] = excl + a0; s_hist[c0 + 2] = excl + a0 + a1; s_hist[c0 + 3] = excl + a0 + a1 + a2;
  }
  __syncthreads();
  // ---- P4: scatter into bucket order -----------------------------------------------------------------
  for (int k = tid; k < N; k += BLOCK) {
    const float x = xyz[k * 3 + 0], y = xyz[k * 3 + 1], z = xyz[k * 3 + 2];
    const int slot = atomicAdd(&s_hist[cell_of(x, y, z)], 1);
    planes[0 * NPAD + slot] = x; planes[1 * NPAD + slot] = y; planes[2 * NPAD + slot] = z;
    if (PERM_LDS) s_perm[slot] = (unsigned short)k; else gperm[slot] = (unsigned)k;
  }
  for (int s = N + tid; s < NPAD; s += BLOCK) {
    planes[0 * NPAD + s] = 0.f; planes[1 * NPAD + s] = 0.f; planes[2 * NPAD + s] = 0.f;
    if (PERM_LDS) s_perm[s] = 0xFFFFu; else gperm[s] = 0xFFFFFFFFu;
  }
  if (tid == 0) idxs[0] = 0;
  __threadfence_block();
  __syncthreads();

  // ---- P5: per-lane state: temp of 4 * NB slots; per-bucket box + max (bucket b lives in lane b) -------
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)planes, 0, 3 * NPAD * 4, 0x00020000);
  f32x4 t[NB];
  int gm[NB];
  float blx = INFINITY, bly = INFINITY, blz = INFINITY, bhx = -INFINITY, bhy = -INFINITY, bhz = -INFINITY;
  float gmv = -1.0f;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int slot0 = ((b * NW + wid) * 64 + lane) * 4;
    const f32x4 x = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, slot0 * 4, 0 * NPAD * 4, 0));
    const f32x4 y = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, slot0 * 4, 1 * NPAD * 4, 0));
    const f32x4 z = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, slot0 * 4, 2 * NPAD * 4, 0));
    float mnx = INFINITY, mny = INFINITY, mnz = INFINITY, mxx = -INFINITY, mxy = -INFINITY, mxz = -INFINITY;
    f32x4 tt;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float mag = (x[u] * x[u]) + (y[u] * y[u]) + (z[u] * z[u]);
      const bool pad = PERM_LDS ? (s_perm[slot0 + u] == 0xFFFFu) : (gperm[slot0 + u] == 0xFFFFFFFFu);
      const bool skip = pad || ((double)mag <= 1e-3);
      tt[u] = skip ? -1.0f : 1e10f;
      if (!skip) {
        mnx = fminf(mnx, x[u]); mny = fminf(mny, y[u]); mnz = fminf(mnz, z[u]);
        mxx = fmaxf(mxx, x[u]); mxy = fmaxf(mxy, y[u]); mxz = fmaxf(mxz, z[u]);
      }
    }
    t[b] = tt;
    mnx = wave_min(mnx); mny = wave_min(mny); mnz = wave_min(mnz);
    mxx = wave_max(mxx); mxy = wave_max(mxy); mxz = wave_max(mxz);
    const int lm = max(max(__float_as_int(tt.x), __float_as_int(tt.y)), max(__float_as_int(tt.z), __float_as_int(tt.w)));
    gm[b] = wave_max_i32_fast(lm);
    if (lane == b) {
      blx = mnx; bly = mny; blz = mnz; bhx = mxx; bhy = mxy; bhz = mxz;
      gmv = __int_as_float(gm[b]);
    }
  }

  // ---- rounds ------------------------------------------------------------------------------------------
  // One barrier per round.  Every wave keeps a cached candidate -- the maximum temp among its buckets and the
  // winning key among the points that hold it -- which stays valid until the bucket it lives in is touched
  // (temps only decrease, so an untouched candidate can only be overtaken by itself).  Each round the waves
  // publish their candidates in LDS (double-buffered by round parity), meet at the barrier, and every thread
  // picks the overall winner; its coordinates come through the scalar cache (wave-uniform index).
  float x1 = xyz[0], y1 = xyz[1], z1 = xyz[2];
  int cand_w = __float_as_int(-1.0f), cand_b = 0;
  unsigned cand_key = 0xFFFFFFFFu;
  bool stale = true;  // candidate must be (re)computed
  for (int j = 1; j < m; ++j) {
    // lower bound of the squared distance from the new sample to each bucket's box (lane b <-> bucket b)
    const float ex = fmaxf(fmaxf(blx - x1, x1 - bhx), 0.f);
    const float ey = fmaxf(fmaxf(bly - y1, y1 - bhy), 0.f);
    const float ez = fmaxf(fmaxf(blz - z1, z1 - bhz), 0.f);
    const float lb2 = ex * ex + ey * ey + ez * ez;
    // A bucket may be left alone iff every one of its points has computed d >= temp.  The computed d and the
    // computed lb2 each carry <= 4e-7 relative rounding error; the factor 1 - 1e-5 covers both with margin.
    // NaN anywhere makes the comparison false, i.e. the bucket is processed.
    const bool need = (lane < NB) && !(lb2 * 0.99999f >= gmv);
    const unsigned bm = (unsigned)__ballot(need);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (bm & (1u << b)) {  // wave-uniform
        const int slot0 = ((b * NW + wid) * 64 + lane) * 4;
        const f32x4 x = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, slot0 * 4, 0 * NPAD * 4, 0));
        const f32x4 y = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, slot0 * 4, 1 * NPAD * 4, 0));
        const f32x4 z = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, slot0 * 4, 2 * NPAD * 4, 0));
        const f32x4 dx = x - x1, dy = y - y1, dz = z - z1;
        const f32x4 d = dx * dx + dy * dy + dz * dz;
        f32x4 tt = t[b];
        tt.x = vmin_f32(d.x, tt.x); tt.y = vmin_f32(d.y, tt.y); tt.z = vmin_f32(d.z, tt.z); tt.w = vmin_f32(d.w, tt.w);
        t[b] = tt;
        const int lm = max(max(__float_as_int(tt.x), __float_as_int(tt.y)), max(__float_as_int(tt.z), __float_as_int(tt.w)));
        gm[b] = wave_max_i32_fast(lm);
        if (lane == b) gmv = __int_as_float(gm[b]);
      }
    }
    if (stale || ((bm >> cand_b) & 1u)) {  // wave-uniform: this wave's candidate may have changed
      int wmax = gm[0];
#pragma unroll
      for (int b = 1; b < NB; ++b) wmax = max(wmax, gm[b]);
      unsigned key = 0xFFFFFFFFu;
      int kslot = 0;
      if (wmax >= 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          if (gm[b] == wmax) {  // wave-uniform
            const int slot0 = ((b * NW + wid) * 64 + lane) * 4;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              if (__float_as_int(t[b][u]) == wmax) {
                const unsigned ku = fps_key(PERM_LDS ? (int)s_perm[slot0 + u] : (int)gperm[slot0 + u], lg);
                if (ku < key) { key = ku; kslot = slot0 + u; }
              }
            }
          }
        }
      }
      const unsigned kmin = wave_min_u32_fast(key);
      const unsigned long long owners = __ballot(key == kmin);
      const int src = (int)__builtin_ctzll(owners | (1ull << 63));
      cand_w = wmax;
      cand_key = kmin;
      cand_b = (__shfl(kslot, src) >> 8) / NW;  // bucket g = slot / 256 belongs to wave g % NW as its (g / NW)-th
      cand_b = __builtin_amdgcn_readfirstlane(cand_b);
      stale = false;
    }
    int *rec = &s_cand[((j & 1) * NW + wid) * 8];
    if (lane == 0) { rec[0] = cand_w; rec[1] = (int)cand_key; }
    __syncthreads();
    // winner = max value, then min key: lanes 0..15 read one record each, two DPP reductions decide
    int rw = (int)0x80000000;
    unsigned rk = 0xFFFFFFFFu;
    if (lane < NW) {
      rw = s_cand[((j & 1) * NW + lane) * 8 + 0];
      rk = (unsigned)s_cand[((j & 1) * NW + lane) * 8 + 1];
    }
    const int bw = wave_max_i32_fast(rw);
    const unsigned bk = wave_min_u32_fast(rw == bw ? rk : 0xFFFFFFFFu);
    int old = (bw < 0) ? 0 : fps_unkey(bk, lg);  // every point skipped: the reference returns index 0
    old = __builtin_amdgcn_readfirstlane(old);
    x1 = xyz[old * 3 + 0]; y1 = xyz[old * 3 + 1]; z1 = xyz[old * 3 + 2];  // wave-uniform index: scalar loads
    if (tid == 0) idxs[j] = old;
  }
}

static inline void launch_fps_bucket(const float *xyz, float *ws, int B, int N, int m, int lg, int32_t *idx,
                                     hipStream_t s) {
  const int nb = fps_bucket_nb(N);  // the same value the workspace was sized with
#define FPSB_CASE(NBV, PL)                                                                                    \
  if (nb == NBV) {                                                                                            \
    hipLaunchKernelGGL((fps_bucket_kernel<NBV, PL>), dim3(B), dim3(1024), 0, s, xyz, ws, N, m, lg, idx);      \
    return;                                                                                                   \
  }
  if (N <= 65535) {
    FPSB_CASE(3, true) FPSB_CASE(4, true) FPSB_CASE(5, true) FPSB_CASE(6, true) FPSB_CASE(8, true)
    FPSB_CASE(10, true) FPSB_CASE(12, true) FPSB_CASE(16, true)
  }
  FPSB_CASE(16, false) FPSB_CASE(20, false)
#undef FPSB_CASE
}
