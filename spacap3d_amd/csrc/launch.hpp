// Launch policy shared by the host side of libspacap_hip.so: the process-wide launch state and the ONE definition of how a
// persistent grid is sized.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

namespace spacap {

// Process-wide launch state, each defined ONCE in capi.hip: the CUs a caller asked the persistent grids to leave to side-stream
// work (spacap_sa_reserve_cus), the device's CU count, and the library's one environment switch, SPACAP_SA_F32MFMA=1, which
// keeps every shared-MLP product (forward layers, data gradient, plain row products, pooling candidates from the epilogue) on
// the fp32-MFMA kernels instead of the split-bf16 streaming ones -- the reference implementation the split kernels are gated
// against (tests/test_sa_gemm_kernels_gpu.py).
int sa_reserved_cus();
int device_cus();
bool sa_f32_mfma_only();

// Grid sizing; users say `using namespace spacap::launch;` inside their own namespace.
namespace launch {

constexpr int NPART = 1024;   // the most workgroups of a persistent grid (= partial-sum rows of every statistics reduction)

// Workgroups (256 threads) of `kernel` that are resident on the whole device at once.  The GEMM kernels are
// persistent: a grid larger than this would run its surplus as a second, nearly empty round.
template <typename K>
int resident_blocks(K kernel, size_t lds) {
  int per = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, 256, lds) != hipSuccess || per < 1) per = 1;
  (void)hipGetLastError();
  return per * device_cus();
}

// CUs left to the side stream by the FORWARD layer kernels (spacap_sa_reserve_cus).  While the next batch's sampling chain
// runs beside the step (one workgroup per scene: 8 CUs for the first ~4.4 of the step's ~9.8 ms, i.e. during the backbone's
// forward), a persistent grid sized to ALL CUs leaves its last workgroups waiting for a free CU: they run as a second round
// and the kernel takes 1.3 - 2.1x as long (tools/lab/fps_interference.py; the side-stream work cost the main stream 0.86 ms
// per step, tools/lab/step_without_side_stream.py).  A grid of (CUs - 8) workgroups costs one more tile round in nine
// when nothing runs beside it.
// Kernels with several workgroups per CU need slack beyond the occupied CUs themselves (the dispatcher does not pack the rest
// perfectly: measured, the relation tail beside the sampling kernel runs 1.5x as long with 8 CUs left out and 1.04x with 24).
// This is the one place that factor is written down: the CUs a forward grid of `per_cu` workgroups per CU leaves free.
inline int fwd_cus_left_free(int per_cu) { return sa_reserved_cus() * (per_cu > 1 ? 3 : 1); }
// resident workgroups of a FORWARD kernel with those CUs left out (used by the relation tail; the HBM-bound 64-channel
// fp32 layer kernel runs 1.3x as long beside the sampling kernel with or without it and only loses from a smaller grid when
// alone, so it keeps the full one)
inline int fwd_resident(int resident) {
  const int per = resident / device_cus();
  return resident - per * fwd_cus_left_free(per);
}
// The BACKWARD kernels with persistent grids leave the reserved CUs out as well: the sampling chain of the next batch now runs
// beside the first ~5.8 ms of a ~7.4 ms step, i.e. beside the captioner's and most of the detector's backward, and a whole-CU
// workgroup that finds its CU taken runs as a second round (tools/lab/beside.py: 1.5 - 1.9x beside ANY 8 resident workgroups).
// They leave out (resident workgroups per CU) x (reserved CUs).
inline int bwd_resident(int resident) {
  const int per = resident / device_cus();
  return resident - per * sa_reserved_cus();
}
// the CUs a forward / backward kernel with ONE workgroup per CU may take
inline int fwd_cus() { return fwd_resident(device_cus()); }
inline int bwd_cus() { return bwd_resident(device_cus()); }

// grid.x of a persistent kernel with gy column blocks: what is resident over the column blocks, at most NPART, at most one
// workgroup per tile
inline int grid_rows(int resident, int gy, long tiles) {
  long g = resident / gy;
  if (g > NPART) g = NPART;
  if (g > tiles) g = tiles;
  return (int)(g < 1 ? 1 : g);
}
// grid.x of a streaming split-bf16 kernel (one 8-wave workgroup per CU, every wave owns 32-row tiles) over R rows with gy column
// blocks: the CUs it may take (fwd_cus / bwd_cus) over the column blocks, at most NPART, at most one workgroup per 8 wave tiles
inline unsigned stream_grid(int cus, int gy, long R) {
  const long wtiles = (R + 31) / 32;
  long gx = cus / gy;
  gx = gx > NPART ? NPART : gx;
  gx = gx > (wtiles + 7) / 8 ? (wtiles + 7) / 8 : gx;
  return (unsigned)gx;
}

inline unsigned nblocks(long work, int per) {
  long g = (work + per - 1) / per;
  return (unsigned)(g < 1 ? 1 : g);
}

}  // namespace launch
}  // namespace spacap
