// Library-level entry points of libspacap_hip.so: version, error text, device probe, the reference's launch-size helper
// restated for the host side, and the process-wide launch state (launch.hpp) with spacap_sa_reserve_cus.
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>

#include <atomic>

#include "common.hpp"
#include "launch.hpp"

namespace spacap {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- the process-wide launch state (launch.hpp): defined and, for the switch, read HERE only ---------------------------------
static std::atomic<int> g_reserved_cus{0};
int sa_reserved_cus() { return g_reserved_cus.load(std::memory_order_relaxed); }
int device_cus() {
  static const int n = [] {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    (void)hipGetLastError();
    return cus;
  }();
  return n;
}
bool sa_f32_mfma_only() {
  static const bool on = getenv("SPACAP_SA_F32MFMA") != nullptr && atoi(getenv("SPACAP_SA_F32MFMA")) != 0;
  return on;
}

}  // namespace spacap

/* n CUs are left free by the persistent grids (0 <= n <= 64): set by a caller that runs other work (the next batch's sampling
   chain) beside the step. */
extern "C" int spacap_sa_reserve_cus(int n) {
  if (n < 0 || n > 64) return SPACAP_E_INVALID;
  spacap::g_reserved_cus.store(n, std::memory_order_relaxed);
  return SPACAP_OK;
}

extern "C" int spacap_abi_version(void) { return SPACAP_ABI_VERSION; }

extern "C" const char *spacap_last_error(void) { return spacap::g_err; }

extern "C" int spacap_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    spacap::set_error("hipGetDeviceCount: %s", hipGetErrorString(e));
    return SPACAP_E_NO_DEVICE;
  }
  return n;
}

// include/cuda_utils.h:15-19 of the reference: pow_2 = (int)(log(w) / log(2)); clamp(1 << pow_2, 1, 512).
extern "C" int spacap_opt_n_threads(int work_size) {
  const int pow_2 = (int)(log((double)work_size) / log(2.0));
  int t = 1 << pow_2;
  if (t > 512) t = 512;
  if (t < 1) t = 1;
  return t;
}
