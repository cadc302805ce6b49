// Host: the compute-unit count the launchers size their resident grids with.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace uhdr {

// Compute units of the CURRENT device (the entry points make their context's device current first), 256 when the runtime does
// not say.  Cached per device id: a process that drives contexts on different devices must not inherit the first one's count.
inline int device_cu_count() {
  static std::atomic<int> cus_of[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  const bool cached = dev >= 0 && dev < 64;
  int cus = cached ? cus_of[dev].load(std::memory_order_relaxed) : 0;
  if (cus == 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    if (cached) cus_of[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}

}  // namespace uhdr
