// Host-side launch helpers of the kernels' translation units (*.hip).
#pragma once
#include <hip/hip_runtime.h>

// every launch is checked where it is issued: a failed launch in the middle of
// the pipeline returns its own error instead of surfacing at the end
#define FVAD_LAUNCH_TRY(x)            \
  do {                                \
    const hipError_t e_ = (x);        \
    if (e_ != hipSuccess) return e_;  \
  } while (0)
#define FVAD_KERNEL_TRY(...)                   \
  do {                                         \
    hipLaunchKernelGGL(__VA_ARGS__);           \
    FVAD_LAUNCH_TRY(hipGetLastError());        \
  } while (0)

namespace fvad {

// Workgroups of `threads` threads of a kernel that one CU holds (occupancy
// calculator; 1 when it fails).  Persistent grids are exactly the resident
// capacity (this x CUs), so no workgroup starts late and leaves a tail; the
// callers evaluate it once per process (static const).
template <typename K>
int resident_per_cu(K kernel, int threads) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess || per_cu < 1) per_cu = 1;
  return per_cu;
}

}  // namespace fvad
