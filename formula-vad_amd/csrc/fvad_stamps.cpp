// Diagnostic entry point of the FVAD_STAMPS builds (make stamps; tools/stamps.py):
// not part of the C API of include/fvad.h, so it lives outside the engine's
// translation units.
#include <algorithm>

#include "fvad_engine_impl.h"

// per-phase cycle totals of k_frame (thread 0 of every workgroup); the first
// call allocates and zeroes the buffer
extern "C" int fvad_engine_stamps(fvad_engine *e, unsigned long long *out, int n) {
  if (!e) return FVAD_EINVAL;
  if (!e->d_stamps) {
    if (const int rc = fvad::make_dev(e->d_stamps, 128)) return rc;
    HIP_TRY(hipMemset(e->d_stamps.get(), 0, 128 * sizeof(unsigned long long)));
    return FVAD_OK;
  }
  HIP_TRY(hipStreamSynchronize(e->stream.get()));
  if (out)
    HIP_TRY(hipMemcpy(out, e->d_stamps.get(), std::min(n, 128) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return FVAD_OK;
}
