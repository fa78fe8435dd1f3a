// Both resamplers' kernel launches (fvad_resample.hip, fvad_resample_out.hip)
// for build/engine_alloc_harness, which links the engine's host objects
// without the kernels: its resampling engines' pushes, resets and rate changes
// end here.
#include "fvad_resample.h"
#include "fvad_resample_out.h"

namespace fvad {
hipError_t launch_resample(const ResampleArgs &, hipStream_t) { return hipSuccess; }
hipError_t launch_resample_ps(const ResamplePsPush &, hipStream_t) { return hipSuccess; }
hipError_t launch_resample_clear(const ResampleClearArgs &, hipStream_t) { return hipSuccess; }
hipError_t launch_resample_out(const ResampleOutArgs &, hipStream_t) { return hipSuccess; }
hipError_t launch_resample_out_ps(const ResampleOutPsPush &, hipStream_t) { return hipSuccess; }
}  // namespace fvad
