// The input resampling's kernel launches (fvad_resample.hip) for
// build/engine_alloc_harness, which links the engine's host objects without
// the kernels: no scenario of the harness creates a resampling engine, so
// these only resolve the symbols the engine's objects refer to.
#include "fvad_resample.h"

namespace fvad {
hipError_t launch_resample(const ResampleArgs &, hipStream_t) { return hipSuccess; }
hipError_t launch_resample_clear(const ResampleClearArgs &, hipStream_t) { return hipSuccess; }
}  // namespace fvad
