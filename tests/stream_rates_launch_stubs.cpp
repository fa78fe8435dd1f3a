// The per-stream resampling's kernel launches (fvad_resample.hip) for
// build/engine_alloc_harness, which links the engine's host objects without
// the kernels: no scenario of the harness creates a per-stream engine, so
// this only resolves the symbol the engine's objects refer to.
#include "fvad_resample.h"

namespace fvad {
hipError_t launch_resample_ps(const ResamplePsPush &, hipStream_t) { return hipSuccess; }
}  // namespace fvad
