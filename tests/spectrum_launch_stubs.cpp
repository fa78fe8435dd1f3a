// The spectral sweep's kernel launch (k_sweep_bandmin, fvad_sweep.hip) for
// build/engine_alloc_harness, which links the sweep's host object without the
// kernels: no scenario of the harness creates a spectral sweep, so this only
// resolves the symbol fvad_sweep.cpp refers to.
#include "fvad_sweep.h"

namespace fvad {
hipError_t launch_sweep_bandmin(const BandMinArgs &, hipStream_t) { return hipSuccess; }
}  // namespace fvad
