// A window's band energy from its magnitude spectrum, for host and device:
// k_sweep_bandmin (fvad_sweep.hip) and the host path of a spectral sweep
// (fvad_sweep.cpp) run this code, so both give the bits FFT B gives
// (fftb_bands, k_fftb: acc += mag[k - lo] in bin order) and the bits of
// k_sweep_min's reduction over the channels.
//
// Nothing here may be reassociated or contracted: a band sum is one f32 chain
// from 0.0f over the bins lo..hi ascending, and a window's band minimum the
// minimum of its channels' sums from 999 with strict < (VADMachine.zig's fold
// over the channels, as vadm_stream and k_sweep_min take it).
#pragma once
#pragma clang fp contract(off)
#include "fvad_exact.h"

namespace fvad {

// mag: one channel's magnitudes, mag[0] = bin spec_lo; spec_lo <= lo <= hi
FVAD_HD inline float band_chain(const float *mag, int spec_lo, int lo, int hi) {
  float acc = 0.0f;
  for (int k = lo; k <= hi; k++) acc += mag[k - spec_lo];
  return acc;
}

// mag: a window's [n_channels][n_spec] magnitudes
FVAD_HD inline float band_min(const float *mag, int n_channels, int n_spec, int spec_lo, int lo, int hi) {
  float min_v = 999;
  for (int c = 0; c < n_channels; c++) {
    const float v = band_chain(mag + c * n_spec, spec_lo, lo, hi);
    if (v < min_v) min_v = v;
  }
  return min_v;
}

}  // namespace fvad
