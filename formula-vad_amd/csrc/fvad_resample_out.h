// The denoised PCM at another rate on the device (fvad_engine_config.
// denoised_rate): the argument block and launcher of fvad_resample_out.hip, and
// the host's tap table (fvad_resample.cpp).
//
//   den    [tick][stream][channel][480]    the push's 48 kHz denoised rows (d_den)
//   taps   [L][K]                          the table fvad_resample_out_taps returns
//   tails  [stream][channel][K - 1]        each row's last K - 1 denoised samples
//   out    [tick][stream][channel][n_out]  what the host receives (d_den_out)
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "fvad_resample_core.h"

namespace fvad {

struct ResampleOutArgs {
  const float *den;
  const float *taps;
  float *tails;
  const int *ticks_valid;  // [stream], nullable: every stream has n_ticks
  float *out;
  int n_streams, n_channels, n_ticks;
  rs::DescOut d;
};
// k_resample_out over the push's valid ticks (the ticks past a stream's
// ticks_valid are written as zeros), then k_resample_out_tail behind it: a
// row's tail is read by the workgroup of its first tick and replaced from its
// last valid tick, so the replacing is a launch of its own, in stream order.
// (fvad_engine_reset_streams clears tails with fvad_resample.h's
// launch_resample_clear.)
hipError_t launch_resample_out(const ResampleOutArgs &a, hipStream_t stream);

// the [L][K] table of a listed rate (designed on first use, kept)
const std::vector<float> &resample_out_table(const rs::DescOut &d);

}  // namespace fvad
