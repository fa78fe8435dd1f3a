// Input resampling to 48 kHz on the device (fvad_engine_config.input_rate):
// the argument blocks and launchers of fvad_resample.hip, and the host's tap
// table (fvad_resample.cpp).
//
//   raw    [tick][stream][channel][n_in]   the push as the host sent it (float or int16)
//   taps   [L][K]                          the table fvad_resample_taps returns
//   tails  [stream][channel][K - 1]        each row's last K - 1 input samples, as float
//   out    [tick][stream][channel][480]    the engine's ordinary device input
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "fvad_lifecycle.h"  // IdList
#include "fvad_resample_core.h"

namespace fvad {

struct ResampleArgs {
  const void *raw;
  const float *taps;
  float *tails;
  const int *ticks_valid;  // [stream], nullable: every stream has n_ticks
  float *out;
  int n_streams, n_channels, n_ticks;
  int in16;  // raw holds int16 samples
  rs::Desc d;
};
// k_resample over the push's valid ticks (the ticks past a stream's
// ticks_valid are written as zeros), then k_resample_tail behind it: a row's
// tail is read by the workgroup of its first tick and replaced from its last
// valid tick, so the replacing is a launch of its own, in stream order.
hipError_t launch_resample(const ResampleArgs &a, hipStream_t stream);

// fvad_engine_reset_streams: the listed streams' tails become zeros
struct ResampleClearArgs {
  float *tails;
  int row_words;  // n_channels * (K - 1)
  IdList ids;
};
hipError_t launch_resample_clear(const ResampleClearArgs &a, hipStream_t stream);

// the [L][K] table of a listed rate (designed on first use, kept)
const std::vector<float> &resample_table(const rs::Desc &d);

}  // namespace fvad
