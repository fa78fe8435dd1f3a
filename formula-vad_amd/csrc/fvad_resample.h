// Input resampling to 48 kHz on the device (fvad_engine_config.input_rate):
// the argument blocks and launchers of fvad_resample.hip, and the host's tap
// table (fvad_resample.cpp).
//
//   raw    [tick][stream][channel][n]      the push as the host sent it (float or int16), n = rate / 100
//   taps   [L][K]                          the table fvad_resample_taps returns
//   tails  [stream][channel][K - 1]        each row's last K - 1 input samples, as float
//   out    [tick][stream][channel][480]    the engine's ordinary device input
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "fvad_lifecycle.h"  // IdList
#include "fvad_resample_core.h"
#include "fvad_resample_ps.h"

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

// Per-stream rates (FVAD_INPUT_RATE_PER_STREAM; DESIGN.md section 7, "Per-stream
// rates"): a push is packed [tick][stream][channel][rate(stream) / 100]; its
// tables are fvad_resample_ps.h's PsTables, described there once for both
// directions and filled by the engine's eng::RatePlan (fvad_engine_impl.h), and
//
//   tails    [stream][channel][rs::kMaxTail]   a row's K - 1 words lie at its front
//
// k_resample_ps is k_resample's unit body over one rate's list: a unit is
// (tick, listed stream, channel), its row starts at
// raw[tick * tick_len + offsets[s] + c * n].
struct ResamplePsArgs {
  ResampleArgs r;  // taps, d: this launch's rate; n_streams: the engine's; tails as above
  const int *list;
  const long long *offsets;
  long long tick_len;
  int n_list;
};
struct ResampleTailPsArgs {
  const void *raw;
  float *tails;
  const int *ticks_valid, *rate_idx;
  const long long *offsets;
  long long tick_len;
  int n_streams, n_channels, n_ticks, in16;
  int hist[rs::kPsRates], n_in[rs::kPsRates];  // K - 1 (0 at 48000) and rate / 100 by rate index
};
// a push of a per-stream engine: r as for launch_resample but for taps and d,
// which each launch takes from the tables
struct ResamplePsPush {
  ResampleArgs r;
  PsTables ps;
};
// One k_resample_ps launch per rate present, in the variant launch_resample
// picks for that rate; the 48000 streams through k_resample_copy (convert
// only); then one k_resample_tail_ps over every row, each with its own K - 1
// and n (none when only 48000 streams are present).
hipError_t launch_resample_ps(const ResamplePsPush &p, hipStream_t stream);

// fvad_engine_reset_streams, fvad_engine_set_stream_rates: the listed streams'
// tails become zeros
struct ResampleClearArgs {
  float *tails;
  int row_words;  // n_channels * (K - 1); per-stream rates: n_channels * rs::kMaxTail
  IdList ids;
};
hipError_t launch_resample_clear(const ResampleClearArgs &a, hipStream_t stream);

// the [L][K] table of a listed rate in either direction (designed on first
// use, kept)
const std::vector<float> &resample_table(rs::Dir dir, const rs::Desc &d);

}  // namespace fvad
