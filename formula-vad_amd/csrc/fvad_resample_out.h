// The denoised PCM at another rate on the device (fvad_engine_config.
// denoised_rate): the argument block and launcher of fvad_resample_out.hip, and
// the host's tap table (fvad_resample.h's resample_table).
//
//   den    [tick][stream][channel][480]    the push's 48 kHz denoised rows (d_den)
//   taps   [L][K]                          the table fvad_resample_out_taps returns
//   tails  [stream][channel][K - 1]        each row's last K - 1 denoised samples
//   out    [tick][stream][channel][n]      what the host receives (d_den_out), n = rate / 100
#pragma once
#include <hip/hip_runtime.h>

#include "fvad_resample_core.h"
#include "fvad_resample_ps.h"

namespace fvad {

struct ResampleOutArgs {
  const float *den;
  const float *taps;
  float *tails;
  const int *ticks_valid;  // [stream], nullable: every stream has n_ticks
  float *out;
  int n_streams, n_channels, n_ticks;
  rs::Desc d;
};
// k_resample_out over the push's valid ticks (the ticks past a stream's
// ticks_valid are written as zeros), then k_resample_out_tail behind it: a
// row's tail is read by the workgroup of its first tick and replaced from its
// last valid tick, so the replacing is a launch of its own, in stream order.
// (fvad_engine_reset_streams clears tails with fvad_resample.h's
// launch_resample_clear.)
hipError_t launch_resample_out(const ResampleOutArgs &a, hipStream_t stream);

// Per-stream rates (FVAD_DENOISED_RATE_PER_STREAM; DESIGN.md section 7,
// "Per-stream denoised rates"): out is packed [tick][stream][channel]
// [rate(stream) / 100]; its tables are fvad_resample_ps.h's PsTables, the same
// as the input direction's and from the same eng::RatePlan (rate_idx is not
// read in this direction), and
//
//   tails    [stream][channel][rs::kMaxTailOut]   a row's last 287 48 kHz denoised samples, whatever
//                              its rate; a launch at K taps reads the last K - 1 of them
//
// k_resample_out_ps is k_resample_out's unit body over one rate's list: a unit
// is (tick, listed stream, channel), its 48 kHz row den[((tick * n_streams + s)
// * n_channels + c) * 480], its outputs out[tick * tick_len + offsets[s] + c * n].
struct ResampleOutPsArgs {
  ResampleOutArgs r;  // taps, d: this launch's rate; n_streams: the engine's; tails, out as above
  const int *list;
  const long long *offsets;
  long long tick_len;
  int n_list;
};
// a push of a per-stream engine: r as for launch_resample_out but for taps and
// d, which each launch takes from the tables
struct ResampleOutPsPush {
  ResampleOutArgs r;
  PsTables ps;
};
// One k_resample_out_ps launch per listed rate present, in the variant
// launch_resample_out picks for that rate; the 48000 streams through
// k_resample_out_copy (their rows by the bits); then one k_resample_out_tail_ps
// over every row.
hipError_t launch_resample_out_ps(const ResampleOutPsPush &p, hipStream_t stream);

}  // namespace fvad
