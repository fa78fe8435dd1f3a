// Per-stream rates, what the two directions' launchers share (fvad_resample.hip,
// fvad_resample_out.hip): the tables of a push and the walk over its rates.
// The host side of the tables is eng::RatePlan (fvad_engine_impl.h), which
// fills a PsTables per push.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fvad_resample_core.h"

namespace fvad {

// The device tables of a per-stream push,
//
//   offsets  [stream + 1]   a stream's first sample inside a tick of the packed rows
//                           [tick][stream][channel][rate(stream) / 100]; [n_streams]: a tick's length
//   rate_idx [stream]       rs::rate_index of the stream's rate
//   lists    [stream]       the streams by rate, rate index ascending: rate i's are
//                           lists[list_at[i] .. list_at[i + 1])
//
// and by value the lists' bounds and the rates' descriptions and tap tables
// (null at 48000 and above the engine's largest rate).
struct PsTables {
  const long long *offsets;
  const int *rate_idx, *lists;
  long long tick_len;
  int list_at[rs::kPsRates + 1];
  const float *taps[rs::kPsRates];
  rs::Desc d[rs::kPsRates];
};

// about 2048 workgroups: (ticks x channels) rows of them side by side over a
// list of n units (or groups of units)
inline dim3 ps_grid(unsigned n, int n_ticks, int n_channels) {
  const unsigned across = (unsigned)n_ticks * n_channels;
  return dim3(std::max(1u, std::min(n, 2048u / across)), n_ticks, n_channels);
}

// One launch per rate present, rate index ascending: `a` (a Resample[Out]PsArgs
// whose r the caller filled) gets the rate's list, taps and description, and
// launch(a, copy) runs it, copy for the 48000 streams.
template <typename PsArgs, typename Launch>
hipError_t ps_launches(const PsTables &t, PsArgs a, Launch launch) {
  a.offsets = t.offsets;
  a.tick_len = t.tick_len;
  for (int i = 0; i < rs::kPsRates; i++) {
    a.n_list = t.list_at[i + 1] - t.list_at[i];
    if (a.n_list < 1) continue;
    a.list = t.lists + t.list_at[i];
    a.r.taps = t.taps[i];
    a.r.d = t.d[i];
    const bool copy = i == rs::kPsIndex48;
    if (!copy && !a.r.taps) return hipErrorInvalidValue;
    const hipError_t rc = launch(a, copy);
    if (rc != hipSuccess) return rc;
  }
  return hipSuccess;
}

}  // namespace fvad
