// The VADMachine's host side (VADMachine.zig:18-310): how a config becomes a
// machine, the device state in the reference's terms, and the host reference
// machine (fvad_vadm_*, the sweep's host path).  Host code with no HIP call
// and no engine type: it links into any harness.  Its users are the engine's
// device machines (fvad_engine_vadm.cpp), the sweep (fvad_sweep.cpp) and the
// pipelines (fvad_host.cpp).
#pragma once
#include <cstddef>
#include <vector>

#include "../../include/fvad.h"
#include "fvad_staged.h"

namespace fvad {

// the device writes its segments as the API returns them: they are copied
// from device memory straight into fvad_segment storage
static_assert(sizeof(VadmSeg) == sizeof(fvad_segment) &&
                  offsetof(VadmSeg, sample_from) == offsetof(fvad_segment, sample_from) &&
                  offsetof(VadmSeg, sample_to) == offsetof(fvad_segment, sample_to) &&
                  offsetof(VadmSeg, debug_rnn_vad) == offsetof(fvad_segment, debug_rnn_vad) &&
                  offsetof(VadmSeg, debug_avg_speech_vol_ratio) == offsetof(fvad_segment, debug_avg_speech_vol_ratio),
              "the device's segment record is fvad_segment");

// A config as a machine (VADMachine.zig:75-100): K holds the RollingAverage
// lengths, the long-term row pitch, the thresholds in samples and the config's
// factors; s0 is a freshly constructed machine, the initial long-term average
// folded as RollingAverage.init does; lo / hi are the speech band as FFT-B bins
// (FFT.freqToBin).  K's buffer offsets (lt_off, st_off, r_off) and band slot
// are the caller's.  The one derivation: the device machines, the sweep and
// the host machine all take theirs from here.
struct VadmDerived {
  VadmConst K;
  VadmState s0;
  int lo, hi;
};
VadmDerived vadm_derive(const fvad_vadm_config &c, int sample_rate, int fft_size);

// d as a row of the per-stream constant table (fvad_staged.h VadmRow: the
// engines attached with fvad_engine_attach_vadm_ex); slot: the engine band
// slot of d's speech band
VadmRow vadm_row(const VadmDerived &d, int slot);

// the slot b with band_lo[b] == lo and band_hi[b] == hi (the last, should the
// bands repeat), or -1
int band_slot(const int *band_lo, const int *band_hi, int n_bands, int lo, int hi);

// VadmState in the reference's terms (fvad_engine_vadm_snapshot, fvad_sweep_snapshot)
void vadm_snapshot_of(const VadmState &st, fvad_vadm_snapshot *out);

// The host VADMachine over one window sequence from a fresh machine: band
// [n_windows][n_channels][n_bands], the machine reads slot `slot`; vad /
// vol_ratio [n_windows]; window w enters with index w * fft_size.
void host_vadm_lane(const fvad_vadm_config &c, int sample_rate, int fft_size, int n_channels, int n_bands, int slot,
                    size_t n_windows, const float *band, const float *vad, const float *vol_ratio,
                    fvad_vadm_snapshot *snap, std::vector<fvad_segment> *segs);

}  // namespace fvad
