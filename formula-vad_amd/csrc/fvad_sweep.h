// Config sweep (include/fvad.h: fvad_sweep_*): many VADMachine configs over
// recorded window sequences.  The kernel side (fvad_sweep.hip,
// fvad_sweep_score.hip) as fvad_sweep.cpp sees it: the kernels' arguments and
// their launchers.
#pragma once
#include "../../include/fvad.h"
#include "fvad_staged.h"

namespace fvad {

// k_sweep_min + k_vadm_sweep's arguments.  A lane is (stream s, config c of
// the chunk): lane index s * n_cfgs + c.
struct SweepArgs {
  int n_streams, n_cfgs;         // configs of this chunk
  int n_channels, n_bands, seg_cap;
  const VadmConst *K;            // [n_cfgs] device; lt_off / lt_pitch: the config's rows [stream][lt_pitch] in lt
  VadmState *st;                 // [lane]
  float *lt;                     // long-term rows, contiguous per lane, 16-byte aligned
  float *sbuf, *rbuf;            // short-term and ratio entries [entry][lane]
  VadmSeg *seg;                  // [lane][seg_cap]
  const long long *win_off;      // [n_streams] first window of stream s in the arrays below
  const int *n_win;              // [n_streams]
  const float *band;             // [window][channel][band]
  float *wmin;                   // [window][band]  min over channels (k_sweep_min)
  const float *wvad, *wvr;       // [window]
  long long n_windows;           // all streams'
  unsigned long long fft;
  double bound_scale;            // test hooks, as VadmArgs'
  unsigned defer_max;
  unsigned long long *count;     // null, or [kVadmCounts]
};
constexpr int kSweepBlock = 64;  // windows per walk: a lane re-decides lazy / non-lazy and may settle an owed fold
hipError_t launch_sweep_min(const SweepArgs &a, hipStream_t stream);
hipError_t launch_vadm_sweep(const SweepArgs &a, hipStream_t stream);

// k_sweep_bandmin's arguments (spectral sweeps, fvad_sweep_create_spectral):
// the recorded spectra in, the chunk's wmin out -- what k_sweep_min makes of
// recorded band sums, for the chunk's D distinct bands.
struct BandMinArgs {
  int n_channels, n_spec, spec_lo;  // a window's magnitudes: [channel][n_spec], bin spec_lo first
  int n_bands;                      // D
  long long n_windows;              // all streams'
  const float *spec;                // [window][channel][n_spec]
  const int2 *bands;                // [D] inclusive bins (lo, hi) inside [spec_lo, spec_lo + n_spec)
  float *wmin;                      // [window][D]
};
// floats of a window k_sweep_bandmin stages in LDS: 8 channels of fft_size
// 2048's 1 025 bins; a larger window is read from HBM by every thread
constexpr int kBandMinStage = FVAD_MAX_CHANNELS * 1025;
hipError_t launch_sweep_bandmin(const BandMinArgs &a, hipStream_t stream);

// k_sweep_score's arguments (fvad_sweep_score.hip): a chunk's lanes as
// SweepArgs', scored where k_vadm_sweep left them.
struct ScoreArgs {
  int n_streams, n_cfgs, seg_cap;  // configs of this chunk
  const VadmState *st;             // [lane]  n_segs
  const VadmSeg *seg;              // [lane][seg_cap]
  const float *lab;                // every stream's labels as (from, to) seconds, each stream's stably sorted by start
  const long long *lab_off;        // [n_streams + 1] first label of stream s in lab
  const fvad_stat_config *stat;    // the chunk's first config's; config c reads stat[c * stat_stride]
  int stat_stride;                 // 0: one for all, 1: one per config
  fvad_single_stats *single;       // [lane], written where status is kEvalScored (fvad_eval_core.h)
  unsigned *status;                // [lane] kEvalScored / kEvalOverCapacity / kEvalUnsorted
};
hipError_t launch_sweep_score(const ScoreArgs &a, hipStream_t stream);

}  // namespace fvad
