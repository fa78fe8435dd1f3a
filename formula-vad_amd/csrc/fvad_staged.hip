// Staged (time-parallel) MI355X pipeline for the Formula-VAD hot path.
//
// rnnoise_process_frame splits into work that depends only on the input
// samples of the (virtual, channel-interleaved) stream and a thin recurrence.
// A push's kernels in the order they run, each with its launch function in
// its own translation unit; this file holds the launcher that chains them:
//
//   k_prep3   lane/stream   HP biquad (serial IIR), s16 scaling, RMS volume
//                           ratio; x written stream-contiguous with 1248 samples
//                           of pitch history in front of the launch's frames
//                           (fvad_prep.hip)
//   k_fftAw   wave/frame    analysis window + FFT A, band energies Ex, the
//                           log/floor chain (Ly, E, silence gate), DCT(Ly)
//                           (fvad_wave.hip)
//   k_plpc    lane/frame    pitch_downsample (x_lp, autocorr, LPC, FIR5) and
//                           the serial energy recurrences Syy and xx
//                           (fvad_plpc.hip)
//   k_pcorr   wg/8 frames   coarse and fine xcorr + find_best_pitch, every
//                           remove_doubling inner product for every candidate
//                           period (fvad_pitch.hip)
//   k_select  lane/(stream, candidate)  remove_doubling's sequential candidate
//                           selection (needs last_period / last_gain) -> pitch
//                           (at the end of fvad_vadm.hip)
//   k_pspecw  wave/frame    pitch window + FFT A -> P, Ep, Exp, DCT(Exp)
//                           (fvad_wave.hip)
//   k_rnn3    wg/8 streams  the true recurrence: cepstral memory, spectral
//                           variability, GRU stack, gain smoothing
//                           (fvad_rnn3.hip; k_rnn3f in f32_fast mode; k_gru16
//                           in fp16 mode and k_fused16, which is k_pspecw too,
//                           in fp16_fused mode: fvad_gru16.hip)
//   k_synthw  wave/frame    pitch filter, gains, Hermitian extension + FFT A +
//                           synthesis window, overlap-add within a wave's batch
//                           (fvad_wave.hip)
//   k_olafb   wave/stream   the tail in one kernel for fft_size 2048 and <= 4
//                           channels (fvad_wave.hip); otherwise (fvad_tail.hip):
//   k_ola     per sample    overlap-add at the seams, 1/32767, re-block ring,
//                           per-tick vad
//   k_winmeta lane/stream   window completion, share-weighted ratio, state
//   k_fftbw   wave/window   FFT B (kissfft radix-4), magnitudes, band sums
//                           (k_fftb, workgroup per window, for fft_size != 2048)
//   k_vadm_hbm lane/stream  VADMachine.run per completed window (side stream,
//                           launch_vadm; fvad_vadm.hip)
//
// staged_kernels() (fvad_staged.h) is the same list as data: which of these
// run in a variant, and the timing events around each.
//
// The wave kernels are persistent (batches of frames from per-XCD queues) so
// per-lane table values stay in registers across frames.  All arithmetic
// reproduces the oracle's operation order (see fvad_kernels.hip), so results
// are bit-identical to the fused kernel and the CPU oracle.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "fvad_launch.h"
#include "fvad_staged.h"

namespace fvad {

// the fused synthesis tail (k_olafb) serves fft_size 2048 with <= 4 channels;
// FVAD_OLAFB=0 selects k_ola + k_winmeta + k_fftbw (A/B)
bool olafb_fused(const StagedArgs &a) {
  static const bool off = [] {
    const char *v = getenv("FVAD_OLAFB");
    return v && atoi(v) == 0;
  }();
  return !off && a.nfft_b == 2048 && a.n_channels <= 4;
}

hipError_t launch_staged(const StagedArgs &a, int n_cu, hipStream_t stream, hipEvent_t *ev, hipEvent_t fft_a_done,
                         hipStream_t fa_stream, hipEvent_t fa_after, hipEvent_t synth_done) {
  const StagedVariant var = staged_variant(a);
  (void)hipGetLastError();
#define REC(k) \
  if (ev) FVAD_LAUNCH_TRY(hipEventRecord(ev[k], stream))
  // k_fftAw and the pitch branch (k_plpc -> k_pcorr -> k_select) run in
  // order (side by side on two streams they stretch each other: 15.0 vs 14.1
  // ms per push in r1); k_fftAw itself may run on fa_stream beside the
  // previous push's k_olafb (fvad_staged.h)
  if (fa_stream && fft_a_done) {
    // k_fftAw on fa_stream beside the previous push's k_olafb: it writes
    // nothing that kernel reads, only what the previous push's k_synthw read
    if (fa_after) FVAD_LAUNCH_TRY(hipStreamWaitEvent(fa_stream, fa_after, 0));
    if (ev) FVAD_LAUNCH_TRY(hipEventRecord(ev[kEvFftABegin], fa_stream));
    FVAD_LAUNCH_TRY(launch_wave(kWaveFftA, a, n_cu, fa_stream));
    if (ev) FVAD_LAUNCH_TRY(hipEventRecord(ev[kEvFftAEnd], fa_stream));
    FVAD_LAUNCH_TRY(hipEventRecord(fft_a_done, fa_stream));
    FVAD_LAUNCH_TRY(hipStreamWaitEvent(stream, fft_a_done, 0));
  } else {
    REC(kEvFftABegin);
    FVAD_LAUNCH_TRY(launch_wave(kWaveFftA, a, n_cu, stream));
    if (fft_a_done) FVAD_LAUNCH_TRY(hipEventRecord(fft_a_done, stream));
    REC(kEvFftAEnd);
  }
  {
    const long long tiles = (long long)((a.n_streams + 63) / 64) * a.n_ticks * a.n_channels;
    REC(kEvPlpcBegin);
    FVAD_LAUNCH_TRY(launch_plpc(a, tiles, n_cu, stream));
    REC(kEvPlpcEnd);
    FVAD_LAUNCH_TRY(launch_pcorr(a, tiles, n_cu, stream));
  }
  REC(kEvPcorrEnd);
  FVAD_LAUNCH_TRY(launch_select(a, stream));
  REC(kEvSelectEnd);
  REC(kEvPspecBegin);
  if (!var.fuse16)  // FVAD_MODE_FP16_FUSED: k_fused16 computes the pitch spectra
    FVAD_LAUNCH_TRY(launch_wave(kWavePspec, a, n_cu, stream));
  REC(kEvPspecEnd);
  if (var.fp16)  // FVAD_MODE_FP16: the GRU stack on the matrix cores (configs[4])
    FVAD_LAUNCH_TRY(launch_gru16(a, stream));
  else  // k_rnn3, or k_rnn3f (FVAD_MODE_F32_FAST)
    FVAD_LAUNCH_TRY(launch_rnn3(a, stream));
  REC(kEvRnnEnd);
  FVAD_LAUNCH_TRY(launch_wave(kWaveSynth, a, n_cu, stream));
  if (ev && synth_done) {
    // a timed push: its timing event kEvSynthEnd (k_synthw's end, the tail's
    // start) is also the one the next push's k_fftAw waits for, so every push
    // has one event record between k_synthw and the tail.  (With a second one
    // in the timed pushes the tail's dispatch fell behind the next k_fftAw's,
    // whose persistent grid then took the CUs first: k_plpc ~130 us late in
    // every timed push.)
    FVAD_LAUNCH_TRY(hipEventRecord(ev[kEvSynthEnd], stream));
  } else {
    if (synth_done) FVAD_LAUNCH_TRY(hipEventRecord(synth_done, stream));
    REC(kEvSynthEnd);
  }
  if (var.olafb) {
    // overlap-add, window bookkeeping and FFT B in one kernel (k_olafb);
    // the k_ola / k_winmeta events bracket nothing
    FVAD_LAUNCH_TRY(launch_wave(kWaveOlaFb, a, n_cu, stream));
    REC(kEvOlaEnd);
    REC(kEvWinmetaEnd);
    REC(kEvFftBEnd);
  } else {
    FVAD_LAUNCH_TRY(launch_ola(a, stream));
    REC(kEvOlaEnd);
    FVAD_LAUNCH_TRY(launch_winmeta(a, stream));
    REC(kEvWinmetaEnd);
    FVAD_LAUNCH_TRY(launch_fftb(a, n_cu, stream));
    REC(kEvFftBEnd);
  }
#undef REC
  return hipSuccess;
}

}  // namespace fvad
