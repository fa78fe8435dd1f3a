// Config sweep kernels (fvad_sweep_run): many VADMachine configs over recorded
// window sequences.
//
//   k_sweep_min    thread/(window, band)  min over channels of a window's band
//                                         sums (from 999, strict <: vadm_stream's
//                                         reduction, exact in f32), once per
//                                         (window, band slot) instead of per lane
//   k_sweep_bandmin  workgroup/window     spectral sweeps: the window's magnitudes
//                                         (staged in LDS once) into the minimum
//                                         over channels of every distinct band's
//                                         sum, a thread per band walking its f32
//                                         chain in bin order (fvad_bandsum_core.h:
//                                         FFT B's band sums, k_sweep_min's minimum)
//   k_vadm_sweep   lane/(stream, config)  the device VADMachine (fvad_vadm_dev.h:
//                                         the code k_vadm_hbm runs) over the
//                                         stream's whole sequence
//
// k_vadm_sweep's shape: a wave is 64 configs of one stream (grid.y = stream),
// so a window's vad and ratio are wave-uniform loads and its band minima one
// 16-byte line that every lane reads (slot differs per config).  Per lane:
// the state in registers for the whole walk, a long-term row of its own
// (contiguous, 16-byte aligned: lt_sum_row's float4 path), short-term and
// ratio entries [entry][lane] so the lanes of a wave touch one line per entry.
// The sequence is walked in blocks of kSweepBlock windows, each one vadm_walk
// run -- exactly a push of the engine's machine: lazy or not is decided per
// block (a buffer that fills up turns lazy at the next block), an owed fold
// rides in the state across blocks, is settled at a block's end once
// defer_max long pushes are owed, and at the end of the stream (final), the
// sweep's one sync point.  Lanes past n_cfgs leave at once and touch nothing.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fvad_bandsum_core.h"
#include "fvad_sweep.h"
#include "fvad_vadm_dev.h"

namespace fvad {

__global__ void __launch_bounds__(256) k_sweep_min(SweepArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_windows * a.n_bands) return;
  const long long w = i / a.n_bands;
  const int b = (int)(i % a.n_bands);
  float min_v = 999;
  for (int c = 0; c < a.n_channels; c++) {
    const float v = a.band[(w * a.n_channels + c) * a.n_bands + b];
    if (v < min_v) min_v = v;
  }
  a.wmin[i] = min_v;
}

// kStage: the window's n_channels * n_spec <= kBandMinStage magnitudes go
// through LDS (32 800 bytes), read from HBM once, coalesced; otherwise every
// thread reads its bands' bins from HBM.  wmin's stores run along the bands.
template <bool kStage>
__global__ void __launch_bounds__(256) k_sweep_bandmin(BandMinArgs a) {
  __shared__ float mag[kStage ? kBandMinStage : 1];
  const int per = a.n_channels * a.n_spec;
  for (long long w = blockIdx.x; w < a.n_windows; w += gridDim.x) {
    const float *row = a.spec + (size_t)w * per;
    if constexpr (kStage) {
      for (int i = threadIdx.x; i < per; i += 256) mag[i] = row[i];
      __syncthreads();
    }
    for (int d = threadIdx.x; d < a.n_bands; d += 256) {
      const int2 b = a.bands[d];
      a.wmin[(size_t)w * a.n_bands + d] = band_min(kStage ? mag : row, a.n_channels, a.n_spec, a.spec_lo, b.x, b.y);
    }
    if constexpr (kStage) __syncthreads();  // the next window's magnitudes replace these
  }
}

__global__ void __launch_bounds__(64) k_vadm_sweep(SweepArgs a) {
  const int c = blockIdx.x * 64 + threadIdx.x, s = blockIdx.y;
  if (c >= a.n_cfgs) return;
  const size_t lane = (size_t)s * a.n_cfgs + c, lanes = (size_t)a.n_streams * a.n_cfgs;
  const VadmConst K = a.K[c];
  VadmState S = a.st[lane];
  float *lt = a.lt + K.lt_off + (size_t)s * K.lt_pitch;
  float *st = a.sbuf + lane, *rb = a.rbuf + lane;
  VadmSeg *seg = a.seg + lane * a.seg_cap;
  const VadmEvLane ev{nullptr, nullptr, 0};
  const int nw = a.n_win[s], nb = a.n_bands;
  const float *wmin = a.wmin + a.win_off[s] * nb + K.slot, *wvad = a.wvad + a.win_off[s], *wvr = a.wvr + a.win_off[s];
  for (int w0 = 0; w0 < nw; w0 += kSweepBlock) {
    const int w1 = min(nw, w0 + kSweepBlock);
    vadm_walk(S, K, st, rb, (int)lanes, lt, 1, seg, a.seg_cap, ev, a.fft, a.bound_scale, a.defer_max, a.count,
              w1 == nw, [&](auto &&window) {
                for (int w = w0; w < w1; w++) window(wmin[(size_t)w * nb], wvad[w], wvr[w]);
              });
  }
  a.st[lane] = S;
}

hipError_t launch_sweep_min(const SweepArgs &a, hipStream_t stream) {
  const long long n = a.n_windows * a.n_bands;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_sweep_min, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_sweep_bandmin(const BandMinArgs &a, hipStream_t stream) {
  if (a.n_windows <= 0 || a.n_bands <= 0) return hipSuccess;
  const dim3 grid((unsigned)std::min<long long>(a.n_windows, 1 << 20));
  if (a.n_channels * (long long)a.n_spec <= kBandMinStage)
    hipLaunchKernelGGL(k_sweep_bandmin<true>, grid, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(k_sweep_bandmin<false>, grid, dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_vadm_sweep(const SweepArgs &a, hipStream_t stream) {
  if (a.n_cfgs <= 0 || a.n_streams <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_vadm_sweep, dim3((unsigned)((a.n_cfgs + 63) / 64), (unsigned)a.n_streams), dim3(64), 0, stream,
                     a);
  return hipGetLastError();
}

}  // namespace fvad
