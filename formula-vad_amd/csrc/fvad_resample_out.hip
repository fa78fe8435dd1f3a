// k_resample_out: a push's 48 kHz denoised rows (d_den) to the engine's
// denoised_rate (8 .. 96 kHz), the rows the host receives (fvad_resample_out.h;
// the arithmetic is fvad_resample_core.h's, shared with the host mirror
// fvad_resample_out_host, so the two agree by the bits).  It is k_resample
// (fvad_resample.hip) with the roles swapped: 480 samples in, n_out out.
//
// A workgroup works on U (tick, row) units at a time, row = (stream, channel),
// S threads on each: they stage the tick's 480 denoised samples behind the
// K - 1 before them in LDS -- the end of the previous tick of the push (valid
// whenever this one is), or the row's tail for tick 0 -- and every thread
// computes the outputs r, r + S, ... r + (NOUT - 1) S of the tick,
// S NOUT = n_out.  S is chosen so that S M is a multiple of L: a thread's
// outputs then share one phase, read each tap once, and their inputs lie
// S M / L apart.  The tap table lies in LDS as [k][p].  At 44.1 kHz
// p(r) = 160 r mod 147 = 13 r mod 147 runs through all 147 phases: a block of
// 147 threads, three outputs each, one unit (the table, 56 448 B, leaves room
// for one window); 32 consecutive lanes read 32 distinct words of a [k] row on
// 29 or 30 of the 32 banks (the wrap at 147 folds two or three of them: 2-way
// at the worst).  At L = 1 (8, 16, 24 kHz) every lane reads the same tap (a
// broadcast).  The short ticks are packed rather than run as short blocks,
// which would leave a CU's wave slots to the workgroup limit and load the table
// once per unit: 8 kHz has 80 outputs a tick, so eight units share a workgroup
// of 320 threads, 40 threads with two outputs each on a unit (four units of 80
// threads with one output each, which read every tap per output, measured
// 0.2 ms slower at the bench's shape); at 16, 24 and
// 32 kHz four units of 80 threads with 2, 3 and 4 outputs a thread.  A
// workgroup loads the table once and walks a grid-stride over the groups of U
// units.
//
// Bounds: a unit u < units reads den[u * 480 .. + 480) and, for tick > 0, the
// K - 1 words before den[(u - rows) * 480 + 480), all inside the push; LDS
// indices are hist + i + n S M / L - k with 0 <= i + n S M / L <= 479
// (n_out M / L = 480) and 0 <= k <= K - 1 = hist, inside XCAP >= hist + 480.
// launch_resample_out picks the variant whose static arrays hold the rate's
// table and window.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fvad_resample_out.h"

namespace fvad {

template <int S, int NOUT, int U, int TAPCAP, int XCAP>
__global__ void __launch_bounds__(S *U) k_resample_out(ResampleOutArgs a) {
  __shared__ float s_tap[TAPCAP];   // [k][p]
  __shared__ float s_y[U * XCAP];   // per unit: [the K - 1 samples before the tick | the tick]
  const int tid = threadIdx.x, sub = tid / S, r0 = tid - sub * S;
  const int L = a.d.L, M = a.d.M, K = a.d.K, n_out = a.d.n_out, hist = K - 1;
  for (int j = tid; j < L * K; j += S * U) {
    const int p = j / K, k = j - p * K;
    s_tap[k * L + p] = a.taps[j];
  }
  int i0, p;
  rs::position(r0, L, M, i0, p);
  const int step = S * M / L;  // exact: S M is a multiple of L
  const size_t rows = (size_t)a.n_streams * a.n_channels, units = rows * (size_t)a.n_ticks;
  const size_t groups = (units + U - 1) / U;
  float *y = s_y + sub * XCAP;
  for (size_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const size_t u = g * U + sub;
    bool live = u < units;  // (uniform over a unit's S threads)
    size_t tick = 0, row = 0;
    if (live) {
      tick = u / rows;
      row = u - tick * rows;
      const int s = (int)(row / (size_t)a.n_channels);
      const int tv = a.ticks_valid ? a.ticks_valid[s] : a.n_ticks;
      if (tick >= (size_t)tv) {  // past the stream's valid ticks: zeros, nothing read
        float *dst = a.out + u * (size_t)n_out;
        for (int n = 0; n < NOUT; n++) dst[r0 + n * S] = 0.0f;
        live = false;
      }
    }
    __syncthreads();  // the last group's reads of s_y are done
    if (live) {
      const float *cur = a.den + u * (size_t)rs::kIn;
      for (int j = r0; j < rs::kIn; j += S) y[hist + j] = cur[j];
      const float *before = tick > 0 ? cur - rows * (size_t)rs::kIn + (rs::kIn - hist) : a.tails + row * (size_t)hist;
      for (int j = r0; j < hist; j += S) y[j] = before[j];
    }
    __syncthreads();  // (the first one also covers s_tap)
    if (live) {
      float acc[NOUT];
      const float *yp = y + hist + i0;
      rs::accumulate<NOUT>(
          K, [&](int k) { return s_tap[k * L + p]; }, [&](int n, int k) { return yp[n * step - k]; }, acc);
      float *dst = a.out + u * (size_t)n_out;
      for (int n = 0; n < NOUT; n++) dst[r0 + n * S] = acc[n];
    }
  }
}

// a row's tail: the last K - 1 denoised samples of its last valid tick; a row
// without a valid tick keeps its tail.  Queued behind k_resample_out, which
// reads the tails.
__global__ void __launch_bounds__(256) k_resample_out_tail(ResampleOutArgs a) {
  const int hist = a.d.K - 1;
  const size_t rows = (size_t)a.n_streams * a.n_channels;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * (size_t)hist) return;
  const size_t row = idx / (size_t)hist;
  const int j = (int)(idx - row * (size_t)hist), s = (int)(row / (size_t)a.n_channels);
  const int tv = a.ticks_valid ? a.ticks_valid[s] : a.n_ticks;
  if (tv < 1) return;
  a.tails[idx] = a.den[((size_t)(tv - 1) * rows + row) * (size_t)rs::kIn + (rs::kIn - hist) + j];
}

namespace {

template <int S, int NOUT, int U, int TAPCAP, int XCAP>
hipError_t run(const ResampleOutArgs &a, hipStream_t stream) {
  if (a.d.L * a.d.K > TAPCAP || rs::kIn + a.d.K - 1 > XCAP || S * NOUT != a.d.n_out || (S * a.d.M) % a.d.L)
    return hipErrorInvalidValue;
  const size_t units = (size_t)a.n_streams * a.n_channels * (size_t)a.n_ticks, groups = (units + U - 1) / U;
  const unsigned grid = (unsigned)std::min<size_t>(groups, 2048);
  hipLaunchKernelGGL((k_resample_out<S, NOUT, U, TAPCAP, XCAP>), dim3(grid), dim3(S * U), 0, stream, a);
  return hipGetLastError();
}

// the table and the window of the rates below 44.1 kHz and of 96 kHz: 288
// taps and 480 + 287 samples at 8 kHz are the largest
constexpr int kTapCap = 288, kXCap = rs::kIn + rs::kMaxTailOut;

}  // namespace

hipError_t launch_resample_out(const ResampleOutArgs &a, hipStream_t stream) {
  if (a.n_ticks < 1 || a.n_streams < 1 || a.n_channels < 1) return hipSuccess;
  (void)hipGetLastError();
  hipError_t rc;
  // S NOUT = n_out, S M a multiple of L, U units of S threads in a workgroup
  switch (a.d.rate) {
    case 8000: rc = run<40, 2, 8, kTapCap, kXCap>(a, stream); break;
    case 16000: rc = run<80, 2, 4, kTapCap, kXCap>(a, stream); break;
    case 24000: rc = run<80, 3, 4, kTapCap, kXCap>(a, stream); break;
    case 32000: rc = run<80, 4, 4, kTapCap, kXCap>(a, stream); break;
    case 44100: rc = run<147, 3, 1, rs::kMaxTapsOut, rs::kIn + 95>(a, stream); break;
    case 96000: rc = run<320, 3, 1, kTapCap, kXCap>(a, stream); break;
    default: return hipErrorInvalidValue;
  }
  if (rc != hipSuccess) return rc;
  const size_t words = (size_t)a.n_streams * a.n_channels * (size_t)(a.d.K - 1);
  hipLaunchKernelGGL(k_resample_out_tail, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace fvad
