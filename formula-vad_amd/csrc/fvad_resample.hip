// k_resample: a resampling engine's raw push (8 .. 96 kHz, float or int16) to
// the 48 kHz f32 device input k_prep3 and the kernels behind it read
// (fvad_resample.h; the arithmetic is fvad_resample_core.h's, shared with the
// host mirror fvad_resample_host, so the two agree by the bits).
//
// One workgroup works on one (tick, row) at a time, row = (stream, channel):
// it stages the tick's n_in inputs behind the K - 1 before them in LDS -- the
// previous tick's end in the push, or the row's tail for tick 0 -- and every
// thread computes the outputs r, r + S, r + 2 S, ... of the tick.  S (the
// block size) is chosen so that S M is a multiple of L: a thread's outputs
// then share one phase, read each tap once, and their inputs lie S M / L
// apart.  The tap table lies in LDS as [k][p]: at 44.1 kHz p(r) = 147 r mod
// 160 runs through all phases, 32 consecutive lanes read 32 distinct banks
// (13 is odd); at the other rates neighbouring lanes read the same few words.
// A workgroup loads the table once (30 KB at 44.1 kHz) and walks a
// grid-stride over the units.
//
// Bounds: a unit reads raw[u * n_in .. + n_in) and, for tick > 0, the K - 1
// words before raw[(u - rows) * n_in + n_in), all inside the push; LDS
// indices are hist + i - k with 0 <= i <= n_in - 1 (480 M / L = n_in) and
// 0 <= k <= K - 1 = hist.  launch_resample picks the variant whose static
// arrays hold the rate's table and window.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fvad_resample.h"

namespace fvad {

namespace {
template <typename In>
__device__ __forceinline__ float load_in(const In *p) {
  return rs::sample(*p);
}
}  // namespace

template <typename In, int S, int TAPCAP, int XCAP>
__global__ void __launch_bounds__(S) k_resample(ResampleArgs a) {
  constexpr int NOUT = rs::kOut / S;
  static_assert(NOUT * S == rs::kOut, "a thread's outputs cover the tick");
  __shared__ float s_tap[TAPCAP];  // [k][p]
  __shared__ float s_x[XCAP];      // [the K - 1 inputs before the tick | the tick]
  const int tid = threadIdx.x;
  const int L = a.d.L, M = a.d.M, K = a.d.K, n_in = a.d.n_in, hist = K - 1;
  for (int j = tid; j < L * K; j += S) {
    const int p = j / K, k = j - p * K;
    s_tap[k * L + p] = a.taps[j];
  }
  int i0, p;
  rs::position(tid, L, M, i0, p);
  const int step = S * M / L;  // exact: S M is a multiple of L
  const size_t rows = (size_t)a.n_streams * a.n_channels, units = rows * (size_t)a.n_ticks;
  const In *raw = static_cast<const In *>(a.raw);
  for (size_t u = blockIdx.x; u < units; u += gridDim.x) {
    const size_t tick = u / rows, row = u - tick * rows;
    const int s = (int)(row / (size_t)a.n_channels);
    const int tv = a.ticks_valid ? a.ticks_valid[s] : a.n_ticks;
    float *dst = a.out + u * rs::kOut;
    if (tick >= (size_t)tv) {  // (the whole workgroup: u and tv are uniform)
      for (int n = 0; n < NOUT; n++) dst[tid + n * S] = 0.0f;
      continue;
    }
    __syncthreads();  // the last unit's reads of s_x are done
    const In *cur = raw + u * (size_t)n_in;
    for (int j = tid; j < n_in; j += S) s_x[hist + j] = load_in(cur + j);
    if (tick > 0) {
      const In *prev = cur - rows * (size_t)n_in + (n_in - hist);
      for (int j = tid; j < hist; j += S) s_x[j] = load_in(prev + j);
    } else {
      const float *tail = a.tails + row * (size_t)hist;
      for (int j = tid; j < hist; j += S) s_x[j] = tail[j];
    }
    __syncthreads();  // (the first one also covers s_tap)
    float acc[NOUT];
    const float *xp = s_x + hist + i0;
    rs::accumulate<NOUT>(
        K, [&](int k) { return s_tap[k * L + p]; }, [&](int n, int k) { return xp[n * step - k]; }, acc);
    for (int n = 0; n < NOUT; n++) dst[tid + n * S] = acc[n];
  }
}

// a row's tail: the last K - 1 inputs of its last valid tick; a row without a
// valid tick keeps its tail.  Queued behind k_resample, which reads the tails.
template <typename In>
__global__ void __launch_bounds__(256) k_resample_tail(ResampleArgs a) {
  const int hist = a.d.K - 1;
  const size_t rows = (size_t)a.n_streams * a.n_channels;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * (size_t)hist) return;
  const size_t row = idx / (size_t)hist;
  const int j = (int)(idx - row * (size_t)hist), s = (int)(row / (size_t)a.n_channels);
  const int tv = a.ticks_valid ? a.ticks_valid[s] : a.n_ticks;
  if (tv < 1) return;
  const In *raw = static_cast<const In *>(a.raw);
  a.tails[idx] = load_in(raw + ((size_t)(tv - 1) * rows + row) * (size_t)a.d.n_in + (a.d.n_in - hist) + j);
}

// listed stream blockIdx.x: its channels' tails become zeros
__global__ void __launch_bounds__(256) k_resample_clear(ResampleClearArgs a) {
  float *row = a.tails + (size_t)a.ids.id[blockIdx.x] * a.row_words;
  for (int j = threadIdx.x; j < a.row_words; j += 256) row[j] = 0.0f;
}

namespace {

template <typename In, int S, int TAPCAP, int XCAP>
hipError_t run(const ResampleArgs &a, unsigned grid, hipStream_t stream) {
  if (a.d.L * a.d.K > TAPCAP || a.d.n_in + a.d.K - 1 > XCAP || (S * a.d.M) % a.d.L) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_resample<In, S, TAPCAP, XCAP>), dim3(grid), dim3(S), 0, stream, a);
  return hipGetLastError();
}

template <typename In>
hipError_t launch_typed(const ResampleArgs &a, hipStream_t stream) {
  const size_t rows = (size_t)a.n_streams * a.n_channels, units = rows * (size_t)a.n_ticks;
  const unsigned grid = (unsigned)std::min<size_t>(units, 2048);
  hipError_t rc;
  // the block size divides 480 and makes S M a multiple of L; the arrays hold
  // the largest table and window of the variant's rates
  if (a.d.L == 160)  // 44.1 kHz
    rc = run<In, 160, rs::kMaxTaps, 441 + 47>(a, grid, stream);
  else if (a.d.L <= 2)  // 24 kHz (L = 2), 96 kHz (L = 1, K = 96)
    rc = run<In, 160, 96, 960 + rs::kMaxTail>(a, grid, stream);
  else  // 8 kHz (L = 6), 16 and 32 kHz (L = 3)
    rc = run<In, 240, 6 * 48, 320 + 47>(a, grid, stream);
  if (rc != hipSuccess) return rc;
  const size_t words = rows * (size_t)(a.d.K - 1);
  hipLaunchKernelGGL(k_resample_tail<In>, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_resample(const ResampleArgs &a, hipStream_t stream) {
  if (a.n_ticks < 1 || a.n_streams < 1 || a.n_channels < 1) return hipSuccess;
  (void)hipGetLastError();
  return a.in16 ? launch_typed<short>(a, stream) : launch_typed<float>(a, stream);
}

hipError_t launch_resample_clear(const ResampleClearArgs &a, hipStream_t stream) {
  if (a.ids.n < 1) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_resample_clear, dim3((unsigned)a.ids.n), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace fvad
