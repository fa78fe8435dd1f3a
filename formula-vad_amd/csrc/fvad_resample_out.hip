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
//
// The unit body is written once, resample_out_units, over a row map that
// places a unit: OutRowsAll for k_resample_out (the arithmetic above),
// OutRowsListed for k_resample_out_ps, a per-stream engine's launch over the
// streams of one rate (fvad_resample_out.h).  k_resample_out_copy passes such
// an engine's 48000 streams through, and k_resample_out_tail_ps replaces every
// row's history behind them.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fvad_resample_out.h"

namespace fvad {

// A unit's place, filled by its row map's place(), which returns the unit's
// stream: its tick and its row [stream][channel].  The map turns it into the
// tick's first sample in den (cur), the K - 1 words of the row's tail and the
// tick's n_out outputs (dst), in words.
struct OutUnit {
  size_t tick;
  size_t row, at;  // its row [stream][channel]; OutRowsListed: the stream's offset in a tick of out
};

// k_resample_out's row map: unit u is row u of [tick][stream][channel], at one rate
struct OutRowsAll {
  size_t rows;
  int n_channels, n_ticks, n_out, hist;
  using Index = size_t;
  __device__ __forceinline__ size_t units() const { return rows * (size_t)n_ticks; }
  template <bool kUniform>
  __device__ __forceinline__ int place(size_t u, OutUnit &w) const {
    w.tick = u / rows;
    w.row = u - w.tick * rows;
    return (int)(w.row / (size_t)n_channels);
  }
  __device__ __forceinline__ size_t cur(const OutUnit &, size_t u) const { return u * (size_t)rs::kIn; }
  __device__ __forceinline__ size_t tail(const OutUnit &w) const { return w.row * (size_t)hist; }
  __device__ __forceinline__ size_t dst(const OutUnit &, size_t u) const { return u * (size_t)n_out; }
};

// k_resample_out_ps's: a workgroup keeps one tick (blockIdx.y) and one channel
// (blockIdx.z) and walks one rate's list, so placing a unit takes no division.
// kUniform: the workgroup works on one unit (U = 1), whose list entry and
// offset are then kept in scalar registers; the U-packed workgroups' units
// straddle waves, so there every thread reads its own unit's.
struct OutRowsListed {
  const int *list;
  const long long *offsets;
  size_t len;  // a tick's length in output samples
  int n_list, n_streams, n_channels, n_out, hist;
  using Index = unsigned;
  __device__ __forceinline__ unsigned units() const { return (unsigned)n_list; }
  template <bool kUniform>
  __device__ __forceinline__ int place(unsigned li, OutUnit &w) const {
    int s;
    w.tick = blockIdx.y;
    if constexpr (kUniform) {
      s = __builtin_amdgcn_readfirstlane(list[li]);
      const unsigned long long off = (unsigned long long)offsets[s];
      w.at = ((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(off >> 32)) << 32) |
             (unsigned)__builtin_amdgcn_readfirstlane((int)off);
    } else {
      s = list[li];
      w.at = (size_t)offsets[s];
    }
    w.row = (size_t)s * n_channels + blockIdx.z;
    return s;
  }
  __device__ __forceinline__ size_t cur(const OutUnit &w, unsigned) const {
    return (w.tick * ((size_t)n_streams * n_channels) + w.row) * (size_t)rs::kIn;
  }
  __device__ __forceinline__ size_t tail(const OutUnit &w) const {
    return w.row * (size_t)rs::kMaxTailOut + (size_t)(rs::kMaxTailOut - hist);
  }
  __device__ __forceinline__ size_t dst(const OutUnit &w, unsigned) const {
    return w.tick * len + w.at + blockIdx.z * (size_t)n_out;
  }
};

// the unit body of k_resample_out and k_resample_out_ps
template <int S, int NOUT, int U, int TAPCAP, int XCAP, typename Map>
__device__ __forceinline__ void resample_out_units(const ResampleOutArgs &a, const Map &m) {
  __shared__ float s_tap[TAPCAP];   // [k][p]
  __shared__ float s_y[U * XCAP];   // per unit: [the K - 1 samples before the tick | the tick]
  // (U = 1: tid < S, so the unit of a thread is a constant and r0 its index)
  const int tid = threadIdx.x, sub = U == 1 ? 0 : tid / S, r0 = tid - sub * S;
  const int L = a.d.L, M = a.d.M, K = a.d.K, hist = K - 1;
  for (int j = tid; j < L * K; j += S * U) {
    const int p = j / K, k = j - p * K;
    s_tap[k * L + p] = a.taps[j];
  }
  int i0, p;
  rs::position(r0, L, M, i0, p);
  const int step = S * M / L;  // exact: S M is a multiple of L
  const size_t rows = (size_t)a.n_streams * a.n_channels;
  using Index = typename Map::Index;
  const Index units = m.units(), groups = (units + U - 1) / U;
  float *y = s_y + sub * XCAP;
  for (Index g = blockIdx.x; g < groups; g += gridDim.x) {
    const Index u = g * U + sub;
    bool live = u < units;  // (uniform over a unit's S threads)
    OutUnit w{};
    if (live) {
      const int s = m.template place<U == 1>(u, w);
      const int tv = a.ticks_valid ? a.ticks_valid[s] : a.n_ticks;
      if (w.tick >= (size_t)tv) {  // past the stream's valid ticks: zeros, nothing read
        float *dst = a.out + m.dst(w, u);
        for (int n = 0; n < NOUT; n++) dst[r0 + n * S] = 0.0f;
        live = false;
      }
    }
    __syncthreads();  // the last group's reads of s_y are done
    if (live) {
      const float *cur = a.den + m.cur(w, u);
      for (int j = r0; j < rs::kIn; j += S) y[hist + j] = cur[j];
      const float *before = w.tick > 0 ? cur - rows * (size_t)rs::kIn + (rs::kIn - hist) : a.tails + m.tail(w);
      for (int j = r0; j < hist; j += S) y[j] = before[j];
    }
    __syncthreads();  // (the first one also covers s_tap)
    if (live) {
      float acc[NOUT];
      const float *yp = y + hist + i0;
      rs::accumulate<NOUT>(
          K, [&](int k) { return s_tap[k * L + p]; }, [&](int n, int k) { return yp[n * step - k]; }, acc);
      float *dst = a.out + m.dst(w, u);
      for (int n = 0; n < NOUT; n++) dst[r0 + n * S] = acc[n];
    }
  }
}

template <int S, int NOUT, int U, int TAPCAP, int XCAP>
__global__ void __launch_bounds__(S *U) k_resample_out(ResampleOutArgs a) {
  const OutRowsAll m{(size_t)a.n_streams * a.n_channels, a.n_channels, a.n_ticks, a.d.n, a.d.K - 1};
  resample_out_units<S, NOUT, U, TAPCAP, XCAP>(a, m);
}

// Bounds: list[li] < n_streams and offsets[s] + n_channels * n_out <=
// offsets[s + 1] <= tick_len for every listed s (the host writes offsets and
// lists from one set of rates: fvad_denoised_layout), so a unit's outputs lie
// inside its tick of out; its 48 kHz row and, for tick > 0, the previous
// tick's row lie inside den, and its K - 1 <= kMaxTailOut tail words inside
// its row of tails.
template <int S, int NOUT, int U, int TAPCAP, int XCAP>
__global__ void __launch_bounds__(S *U) k_resample_out_ps(ResampleOutPsArgs a) {
  const OutRowsListed m{a.list,      a.offsets,      (size_t)a.tick_len, a.n_list,
                        a.r.n_streams, a.r.n_channels, a.r.d.n,        a.r.d.K - 1};
  resample_out_units<S, NOUT, U, TAPCAP, XCAP>(a.r, m);
}

// the 48000 streams of a per-stream engine: the 48 kHz rows by their bits,
// zeros past the stream's ticks_valid
__global__ void __launch_bounds__(256) k_resample_out_copy(ResampleOutPsArgs a) {
  const OutRowsListed m{a.list, a.offsets, (size_t)a.tick_len, a.n_list, a.r.n_streams, a.r.n_channels, rs::kIn, 0};
  const unsigned units = m.units();
  const unsigned *den = reinterpret_cast<const unsigned *>(a.r.den);
  unsigned *out = reinterpret_cast<unsigned *>(a.r.out);
  for (unsigned u = blockIdx.x; u < units; u += gridDim.x) {
    OutUnit w{};
    const int s = m.place<true>(u, w);
    const int tv = a.r.ticks_valid ? a.r.ticks_valid[s] : a.r.n_ticks;
    const bool valid = w.tick < (size_t)tv;
    const size_t cur = m.cur(w, u), dst = m.dst(w, u);
    for (int j = threadIdx.x; j < rs::kIn; j += 256) out[dst + j] = valid ? den[cur + j] : 0u;
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

// k_resample_out_tail over a per-stream engine's rows [stream][channel]
// [kMaxTailOut]: every row's last kMaxTailOut 48 kHz samples of its last valid
// tick, whatever its rate (the 48000 rows too: a stream may take a listed rate
// later).  kMaxTailOut < 480: they lie inside that tick.
__global__ void __launch_bounds__(256) k_resample_out_tail_ps(ResampleOutArgs a) {
  const size_t rows = (size_t)a.n_streams * a.n_channels;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * (size_t)rs::kMaxTailOut) return;
  const size_t row = idx / (size_t)rs::kMaxTailOut;
  const int j = (int)(idx - row * (size_t)rs::kMaxTailOut), s = (int)(row / (size_t)a.n_channels);
  const int tv = a.ticks_valid ? a.ticks_valid[s] : a.n_ticks;
  if (tv < 1) return;
  a.tails[idx] = a.den[((size_t)(tv - 1) * rows + row) * (size_t)rs::kIn + (rs::kIn - rs::kMaxTailOut) + j];
}

namespace {

template <int S, int NOUT, int U, int TAPCAP, int XCAP>
hipError_t run(const ResampleOutArgs &a, hipStream_t stream) {
  if (a.d.L * a.d.K > TAPCAP || rs::kIn + a.d.K - 1 > XCAP || S * NOUT != a.d.n || (S * a.d.M) % a.d.L)
    return hipErrorInvalidValue;
  const size_t units = (size_t)a.n_streams * a.n_channels * (size_t)a.n_ticks, groups = (units + U - 1) / U;
  const unsigned grid = (unsigned)std::min<size_t>(groups, 2048);
  hipLaunchKernelGGL((k_resample_out<S, NOUT, U, TAPCAP, XCAP>), dim3(grid), dim3(S * U), 0, stream, a);
  return hipGetLastError();
}

// k_resample_out_ps: (ticks x channels) rows of workgroups side by side over
// the list's groups of U, about 2048 in all, as above
template <int S, int NOUT, int U, int TAPCAP, int XCAP>
hipError_t run(const ResampleOutPsArgs &a, hipStream_t stream) {
  if (a.r.d.L * a.r.d.K > TAPCAP || rs::kIn + a.r.d.K - 1 > XCAP || S * NOUT != a.r.d.n || (S * a.r.d.M) % a.r.d.L)
    return hipErrorInvalidValue;
  const dim3 grid = ps_grid(((unsigned)a.n_list + U - 1) / U, a.r.n_ticks, a.r.n_channels);
  hipLaunchKernelGGL((k_resample_out_ps<S, NOUT, U, TAPCAP, XCAP>), grid, dim3(S * U), 0, stream, a);
  return hipGetLastError();
}

// the table and the window of the rates below 44.1 kHz and of 96 kHz: 288
// taps and 480 + 287 samples at 8 kHz are the largest
constexpr int kTapCap = 288, kXCap = rs::kIn + rs::kMaxTailOut;

// the variant of a rate: S NOUT = n_out, S M a multiple of L, U units of S threads in a workgroup
template <typename Args>
hipError_t run_rate(int rate, const Args &a, hipStream_t stream) {
  switch (rate) {
    case 8000: return run<40, 2, 8, kTapCap, kXCap>(a, stream);
    case 16000: return run<80, 2, 4, kTapCap, kXCap>(a, stream);
    case 24000: return run<80, 3, 4, kTapCap, kXCap>(a, stream);
    case 32000: return run<80, 4, 4, kTapCap, kXCap>(a, stream);
    case 44100: return run<147, 3, 1, rs::kMaxTapsOut, rs::kIn + 95>(a, stream);
    case 96000: return run<320, 3, 1, kTapCap, kXCap>(a, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t launch_resample_out(const ResampleOutArgs &a, hipStream_t stream) {
  if (a.n_ticks < 1 || a.n_streams < 1 || a.n_channels < 1) return hipSuccess;
  (void)hipGetLastError();
  const hipError_t rc = run_rate(a.d.rate, a, stream);
  if (rc != hipSuccess) return rc;
  const size_t words = (size_t)a.n_streams * a.n_channels * (size_t)(a.d.K - 1);
  hipLaunchKernelGGL(k_resample_out_tail, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_resample_out_ps(const ResampleOutPsPush &p, hipStream_t stream) {
  if (p.r.n_ticks < 1 || p.r.n_streams < 1 || p.r.n_channels < 1) return hipSuccess;
  if (p.r.n_ticks > 65535 || p.r.n_channels > 65535) return hipErrorInvalidValue;  // (grid y and z)
  (void)hipGetLastError();
  ResampleOutPsArgs a{};
  a.r = p.r;
  const hipError_t rc = ps_launches(p.ps, a, [&](const ResampleOutPsArgs &l, bool copy) {
    if (!copy) return run_rate(l.r.d.rate, l, stream);
    const dim3 grid = ps_grid((unsigned)l.n_list, p.r.n_ticks, p.r.n_channels);
    hipLaunchKernelGGL(k_resample_out_copy, grid, dim3(256), 0, stream, l);
    return hipGetLastError();
  });
  if (rc != hipSuccess) return rc;
  // every row's history, the 48000 rows' too, behind the launches that read it
  const size_t words = (size_t)p.r.n_streams * p.r.n_channels * rs::kMaxTailOut;
  hipLaunchKernelGGL(k_resample_out_tail_ps, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, p.r);
  return hipGetLastError();
}

}  // namespace fvad
