// k_resample: a resampling engine's raw push (8 .. 96 kHz, float or int16) to
// the 48 kHz f32 device input k_prep3 and the kernels behind it read
// (fvad_resample.h; the arithmetic is fvad_resample_core.h's, shared with the
// host mirror fvad_resample_host, so the two agree by the bits).
//
// One workgroup works on one (tick, row) at a time, row = (stream, channel):
// it stages the tick's n inputs behind the K - 1 before them in LDS -- the
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
//
// The unit body is written once, resample_units, over a row map that places a
// unit: RowsAll for k_resample (the arithmetic above), RowsListed for
// k_resample_ps, a per-stream engine's launch over the streams of one rate
// (fvad_resample.h).  k_resample_copy passes such an engine's 48000 streams
// through, and k_resample_tail_ps replaces every row's tail behind them.
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

// A unit's place: its tick and stream, and where its row lies -- the tick's
// first sample in raw, the row's tail, the tick's 480 outputs (in words).
struct Unit {
  size_t tick;
  int s;
  size_t cur, tail, dst;
};

// k_resample's row map: unit u is row u of [tick][stream][channel], at one rate
struct RowsAll {
  size_t rows;
  int n_channels, n_ticks, n_in, hist;
  using Index = size_t;
  __device__ __forceinline__ size_t units() const { return rows * (size_t)n_ticks; }
  __device__ __forceinline__ size_t tick_len() const { return rows * (size_t)n_in; }
  __device__ __forceinline__ Unit unit(size_t u) const {
    Unit w;
    w.tick = u / rows;
    const size_t row = u - w.tick * rows;
    w.s = (int)(row / (size_t)n_channels);
    w.cur = u * (size_t)n_in;
    w.tail = row * (size_t)hist;
    w.dst = u * rs::kOut;
    return w;
  }
};

// k_resample_ps's: a workgroup keeps one tick (blockIdx.y) and one channel
// (blockIdx.z) and walks one rate's list, so placing a unit takes no division
struct RowsListed {
  const int *list;
  const long long *offsets;
  size_t len;  // a tick's length in samples
  int n_list, n_streams, n_channels, n_in;
  using Index = unsigned;
  __device__ __forceinline__ unsigned units() const { return (unsigned)n_list; }
  __device__ __forceinline__ size_t tick_len() const { return len; }
  __device__ __forceinline__ Unit unit(unsigned li) const {
    Unit w;
    const unsigned c = blockIdx.z;
    w.tick = blockIdx.y;
    // (uniform over the workgroup: kept in scalar registers)
    w.s = __builtin_amdgcn_readfirstlane(list[li]);
    const unsigned long long off = (unsigned long long)offsets[w.s];
    const size_t at = ((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(off >> 32)) << 32) |
                      (unsigned)__builtin_amdgcn_readfirstlane((int)off);
    const size_t row = (size_t)w.s * n_channels + c;
    w.cur = w.tick * len + at + c * (size_t)n_in;
    w.tail = row * rs::kMaxTail;
    w.dst = (w.tick * ((size_t)n_streams * n_channels) + row) * rs::kOut;
    return w;
  }
};

// the unit body of k_resample and k_resample_ps
template <typename In, int S, int TAPCAP, int XCAP, typename Map>
__device__ __forceinline__ void resample_units(const ResampleArgs &a, const Map &m) {
  constexpr int NOUT = rs::kOut / S;
  static_assert(NOUT * S == rs::kOut, "a thread's outputs cover the tick");
  __shared__ float s_tap[TAPCAP];  // [k][p]
  __shared__ float s_x[XCAP];      // [the K - 1 inputs before the tick | the tick]
  const int tid = threadIdx.x;
  const int L = a.d.L, M = a.d.M, K = a.d.K, n_in = a.d.n, hist = K - 1;
  for (int j = tid; j < L * K; j += S) {
    const int p = j / K, k = j - p * K;
    s_tap[k * L + p] = a.taps[j];
  }
  int i0, p;
  rs::position(tid, L, M, i0, p);
  const int step = S * M / L;  // exact: S M is a multiple of L
  using Index = typename Map::Index;
  const Index units = m.units();
  const In *raw = static_cast<const In *>(a.raw);
  for (Index u = blockIdx.x; u < units; u += gridDim.x) {
    const Unit w = m.unit(u);
    const int tv = a.ticks_valid ? a.ticks_valid[w.s] : a.n_ticks;
    float *dst = a.out + w.dst;
    if (w.tick >= (size_t)tv) {  // (the whole workgroup: u and tv are uniform)
      for (int n = 0; n < NOUT; n++) dst[tid + n * S] = 0.0f;
      continue;
    }
    __syncthreads();  // the last unit's reads of s_x are done
    const In *cur = raw + w.cur;
    for (int j = tid; j < n_in; j += S) s_x[hist + j] = load_in(cur + j);
    if (w.tick > 0) {
      const In *prev = cur - m.tick_len() + (n_in - hist);
      for (int j = tid; j < hist; j += S) s_x[j] = load_in(prev + j);
    } else {
      const float *tail = a.tails + w.tail;
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

template <typename In, int S, int TAPCAP, int XCAP>
__global__ void __launch_bounds__(S) k_resample(ResampleArgs a) {
  const RowsAll m{(size_t)a.n_streams * a.n_channels, a.n_channels, a.n_ticks, a.d.n, a.d.K - 1};
  resample_units<In, S, TAPCAP, XCAP>(a, m);
}

// Bounds: list[li] < n_streams and offsets[s] + n_channels * n_in <=
// offsets[s + 1] <= tick_len for every listed s (the host writes rate_idx,
// offsets and lists from one set of rates: fvad_input_layout), so a unit's
// row and the K - 1 <= n_in words before it lie inside the push.
template <typename In, int S, int TAPCAP, int XCAP>
__global__ void __launch_bounds__(S) k_resample_ps(ResamplePsArgs a) {
  const RowsListed m{a.list, a.offsets, (size_t)a.tick_len, a.n_list, a.r.n_streams, a.r.n_channels, a.r.d.n};
  resample_units<In, S, TAPCAP, XCAP>(a.r, m);
}

// the 48000 streams of a per-stream engine: nothing to filter, a tick's 480
// samples as floats (rs::sample), zeros past the stream's ticks_valid
template <typename In>
__global__ void __launch_bounds__(256) k_resample_copy(ResamplePsArgs a) {
  const RowsListed m{a.list, a.offsets, (size_t)a.tick_len, a.n_list, a.r.n_streams, a.r.n_channels, rs::kOut};
  const unsigned units = m.units();
  const In *raw = static_cast<const In *>(a.r.raw);
  for (unsigned u = blockIdx.x; u < units; u += gridDim.x) {
    const Unit w = m.unit(u);
    const int tv = a.r.ticks_valid ? a.r.ticks_valid[w.s] : a.r.n_ticks;
    const bool valid = w.tick < (size_t)tv;
    for (int j = threadIdx.x; j < rs::kOut; j += 256) a.r.out[w.dst + j] = valid ? load_in(raw + w.cur + j) : 0.0f;
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
  a.tails[idx] = load_in(raw + ((size_t)(tv - 1) * rows + row) * (size_t)a.d.n + (a.d.n - hist) + j);
}

// k_resample_tail over a per-stream engine's rows [stream][channel][kMaxTail]:
// each with its stream's own K - 1 and n_in (a 48000 stream has no tail)
template <typename In>
__global__ void __launch_bounds__(256) k_resample_tail_ps(ResampleTailPsArgs a) {
  const size_t rows = (size_t)a.n_streams * a.n_channels;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * (size_t)rs::kMaxTail) return;
  const size_t row = idx / (size_t)rs::kMaxTail;
  const int j = (int)(idx - row * (size_t)rs::kMaxTail), s = (int)(row / (size_t)a.n_channels);
  const int c = (int)(row - (size_t)s * a.n_channels), ri = a.rate_idx[s];
  const int hist = a.hist[ri], n_in = a.n_in[ri];
  if (j >= hist) return;
  const int tv = a.ticks_valid ? a.ticks_valid[s] : a.n_ticks;
  if (tv < 1) return;
  const In *raw = static_cast<const In *>(a.raw);
  a.tails[idx] = load_in(raw + (size_t)(tv - 1) * (size_t)a.tick_len + (size_t)a.offsets[s] + (size_t)c * n_in +
                         (n_in - hist) + j);
}

// listed stream blockIdx.x: its channels' tails become zeros
__global__ void __launch_bounds__(256) k_resample_clear(ResampleClearArgs a) {
  float *row = a.tails + (size_t)a.ids.id[blockIdx.x] * a.row_words;
  for (int j = threadIdx.x; j < a.row_words; j += 256) row[j] = 0.0f;
}

namespace {

template <typename In, int S, int TAPCAP, int XCAP>
hipError_t run(const ResampleArgs &a, dim3 grid, hipStream_t stream) {
  if (a.d.L * a.d.K > TAPCAP || a.d.n + a.d.K - 1 > XCAP || (S * a.d.M) % a.d.L) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_resample<In, S, TAPCAP, XCAP>), grid, dim3(S), 0, stream, a);
  return hipGetLastError();
}
template <typename In, int S, int TAPCAP, int XCAP>
hipError_t run(const ResamplePsArgs &a, dim3 grid, hipStream_t stream) {
  if (a.r.d.L * a.r.d.K > TAPCAP || a.r.d.n + a.r.d.K - 1 > XCAP || (S * a.r.d.M) % a.r.d.L)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_resample_ps<In, S, TAPCAP, XCAP>), grid, dim3(S), 0, stream, a);
  return hipGetLastError();
}

// the variant of a rate: the block size divides 480 and makes S M a multiple
// of L; the arrays hold the largest table and window of the variant's rates
template <typename In, typename Args>
hipError_t run_rate(const rs::Desc &d, const Args &a, dim3 grid, hipStream_t stream) {
  if (d.L == 160)  // 44.1 kHz
    return run<In, 160, rs::kMaxTaps, 441 + 47>(a, grid, stream);
  if (d.L <= 2)  // 24 kHz (L = 2), 96 kHz (L = 1, K = 96)
    return run<In, 160, 96, 960 + rs::kMaxTail>(a, grid, stream);
  // 8 kHz (L = 6), 16 and 32 kHz (L = 3)
  return run<In, 240, 6 * 48, 320 + 47>(a, grid, stream);
}

template <typename In>
hipError_t launch_typed(const ResampleArgs &a, hipStream_t stream) {
  const size_t rows = (size_t)a.n_streams * a.n_channels, units = rows * (size_t)a.n_ticks;
  const unsigned grid = (unsigned)std::min<size_t>(units, 2048);
  const hipError_t rc = run_rate<In>(a.d, a, dim3(grid), stream);
  if (rc != hipSuccess) return rc;
  const size_t words = rows * (size_t)(a.d.K - 1);
  hipLaunchKernelGGL(k_resample_tail<In>, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

template <typename In>
hipError_t launch_typed_ps(const ResamplePsPush &p, hipStream_t stream) {
  ResamplePsArgs a{};
  a.r = p.r;
  bool tails = false;
  const hipError_t rc = ps_launches(p.ps, a, [&](const ResamplePsArgs &l, bool copy) {
    // about 2048 workgroups, as launch_resample
    const dim3 grid = ps_grid((unsigned)l.n_list, p.r.n_ticks, p.r.n_channels);
    if (!copy) {
      tails = true;
      return run_rate<In>(l.r.d, l, grid, stream);
    }
    hipLaunchKernelGGL(k_resample_copy<In>, grid, dim3(256), 0, stream, l);
    return hipGetLastError();
  });
  if (rc != hipSuccess || !tails) return rc;
  ResampleTailPsArgs t{};
  t.raw = p.r.raw;
  t.tails = p.r.tails;
  t.ticks_valid = p.r.ticks_valid;
  t.rate_idx = p.ps.rate_idx;
  t.offsets = p.ps.offsets;
  t.tick_len = p.ps.tick_len;
  t.n_streams = p.r.n_streams;
  t.n_channels = p.r.n_channels;
  t.n_ticks = p.r.n_ticks;
  t.in16 = p.r.in16;
  for (int i = 0; i < rs::kPsRates; i++) {
    t.hist[i] = p.ps.d[i].K - 1;
    t.n_in[i] = p.ps.d[i].n;
  }
  const size_t words = (size_t)p.r.n_streams * p.r.n_channels * rs::kMaxTail;
  hipLaunchKernelGGL(k_resample_tail_ps<In>, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, t);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_resample(const ResampleArgs &a, hipStream_t stream) {
  if (a.n_ticks < 1 || a.n_streams < 1 || a.n_channels < 1) return hipSuccess;
  (void)hipGetLastError();
  return a.in16 ? launch_typed<short>(a, stream) : launch_typed<float>(a, stream);
}

hipError_t launch_resample_ps(const ResamplePsPush &p, hipStream_t stream) {
  if (p.r.n_ticks < 1 || p.r.n_streams < 1 || p.r.n_channels < 1) return hipSuccess;
  if (p.r.n_ticks > 65535 || p.r.n_channels > 65535) return hipErrorInvalidValue;  // (grid y and z)
  (void)hipGetLastError();
  return p.r.in16 ? launch_typed_ps<short>(p, stream) : launch_typed_ps<float>(p, stream);
}

hipError_t launch_resample_clear(const ResampleClearArgs &a, hipStream_t stream) {
  if (a.ids.n < 1) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_resample_clear, dim3((unsigned)a.ids.n), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace fvad
