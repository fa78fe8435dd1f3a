// Ingest kernels of the staged pipeline: k_prep3 (high-pass, volume ratio,
// pitch history; the pipeline's first kernel, fvad_staged.hip) and k_pcm16
// (the 16-bit ingest's conversion to float).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fvad_device.h"
#include "fvad_internal.h"
#include "fvad_launch.h"
#include "fvad_staged.h"
#include "fvad_staged_dev.h"

namespace fvad {

// ---------------------------------------------------------------------------
// k_prep3: high-pass biquad (a serial IIR with f64 intermediates: no exact
// parallel form exists, so one lane walks one stream), s16 scaling, RMS volume
// ratio, pitch history.  It uses no LDS and one wave per 64 channel-slots:
// the engine runs it on its own stream beside the previous push's kernels
// (xs, ratio and ticks are double-buffered), where it must not take the LDS
// or the wave slots those kernels are sized for.  Lane = stream: the biquad
// chain straight from the input rows (16-byte loads through an 8-deep
// prefetch ring, 16-byte stores into the stream's xs row), and beside it, off
// the chain's dependency path, each channel's RMS sum and per tick the volume
// ratio.  (A second wave that re-read the input for the RMS sums cost the
// co-running kernels 0.17 ms per push.)
// ---------------------------------------------------------------------------
#ifndef FVAD_PREP_SLOTS
#define FVAD_PREP_SLOTS 64
#endif
constexpr int kPrepSlots = FVAD_PREP_SLOTS;  // channel-slots per workgroup (32 stereo streams)
__host__ __device__ constexpr int prep_streams(int C) { return kPrepSlots / C < 64 ? kPrepSlots / C : 64; }
#ifndef FVAD_PREP_RING
#define FVAD_PREP_RING 8
#endif
constexpr int kPrepRing = FVAD_PREP_RING;  // float4 loads in flight per lane
// blocks per trip of the chain loop: the compiler's wait at the loop header
// drains every load and store in flight, so it is paid once per trip
#ifndef FVAD_PREP_UNROLL
#define FVAD_PREP_UNROLL 4
#endif
static_assert((kFrame / 4) % kPrepRing == 0, "prep ring must divide a frame");

// One lane walks its stream's input in blocks of kPrepRing float4 chunks: per
// tick the C * 480 samples of stream s are contiguous, ticks B * C * 480
// floats apart, and a tick holds a whole number of blocks, so a block is one
// base pointer and kPrepRing immediate offsets.  The next block's chunks load
// while this block's are filtered (the last block reloads itself).
// A chunk is 4 samples: a float4 of the float input, or a uint2 of 16-bit
// samples k (fvad_engine_submit_i16), read as k / 32768.0f -- k_pcm16's
// conversion, exact in f32, done here so the 16-bit push needs no float copy
// of its input (half k_prep3's input bytes, and no conversion kernel).
__device__ __forceinline__ float4 chunk4(float4 v) { return v; }
__device__ __forceinline__ float4 chunk4(uint2 v) {
  constexpr float k = 1.0f / 32768.0f;
  return make_float4((float)(short)(v.x & 0xffffu) * k, (float)(short)(v.x >> 16) * k,
                     (float)(short)(v.y & 0xffffu) * k, (float)(short)(v.y >> 16) * k);
}
template <bool Scaled, typename In>
__device__ __forceinline__ void prep_chain(const StagedArgs &a, const void *src, int s, int nt, float &mem0,
                                           float &mem1) {
  constexpr int kChunksCh = kFrame / 4;  // chunks of one channel's frame
  static_assert(kChunksCh % kPrepRing == 0, "ring blocks end at channel boundaries");
  const int C = a.n_channels;
  const int per_tick = C * kChunksCh;
  const int bpt = per_tick / kPrepRing;  // blocks per tick
  const int nb = nt * bpt;
  const size_t tick_stride = (size_t)a.n_streams * per_tick;  // in chunks
  const In *tick_row = reinterpret_cast<const In *>(src) + (size_t)s * per_tick;
  float4 *dst = reinterpret_cast<float4 *>(a.xs + (size_t)s * a.L + kHist);
  In ring[kPrepRing];
#pragma unroll
  for (int u = 0; u < kPrepRing; u++) ring[u] = tick_row[u];
  int rn = 1;  // block within the tick of the next block
  const float b0 = -2.0f, b1 = 1.0f, a0 = -1.99599f, a1 = 0.99600f;
  const float scalar = (float)32767;
  // b*x and a*y are exact in double (24-bit x 24-bit significands), so one
  // fma rounds b*x - a*y exactly once, as the C expression does
  auto step = [&](float v) -> float {
    const float xi = Scaled ? v * scalar : v;
    const float yi = xi + mem0;
    const double yd = (double)yi;
    mem0 = (float)((double)mem1 + __builtin_fma(-(double)a0, yd, b0 * (double)xi));
    mem1 = (float)__builtin_fma(-(double)a1, yd, b1 * (double)xi);
    return yi;
  };
  // RMS volume (VAD.zig:253-272): sum of squares of the raw samples of each
  // channel's frame in sample order, vol = sqrt(sum / 480), ratio = min / max
  // over the stream's channels in channel order
  float sum = 0, vmin = 1, vmax = 0;
  int jt = 0, t = 0;  // chunk within the tick, tick
#pragma unroll FVAD_PREP_UNROLL
  for (int b = 0; b < nb; b++) {
    if (rn == bpt && b + 1 < nb) {
      rn = 0;
      tick_row += tick_stride;
    }
    const In *q = tick_row + (b + 1 < nb ? rn : rn - 1) * kPrepRing;
    rn++;
#pragma unroll
    for (int u = 0; u < kPrepRing; u++) {
      const float4 x = chunk4(ring[u]);
      ring[u] = q[u];
      float4 y;
      y.x = step(x.x);
      y.y = step(x.y);
      y.z = step(x.z);
      y.w = step(x.w);
      dst[b * kPrepRing + u] = y;
      sum += x.x * x.x;
      sum += x.y * x.y;
      sum += x.z * x.z;
      sum += x.w * x.w;
    }
    jt += kPrepRing;
    if (jt % kChunksCh == 0) {
      const float vol = sqrtf(sum / (float)kFrame);
      sum = 0;
      if (vol < vmin) vmin = vol;
      if (vol > vmax) vmax = vol;
      if (jt == per_tick) {
        a.ratio[(size_t)t * a.n_streams + s] = (vmax == 0) ? 0 : vmin / vmax;
        vmin = 1;
        vmax = 0;
        jt = 0;
        t++;
      }
    }
  }
}

typedef float f4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(64) k_prep3(StagedArgs a) {
  const int tid = threadIdx.x, lane = tid;
  const int C = a.n_channels, S = prep_streams(C), sb = blockIdx.x * S;
  const int ns = min(S, a.n_streams - sb);  // streams in this workgroup
  if (ns <= 0) return;
  // pitch history of every stream -> xs[s][0..1248), and its x_lp values
  // (the first frame's x_lp[1..623]; k_fftAw writes the rest): flat over the
  // workgroup's streams, each lane's loads in batches of 8 before their
  // stores (a stream with no ticks gets a copy nobody reads)
  {
    constexpr int kH4 = kHist / 4, B = 8;
    f4 v[B];  // (a native vector: arrays of float4 structs stayed in scratch)
    float w[B];
    for (int i0 = 0; i0 < ns * kH4; i0 += 64 * B) {
#pragma unroll
      for (int u = 0; u < B; u++) {  // (clamped: every load unconditional)
        const int i = min(i0 + lane + 64 * u, ns * kH4 - 1), s = i / kH4, j = i - s * kH4;
        v[u] = reinterpret_cast<const f4 *>(a.state + (size_t)(sb + s) * st::kWords + st::kPitch + kFrame)[j];
      }
#pragma unroll
      for (int u = 0; u < B; u++) {
        const int i = i0 + lane + 64 * u, s = i / kH4, j = i - s * kH4;
        if (i < ns * kH4) reinterpret_cast<f4 *>(a.xs + (size_t)(sb + s) * a.L)[j] = v[u];
      }
    }
    for (int i0 = 0; i0 < ns * kXlpHist; i0 += 64 * B) {
#pragma unroll
      for (int u = 0; u < B; u++) {
        const int i = min(i0 + lane + 64 * u, ns * kXlpHist - 1), s = i / kXlpHist, m = max(i - s * kXlpHist, 1);
        const float *h = a.state + (size_t)(sb + s) * st::kWords + st::kPitch + kFrame;
        w[u] = xlp_value(h[2 * m - 1], h[2 * m], h[2 * m + 1]);
      }
#pragma unroll
      for (int u = 0; u < B; u++) {
        const int i = i0 + lane + 64 * u, s = i / kXlpHist, m = i - s * kXlpHist;
        if (i < ns * kXlpHist && m > 0) a.xlp[(size_t)(sb + s) * a.LX + m] = w[u];
      }
    }
  }
  {
    // the chain wave shares its SIMD with the previous push's kernels: its
    // latency-bound instruction stream goes first
    __builtin_amdgcn_s_setprio(3);
    if (lane < ns) {
      const int s = sb + lane, nt = ticks_of(a, s);
      if (nt > 0) {
        float *hp = a.state + (size_t)s * st::kWords + st::kHp;
        float mem0 = hp[0], mem1 = hp[1];
        if (a.raw_s16)
          prep_chain<false, float4>(a, a.pcm, s, nt, mem0, mem1);
        else if (a.pcm16)
          prep_chain<true, uint2>(a, a.pcm16, s, nt, mem0, mem1);
        else
          prep_chain<true, float4>(a, a.pcm, s, nt, mem0, mem1);
        hp[0] = mem0;
        hp[1] = mem1;
      }
    }
  }
  __syncthreads();
  // pitch_buf after the last frame = the last 1728 samples of the row (flat
  // over the workgroup's streams, as the history copies)
  {
    constexpr int kP4 = kPitchBuf / 4, B = 8;
    f4 v[B];
    for (int i0 = 0; i0 < ns * kP4; i0 += 64 * B) {
#pragma unroll
      for (int u = 0; u < B; u++) {
        const int i = min(i0 + lane + 64 * u, ns * kP4 - 1), s = i / kP4, j = i - s * kP4;
        const int nt = max(ticks_of(a, sb + s), 1);
        v[u] = reinterpret_cast<const f4 *>(a.xs + (size_t)(sb + s) * a.L + (size_t)(nt * C - 1) * kFrame)[j];
      }
#pragma unroll
      for (int u = 0; u < B; u++) {
        const int i = i0 + lane + 64 * u, s = i / kP4, j = i - s * kP4;
        const int nt = i < ns * kP4 ? ticks_of(a, sb + s) : 0;
        if (nt > 0) reinterpret_cast<f4 *>(a.state + (size_t)(sb + s) * st::kWords + st::kPitch)[j] = v[u];
      }
    }
  }
}

hipError_t launch_prep(const StagedArgs &a, hipStream_t stream, hipEvent_t *ev) {
  (void)hipGetLastError();
  if (ev) FVAD_LAUNCH_TRY(hipEventRecord(ev[kEvPrepBegin], stream));
  const int S = prep_streams(a.n_channels);
  FVAD_KERNEL_TRY(k_prep3, dim3((a.n_streams + S - 1) / S), dim3(64), 0, stream, a);
  if (ev) FVAD_LAUNCH_TRY(hipEventRecord(ev[kEvPrepEnd], stream));
  return hipSuccess;
}

// ---------------------------------------------------------------------------
// k_pcm16: the 16-bit ingest's conversion (fvad_engine_submit_i16), samples
// k -> k / 32768.0f, libsndfile's short -> float normalisation (the simulator's
// WAV reader does the same), exact in f32.  HBM-bound streaming: 16 B in and
// 32 B out per thread and step, grid-stride over the push.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pcm16(const int4 *__restrict__ src, float4 *__restrict__ dst, size_t n8) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
    const int4 v = src[i];
    const int w[4] = {v.x, v.y, v.z, v.w};
    float o[8];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      o[2 * k] = (float)(short)(w[k] & 0xffff) * (1.0f / 32768.0f);
      o[2 * k + 1] = (float)(short)(w[k] >> 16) * (1.0f / 32768.0f);
    }
    dst[2 * i] = make_float4(o[0], o[1], o[2], o[3]);
    dst[2 * i + 1] = make_float4(o[4], o[5], o[6], o[7]);
  }
}

hipError_t launch_pcm16(const int16_t *src, float *dst, size_t n, hipStream_t stream) {
  if (n % 8) return hipErrorInvalidValue;
  const size_t n8 = n / 8;
  const unsigned grid = (unsigned)std::min<size_t>((n8 + 255) / 256, 256 * 16);
  if (grid == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pcm16, dim3(grid), dim3(256), 0, stream, reinterpret_cast<const int4 *>(src),
                     reinterpret_cast<float4 *>(dst), n8);
  return hipGetLastError();
}

}  // namespace fvad
