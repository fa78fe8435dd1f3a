// Per-stream lifecycle kernels: clear, retarget (a stream's machine config),
// gather and scatter over the engine's
// per-stream layouts (fvad_lifecycle.h).  One workgroup per (listed stream,
// part), float4 accesses where the layout is 16-byte aligned (the state
// record, the long-term row, VadmState, the blob's sections); the re-block
// ring's pending part starts at any even sample and the short-term / ratio
// buffers are [i][stream] columns, so those go word by word.  No LDS.
//
// Every index a kernel uses was checked on the host (fvad_engine.cpp): the
// listed slots are < n_streams, the record indices < the staging buffer's
// count, and a restored record's counters and write indices are in range.
#include <hip/hip_runtime.h>

#include "fvad_lifecycle.h"

namespace fvad {

namespace {
constexpr int kNT = 256;

// samples the stream of a state record has consumed: frames_done frames with
// the denoiser, st::kNdSamples (u64) without
__device__ __forceinline__ unsigned long long record_samples(const float *rec, int use_denoiser) {
  if (use_denoiser) return (unsigned long long)reinterpret_cast<const int *>(rec)[st::kFramesDone] * kFrame;
  return *reinterpret_cast<const unsigned long long *>(rec + st::kNdSamples);
}

__device__ __forceinline__ void copy4(float *dst, const float *src, long long words, int tid) {
  for (long long q = tid; q < words / 4; q += kNT)
    reinterpret_cast<float4 *>(dst)[q] = reinterpret_cast<const float4 *>(src)[q];
}
__device__ __forceinline__ void zero4(float *dst, long long words, int tid) {
  for (long long q = tid; q < words / 4; q += kNT) reinterpret_cast<float4 *>(dst)[q] = make_float4(0, 0, 0, 0);
}
}  // namespace

// part 0: the state record's words of a.mode; part 1 + c: channel c's ring row
__global__ void __launch_bounds__(kNT) k_stream_clear(ClearArgs a) {
  const int s = a.ids.id[blockIdx.x], part = blockIdx.y, tid = threadIdx.x;
  if (part > 0) {
    zero4(a.ring + ((size_t)s * a.n_channels + (part - 1)) * a.ring_len, a.ring_len, tid);
    return;
  }
  float *stp = a.state + (size_t)s * st::kWords;
  if (a.mode == kClearAll) {
    zero4(stp, st::kWords, tid);
  } else if (a.mode == kClearPrep) {
    zero4(stp + st::kPitch, kPitchBuf, tid);
    if (tid < 2) stp[st::kHp + tid] = 0.0f;
  } else {
    // [kSyn, kWords) but the two high-pass words
    for (int q = st::kSyn / 4 + tid; q < st::kWords / 4; q += kNT) {
      if (q != st::kHp / 4) {
        reinterpret_cast<float4 *>(stp)[q] = make_float4(0, 0, 0, 0);
      } else {
        for (int w = 4 * q; w < 4 * q + 4; w++)
          if (w != st::kHp && w != st::kHp + 1) stp[w] = 0.0f;
      }
    }
  }
}

// machine blockIdx.y of a listed stream: its initial state, empty rolling
// buffers (entries 0.0f, as vadm_reset's memset), no segments (n_segs = 0)
__global__ void __launch_bounds__(kNT) k_stream_vclear(VClearArgs a) {
  const int s = a.ids.id[blockIdx.x], m = blockIdx.y, tid = threadIdx.x;
  const VadmConst &K = a.vadm.c[m];
  const size_t B = a.n_streams;
  // (per-stream configs: a fresh machine of the stream's own row, which stays;
  // K's lengths are then the room's, the whole of what the stream may use)
  if (tid == 0) {
    if (a.vadm.tab) {
      const VadmRow *r = a.vadm.tab + (size_t)m * B + s;
      a.vadm.st[(size_t)m * B + s] = vadm_fresh(r->has_init, r->n_lt, r->lt0, 0, 0);
    } else {
      a.vadm.st[(size_t)m * B + s] = a.init[m];
    }
  }
  zero4(a.vadm.buf + K.lt_off + (size_t)s * K.lt_pitch, K.lt_pitch, tid);
  for (int i = tid; i < K.n_st; i += kNT) a.vadm.buf[K.st_off + (size_t)i * B + s] = 0.0f;
  for (int i = tid; i < K.n_r; i += kNT) a.vadm.buf[K.r_off + (size_t)i * B + s] = 0.0f;
}

// listed stream blockIdx.x: machine a.machine becomes a fresh machine of
// a.row[blockIdx.x] -- the table row, the state (its window count and segment
// count stay), and rolling buffers empty over the machine's room, whatever
// the old and the new lengths are.  Runs on the side stream between two
// machine passes, so nothing else touches the lane.
__global__ void __launch_bounds__(kNT) k_vadm_retarget(RetargetArgs a) {
  const int i = blockIdx.x, s = a.id[i], tid = threadIdx.x;
  const size_t B = a.n_streams, idx = (size_t)a.machine * B + s;
  if (tid == 0) {
    a.tab[idx] = a.row[i];
    a.st[idx] = vadm_fresh(a.row[i].has_init, a.row[i].n_lt, a.row[i].lt0, a.st[idx].windows_done, a.st[idx].n_segs);
  }
  zero4(a.buf + a.lt_off + (size_t)s * a.lt_pitch, a.lt_pitch, tid);
  for (int k = tid; k < a.n_st; k += kNT) a.buf[a.st_off + (size_t)k * B + s] = 0.0f;
  for (int k = tid; k < a.n_r; k += kNT) a.buf[a.r_off + (size_t)k * B + s] = 0.0f;
}

// stream slots[i] -> record recs[i].  part 0: state; 1 + c: channel c's
// pending window part; 1 + C + m: machine m; 1 + C + n_mach: the channels'
// resampler tails, the input's (a resampling engine) and the output's (an
// engine with denoised_rate)
__global__ void __launch_bounds__(kNT) k_stream_gather(XferArgs a) {
  const int s = a.slots.id[blockIdx.x], part = blockIdx.y, tid = threadIdx.x;
  const BlobLayout &L = a.lay;
  const int C = L.n_channels;
  float *rec = a.blob + (size_t)a.recs.id[blockIdx.x] * L.words;
  const float *stp = a.state + (size_t)s * st::kWords;
  if (part == 0) {
    copy4(rec, stp, st::kWords, tid);
  } else if (part == 1 + C + L.n_mach) {
    if (L.rs_tail > 0) {
      const float *tails = a.rs_tails + (size_t)s * C * L.rs_tail;
      for (int c = 0; c < C; c++)
        for (int j = tid; j < (int)L.rs_pad; j += kNT)
          rec[L.o_rs + (size_t)c * L.rs_pad + j] = j < L.rs_tail ? tails[(size_t)c * L.rs_tail + j] : 0.0f;
    }
    if (L.ro_tail > 0) {
      const float *tails = a.ro_tails + (size_t)s * C * L.ro_tail;
      for (int c = 0; c < C; c++)
        for (int j = tid; j < (int)L.ro_pad; j += kNT)
          rec[L.o_ro + (size_t)c * L.ro_pad + j] = j < L.ro_tail ? tails[(size_t)c * L.ro_tail + j] : 0.0f;
    }
  } else if (part <= C) {
    const int c = part - 1;
    const unsigned long long total = record_samples(stp, L.use_denoiser);
    const long long pend = (long long)(total % (unsigned)L.fft_size);
    const unsigned long long w0 = total - (unsigned long long)pend;
    const float *ring = a.ring + ((size_t)s * C + c) * a.ring_len;
    float *dst = rec + L.o_ring + (size_t)c * L.pend_pad;
    for (long long j = tid; j < L.pend_pad; j += kNT)
      dst[j] = j < pend ? ring[(w0 + (unsigned long long)j) % (unsigned)a.ring_len] : 0.0f;
  } else {
    const int m = part - 1 - C;
    const VadmConst &K = a.vadm.c[m];
    const size_t B = a.n_streams, idx = (size_t)m * B + s;
    float *dst = rec + L.o_mach[m];
    copy4(dst, reinterpret_cast<const float *>(a.vadm.st + idx), kVadmStateWords, tid);
    dst += kVadmStateWords;
    copy4(dst, a.vadm.buf + K.lt_off + (size_t)s * K.lt_pitch, K.lt_pitch, tid);
    dst += pad4(K.lt_pitch);
    for (int i = tid; i < (int)pad4(K.n_st); i += kNT) dst[i] = i < K.n_st ? a.vadm.buf[K.st_off + (size_t)i * B + s] : 0.0f;
    dst += pad4(K.n_st);
    for (int i = tid; i < (int)pad4(K.n_r); i += kNT) dst[i] = i < K.n_r ? a.vadm.buf[K.r_off + (size_t)i * B + s] : 0.0f;
    dst += pad4(K.n_r);
    // the stored segments (the list keeps the first seg_cap), zeros after
    const unsigned stored = min(a.vadm.st[idx].n_segs, (unsigned)a.vadm.seg_cap);
    const unsigned *seg = reinterpret_cast<const unsigned *>(a.vadm.seg + idx * a.vadm.seg_cap);
    unsigned *sd = reinterpret_cast<unsigned *>(dst);
    const long long nw = (long long)kVadmSegWords * stored;
    for (long long w = tid; w < pad4((long long)kVadmSegWords * L.seg_cap); w += kNT) sd[w] = w < nw ? seg[w] : 0u;
  }
}

// record recs[i] -> stream slots[i]: the reverse.  The pending window part
// goes to this engine's ring positions (absolute sample mod ring_len); a
// smaller segment capacity keeps the first seg_cap segments and the true total.
__global__ void __launch_bounds__(kNT) k_stream_scatter(XferArgs a) {
  const int s = a.slots.id[blockIdx.x], part = blockIdx.y, tid = threadIdx.x;
  const BlobLayout &L = a.lay;
  const int C = L.n_channels;
  const float *rec = a.blob + (size_t)a.recs.id[blockIdx.x] * L.words;
  if (part == 0) {
    copy4(a.state + (size_t)s * st::kWords, rec, st::kWords, tid);
  } else if (part == 1 + C + L.n_mach) {
    if (L.rs_tail > 0) {
      float *tails = a.rs_tails + (size_t)s * C * L.rs_tail;
      for (int c = 0; c < C; c++)
        for (int j = tid; j < L.rs_tail; j += kNT) tails[(size_t)c * L.rs_tail + j] = rec[L.o_rs + (size_t)c * L.rs_pad + j];
    }
    if (L.ro_tail > 0) {
      float *tails = a.ro_tails + (size_t)s * C * L.ro_tail;
      for (int c = 0; c < C; c++)
        for (int j = tid; j < L.ro_tail; j += kNT) tails[(size_t)c * L.ro_tail + j] = rec[L.o_ro + (size_t)c * L.ro_pad + j];
    }
  } else if (part <= C) {
    const int c = part - 1;
    const unsigned long long total = record_samples(rec, L.use_denoiser);
    const long long pend = (long long)(total % (unsigned)L.fft_size);
    const unsigned long long w0 = total - (unsigned long long)pend;
    float *ring = a.ring + ((size_t)s * C + c) * a.ring_len;
    const float *src = rec + L.o_ring + (size_t)c * L.pend_pad;
    for (long long j = tid; j < pend; j += kNT) ring[(w0 + (unsigned long long)j) % (unsigned)a.ring_len] = src[j];
  } else {
    const int m = part - 1 - C;
    const VadmConst &K = a.vadm.c[m];
    const size_t B = a.n_streams, idx = (size_t)m * B + s;
    const float *src = rec + L.o_mach[m];
    const unsigned n_segs = reinterpret_cast<const VadmState *>(src)->n_segs;
    copy4(reinterpret_cast<float *>(a.vadm.st + idx), src, kVadmStateWords, tid);
    src += kVadmStateWords;
    copy4(a.vadm.buf + K.lt_off + (size_t)s * K.lt_pitch, src, K.lt_pitch, tid);
    src += pad4(K.lt_pitch);
    for (int i = tid; i < K.n_st; i += kNT) a.vadm.buf[K.st_off + (size_t)i * B + s] = src[i];
    src += pad4(K.n_st);
    for (int i = tid; i < K.n_r; i += kNT) a.vadm.buf[K.r_off + (size_t)i * B + s] = src[i];
    src += pad4(K.n_r);
    const unsigned keep = min(min(n_segs, (unsigned)L.seg_cap), (unsigned)a.vadm.seg_cap);
    unsigned *seg = reinterpret_cast<unsigned *>(a.vadm.seg + idx * a.vadm.seg_cap);
    const unsigned *ss = reinterpret_cast<const unsigned *>(src);
    const long long nw = (long long)kVadmSegWords * keep;
    for (long long w = tid; w < (long long)kVadmSegWords * a.vadm.seg_cap; w += kNT) seg[w] = w < nw ? ss[w] : 0u;
  }
}

namespace {
hipError_t launched() { return hipGetLastError(); }
}  // namespace

hipError_t launch_stream_clear(const ClearArgs &a, hipStream_t stream) {
  if (a.ids.n < 1) return hipSuccess;
  (void)hipGetLastError();
  const unsigned parts = a.mode == kClearPrep ? 1u : 1u + (unsigned)a.n_channels;
  hipLaunchKernelGGL(k_stream_clear, dim3((unsigned)a.ids.n, parts), dim3(kNT), 0, stream, a);
  return launched();
}

hipError_t launch_stream_vclear(const VClearArgs &a, hipStream_t stream) {
  if (a.ids.n < 1 || a.vadm.n < 1) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_stream_vclear, dim3((unsigned)a.ids.n, (unsigned)a.vadm.n), dim3(kNT), 0, stream, a);
  return launched();
}

hipError_t launch_vadm_retarget(const RetargetArgs &a, hipStream_t stream) {
  if (a.n < 1) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_vadm_retarget, dim3((unsigned)a.n), dim3(kNT), 0, stream, a);
  return launched();
}

hipError_t launch_stream_gather(const XferArgs &a, hipStream_t stream) {
  if (a.slots.n < 1) return hipSuccess;
  (void)hipGetLastError();
  const unsigned parts = 1u + (unsigned)a.lay.n_channels + (unsigned)a.lay.n_mach + (a.lay.rs_tail > 0 || a.lay.ro_tail > 0 ? 1u : 0u);
  hipLaunchKernelGGL(k_stream_gather, dim3((unsigned)a.slots.n, parts), dim3(kNT), 0, stream, a);
  return launched();
}

hipError_t launch_stream_scatter(const XferArgs &a, hipStream_t stream) {
  if (a.slots.n < 1) return hipSuccess;
  (void)hipGetLastError();
  const unsigned parts = 1u + (unsigned)a.lay.n_channels + (unsigned)a.lay.n_mach + (a.lay.rs_tail > 0 || a.lay.ro_tail > 0 ? 1u : 0u);
  hipLaunchKernelGGL(k_stream_scatter, dim3((unsigned)a.slots.n, parts), dim3(kNT), 0, stream, a);
  return launched();
}

}  // namespace fvad
