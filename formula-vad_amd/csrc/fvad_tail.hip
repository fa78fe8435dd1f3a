// The three-kernel synthesis tail of the staged pipeline (k_ola, k_winmeta,
// FFT B: k_fftb, or k_fftbw of fvad_wave.hip for fft_size 2048), run where the
// fused k_olafb (fvad_wave.hip) does not apply, and the no-denoiser path
// (k_ndring, k_ndmeta, k_ndvol, FFT B).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fvad_device.h"
#include "fvad_internal.h"
#include "fvad_launch.h"
#include "fvad_staged.h"
#include "fvad_staged_dev.h"

namespace fvad {

// ---------------------------------------------------------------------------
// k_ola: out = x[0..479] + synthesis_mem (at the seams k_synthw leaves, done
// in its registers elsewhere); denoised * 1/32767; re-block ring;
// per-tick vad_low (min over channels in channel order).  Two frames per
// 256-thread workgroup, a float4 of samples per thread (32-bit frame
// arithmetic; the ring position of a frame is reduced once per thread).
// ---------------------------------------------------------------------------
static_assert(st::kSyn % 4 == 0 && kFrame % 4 == 0, "k_ola float4 rows");
__global__ void __launch_bounds__(256) k_ola(StagedArgs a) {
  const int C = a.n_channels, V = a.V;
  const int q = threadIdx.x & 127;
  const long long fl = (long long)blockIdx.x * 2 + (threadIdx.x >> 7);
  if (fl >= (long long)a.n_streams * V || q >= kFrame / 4) return;
  const int s = (int)(fl / V), v = (int)(fl - (long long)s * V);
  const int nt = ticks_of(a, s);
  if (v >= nt * C) return;
  const int t = v / C, c = v - t * C, i = 4 * q;
  const float *stp = a.state + (size_t)s * st::kWords;
  const size_t f = (size_t)s * V + v;
  // k_synthw has added the previous half already except at a seam (ys rows,
  // fvad_staged.h); adding a zero elsewhere would turn a -0 into +0
  float4 o = *reinterpret_cast<const float4 *>(a.ys + f * kWin + i);
  if (ys_seam((long long)f, v)) {
    const float4 prev = (v == 0) ? *reinterpret_cast<const float4 *>(stp + st::kSyn + i)
                                 : *reinterpret_cast<const float4 *>(a.ys + (f - 1) * kWin + kFrame + i);
    o = make_float4(o.x + prev.x, o.y + prev.y, o.z + prev.z, o.w + prev.w);
  }
  if (!a.raw_s16) {
    const float k = 1.0f / (float)32767;
    o = make_float4(o.x * k, o.y * k, o.z * k, o.w * k);
  }
  const int frames_done = reinterpret_cast<const int *>(stp)[st::kFramesDone];
  long long ri = (long long)(frames_done + t) * kFrame % a.ring_len + i;  // ring_len % 4 == 0: no float4 wraps
  if (ri >= a.ring_len) ri -= a.ring_len;
  *reinterpret_cast<float4 *>(a.ring + ((size_t)s * C + c) * a.ring_len + ri) = o;
  if (a.out_den) *reinterpret_cast<float4 *>(a.out_den + (((size_t)t * a.n_streams + s) * C + c) * kFrame + i) = o;
  if (i == 0 && c == 0) {
    float vad_low = 1;
    for (int cc = 0; cc < C; cc++) {
      const float vv = a.vadf[(size_t)s * V + t * C + cc];
      if (vv < vad_low) vad_low = vv;
    }
    a.out_vad[(size_t)t * a.n_streams + s] = vad_low;
  }
}

// ---------------------------------------------------------------------------
// k_winmeta: window completion bookkeeping (VAD.zig:298-348): lane per stream
// for the serial tick walk (16 streams per 64-thread workgroup), then the
// whole workgroup copies the streams' synthesis memory (second half of each
// stream's last frame) into the state.
// ---------------------------------------------------------------------------
constexpr int kWmS = 16;
__global__ void __launch_bounds__(64) k_winmeta(StagedArgs a) {
  const int sb = blockIdx.x * kWmS, tid = threadIdx.x;
  if (tid < kWmS && sb + tid < a.n_streams) {
    const int s = sb + tid;
    const int nt = ticks_of(a, s);
    int *wt = a.win_tick + (size_t)s * a.wmax;
    long long *wsx = a.win_start + (size_t)s * a.wmax;
    int j = 0;
    if (nt > 0) {
      float *stp = a.state + (size_t)s * st::kWords;
      int *istp = reinterpret_cast<int *>(stp);
      int fd = istp[st::kFramesDone];
      float vol = stp[st::kVolAcc];
      const int FB = a.plan->nfft_b, wpt = a.wpt;
      // the per-tick inputs (ratio, vad) of 8 ticks load before any of their
      // outputs is stored (stores between the loads would serialise them)
      constexpr int kWmT = 8;
      for (int t0 = 0; t0 < nt; t0 += kWmT) {
        float rr[kWmT], vv[kWmT];
#pragma unroll
        for (int u = 0; u < kWmT; u++) {
          const size_t o = (size_t)(t0 + u) * a.n_streams + s;
          rr[u] = t0 + u < nt ? a.ratio[o] : 0.0f;
          vv[u] = t0 + u < nt ? a.out_vad[o] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kWmT; u++) {
          const int t = t0 + u;
          if (t < nt) {
            const size_t o = (size_t)t * a.n_streams + s, ow = o * wpt;
            const float ratio = rr[u];
            // fftBufferStep (VAD.zig:307-347): the frame goes into the FFT
            // buffer in pieces of min(room left, samples left); each piece
            // adds ratio * written / fft_size, a full buffer is a window
            // (vad = this frame's); fft_size < 480 completes several per tick
            const long long a0 = (long long)fd * kFrame;
            int off = 0, nw = 0;
            while (off < kFrame) {
              const long long pos = a0 + off, wdone = pos / FB, next_end = (wdone + 1) * FB;
              const int written = (int)min((long long)(kFrame - off), next_end - pos);
              vol += ratio * ((float)written / (float)FB);
              off += written;
              if (pos + written == next_end) {
                a.out_win_ratio[ow + nw] = vol;
                a.out_win_vad[ow + nw] = vv[u];
                vol = 0;
                wt[j] = t * wpt + nw;
                wsx[j] = wdone * FB;
                j++;
                nw++;
              }
            }
            // slots without a window: band sums, ratio and vad defined as 0
            for (int w = nw; w < wpt; w++) {
              a.out_win_ratio[ow + w] = 0.0f;
              a.out_win_vad[ow + w] = 0.0f;
              for (int i = 0; i < a.n_channels * a.n_bands; i++)
                a.out_band[(ow + w) * a.n_channels * a.n_bands + i] = 0.0f;
            }
            a.out_win_flag[o] = nw;
            fd++;
          }
        }
      }
      istp[st::kFramesDone] = fd;
      stp[st::kVolAcc] = vol;
    }
    for (; j < a.wmax; j++) wt[j] = -1;
  }
  // synthesis_mem for the next launch = second half of the last frame's
  // window (a tail ys_tail_kept keeps in the ys row); each lane's float4
  // loads go out before its stores (a store
  // between them would make every load wait for the one before)
  // (4 streams per pass: lane = float4 q and q + 64 of each stream's 120)
  constexpr int kSynQ = kFrame / 4, kSynS = 4;
  static_assert(kSynQ <= 128 && kWmS % kSynS == 0, "synthesis copy");
  for (int s0 = 0; s0 < kWmS; s0 += kSynS) {
    float4 v[kSynS][2];
    bool ok[kSynS][2];
#pragma unroll
    for (int k = 0; k < kSynS; k++) {
      const int s = sb + s0 + k;
      const int nt = s < a.n_streams ? ticks_of(a, s) : 0;
      const float4 *yl = reinterpret_cast<const float4 *>(
          a.ys + ((size_t)s * a.V + (size_t)max(nt, 1) * a.n_channels - 1) * kWin + kFrame);
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int q = tid + 64 * h;
        ok[k][h] = nt > 0 && q < kSynQ;
        v[k][h] = ok[k][h] ? yl[q] : make_float4(0, 0, 0, 0);
      }
    }
#pragma unroll
    for (int k = 0; k < kSynS; k++)
#pragma unroll
      for (int h = 0; h < 2; h++)
        if (ok[k][h])
          reinterpret_cast<float4 *>(a.state + (size_t)(sb + s0 + k) * st::kWords + st::kSyn)[tid + 64 * h] = v[k][h];
  }
}

hipError_t launch_ola(const StagedArgs &a, hipStream_t stream) {
  const long long frames = (long long)a.n_streams * a.V;
  FVAD_KERNEL_TRY(k_ola, dim3((unsigned)((frames + 1) / 2)), dim3(256), 0, stream, a);
  return hipSuccess;
}

hipError_t launch_winmeta(const StagedArgs &a, hipStream_t stream) {
  FVAD_KERNEL_TRY(k_winmeta, dim3((a.n_streams + kWmS - 1) / kWmS), dim3(64), 0, stream, a);
  return hipSuccess;
}

// ---------------------------------------------------------------------------
// k_fftb: one workgroup per (stream, completed window): FFT B per channel.
// kLds: the transform's work arrays in dynamic LDS (fft_size <= kMaxFftB);
// otherwise each of the grid's workgroups owns a slice of device scratch and
// walks the (stream, window) units grid-stride.  Output index of a window:
// its slot (tick * wpt + rank in the tick, k_winmeta / k_ndmeta).
// ---------------------------------------------------------------------------
__device__ __forceinline__ size_t win_out(const StagedArgs &a, int s, int slot) {
  const int t = slot / a.wpt;
  return ((size_t)t * a.n_streams + s) * a.wpt + (slot - t * a.wpt);
}

// kiss_fftr's split for bin k (0..nc) of the nc-point transform in W, and the
// bin's magnitude
__device__ __forceinline__ float fftr_mag(const float2 *W, const float2 *__restrict__ sup, int k, int nc, float norm) {
  float re, imv;
  if (k == 0) {
    re = W[0].x + W[0].y;
    imv = 0;
  } else if (k == nc) {
    re = W[0].x - W[0].y;
    imv = 0;
  } else {
    const int kk = (2 * k < nc) ? k : nc - k;
    const float2 fpk = W[kk];
    const float2 fpnk = make_float2(W[nc - kk].x, -W[nc - kk].y);
    const float2 f1k = cadd(fpk, fpnk), f2k = csub(fpk, fpnk);
    const float2 tw2 = cmul(f2k, sup[kk - 1]);
    if (2 * k < nc) {
      re = (f1k.x + tw2.x) * ((float).5);
      imv = (f1k.y + tw2.y) * ((float).5);
    } else {
      re = (f1k.x - tw2.x) * ((float).5);
      imv = (tw2.y - f1k.y) * ((float).5);
    }
  }
  const float r2 = re * re, i2 = imv * imv;
  return sqrtf(r2 + i2) * norm;
}

// kTap (want_spectrum): the magnitudes of the bins a.spec_lo..a.spec_hi also go
// to the window's row of a.spec, a thread per bin (coalesced stores).
template <int NT, bool kLds, bool kTap>
__global__ void __launch_bounds__(NT) k_fftb(StagedArgs a) {
  // W[nc] (+ S[nc] with a radix > 5), then the magnitudes of the reported bins
  extern __shared__ __attribute__((aligned(16))) float2 Wl[];
  const Plan *__restrict__ P = a.plan;
  const int nc = P->ncfft_b, C = a.n_channels;
  float2 *W = kLds ? Wl : a.fb_work + (size_t)blockIdx.x * a.fb_work_stride;
  float2 *S = W + nc;
  float *mag = reinterpret_cast<float *>(W + (P->generic_b ? 2 * nc : nc));
  const int tid = threadIdx.x;
  const float2 *__restrict__ twb = a.fb_tw;
  const float2 *__restrict__ sup = a.fb_sup;
  const int *__restrict__ perm = a.fb_perm;
  const float *__restrict__ hann = a.fb_hann;
  const long long units = (long long)a.n_streams * a.wmax;
  for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int s = (int)(unit / a.wmax), j = (int)(unit - (long long)s * a.wmax);
    const int slot = a.win_tick[(size_t)s * a.wmax + j];
    if (slot < 0) continue;  // uniform over the workgroup
    const long long wstart = a.win_start[(size_t)s * a.wmax + j];
    const size_t o = win_out(a, s, slot);
    for (int c = 0; c < C; c++) {
      const float *ring = a.ring + ((size_t)s * C + c) * a.ring_len;
      for (int k = tid; k < nc; k += NT) {
        const int n = perm[k];
        const float t0 = ring[(wstart + 2 * n) % a.ring_len] * hann[2 * n];
        const float t1 = ring[(wstart + 2 * n + 1) % a.ring_len] * hann[2 * n + 1];
        W[k] = make_float2(t0, t1);
      }
      __syncthreads();
      kiss_stages(W, S, P->fac_b, P->nfac_b, nc, twb, tid, NT);
      const int lo = a.bin_lo_all, hi = a.bin_hi_all;
      for (int k = lo + tid; k <= hi; k += NT) mag[k - lo] = fftr_mag(W, sup, k, nc, P->norm_b);
      if constexpr (kTap) {
        float *spec = a.spec + (o * C + c) * (size_t)(a.spec_hi - a.spec_lo + 1);
        for (int k = a.spec_lo + tid; k <= a.spec_hi; k += NT) spec[k - a.spec_lo] = fftr_mag(W, sup, k, nc, P->norm_b);
      }
      __syncthreads();
      if (tid < a.n_bands) {
        float acc = 0.0f;
        for (int k = a.band_lo[tid]; k <= a.band_hi[tid]; k++) acc += mag[k - lo];
        a.out_band[(o * C + c) * a.n_bands + tid] = acc;
      }
      __syncthreads();
    }
  }
}

// FFT B of every completed window: the wave-per-window kernel for 2048 points
// (one window per tick at most), the block kernel k_fftb (mixed radix) for
// every other size -- work arrays in LDS up to kMaxFftB and 160 KB, else in
// device scratch (the engine sizes a.fb_work by fftb_work_stride)
bool fftb_generic(int nc) {  // kf_factor(nc) has a radix > 5
  int n = nc;
  for (int p : {4, 2, 3, 5})
    while (n % p == 0) n /= p;
  return n > 1;
}

long long fftb_work_stride(int nfft_b, int bin_lo_all, int bin_hi_all, int generic) {
  const long long nc = nfft_b / 2, bins = bin_hi_all - bin_lo_all + 1;
  const long long lds = (long long)sizeof(float2) * nc * (generic ? 2 : 1) + (long long)sizeof(float) * bins;
  if (nfft_b <= kMaxFftB && lds <= 160 * 1024) return 0;
  return (nc * (generic ? 2 : 1) + (bins + 1) / 2 + 1) & ~1LL;  // float2 units, 16-byte aligned slices
}

template <bool kTap>
static hipError_t launch_fftb_block(const StagedArgs &a, hipStream_t stream) {
  static const bool attr = [] {
    bool ok = true;
    for (const void *k : {reinterpret_cast<const void *>(&k_fftb<256, true, kTap>),
                          reinterpret_cast<const void *>(&k_fftb<64, true, kTap>)})
      ok &= hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
    return ok;
  }();
  (void)attr;
  const long long units = (long long)a.n_streams * a.wmax;
  if (a.fb_work) {
    const unsigned grid = (unsigned)std::min<long long>(units, a.fb_work_blocks);
    FVAD_KERNEL_TRY((k_fftb<256, false, kTap>), dim3(grid), dim3(256), 0, stream, a);
    return hipSuccess;
  }
  const int nc = a.nfft_b / 2;
  const size_t lds = sizeof(float2) * (size_t)nc * (fftb_generic(nc) ? 2 : 1) +
                     sizeof(float) * (size_t)(a.bin_hi_all - a.bin_lo_all + 1);
  const unsigned grid = (unsigned)std::min<long long>(units, 1 << 16);
  if (nc <= 64)  // fft_size <= 128: a wave per window
    FVAD_KERNEL_TRY((k_fftb<64, true, kTap>), dim3(grid), dim3(64), lds, stream, a);
  else
    FVAD_KERNEL_TRY((k_fftb<256, true, kTap>), dim3(grid), dim3(256), lds, stream, a);
  return hipSuccess;
}

hipError_t launch_fftb(const StagedArgs &a, int n_cu, hipStream_t stream) {
  if (a.nfft_b == 2048) return launch_wave(kWaveFftB, a, n_cu, stream);
  // want_spectrum (a.spec): the tap instantiations
  return a.spec ? launch_fftb_block<true>(a, stream) : launch_fftb_block<false>(a, stream);
}

// ---------------------------------------------------------------------------
// use_denoiser = false (VAD.zig:206-212,239-249): the pipeline reads fft_size
// frames of raw input straight into FFT B; no rnnoise, no per-frame vad.  The
// reference takes a window as soon as fft_size samples are in, whatever the
// size of the pushes, so this path counts samples, not ticks: a stream's last
// valid tick may hold only a.tail[s] real samples (the end of a stream, or the
// remainder of an AudioPipeline push), and st::kNdSamples (u64) is the
// stream's absolute sample count.
// k_ndring: the real input samples -> the stream's re-block ring, per-tick vad
// / ratio set to -1 (not produced by the reference on this path), the raw
// input as the "denoised" output.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int nd_real(const StagedArgs &a, int s, int t, int nt) {
  return (a.tail && t == nt - 1) ? a.tail[s] : kFrame;
}
__device__ __forceinline__ unsigned long long *nd_count(const StagedArgs &a, int s) {
  return reinterpret_cast<unsigned long long *>(a.state + (size_t)s * st::kWords + st::kNdSamples);
}

__global__ void __launch_bounds__(256) k_ndring(StagedArgs a) {
  const int C = a.n_channels, V = a.V;
  const int q = threadIdx.x & 127;
  const long long fl = (long long)blockIdx.x * 2 + (threadIdx.x >> 7);
  if (fl >= (long long)a.n_streams * V || q >= kFrame / 4) return;
  const int s = (int)(fl / V), v = (int)(fl - (long long)s * V);
  const int nt = ticks_of(a, s);
  if (v >= nt * C) return;
  const int t = v / C, c = v - t * C, i = 4 * q;
  const size_t o = (size_t)t * a.n_streams + s;
  const float4 x = *reinterpret_cast<const float4 *>(a.pcm + (o * C + c) * kFrame + i);
  const int n = nd_real(a, s, t, nt);
  const unsigned long long p0 = *nd_count(a, s) + (unsigned long long)t * kFrame + i;
  float *ring = a.ring + ((size_t)s * C + c) * a.ring_len;
  const float xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int e = 0; e < 4; e++)
    if (i + e < n) ring[(p0 + e) % (unsigned long long)a.ring_len] = xv[e];
  if (a.out_den) *reinterpret_cast<float4 *>(a.out_den + (o * C + c) * kFrame + i) = x;
  if (i == 0 && c == 0) {
    a.out_vad[o] = -1.0f;
    a.ratio[o] = -1.0f;
  }
}

// k_ndmeta: window completion per tick (a window completes in the tick that
// brings its last sample; fft_size < 480: several per tick), lane per stream;
// the completed windows' volume ratios are k_ndvol's.
__global__ void __launch_bounds__(64) k_ndmeta(StagedArgs a) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= a.n_streams) return;
  const int nt = ticks_of(a, s), C = a.n_channels, FB = a.nfft_b;
  int *wt = a.win_tick + (size_t)s * a.wmax;
  long long *wsx = a.win_start + (size_t)s * a.wmax;
  int j = 0;
  if (nt > 0) {
    unsigned long long *cnt = nd_count(a, s);
    const unsigned long long sd0 = *cnt;
    for (int t = 0; t < nt; t++) {
      const size_t o = (size_t)t * a.n_streams + s, ow = o * a.wpt;
      // the tick's samples [a0, end) complete every window ending in (a0, end]
      // (fft_size < 480: several)
      const unsigned long long a0 = sd0 + (unsigned long long)t * kFrame;
      const unsigned long long end = a0 + (unsigned)nd_real(a, s, t, nt);
      unsigned long long next_end = (a0 / (unsigned)FB + 1) * (unsigned)FB;
      int nw = 0;
      for (; next_end <= end; next_end += (unsigned)FB, nw++) {
        a.out_win_vad[ow + nw] = -1.0f;
        wt[j] = t * a.wpt + nw;
        wsx[j] = (long long)(next_end - (unsigned)FB);
        j++;
      }
      for (int w = nw; w < a.wpt; w++) {
        a.out_win_ratio[ow + w] = 0.0f;
        a.out_win_vad[ow + w] = 0.0f;
        for (int i = 0; i < C * a.n_bands; i++) a.out_band[(ow + w) * C * a.n_bands + i] = 0.0f;
      }
      a.out_win_flag[o] = nw;
    }
    *cnt = sd0 + (unsigned long long)(nt - 1) * kFrame + (unsigned)nd_real(a, s, nt - 1, nt);
  }
  for (; j < a.wmax; j++) wt[j] = -1;
}

// k_ndvol: a completed window's volume ratio, preAnalyzeSegment over its
// fft_size input samples (VAD.zig:253-272: rmsVolume per channel =
// sqrt(sum x^2 / n) with the sum in sample order, audio_utils.zig:14-24; min /
// max over channels in channel order).  The sum is one serial f32 chain per
// channel, so the parallelism is across windows: lane per (stream, window of
// this push) -- ~fft_size / 480 times k_ndmeta's lanes.
__global__ void __launch_bounds__(64) k_ndvol(StagedArgs a) {
  const long long item = (long long)blockIdx.x * 64 + threadIdx.x;
  if (item >= (long long)a.n_streams * a.wmax) return;
  const int s = (int)(item / a.wmax), j = (int)(item - (long long)s * a.wmax);
  const int t = a.win_tick[(size_t)s * a.wmax + j];
  if (t < 0) return;
  const int C = a.n_channels, FB = a.nfft_b;
  const unsigned long long ws = (unsigned long long)a.win_start[(size_t)s * a.wmax + j];
  float vol_min = 1, vol_max = 0;
  for (int c = 0; c < C; c++) {
    const float *ring = a.ring + ((size_t)s * C + c) * a.ring_len;
    long long ri = (long long)(ws % (unsigned long long)a.ring_len);
    float sum = 0.0f;
    for (int n = 0; n < FB; n++) {
      const float x = ring[ri];
      sum += x * x;
      if (++ri == a.ring_len) ri = 0;
    }
    const float vol = sqrtf(sum / (float)FB);
    if (vol < vol_min) vol_min = vol;
    if (vol > vol_max) vol_max = vol;
  }
  a.out_win_ratio[win_out(a, s, t)] = vol_max == 0 ? 0.0f : vol_min / vol_max;
}

hipError_t launch_nodenoise(const StagedArgs &a, int n_cu, hipStream_t stream) {
  (void)hipGetLastError();
  const long long frames = (long long)a.n_streams * a.V;
  FVAD_KERNEL_TRY(k_ndring, dim3((unsigned)((frames + 1) / 2)), dim3(256), 0, stream, a);
  FVAD_KERNEL_TRY(k_ndmeta, dim3((a.n_streams + 63) / 64), dim3(64), 0, stream, a);
  FVAD_KERNEL_TRY(k_ndvol, dim3((unsigned)(((long long)a.n_streams * a.wmax + 63) / 64)), dim3(64), 0, stream, a);
  return launch_fftb(a, n_cu, stream);
}

}  // namespace fvad
