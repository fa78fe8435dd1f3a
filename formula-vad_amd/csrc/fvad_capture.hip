// Clip capture kernels (fvad_capture.h; DESIGN.md section 7, "Clip capture").
//
// k_hist_append / k_hist_advance run on the stream that reads a push's device
// input: the first copies the valid ticks of every stream into the history
// ring and only reads the streams' positions, the second advances them and
// leaves the push's snapshot for its capture pass.  A capture of the denoised
// rows appends with k_den_append on the engine stream instead, in samples of
// the clip rate; an s16 capture copies with k_cap_copy_short.
//
// The capture pass runs on the side stream between a push's machine pass and
// k_vadm_events: k_cap_plan, k_cap_channel, k_cap_copy, k_cap_publish.  The
// decisions (due, cut, queue, room) are fvad_capture_core.h's.
//
// Every index: a stream s < n_streams, a ring index < H (one conditional
// subtraction after an index < 2H, or a % H), a pool index < pool_cap (a
// placed clip is no longer than the pool), a work index < kQueue * n_streams
// (a stream has at most kQueue due clips), a descriptor index % desc_cap.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fvad_capture.h"
#include "fvad_launch.h"

namespace fvad {

namespace {
constexpr int kNT = 256;
constexpr int kVeSegment = 2;  // FVAD_EVENT_SEGMENT (include/fvad.h)
constexpr int kRowQuads = kFrame / 4;
}  // namespace

// ---------------------------------------------------------------------------
// k_hist_append: [t][s][c][480] -> ring [s][c][H], float4 by float4.  A
// stream's ticks start at wpos, a multiple of 480, and H is a multiple of 4,
// so no float4 straddles the ring's end.
// ---------------------------------------------------------------------------
template <bool S16>
__global__ void __launch_bounds__(kNT) k_hist_append(CapAppendArgs a) {
  const long long total = (long long)a.n_ticks * a.n_streams * a.n_channels * kRowQuads;
  for (long long i = (long long)blockIdx.x * kNT + threadIdx.x; i < total; i += (long long)gridDim.x * kNT) {
    const int q = (int)(i % kRowQuads);
    long long r = i / kRowQuads;
    const int c = (int)(r % a.n_channels);
    r /= a.n_channels;
    const int s = (int)(r % a.n_streams), t = (int)(r / a.n_streams);
    const int valid = a.ticks_valid ? a.ticks_valid[s] : a.n_ticks;
    if (t >= valid) continue;
    float4 v;
    if (S16) {
      const short4 k = reinterpret_cast<const short4 *>(a.pcm16)[i];
      v = make_float4((float)k.x / 32768.0f, (float)k.y / 32768.0f, (float)k.z / 32768.0f, (float)k.w / 32768.0f);
    } else {
      v = reinterpret_cast<const float4 *>(a.pcm)[i];
    }
    const unsigned long long w = (a.pos[s].wpos + (unsigned long long)t * kFrame + (unsigned)q * 4u) % a.H;
    *reinterpret_cast<float4 *>(a.hist + ((size_t)s * a.n_channels + c) * a.H + w) = v;
  }
}

// ---------------------------------------------------------------------------
// k_den_append: the denoised rows [t][s][c][n] (n = a.frame samples of
// the clip rate) -> ring [s][c][H], the valid ticks only: the rows past
// ticks_valid[s] hold zeros (k_resample_out) or an older push (d_den).  A
// stream's ticks start at wpos, a multiple of n; H is a multiple of 4.
//
// A4 (n % 4 == 0: every rate but 44.1 kHz): rows and ring places are 16-byte
// aligned, float4 by float4 as k_hist_append.
//
// Otherwise (n = 441): row R starts at float R n and lands at ring index
// (wpos + t n) % H, each of any alignment, and a row may straddle the ring's
// end.  A row is cut into quads that are aligned in the ring: item k covers
// the row's samples j0 .. j0 + 3, j0 = 4 k - lead, lead = (wpos + t n) % 4,
// so ring index (wpos + t n + j0) % H is a multiple of 4 and, H being one
// too, the quad does not straddle the end.  A quad wholly inside the row is
// one float4 store, from one float4 load where the row's place is aligned too
// and from four loads otherwise; the row's head and tail quads go sample by
// sample.
// ---------------------------------------------------------------------------
template <bool A4>
__global__ void __launch_bounds__(kNT) k_den_append(CapAppendArgs a) {
  const int n = a.frame;
  const int items = A4 ? n / 4 : n / 4 + 2;  // quads of a row (the last may lie past it)
  const long long total = (long long)a.n_ticks * a.n_streams * a.n_channels * items;
  for (long long i = (long long)blockIdx.x * kNT + threadIdx.x; i < total; i += (long long)gridDim.x * kNT) {
    const int k = (int)(i % items);
    const long long row = i / items;  // (t * n_streams + s) * n_channels + c
    long long r = row;
    const int c = (int)(r % a.n_channels);
    r /= a.n_channels;
    const int s = (int)(r % a.n_streams), t = (int)(r / a.n_streams);
    const int valid = a.ticks_valid ? a.ticks_valid[s] : a.n_ticks;
    if (t >= valid) continue;
    const float *src = a.den + row * n;
    float *dst = a.hist + ((size_t)s * a.n_channels + c) * a.H;
    const unsigned long long w0 = a.pos[s].wpos + (unsigned long long)t * n;  // ring place of the row's sample 0
    if (A4) {
      *reinterpret_cast<float4 *>(dst + (w0 + 4u * (unsigned)k) % a.H) = reinterpret_cast<const float4 *>(src)[k];
      continue;
    }
    const int j0 = 4 * k - (int)(w0 & 3ull);
    if (j0 >= n) continue;
    if (j0 >= 0 && j0 + 4 <= n) {
      float4 v;
      if ((((unsigned long long)row * (unsigned)n + (unsigned)j0) & 3ull) == 0)
        v = *reinterpret_cast<const float4 *>(src + j0);
      else
        v = make_float4(src[j0], src[j0 + 1], src[j0 + 2], src[j0 + 3]);
      *reinterpret_cast<float4 *>(dst + (w0 + (unsigned)j0) % a.H) = v;
    } else {
      for (int j = j0 < 0 ? 0 : j0; j < j0 + 4 && j < n; j++) dst[(w0 + (unsigned)j) % a.H] = src[j];
    }
  }
}

__global__ void __launch_bounds__(kNT) k_hist_advance(CapAppendArgs a) {
  const int s = blockIdx.x * kNT + threadIdx.x;
  if (s >= a.n_streams) return;
  const int valid = a.ticks_valid ? a.ticks_valid[s] : a.n_ticks;
  CapPos p = a.pos[s];
  p.pos += (unsigned long long)valid * a.frame;
  p.wpos += (unsigned long long)valid * a.frame;
  a.pos[s] = p;
  a.snap[s] = p;
}

hipError_t launch_hist_append(const CapAppendArgs &a, hipStream_t stream) {
  (void)hipGetLastError();
  if (a.den) {  // a capture of the denoised rows
    const bool a4 = a.frame % 4 == 0;
    const long long total = (long long)a.n_ticks * a.n_streams * a.n_channels * (a4 ? a.frame / 4 : a.frame / 4 + 2);
    const int grid = (int)std::min<long long>((total + kNT - 1) / kNT, 4096);
    if (grid > 0) {
      if (a4)
        FVAD_KERNEL_TRY(k_den_append<true>, dim3(grid), dim3(kNT), 0, stream, a);
      else
        FVAD_KERNEL_TRY(k_den_append<false>, dim3(grid), dim3(kNT), 0, stream, a);
    }
    FVAD_KERNEL_TRY(k_hist_advance, dim3((a.n_streams + kNT - 1) / kNT), dim3(kNT), 0, stream, a);
    return hipSuccess;
  }
  const long long total = (long long)a.n_ticks * a.n_streams * a.n_channels * kRowQuads;
  const int grid = (int)std::min<long long>((total + kNT - 1) / kNT, 4096);
  if (grid > 0) {
    if (a.pcm16)
      FVAD_KERNEL_TRY(k_hist_append<true>, dim3(grid), dim3(kNT), 0, stream, a);
    else
      FVAD_KERNEL_TRY(k_hist_append<false>, dim3(grid), dim3(kNT), 0, stream, a);
  }
  FVAD_KERNEL_TRY(k_hist_advance, dim3((a.n_streams + kNT - 1) / kNT), dim3(kNT), 0, stream, a);
  return hipSuccess;
}

// ---------------------------------------------------------------------------
// k_cap_plan: one workgroup, a thread per stream in chunks of kNT.  A stream's
// new SEGMENT records of the chosen machine join its pending queue; the due
// ones leave it, cut to what the ring holds.  An exclusive scan over the
// streams' due counts and lengths (in LDS, chunks chained by carried bases)
// gives every due clip its place in the pass's list -- stream order, then seq
// -- and its pool offset, without atomics.  Room is taken against the host's
// read cursors as they were when the pass was enqueued: the descriptors that
// fit are a prefix of the list, and so are the clips whose audio fits
// (cap::fits), so unread pool words and descriptors are never overwritten.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kNT) k_cap_plan(CapPassArgs a) {
  __shared__ unsigned s_cnt[kNT];
  __shared__ unsigned long long s_len[kNT];
  __shared__ unsigned long long s_lost, s_pool_adv;
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_lost = 0;
    s_pool_adv = 0;
  }
  const unsigned long long desc_wr0 = a.state->desc_wr, pool_wr0 = a.state->pool_wr;
  const unsigned long long desc_room = cap::ring_room(desc_wr0, a.host_desc_read, a.desc_cap);
  const unsigned long long pool_room = cap::ring_room(pool_wr0, a.host_pool_read, a.pool_cap);
  unsigned long long base_cnt = 0, base_len = 0;
  __syncthreads();
  for (int s0 = 0; s0 < a.n_streams; s0 += kNT) {
    const int s = s0 + tid;
    const bool on = s < a.n_streams;
    cap::Pend due[cap::kQueue];  // (indexed by queue place under full unrolling: registers)
    cap::Cut cut[cap::kQueue];
    unsigned due_mask = 0, nd = 0;
    unsigned long long lost = 0, len = 0;
    CapPos P{};
    if (on) {
      cap::Pend *q = a.pend + (size_t)s * cap::kQueue;
      unsigned qn = a.pend_n[s];
      if (qn > (unsigned)cap::kQueue) qn = cap::kQueue;
      if (a.flush_mode == 0) {
        const size_t lane = (size_t)s * a.n_machines + a.machine;
        const unsigned c = min(a.count[lane], (unsigned)a.ev_cap);
        for (unsigned j = 0; j < c; j++) {
          const VadmEvRec r = a.stage[lane * a.ev_cap + j];
          if (r.kind != (unsigned)kVeSegment) continue;
          cap::Pend p;
          p.from = r.sample_from;
          p.to = r.sample_to;
          p.seq = r.seq;
          p.pad = 0;
          if (!cap::queue_push(q, &qn, p)) lost++;
        }
      }
      P = a.pos[s];
      const bool flush = a.flush_mode == 2 || (a.flush_mode == 1 && a.flush[s]);
      unsigned keep = 0;
#pragma unroll
      for (int i = 0; i < cap::kQueue; i++) {
        if ((unsigned)i >= qn) continue;
        due[i] = q[i];
        // the queue keeps the segment's own 48 kHz bounds (the descriptor's);
        // due and cut see them in samples of the clip rate, as pos and base are
        const unsigned long long from = cap::to_rate(due[i].from, a.L, a.M), to = cap::to_rate(due[i].to, a.L, a.M);
        if (cap::due(to, P.pos, flush)) {
          cut[i] = cap::cut(from, to, P.pos, P.base, a.history);
          len += cut[i].n;
          due_mask |= 1u << i;
          nd++;
        } else {
          q[keep++] = due[i];
        }
      }
      a.pend_n[s] = keep;
    }
    // inclusive scans of the chunk's counts and lengths
    s_cnt[tid] = nd;
    s_len[tid] = len;
    __syncthreads();
    for (int d = 1; d < kNT; d <<= 1) {
      const unsigned c = tid >= d ? s_cnt[tid - d] : 0u;
      const unsigned long long l = tid >= d ? s_len[tid - d] : 0ull;
      __syncthreads();
      s_cnt[tid] += c;
      s_len[tid] += l;
      __syncthreads();
    }
    unsigned long long idx = base_cnt + (s_cnt[tid] - nd);
    unsigned long long before = base_len + (s_len[tid] - len);
    unsigned long long pool_end = 0;
#pragma unroll
    for (int k = 0; k < cap::kQueue; k++) {
      if (!(due_mask >> k & 1u)) continue;
      cap::Cut c = cut[k];
      const unsigned long long want = c.n, at = idx++;
      if (at >= desc_room) {  // no descriptor: the clip is lost whole
        lost++;
        before += want;
        continue;
      }
      if (c.n > 0 && !cap::fits(before, c.n, pool_room)) {
        c.n = 0;
        c.flags |= cap::kNoAudio;
      }
      if (c.n == 0) lost++;
      CapWork w;
      w.stream = s;
      w.seq = due[k].seq;
      w.channel = -1;
      w.flags = c.flags;
      w.from = due[k].from;
      w.to = due[k].to;
      w.first = c.first;
      w.n = c.n;
      w.widx = c.n ? (P.wpos - (P.pos - c.first)) % a.H : 0ull;
      w.pool_off = pool_wr0 + before;
      a.work[at] = w;
      if (c.n) pool_end = before + c.n;
      before += want;
    }
    if (lost) atomicAdd(&s_lost, lost);
    if (pool_end) atomicMax(&s_pool_adv, pool_end);
    base_cnt += s_cnt[kNT - 1];
    base_len += s_len[kNT - 1];
    __syncthreads();  // the scan arrays are rewritten by the next chunk
  }
  if (tid == 0) {
    const unsigned long long n_work = base_cnt < desc_room ? base_cnt : desc_room;
    CapState st = *a.state;
    st.desc_wr0 = desc_wr0;
    st.n_work = (unsigned)n_work;
    st.desc_wr = desc_wr0 + n_work;
    st.pool_wr = pool_wr0 + s_pool_adv;
    st.lost += s_lost;
    *a.state = st;
  }
}

// ---------------------------------------------------------------------------
// k_cap_channel: Recorder.findBestChannel (Recorder.zig:95-110) over exactly
// the delivered samples of each work-list entry; a workgroup per entry on a
// fixed grid.  Waves 1..3 square a block of samples of every channel into
// LDS, the first n_channels lanes of wave 0 add the previous block's products
// in index order, one f32 chain per channel ("Numerics": the
// sum is fvad_recording_channel's, term for term).  Then sqrt(sum / (float)n),
// strict < from 9999 in channel order.
// ---------------------------------------------------------------------------
namespace {
constexpr int kChBlk = 512;           // samples of a channel per block
constexpr int kChPitch = kChBlk + 4;  // (the channels' rows start in different banks)
constexpr int kChGrid = 256;
}  // namespace

__global__ void __launch_bounds__(kNT) k_cap_channel(CapPassArgs a) {
  __shared__ __attribute__((aligned(16))) float sq[2][kMaxCh * kChPitch];
  __shared__ float vol[kMaxCh];
  const int tid = threadIdx.x, C = a.n_channels;
  const unsigned n_work = a.state->n_work;
  for (unsigned wi = blockIdx.x; wi < n_work; wi += gridDim.x) {
    const CapWork w = a.work[wi];
    if (w.n == 0) continue;
    const float *rows = a.hist + (size_t)w.stream * C * a.H;
    const unsigned long long nblk = (w.n + kChBlk - 1) / kChBlk;
    // block b of every channel into sq[b & 1], by the threads of waves 1..3
    auto fill = [&](unsigned long long b) {
      const unsigned long long off = b * kChBlk;
      const int m = (int)min((unsigned long long)kChBlk, w.n - off);
      float *dst = sq[b & 1];
      for (int i = tid - 64; i < m * C; i += kNT - 64) {
        const int c = i / m, k = i - c * m;
        unsigned long long idx = w.widx + off + k;  // < 2H: widx < H and off + k < n <= history < H
        if (idx >= a.H) idx -= a.H;
        const float x = rows[(size_t)c * a.H + idx];
        dst[c * kChPitch + k] = x * x;
      }
    };
    if (tid >= 64) fill(0);
    __syncthreads();
    float sum = 0.0f;
    for (unsigned long long b = 0; b < nblk; b++) {
      if (tid >= 64) {
        if (b + 1 < nblk) fill(b + 1);
      } else if (tid < C) {
        const int m = (int)min((unsigned long long)kChBlk, w.n - b * kChBlk);
        const float *p = sq[b & 1] + tid * kChPitch;
        int i = 0;
        for (; i + 4 <= m; i += 4) {
          const float4 v = *reinterpret_cast<const float4 *>(p + i);
          sum += v.x;
          sum += v.y;
          sum += v.z;
          sum += v.w;
        }
        for (; i < m; i++) sum += p[i];
      }
      __syncthreads();
    }
    if (tid < C) vol[tid] = sqrtf(sum / (float)w.n);
    __syncthreads();
    if (tid == 0) {
      int best = 0;
      float best_vol = 9999.0f;
      for (int c = 0; c < C; c++)
        if (vol[c] < best_vol) {
          best = c;
          best_vol = vol[c];
        }
      a.work[wi].channel = best;
    }
    __syncthreads();  // vol is rewritten by the next entry
  }
}

// ---------------------------------------------------------------------------
// k_cap_copy: the chosen channel's samples from the ring to the pinned pool,
// grid-stride over (entry, block of samples)
// ---------------------------------------------------------------------------
namespace {
constexpr int kCopyGridX = 32, kCopyGridY = 16;
}
__global__ void __launch_bounds__(kNT) k_cap_copy(CapPassArgs a) {
  const unsigned n_work = a.state->n_work;
  for (unsigned wi = blockIdx.y; wi < n_work; wi += gridDim.y) {
    const CapWork w = a.work[wi];
    if (w.n == 0 || w.channel < 0 || w.channel >= a.n_channels) continue;
    const float *row = a.hist + ((size_t)w.stream * a.n_channels + w.channel) * a.H;
    const unsigned long long p0 = w.pool_off % a.pool_cap;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kNT + threadIdx.x; i < w.n;
         i += (unsigned long long)gridDim.x * kNT) {
      unsigned long long src = w.widx + i, dst = p0 + i;  // < 2H, < 2 pool_cap (n <= pool_cap: cap::fits)
      if (src >= a.H) src -= a.H;
      if (dst >= a.pool_cap) dst -= a.pool_cap;
      a.pool[dst] = row[src];
    }
  }
}

// k_cap_copy_short: the same into the int16_t pool of an s16 capture, converted
// on the way (cap::to_s16), two samples to a store.  Pair p of a clip holds
// its samples 2 p - odd and 2 p - odd + 1, odd = the clip's first pool index
// & 1, so a pair's first pool index is even until the pool wraps; a pair goes
// out as one 32-bit store where both samples are the clip's, the place is
// even and the pair does not straddle the pool's end, sample by sample
// otherwise (a clip's first and last sample, the pair at the wrap, and the
// pairs behind the wrap of a pool of odd length).
__global__ void __launch_bounds__(kNT) k_cap_copy_short(CapPassArgs a) {
  const unsigned n_work = a.state->n_work;
  for (unsigned wi = blockIdx.y; wi < n_work; wi += gridDim.y) {
    const CapWork w = a.work[wi];
    if (w.n == 0 || w.channel < 0 || w.channel >= a.n_channels) continue;
    const float *row = a.hist + ((size_t)w.stream * a.n_channels + w.channel) * a.H;
    const unsigned long long p0 = w.pool_off % a.pool_cap, odd = p0 & 1ull;
    const unsigned long long pairs = (w.n + odd + 1) / 2;
    auto sample = [&](unsigned long long i) {  // the clip's sample i < n (widx + i < 2H)
      unsigned long long src = w.widx + i;
      if (src >= a.H) src -= a.H;
      return cap::to_s16(row[src]);
    };
    for (unsigned long long p = (unsigned long long)blockIdx.x * kNT + threadIdx.x; p < pairs;
         p += (unsigned long long)gridDim.x * kNT) {
      const unsigned long long hi = 2 * p + 1 - odd;  // the pair's second sample; its first is hi - 1
      const bool has_lo = hi >= 1, has_hi = hi < w.n;
      unsigned long long dst = p0 + (has_lo ? hi - 1 : 0ull);  // < 2 pool_cap (n <= pool_cap: cap::fits)
      if (dst >= a.pool_cap) dst -= a.pool_cap;
      if (has_lo && has_hi && !(dst & 1ull) && dst + 1 < a.pool_cap) {
        const unsigned lo16 = (unsigned short)sample(hi - 1), hi16 = (unsigned short)sample(hi);
        *reinterpret_cast<unsigned *>(a.pool16 + dst) = lo16 | hi16 << 16;
      } else {
        if (has_lo) a.pool16[dst] = sample(hi - 1);
        if (has_hi) {
          unsigned long long d1 = p0 + hi;
          if (d1 >= a.pool_cap) d1 -= a.pool_cap;
          a.pool16[d1] = sample(hi);
        }
      }
    }
  }
}

// k_cap_publish: the pass's descriptors and its header to pinned memory
__global__ void __launch_bounds__(kNT) k_cap_publish(CapPassArgs a) {
  const CapState st = *a.state;
  for (unsigned i = threadIdx.x; i < st.n_work; i += kNT) {
    const CapWork w = a.work[i];
    CapClip d;
    d.stream = w.stream;
    d.seq = w.seq;
    d.channel = w.n ? w.channel : -1;
    d.flags = w.flags;
    d.push = a.push;
    d.sample_from = w.from;
    d.sample_to = w.to;
    d.first_sample = w.first;
    d.n_samples = w.n;
    d.reserved = a.reserved;
    a.desc[(st.desc_wr0 + i) % a.desc_cap] = d;
  }
  if (threadIdx.x == 0) {
    CapHeader h;
    h.pass = a.pass;
    h.desc_end = st.desc_wr;
    h.pool_end = st.pool_wr;
    h.lost = st.lost;
    *a.header = h;
  }
}

hipError_t launch_capture_pass(const CapPassArgs &a, hipStream_t stream) {
  (void)hipGetLastError();
  FVAD_KERNEL_TRY(k_cap_plan, dim3(1), dim3(kNT), 0, stream, a);
  FVAD_KERNEL_TRY(k_cap_channel, dim3(kChGrid), dim3(kNT), 0, stream, a);
  if (a.pool16)
    FVAD_KERNEL_TRY(k_cap_copy_short, dim3(kCopyGridX, kCopyGridY), dim3(kNT), 0, stream, a);
  else
    FVAD_KERNEL_TRY(k_cap_copy, dim3(kCopyGridX, kCopyGridY), dim3(kNT), 0, stream, a);
  FVAD_KERNEL_TRY(k_cap_publish, dim3(1), dim3(kNT), 0, stream, a);
  return hipSuccess;
}

// ---------------------------------------------------------------------------
// reset_streams / restore_streams: the listed streams' position and base (on
// the appending stream; wpos stays), and their pending clips dropped (on the
// side stream, behind the passes already queued)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kNT) k_cap_set_pos(CapSetArgs a) {
  const int i = threadIdx.x;
  if (i >= a.ids.n) return;
  CapPos *p = a.pos + a.ids.id[i];
  p->pos = a.value[i];
  p->base = a.value[i];
}
__global__ void __launch_bounds__(kNT) k_cap_drop(CapSetArgs a) {
  const int i = threadIdx.x;
  if (i < a.ids.n) a.pend_n[a.ids.id[i]] = 0;
}

hipError_t launch_capture_set_pos(const CapSetArgs &a, hipStream_t stream) {
  (void)hipGetLastError();
  static_assert(kListMax <= kNT, "one thread per listed stream");
  FVAD_KERNEL_TRY(k_cap_set_pos, dim3(1), dim3(kNT), 0, stream, a);
  return hipSuccess;
}
hipError_t launch_capture_drop(const CapSetArgs &a, hipStream_t stream) {
  (void)hipGetLastError();
  FVAD_KERNEL_TRY(k_cap_drop, dim3(1), dim3(kNT), 0, stream, a);
  return hipSuccess;
}

}  // namespace fvad
