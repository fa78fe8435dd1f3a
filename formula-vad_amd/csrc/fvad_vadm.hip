// The device VADMachine over a push's window outputs (the engine's side
// stream): k_vadm_hbm in steady state, k_vadm_par at sync points (k_vadm_hbm_ps
// and k_vadm_par_ps where every stream has its own config), and
// k_vadm_events, which packs the speech events a pass staged.  At the end,
// for its code's sake, the pitch front's k_select (see there).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "fvad_device.h"
#include "fvad_exact.h"
#include "fvad_internal.h"
#include "fvad_launch.h"
#include "fvad_staged.h"
#include "fvad_staged_dev.h"
#include "fvad_vadm_dev.h"

namespace fvad {

// ---------------------------------------------------------------------------
// k_vadm: VADMachine.run (VADMachine.zig:126-230) for every completed FFT-B
// window of the push, one lane per stream, every attached machine.  The
// machine's per-window code is fvad_vadm_dev.h's (shared with the config
// sweep, fvad_sweep.hip); here is where a push's windows come from.
// ---------------------------------------------------------------------------
// Where a machine's constants come from.  The uniform kernels (k_vadm_hbm,
// k_vadm_par: engines attached with fvad_engine_attach_vadm) read machine m's
// from the argument block; the per-stream kernels (k_vadm_hbm_ps,
// k_vadm_par_ps: fvad_engine_attach_vadm_ex) read row [m][stream] of the
// device table, once per machine.  The buffer offsets and lt_pitch are always
// the machine's, a.vadm.c[m]: the layout does not depend on the rows.
// kHbmBlock: k_vadm_hbm*'s long-term read-ahead (lt_range's block).  A lane
// of k_vadm_hbm_ps holds its constants in VGPRs where k_vadm_hbm's are SGPRs;
// with half the read-ahead (16 VGPRs less) it keeps k_vadm_hbm's 3 waves per
// SIMD without scratch, and between sync points the folds it serves are rare
// (the lazy walk, fvad_vadm_dev.h).
template <bool kPS>
struct VadmK {
  using type = VadmConst;
  static constexpr int kHbmBlock = FVAD_LT_BLOCK;
  static __device__ __forceinline__ const VadmConst &of(const StagedArgs &a, int m, int) { return a.vadm.c[m]; }
};
template <>
struct VadmK<true> {
  using type = VadmRow;
  static constexpr int kHbmBlock = FVAD_LT_BLOCK / 2;
  // five 16-byte loads (the rows are 16-byte aligned)
  static __device__ __forceinline__ VadmRow of(const StagedArgs &a, int m, int s) {
    return a.vadm.tab[(size_t)m * a.n_streams + s];
  }
};

// One machine over all completed windows of the push for one stream (the
// serial walk, vadm_walk); K its constants, `lt` points at entry 0 of the
// stream's long-term buffer, `lts` is its stride.
template <int kL = FVAD_LT_BLOCK, class KT>
__device__ void vadm_stream(const StagedArgs &a, int m, int s, const KT &K, float *lt, size_t lts, bool final) {
  const int B = a.n_streams, C = a.n_channels, nb = a.n_bands;
  const int nt = ticks_of(a, s);
  VadmState S = a.vadm.st[(size_t)m * B + s];
  float *st = a.vadm.buf + a.vadm.c[m].st_off + s, *rb = a.vadm.buf + a.vadm.c[m].r_off + s;
  VadmSeg *seg = a.vadm.seg + ((size_t)m * B + s) * a.vadm.seg_cap;
  const VadmEvLane ev = vadm_ev_lane(a.vadm, m, s);
  vadm_walk<kL>(S, K, st, rb, B, lt, lts, seg, a.vadm.seg_cap, ev, (unsigned long long)a.plan->nfft_b,
            a.vadm.bound_scale, a.vadm.defer_max, a.vadm.count, final, [&](auto &&window) {
              // every window of the push in order: ticks, then a tick's slots
              // (several when fft_size < 480)
              for (int t = 0; t < nt; t++)
                for (int w = 0, nw = a.out_win_flag[(size_t)t * B + s]; w < nw; w++) {
                  const size_t o = ((size_t)t * B + s) * a.wpt + w;
                  float min_v = 999, max_v = 0;
                  for (int c = 0; c < C; c++) {
                    const float v = a.out_band[(o * C + c) * nb + K.slot];
                    if (v < min_v) min_v = v;
                    if (v > max_v) max_v = v;
                  }
                  if ((long long)S.windows_done == a.vadm.negate_at) min_v = -min_v;  // test hook
                  // fft_input.vad orelse 0 (VADMachine.zig:240-246): no vad without the denoiser
                  window(min_v, a.use_denoiser ? a.out_win_vad[o] : 0.0f, a.out_win_ratio[o]);
                }
            });
  a.vadm.st[(size_t)m * B + s] = S;
}

// ---------------------------------------------------------------------------
// k_vadm_par: the same machine with the long-term averages of a push's
// windows computed side by side.  Once the long-term buffer is full (from
// the start with an initial average) a push at write index w averages
//   acc = P_w + v * s, then acc += e_i * s for i = w + 1 .. n - 1 (C order),
// P_w the cached prefix, a chain of one add per push; the suffix entries are
// the old buffer's, or values pushed earlier in this push (a wrap).  So given
// which windows push, the ~12 averages of a push are independent serial
// chains.  Whether a window pushes (`met` false) depends on the average of the
// last push, so 16 lanes per stream fold the hypothesis "the next 16 windows
// all push" in one round; the stream's leader lane then replays the windows
// in order with the exact averages -- each `met` decided exactly as the
// serial walk does -- and commits every push up to the first window that
// does not push (speech); the next round starts after it.  A round costs one
// suffix chain instead of one per window; windows with no push cost none.
// Bit-identical to vadm_stream (same adds, same order); streams whose buffer
// is not full yet (no initial average) or with more than kVpMaxW windows in
// the push take the serial walk.
// ---------------------------------------------------------------------------
// (48 windows: 4.2 KB of LDS, which fits beside three k_fftAw or four
// k_pcorr workgroups on a CU; the machine state lives in LDS, not in VGPRs)
#ifndef FVAD_VP_BLOCK
#define FVAD_VP_BLOCK 8  // long-term entries per prefetched block
#endif
constexpr int kVpG = 16, kVpS = 4, kVpMaxW = 48;  // lanes per stream, streams per workgroup, windows per push
// acc += e_i * s over old entries [i0, i1): pushed f32 below nw, the initial
// average above (entry i of the stream at lt[i * lts])
__device__ __forceinline__ double lt_fold(double acc, const float *lt, size_t lts, unsigned i0, unsigned i1, unsigned nw,
                                          double init, double scalar) {
  if (i0 >= i1) return acc;
  return lt_range<FVAD_VP_BLOCK>(acc, lt, lts, i0, i1, nw, init, scalar);
}
// (kPS: the four streams' table rows sit in LDS beside their states, Ks[],
// read by the group's lanes where the uniform kernel reads the argument block)
template <bool kPS>
__device__ __forceinline__ void vadm_par_groups(const StagedArgs &a) {
  using KT = typename VadmK<kPS>::type;
  __shared__ float wmin[kVpS][kVpMaxW], wvad[kVpS][kVpMaxW], wvr[kVpS][kVpMaxW];
  __shared__ float pv[kVpS][kVpMaxW];  // values pushed in this push, in push order (committed + the round's hypotheses)
  __shared__ double favg[kVpS][kVpG];
  __shared__ double rpre[kVpS];  // the cached prefix before the round's first push
  __shared__ int rnd[kVpS][4];  // round: first window, pushes committed so far, state (0 run, 1 done, 2 serial)
  __shared__ VadmState Ss[kVpS];
  __shared__ VadmRow Ks[kVpS];  // (kPS only: the uniform kernel never names it, so it has none)
  const int B = a.n_streams, C = a.n_channels, nb = a.n_bands;
  const int g = threadIdx.x / kVpG, r = threadIdx.x % kVpG;
  const int s = blockIdx.x * kVpS + g;
  const bool sok = s < B && ticks_of(a, s) > 0;
  const int nt = sok ? ticks_of(a, s) : 0;
  const unsigned long long fft = (unsigned long long)a.plan->nfft_b;
  const int self = threadIdx.x;
  for (int m = 0; m < a.vadm.n; m++) {
    const VadmConst &M = a.vadm.c[m];  // the layout
    if constexpr (kPS) {
      // the group's row, one 16-byte word per lane (Ks is free: the previous
      // machine's last reads are behind the wave_sync that ends its turn)
      static_assert(sizeof(VadmRow) / 16 <= kVpG, "one lane per word of the row");
      if (r < (int)(sizeof(VadmRow) / 16))
        reinterpret_cast<uint4 *>(&Ks[g])[r] =
            reinterpret_cast<const uint4 *>(a.vadm.tab + (size_t)m * B + (s < B ? s : 0))[r];
      wave_sync();
    }
    const KT &K = [&]() -> const KT & {
      if constexpr (kPS)
        return Ks[g];
      else
        return a.vadm.c[m];
    }();
    float *lt = a.vadm.buf + M.lt_off + (size_t)(sok ? s : 0) * M.lt_pitch;  // the stream's row
    const size_t lts = 1;
    // the push's windows in order -> LDS (16 ticks at a time, positions by a
    // prefix count over the group's lanes)
    int Kw = 0;
    for (int t0 = 0; t0 < nt; t0 += kVpG) {
      const int t = t0 + r;
      const int nwt = t < nt ? a.out_win_flag[(size_t)t * B + s] : 0;
      int pos = nwt;
#pragma unroll
      for (int d = 1; d < kVpG; d <<= 1) {
        const int up = __shfl(pos, self - d);
        if (r >= d) pos += up;
      }
      const int tot = __shfl(pos, g * kVpG + kVpG - 1);
      for (int w = 0; w < nwt; w++) {
        const int k = Kw + pos - nwt + w;
        if (k < kVpMaxW) {
          const size_t o = ((size_t)t * B + s) * a.wpt + w;
          float min_v = 999;
          for (int c = 0; c < C; c++) {
            const float v = a.out_band[(o * C + c) * nb + K.slot];
            if (v < min_v) min_v = v;
          }
          wmin[g][k] = min_v;
          wvad[g][k] = a.use_denoiser ? a.out_win_vad[o] : 0.0f;
          wvr[g][k] = a.out_win_ratio[o];
        }
      }
      Kw += tot;
    }
    if (r == 0) {
      Ss[g] = a.vadm.st[(size_t)m * B + (sok ? s : 0)];
      // k_vadm_par runs at sync points only: a fold owed from earlier pushes
      // first (the walk below needs the exact average), also for a stream
      // with no ticks in this push
      if (sok) {
        lt_resolve(Ss[g], K, lt, lts);
      } else if (s < B) {
        VadmState S2 = a.vadm.st[(size_t)m * B + s];
        if (S2.lt_defer) {
          lt_resolve(S2, K, a.vadm.buf + M.lt_off + (size_t)s * M.lt_pitch, 1);
          a.vadm.st[(size_t)m * B + s] = S2;
        }
      }
    }
    wave_sync();
    if (r == 0 && sok && a.vadm.negate_at >= 0) {  // test hook FVAD_DEBUG_VADM_NEGATE_AT
      const long long k = a.vadm.negate_at - (long long)Ss[g].windows_done;
      if (k >= 0 && k < Kw && k < kVpMaxW) wmin[g][k] = -wmin[g][k];
      wave_sync();
    }
    VadmState &S = Ss[g];
    float *st = a.vadm.buf + M.st_off + (sok ? s : 0), *rb = a.vadm.buf + M.r_off + (sok ? s : 0);
    VadmSeg *seg = a.vadm.seg + ((size_t)m * B + (sok ? s : 0)) * a.vadm.seg_cap;
    const VadmEvLane ev = vadm_ev_lane(a.vadm, m, sok ? s : 0);
    // (n > kVpMaxW: a push wraps around the buffer at most once)
    const bool forced = a.vadm.par_serial_every > 0 && s % a.vadm.par_serial_every == 0;
    const bool fast = sok && !forced && Kw <= kVpMaxW && K.n_lt > kVpMaxW && S.lt_count == (unsigned)K.n_lt &&
                      S.lt_pre_ok;
    const unsigned n = (unsigned)K.n_lt, wbase = S.lt_widx, nw0 = S.lt_nw;
    const double scalar = 1.0 / (double)n;  // the full buffer's
    if (r == 0) {
      rnd[g][0] = 0;
      rnd[g][1] = 0;
      rnd[g][2] = !sok ? 1 : (fast ? 0 : 2);
    }
    wave_sync();
    // leader state across rounds (lane 0 of the group)
    int j = 0, npush = 0;
    double pre = S.lt_pre;
    for (;;) {
      if (r == 0 && rnd[g][2] == 0) {
        // windows that do not push need no fold: replay them up to the next
        // one that does (its short-term pushes done, its long push pending)
        while (j < Kw) {
          const unsigned long long index = S.windows_done * fft;
          const bool met = vadm_short(S, K, st, rb, B, wmin[g][j], wvr[g][j]);
          if (!met) break;  // window j pushes: its short-term pushes are done, its long push waits for the folds
          S.windows_done++;
          vadm_fsm(S, K, index, met, wvad[g][j], wvr[g][j], seg, a.vadm.seg_cap, ev);
          j++;
        }
        if (j >= Kw) rnd[g][2] = 1;
        rnd[g][0] = j;
        rnd[g][1] = npush;
        // the round's hypotheses: windows j, j + 1, ... push in order
        for (int q = 0; q < kVpG && j + q < Kw; q++) pv[g][npush + q] = wmin[g][j + q];
        rpre[g] = pre;
      }
      wave_sync();
      const int state = rnd[g][2];
      if (__ballot(state == 0) == 0) break;  // every group of the wave is done with its fast walk
      if (state == 0) {
        // lane r: the push of window j0 + r after the r pushes before it
        const int j0 = rnd[g][0], np = rnd[g][1];
        if (j0 + r < Kw) {
          const unsigned k = (unsigned)(np + r);  // pushes of this push before it
          const unsigned nw = min(n, nw0 + k + 1);
          // its prefix P_w: the chain of one add per push since the cached
          // one; w: its write index
          double P = rpre[g];
          unsigned w = (wbase + (unsigned)np) % n;
#pragma unroll 1
          for (int q = 0; q < r; q++) {
            P = (w + 1 == n) ? 0.0 : P + (double)pv[g][np + q] * scalar;
            w = (w + 1 == n) ? 0u : w + 1;
          }
          double acc = P + (double)pv[g][np + r] * scalar;
          if (wbase + k < n) {
            // no wrap in this push: every entry past w is the old buffer's
            acc = lt_fold(acc, lt, lts, w + 1, n, nw, K.init, scalar);
          } else {
            // wrapped: (w, wbase) old entries (all pushed by now), [wbase, n) pushed in this push
            acc = lt_fold(acc, lt, lts, w + 1, wbase, nw, K.init, scalar);
            for (unsigned i = wbase; i < n; i++) acc += (double)pv[g][i - wbase] * scalar;
          }
          favg[g][r] = acc;
        }
      }
      wave_sync();
      if (r == 0 && state == 0) {
        // replay in order with the exact averages; commit up to the first
        // window that does not push
        const int j0 = j;
        for (int q = 0; q < kVpG && j0 + q < Kw; q++) {
          const int jj = j0 + q;
          const unsigned long long index = S.windows_done * fft;
          bool met = false;
          if (q > 0) met = vadm_short(S, K, st, rb, B, wmin[g][jj], wvr[g][jj]);
          if (!met) {
            // the long push (ra_push_long's state updates, the average folded above)
            const unsigned w = S.lt_widx;
            S.lt_widx = (w + 1) % n;
            if (S.lt_nw < n) S.lt_nw++;
            pre = (w + 1 == n) ? 0.0 : pre + (double)wmin[g][jj] * scalar;
            S.lt_pre = pre;
            S.lt_last = favg[g][q];
            S.lt_has = 1;
            lt_neg_push(S, n, wmin[g][jj]);
            npush++;
          }
          S.windows_done++;
          vadm_fsm(S, K, index, met, wvad[g][jj], wvr[g][jj], seg, a.vadm.seg_cap, ev);
          j = jj + 1;
          if (met) break;
        }
      }
      wave_sync();
    }
    if (r == 0 && sok) {
      if (rnd[g][2] == 2) {
        // a machine outside the window-parallel case (launch_vadm sends
        // engines whose machines can get here to k_vadm_hbm; the test hook
        // par_serial_every forces it): the serial walk on the leader lane,
        // from the untouched state in HBM
        vadm_stream(a, m, s, K, lt, lts, true);
      } else {
        // the push's long-term values into the buffer (read above as the old entries)
        unsigned w = wbase;
#pragma unroll 1
        for (int q = 0; q < npush; q++) {
          lt[(size_t)w * lts] = pv[g][q];
          w = (w + 1 == n) ? 0u : w + 1;
        }
        a.vadm.st[(size_t)m * B + s] = S;
      }
    }
    wave_sync();
  }
}
__global__ void __launch_bounds__(64) k_vadm_par(StagedArgs a) { vadm_par_groups<false>(a); }
__global__ void __launch_bounds__(64) k_vadm_par_ps(StagedArgs a) { vadm_par_groups<true>(a); }

// k_vadm_hbm: the same machine, long-term buffers walked in HBM, no LDS, one
// wave (kVadmHbmLanes = 64 streams) per workgroup: a light kernel that co-runs
// with the next push's pipeline on the engine's side stream.  k_vadm_hbm_ps:
// the same with each lane's constants its stream's own table row.
#ifndef FVAD_VADM_LANES
#define FVAD_VADM_LANES 64
#endif
constexpr int kVadmHbmLanes = FVAD_VADM_LANES;  // streams per workgroup (one wave); 16 / 32 / 64 measured within noise, 64 takes fewest wave slots
template <bool kPS>
__device__ __forceinline__ void vadm_hbm_lanes(const StagedArgs &a) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.n_streams) return;
  const bool final = a.vadm.vfinal != 0;
  constexpr int kL = VadmK<kPS>::kHbmBlock;
  if (ticks_of(a, s) <= 0) {  // no windows; at a sync point its owed fold is still due
    if (final)
      for (int m = 0; m < a.vadm.n; m++) {
        VadmState *p = a.vadm.st + (size_t)m * a.n_streams + s;
        if (p->lt_defer) {
          VadmState S = *p;
          lt_resolve<kL>(S, VadmK<kPS>::of(a, m, s), a.vadm.buf + a.vadm.c[m].lt_off + (size_t)s * a.vadm.c[m].lt_pitch,
                         1);
          *p = S;
        }
      }
    return;
  }
  for (int m = 0; m < a.vadm.n; m++)
    vadm_stream<kL>(a, m, s, VadmK<kPS>::of(a, m, s),
                    a.vadm.buf + a.vadm.c[m].lt_off + (size_t)s * a.vadm.c[m].lt_pitch, 1, final);
}
__global__ void __launch_bounds__(64) k_vadm_hbm(StagedArgs a) { vadm_hbm_lanes<false>(a); }
__global__ void __launch_bounds__(64) k_vadm_hbm_ps(StagedArgs a) { vadm_hbm_lanes<true>(a); }

hipError_t launch_vadm(const StagedArgs &a, hipStream_t stream, bool fast, bool *ran_par) {
  (void)hipGetLastError();
  // k_vadm_par's case: every machine's long-term buffer full from the start
  // (an initial average) and longer than a push's windows, at most kVpMaxW
  // windows per push (wmax bounds them).  With per-stream rows (a.vadm.tab)
  // the caller has looked at the rows: it asks for `fast` only while every row
  // has an initial average, and a stream whose buffer is no longer than a
  // push's windows takes k_vadm_par_ps' in-kernel serial walk.
  bool par = fast && a.wmax <= kVpMaxW;
  if (!a.vadm.tab)
    for (int m = 0; m < a.vadm.n; m++) par = par && a.vadm.c[m].has_init && a.vadm.c[m].n_lt > kVpMaxW;
  if (ran_par) *ran_par = par;
  const dim3 hbm_grid((a.n_streams + kVadmHbmLanes - 1) / kVadmHbmLanes), par_grid((a.n_streams + kVpS - 1) / kVpS);
  if (a.vadm.tab) {
    if (!par)
      FVAD_KERNEL_TRY(k_vadm_hbm_ps, hbm_grid, dim3(kVadmHbmLanes), 0, stream, a);
    else
      FVAD_KERNEL_TRY(k_vadm_par_ps, par_grid, dim3(kVpS * kVpG), 0, stream, a);
    return hipSuccess;
  }
  if (!par)
    FVAD_KERNEL_TRY(k_vadm_hbm, hbm_grid, dim3(kVadmHbmLanes), 0, stream, a);
  else
    FVAD_KERNEL_TRY(k_vadm_par, par_grid, dim3(kVpS * kVpG), 0, stream, a);
  return hipSuccess;
}

// ---------------------------------------------------------------------------
// k_vadm_events: the records a machine pass staged per lane (lane = stream *
// n_machines + machine), packed into the engine's event ring in lane order,
// each lane's in the order the machine produced them.  One workgroup, right
// after the pass on the same stream: an exclusive scan of the lanes' counts
// (a shuffle scan per wave, the waves' totals through LDS, the chunks of
// kEvThreads lanes chained by a carried base) gives every record its place, so
// the order needs no atomics and is the same whichever machine kernel ran.
// Ring overflow: the pass writes the records that fit behind the cursor --
// room = capacity - (cursor - host_read), host_read the host's read cursor when
// the pass was enqueued, never ahead of the true one -- and counts the rest as
// lost; unread events are never overwritten.  The cursor and the lost count
// live in device memory (passes of an engine run in order on its side stream);
// the header tells the host, once the event recorded behind this kernel has
// completed, how far the ring is valid.  Every count is left at 0 for the
// next pass.
// ---------------------------------------------------------------------------
constexpr int kEvThreads = 256;
__global__ void __launch_bounds__(kEvThreads) k_vadm_events(VadmEventArgs a) {
  __shared__ unsigned wsum[kEvThreads / 64];
  const int tid = threadIdx.x, wl = tid & 63, wave = tid >> 6;
  const unsigned long long wr0 = a.cursor[0];
  const unsigned long long used = wr0 - a.host_read;
  const unsigned long long room = used < a.ring_cap ? a.ring_cap - used : 0ull;
  const int chunk = a.chunk > 0 && a.chunk < kEvThreads ? a.chunk : kEvThreads;
  unsigned long long base = 0;  // records of the lanes before this chunk
  for (int l0 = 0; l0 < a.n_lanes; l0 += chunk) {
    const int l = l0 + tid;
    const bool on = tid < chunk && l < a.n_lanes;
    const unsigned c = on ? min(a.count[l], (unsigned)a.ev_cap) : 0u;
    unsigned inc = c;  // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned up = __shfl_up(inc, d);
      if (wl >= d) inc += up;
    }
    if (wl == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kEvThreads / 64; w++) {
      const unsigned v = wsum[w];
      if (w < wave) before += v;
      total += v;
    }
    const unsigned long long first = base + before + (inc - c);
    for (unsigned j = 0; j < c; j++) {
      const unsigned long long pos = first + j;
      if (pos >= room) break;
      const VadmEvRec r = a.stage[(size_t)l * a.ev_cap + j];
      VadmEvent e;
      e.kind = r.kind;
      e.stream = l / a.n_machines;
      e.machine = l % a.n_machines;
      e.seq = r.seq;
      e.push = a.push;
      e.sample_from = r.sample_from;
      e.sample_to = r.sample_to;
      e.debug_rnn_vad = r.debug_rnn_vad;
      e.debug_avg_speech_vol_ratio = r.debug_avg_speech_vol_ratio;
      a.ring[(wr0 + pos) % a.ring_cap] = e;
    }
    if (c) a.count[l] = 0;
    base += total;
    __syncthreads();  // wsum is rewritten by the next chunk
  }
  if (tid == 0) {
    const unsigned long long written = base < room ? base : room;
    const unsigned long long lost = a.cursor[1] + (base - written);
    a.cursor[0] = wr0 + written;
    a.cursor[1] = lost;
    VadmEventHeader h;
    h.pass = a.pass;
    h.end = wr0 + written;
    h.lost = lost;
    h.n = base;
    *a.header = h;
  }
}

hipError_t launch_vadm_events(const VadmEventArgs &a, hipStream_t stream) {
  (void)hipGetLastError();
  FVAD_KERNEL_TRY(k_vadm_events, dim3(1), dim3(kEvThreads), 0, stream, a);
  return hipSuccess;
}

// ===========================================================================
// k_select lives here, not with k_plpc (fvad_plpc.hip), for its code: compiled
// in a translation unit without the VADMachine kernels it gets another
// register assignment and 6 more instructions (same 126 VGPRs and occupancy);
// beside them it is, instruction for instruction, the kernel the pipeline's
// timings were taken with.  Nothing else ties it to
// this file.
// ===========================================================================
// ---------------------------------------------------------------------------
// k_select: remove_doubling's sequential selection.  The frames of a stream
// stay sequential (prev_period / prev_gain), but a frame's 14 candidate tests
// are independent given them: 16 lanes per stream (4 streams per wave), lane
// k tests candidate k (T1 of k + 2), a ballot finds the last passing one (the
// reference loop keeps overwriting, so the highest k wins) and its values are
// read from its lane.  Every comparison and value is the reference's.  A
// frame's record loads kSelRing - 1 frames ahead through a register ring.
// ---------------------------------------------------------------------------
constexpr int kSelStreams = 4;  // streams per 64-thread workgroup
#ifndef FVAD_SEL_RING
#define FVAD_SEL_RING 8
#endif
constexpr int kSelRing = FVAD_SEL_RING;  // frames of records in flight
struct SelRec {
  int T0, nv, Tk, offk, off0;
  float g0, xy0, yy0, gk, xyk, yyk;
};
__device__ __forceinline__ void sel_load(SelRec &r, const float *__restrict__ row, int k, bool on) {
  if (!on) return;
  r.T0 = __float_as_int(row[rec::kT0]);
  r.nv = __float_as_int(row[rec::kNValid]);
  r.g0 = row[rec::kG0];
  r.xy0 = row[rec::kXy0];
  r.yy0 = row[rec::kYy0];
  r.off0 = __float_as_int(row[rec::kOff0]);
  const float *q = row + rec::kK + min(k, 13) * rec::kKStride;
  r.Tk = __float_as_int(q[0]);
  r.gk = q[1];
  r.xyk = q[2];
  r.yyk = q[3];
  r.offk = __float_as_int(q[4]);
}

__global__ void __launch_bounds__(64) k_select(StagedArgs a) {
  const int lane = threadIdx.x, sl = lane >> 4, k = lane & 15;
  // the persistent kernels' group counters: those of this push's k_fftAw /
  // k_plpc / k_pcorr are done with (they ran before), the rest are used after
  // this kernel; zeroed here instead of by a memset node of their own
  static_assert(kWorkSlots * kQueues <= 64, "one lane per counter");
  if (blockIdx.x == 0 && lane < kWorkSlots * kQueues) a.work[lane] = 0;
  const int s = blockIdx.x * kSelStreams + sl;
  const bool sok = s < a.n_streams;
  const int nf = sok ? ticks_of(a, s) * a.n_channels : 0;
  int nfw = nf;  // frames of the wave's longest stream (shuffles need every lane)
#pragma unroll
  for (int d = 16; d < 64; d <<= 1) nfw = max(nfw, __shfl_xor(nfw, d));
  if (nfw <= 0) return;
  float *stp = a.state + (size_t)(sok ? s : 0) * st::kWords;
  int *istp = reinterpret_cast<int *>(stp);
  int last_period = sok ? istp[st::kLastPeriod] : 0;
  float last_gain = sok ? stp[st::kLastGain] : 0.0f;
  const float *rows = a.rec + (size_t)(sok ? s : 0) * a.V * rec::kSize;
  const int K = k + 2;  // remove_doubling's k for this lane's candidate
  auto step = [&](const SelRec &r, int v) {
    const bool on = v < nf;
    const int prev_period = last_period / 2;
    const float prev_gain = last_gain;
    bool pass = false;
    if (on && k < 14 && k < r.nv) {
      const int T1 = r.Tk;
      float cont;
      if (abs(T1 - prev_period) <= 1)
        cont = prev_gain;
      else if (abs(T1 - prev_period) <= 2 && 5 * K * K < r.T0)
        cont = .5f * prev_gain;
      else
        cont = 0;
      float thresh;
      {
        const float vv = .7f * r.g0 - cont;
        thresh = (.3f > vv) ? .3f : vv;
      }
      if (T1 < 3 * 30) {
        const float vv = .85f * r.g0 - cont;
        thresh = (.4f > vv) ? .4f : vv;
      } else if (T1 < 2 * 30) {
        const float vv = .9f * r.g0 - cont;
        thresh = (.5f > vv) ? .5f : vv;
      }
      pass = r.gk > thresh;
    }
    const unsigned seg = (unsigned)(__ballot(pass) >> (16 * sl)) & 0x3fffu;
    const int win = seg ? 31 - __clz(seg) : 0;
    const int src = 16 * sl + win;
    const float wxy = __shfl(r.xyk, src), wyy = __shfl(r.yyk, src), wg = __shfl(r.gk, src);
    const int wT = __shfl(r.Tk, src), woff = __shfl(r.offk, src);
    float best_xy = seg ? wxy : r.xy0, best_yy = seg ? wyy : r.yy0, gg = seg ? wg : r.g0;
    const int T = seg ? wT : r.T0, offset = seg ? woff : r.off0;
    if (!on) return;
    best_xy = (0 > best_xy) ? 0 : best_xy;
    float pg;
    if (best_yy <= best_xy)
      pg = 1.0f;
    else
      pg = best_xy / (best_yy + 1);
    if (pg > gg) pg = gg;
    int pi = 2 * T + offset;
    if (pi < kPitchMin) pi = kPitchMin;
    if (k == 0) a.pitch[(size_t)s * a.V + v] = pi;
    last_period = pi;
    last_gain = pg;
  };
  // records kSelRing frames ahead through a register ring (static slots: the
  // loop over a ring turn is unrolled)
  SelRec r[kSelRing];
#pragma unroll
  for (int u = 0; u < kSelRing - 1; u++) {
    r[u] = SelRec{};
    sel_load(r[u], rows + (size_t)u * rec::kSize, k, u < nf);
  }
  r[kSelRing - 1] = SelRec{};
  for (int v = 0; v < nfw; v += kSelRing) {
#pragma unroll
    for (int u = 0; u < kSelRing; u++) {
      if (v + u >= nfw) break;
      // slot (u - 1) mod R was consumed last step: frame v + u + R - 1 goes there
      const int ls = (u + kSelRing - 1) % kSelRing;
      sel_load(r[ls], rows + (size_t)(v + u + kSelRing - 1) * rec::kSize, k, v + u + kSelRing - 1 < nf);
      step(r[u], v + u);
    }
  }
  if (sok && nf > 0 && k == 0) {
    istp[st::kLastPeriod] = last_period;
    stp[st::kLastGain] = last_gain;
  }
}

hipError_t launch_select(const StagedArgs &a, hipStream_t stream) {
  FVAD_KERNEL_TRY(k_select, dim3((a.n_streams + kSelStreams - 1) / kSelStreams), dim3(64), 0, stream, a);
  return hipSuccess;
}

}  // namespace fvad
