// The device VADMachine's per-window code, shared by the engine's machine
// kernels (fvad_vadm.hip: k_vadm_hbm, k_vadm_par and their _ps forms) and the config sweep
// (fvad_sweep.hip: k_vadm_sweep), so every kernel runs the same expressions in
// the same order: the rolling averages, the long-term folds, the speech-state
// machine, and the serial walk over a run of windows (vadm_walk), which takes
// a window's (min_v, vad, vr) from a source its caller supplies.
#pragma once
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "fvad_exact.h"
#include "fvad_internal.h"
#include "fvad_staged.h"

namespace fvad {

// ---------------------------------------------------------------------------
// VADMachine.run (VADMachine.zig:126-230), one lane per machine.
// RollingAverage.avg (RollingAverage.zig:34-56) recomputes the mean over the
// whole buffer in array order on every push, in f64 - reproduced as is (an
// incremental mean would round differently).  Short buffers are stored
// [i][lane] (stride B) so the lanes of a wave read one contiguous line per term.
// ---------------------------------------------------------------------------
// Short rolling averages: the plain recompute.
__device__ __forceinline__ double ra_push(float *buf, int B, int n, unsigned &widx, unsigned &count, double &last,
                                          int &has, float sample) {
  buf[(size_t)widx * B] = sample;  // stored as f32: (double)f32 is exact
  widx = (widx + 1) % (unsigned)n;
  if (count < (unsigned)n) count++;
  double acc = 0.0;
  const double scalar = 1.0 / (double)count;
  for (unsigned i = 0; i < count; i++) acc += (double)buf[(size_t)i * B] * scalar;
  last = acc;
  has = 1;
  return acc;
}

// The long-term average (4218 entries by default).  Same operation sequence as
// the full recompute, two savings that keep it bit-identical:
//  * once the buffer is full the scalar 1/n no longer changes, so the running
//    sum over the entries before the write position is exactly what the
//    previous pass had accumulated there (those entries have not changed) -
//    the pass starts from that cached prefix;
//  * entries are read 32 ahead of the f64 add chain (register double buffer),
//    so the chain does not wait on memory per term.
// acc += entry[i] * scalar for i in [i0, i1), C order; entries are pushed f32
// values (read 8 ahead of the add chain) or, for never-written entries, the
// initial average (a double).
#ifndef FVAD_LT_BLOCK
#define FVAD_LT_BLOCK 16
#endif
template <int kL = FVAD_LT_BLOCK>
__device__ __forceinline__ double lt_sum(double acc, const float *buf, size_t bs, unsigned i0, unsigned i1,
                                         double scalar) {
  // blocks of kL entries, the next block's loads issued before this block's
  // adds (two blocks in flight: the chain waits a memory latency per kL
  // entries at most, not per block of its own)
  unsigned i = i0;
  if (i + kL <= i1) {
    float cur[kL];
#pragma unroll
    for (int u = 0; u < kL; u++) cur[u] = buf[(size_t)(i + u) * bs];
    for (; i + 2 * kL <= i1; i += kL) {
      float nxt[kL];
#pragma unroll
      for (int u = 0; u < kL; u++) nxt[u] = buf[(size_t)(i + kL + u) * bs];
#pragma unroll
      for (int u = 0; u < kL; u++) acc += (double)cur[u] * scalar;
#pragma unroll
      for (int u = 0; u < kL; u++) cur[u] = nxt[u];
    }
#pragma unroll
    for (int u = 0; u < kL; u++) acc += (double)cur[u] * scalar;
    i += kL;
  }
  for (; i < i1; i++) acc += (double)buf[(size_t)i * bs] * scalar;
  return acc;
}
// The same over a stream's own contiguous row (the long-term buffers'
// layout, bs == 1): 16-byte loads, blocks of kV of them double-buffered.
template <int kV = FVAD_LT_BLOCK / 4>
__device__ __forceinline__ double lt_sum_row(double acc, const float *row, unsigned i0, unsigned i1, double scalar) {
  unsigned i = i0;
  for (; i < i1 && (i & 3u); i++) acc += (double)row[i] * scalar;  // to a 16-byte boundary
  const float4 *r4 = reinterpret_cast<const float4 *>(row);
  unsigned q = i >> 2;
  const unsigned qe = i < i1 ? i1 >> 2 : q;  // whole float4 in [i, i1)
  if (q + kV <= qe) {
    float4 cur[kV];
#pragma unroll
    for (int u = 0; u < kV; u++) cur[u] = r4[q + u];
    for (; q + 2 * kV <= qe; q += kV) {
      float4 nxt[kV];
#pragma unroll
      for (int u = 0; u < kV; u++) nxt[u] = r4[q + kV + u];
#pragma unroll
      for (int u = 0; u < kV; u++) {
        acc += (double)cur[u].x * scalar;
        acc += (double)cur[u].y * scalar;
        acc += (double)cur[u].z * scalar;
        acc += (double)cur[u].w * scalar;
      }
#pragma unroll
      for (int u = 0; u < kV; u++) cur[u] = nxt[u];
    }
#pragma unroll
    for (int u = 0; u < kV; u++) {
      acc += (double)cur[u].x * scalar;
      acc += (double)cur[u].y * scalar;
      acc += (double)cur[u].z * scalar;
      acc += (double)cur[u].w * scalar;
    }
    q += kV;
  }
  for (; q < qe; q++) {
    const float4 v = r4[q];
    acc += (double)v.x * scalar;
    acc += (double)v.y * scalar;
    acc += (double)v.z * scalar;
    acc += (double)v.w * scalar;
  }
  for (i = i < i1 ? (qe << 2 > i ? qe << 2 : i) : i1; i < i1; i++) acc += (double)row[i] * scalar;  // the tail
  return acc;
}
// entries never written hold the initial average: n adds of one term, done
// per binade (fvad_exact.h: the loop's bits)
__device__ __forceinline__ double lt_sum_init(double acc, double term, unsigned n) {
  return add_const_n(acc, term, n);
}
template <int kL = FVAD_LT_BLOCK>
__device__ __forceinline__ double lt_range(double acc, const float *buf, size_t bs, unsigned p, unsigned q,
                                           unsigned nw, double init, double scalar) {
  const unsigned mid = min(max(nw, p), q);  // [p, mid) written, [mid, q) initial
  acc = bs == 1 ? lt_sum_row<(kL >= 8 ? kL / 4 : 2)>(acc, buf, p, mid, scalar) : lt_sum<kL>(acc, buf, bs, p, mid, scalar);
  return lt_sum_init(acc, init * scalar, q - mid);
}

// The long-term average (4218 entries by default).  Same operation sequence as
// the full recompute, with one exact saving: once the buffer is full the
// scalar 1/n no longer changes, so the running sum over the entries before the
// write position is exactly what the previous pass had accumulated there
// (those entries have not changed) - the pass starts from that cached prefix.
// Entries never written since the machine started hold the initial average
// (a double, RollingAverage.zig init): entry i is a pushed f32 iff i < nw.
// (kL, here and in lt_resolve / vadm_walk: lt_range's block, the entries read
// ahead of the add chain -- registers, not results)
template <int kL = FVAD_LT_BLOCK>
__device__ __forceinline__ double ra_push_long(float *buf, size_t bs, int n, unsigned &widx, unsigned &count,
                                               unsigned &nw, double init, double &last, int &has, double &pre,
                                               int &pre_ok, float sample) {
  const unsigned w = widx;
  buf[(size_t)w * bs] = sample;
  widx = (w + 1) % (unsigned)n;
  if (count < (unsigned)n) count++;
  if (nw < (unsigned)n) nw++;
  const double scalar = 1.0 / (double)count;
  const unsigned start = pre_ok ? w : 0u;
  double acc = pre_ok ? pre : 0.0;
  const unsigned save_at = widx;  // the next pass starts at the next write position
  double save = 0.0;              // (save_at == 0: it starts from 0.0)
  if (save_at > start && save_at < count) {
    acc = lt_range<kL>(acc, buf, bs, start, save_at, nw, init, scalar);
    save = acc;
    acc = lt_range<kL>(acc, buf, bs, save_at, count, nw, init, scalar);
  } else {
    if (save_at == start) save = acc;
    acc = lt_range<kL>(acc, buf, bs, start, count, nw, init, scalar);
  }
  pre = save;
  pre_ok = count == (unsigned)n;
  last = acc;
  has = 1;
  return acc;
}

// VADMachine.run's per-window steps (VADMachine.zig:126-230), shared by the
// serial walk (vadm_stream) and the window-parallel kernel (k_vadm_par).
enum { kVmClosed = 0, kVmOpening = 1, kVmOpen = 2, kVmClosing = 3 };
// short-term and channel-ratio averages (pushed every window); `met`: the
// speech condition against the long-term average of the last long push
// (KT, here and below: the machine's constants, VadmConst from the argument
// block or a stream's own VadmRow -- the same names, the same expressions)
template <class KT>
__device__ __forceinline__ bool vadm_short(VadmState &S, const KT &K, float *st, float *rb, int B, float min_v,
                                           float vr) {
  const double st_avg = ra_push(st, B, K.n_st, S.st_widx, S.st_count, S.st_last, S.st_has, min_v);
  const double r_avg = ra_push(rb, B, K.n_r, S.r_widx, S.r_count, S.r_last, S.r_has, vr);
  double base;
  if (S.lt_has)
    base = S.lt_last;
  else if (K.has_init)
    base = K.init;
  else
    base = st_avg;
  const double threshold = base * (double)K.thr_factor;
  return st_avg > threshold && r_avg > (double)K.ratio_thr;
}
// The event feed's staging area of one lane (stream, machine): ev_cap records
// and their count in HBM, touched only in the two arms that produce an event.
// A window produces at most one event -- the Opening -> Open arm and the
// Closing -> Closed arm (onSpeechEnd) are different cases of one switch -- so a
// lane stages at most as many records as its stream completes windows in the
// push, and ev_cap is the engine's bound on those (its wmax, which also sizes
// win_tick / win_start); the k < cap test below can therefore not drop one.
struct VadmEvLane {
  VadmEvRec *rec;  // null: no event feed
  unsigned *n;
  int cap;
};
__device__ __forceinline__ VadmEvLane vadm_ev_lane(const VadmArgs &v, int m, int s) {
  VadmEvLane l{nullptr, nullptr, 0};
  if (v.ev_stage) {
    const size_t lane = (size_t)s * v.n + m;
    l.rec = v.ev_stage + lane * v.ev_cap;
    l.n = v.ev_count + lane;
    l.cap = v.ev_cap;
  }
  return l;
}
__device__ __forceinline__ void vadm_ev_put(const VadmEvLane &l, unsigned kind, unsigned seq, unsigned long long from,
                                            unsigned long long to, float rnn_vad, float vol_ratio) {
  const unsigned k = *l.n;
  if (k < (unsigned)l.cap) {
    VadmEvRec r;
    r.kind = kind;
    r.seq = seq;
    r.sample_from = from;
    r.sample_to = to;
    r.debug_rnn_vad = rnn_vad;
    r.debug_avg_speech_vol_ratio = vol_ratio;
    l.rec[k] = r;
    *l.n = k + 1;
  }
}
enum { kVeSpeechOpen = 1, kVeSegment = 2 };  // FVAD_EVENT_SPEECH_OPEN, FVAD_EVENT_SEGMENT (include/fvad.h)

// the speech-state transition, segment output and tracking of one window
template <class KT>
__device__ __forceinline__ void vadm_fsm(VadmState &S, const KT &K, unsigned long long index, bool met,
                                         float vad, float vr, VadmSeg *seg, int seg_cap, const VadmEvLane &ev) {
  const int from = S.state;
  bool ended = false;
  switch (from) {
    case kVmClosed:
      if (met) {
        S.state = kVmOpening;
        S.speech_start = index;
      }
      break;
    case kVmOpening:
      if (met && index - S.speech_start >= K.min_open) {
        S.state = kVmOpen;
        if (ev.rec) vadm_ev_put(ev, kVeSpeechOpen, S.n_segs, S.speech_start, index, 0.0f, 0.0f);
      } else if (!met) {
        S.state = kVmClosed;
      }
      break;
    case kVmOpen:
      if (!met) {
        S.state = kVmClosing;
        S.speech_end = index;
      }
      break;
    default:  // kVmClosing
      if (met) {
        S.state = kVmOpen;
      } else if (index - S.speech_end >= K.max_gap) {
        S.state = kVmClosed;
        ended = true;
      }
      break;
  }
  if (ended) {  // onSpeechEnd (before the tracking update of this window, as in VADMachine.zig)
    const unsigned long long len = S.speech_end - S.speech_start;
    const float len_rt = (float)len / K.sr;
    if (len_rt >= K.min_dur) {
      if (S.n_segs < (unsigned)seg_cap || ev.rec) {  // (the feed carries segments past seg_cap too)
        VadmSeg g;
        g.sample_from = K.rec_pad > S.speech_start ? 0ull : S.speech_start - K.rec_pad;
        g.sample_to = S.speech_end + K.rec_pad;
        g.debug_rnn_vad = S.rnn_vad / (float)S.rnn_vad_count;
        g.debug_avg_speech_vol_ratio = S.vol_ratio / (float)S.vol_ratio_count;
        if (S.n_segs < (unsigned)seg_cap) seg[S.n_segs] = g;
        if (ev.rec)
          vadm_ev_put(ev, kVeSegment, S.n_segs, g.sample_from, g.sample_to, g.debug_rnn_vad,
                      g.debug_avg_speech_vol_ratio);
      }
      S.n_segs++;
    }
  }
  // track(vad, vr, from, to)
  if (from == kVmClosed && S.state == kVmOpening) {
    S.rnn_vad = vad;
    S.rnn_vad_count = 1;
    S.vol_ratio = vr;
    S.vol_ratio_count = 1;
  } else if (from == kVmOpening || from == kVmOpen) {
    S.rnn_vad += vad;
    S.rnn_vad_count += 1;
    S.vol_ratio += vr;
    S.vol_ratio_count += 1;
  }
}

// Deferred folds.  Between sync points (k_vadm_hbm, final = false) the exact
// fold a push would end with is owed instead of done: the estimate, its
// bound's magnitude and the exact prefix ride in the state (lt_defer long
// pushes since the last exact fold) and the next push's walk continues from
// them, so a machine folds only for a test the bound does not settle, after
// kLtDeferMax long pushes, or at a sync point (final: k_vadm_par's drain, or
// k_vadm_hbm when the push cannot take k_vadm_par), where every machine is
// resolved -- states and segments read after a sync are the reference's.
// (One fold per stream and push was ~4 000 f64 adds in the full-buffer
// regime: k_vadm_hbm 0.44-0.65 ms beside the next push, which stretched the
// co-running k_prep3 and, through it, k_pspecw.)
#ifndef FVAD_LT_DEFER_MAX
#define FVAD_LT_DEFER_MAX 4096
#endif
constexpr unsigned kLtDeferMax = FVAD_LT_DEFER_MAX;
// the fold a deferred machine owes: vadm_stream's fold, the same adds in the
// same order (the exact prefix through the last pushed index, then the
// entries after it)
// lt_neg's bookkeeping for one long push of v
__device__ __forceinline__ void lt_neg_push(VadmState &S, unsigned n, float v) {
  if (S.lt_neg > 0) S.lt_neg--;
  if (!(v >= 0.0f)) S.lt_neg = (int)n;
}
template <int kL = FVAD_LT_BLOCK, class KT>
__device__ __forceinline__ void lt_resolve(VadmState &S, const KT &K, const float *lt, size_t lts) {
  if (!S.lt_defer) return;
  const unsigned n = (unsigned)K.n_lt;
  double acc = S.lt_fpre;
  if (S.lt_widx != 0) acc = lt_range<kL>(acc, lt, lts, S.lt_widx, n, S.lt_nw, K.init, 1.0 / (double)n);
  S.lt_last = acc;
  S.lt_defer = 0;
}

// One machine over a run of windows in order (a push's, or a block of a
// recorded sequence); `lt` points at entry 0 of the machine's long-term
// buffer, `lts` is its stride; `st` / `rb` at entry 0 of its short-term and
// ratio buffers, stride B.  for_each_window(body) calls body(min_v, vad, vr)
// once per window: min_v the minimum over channels of the machine's band
// (from 999, strict <), vad the window's vad (0 without the denoiser), vr its
// volume ratio.  S is the caller's copy of the state, stored by the caller.
//
// Lazy long-term folds.  Once the long-term buffer is full (from the start
// with an initial average) every window that pushes re-folds ~n - w entries
// (RollingAverage.zig:45-56), ~12 folds per push: 7 ms per push at 2048
// streams once a stream is past its first long_term_speech_avg_sec (a full
// buffer of pushed values, measured with FVAD_DEBUG_VADM_LT_FULL).  But a
// window's average is only *observed* through the next window's test
// st_avg > RN(lt_last * factor), and the last one through the state.  So the
// walk keeps a running estimate of the average (approx += t_new - t_old per
// push, t = RN(entry * 1/n)) with a rigorous bound E on its distance to the
// fold's result -- the fold of nonnegative terms is within (n-1) u of their
// exact sum (u = 2^-53), each estimate update adds <= 2u -- decides every test
// whose outcome the bound settles, runs the exact fold (the same adds in the
// same order as the reference) only for a test it does not settle, and folds
// once at the end of the run for the state (final, or defer_max long pushes
// owed; otherwise the fold stays owed in S, see "Deferred folds" above).  The
// cached prefix P_w advances by one add per push, as in k_vadm_par.  Every
// decision and every stored value is the reference's; typically one fold per
// run instead of one per window.  Used when the buffer is full, the terms are
// nonnegative (band energies, a nonnegative initial average) and the threshold
// factor is nonnegative; otherwise each pushing window folds at once
// (ra_push_long).  Whether the walk is lazy is decided once, at the start of
// the run.
template <int kL = FVAD_LT_BLOCK, class KT, class ForEachWindow>
__device__ __forceinline__ void vadm_walk(VadmState &S, const KT &K, float *st, float *rb, int B, float *lt,
                                          size_t lts, VadmSeg *seg, int seg_cap, const VadmEvLane &ev,
                                          unsigned long long fft, double bound_scale, unsigned defer_max,
                                          unsigned long long *cnt, bool final, ForEachWindow &&for_each_window) {
  const unsigned n = (unsigned)K.n_lt;
  const double f = (double)K.thr_factor, scalar = 1.0 / (double)n;
  const bool lazy = S.lt_count == n && S.lt_pre_ok && S.lt_has && n > 1 && f >= 0.0 &&
                    !(K.has_init && !(K.init >= 0.0)) && S.lt_neg == 0;
  if (!lazy) lt_resolve<kL>(S, K, lt, lts);  // (a deferring machine is lazy; kept for safety)
  // the bound's scale: the test hook's, +inf once a negative entry is pushed
  // (no bound holds then: every later test of the run folds)
  double bscale = bound_scale;
  double approx = S.lt_last, amax = fabs(S.lt_last), fpre = 0.0;
  int pending = 0;  // pushes since lt_last was last folded exactly
  if (S.lt_defer) {  // owed from earlier runs (deferred folds)
    approx = S.lt_approx;
    amax = S.lt_amax;
    fpre = S.lt_fpre;
    pending = (int)S.lt_defer;
  }
  // the exact average of the current buffer: the fold through the last pushed
  // index (fpre) continued over the entries after it, C order
  auto fold = [&]() {
    double acc = fpre;
    if (S.lt_widx != 0) acc = lt_range<kL>(acc, lt, lts, S.lt_widx, n, S.lt_nw, K.init, scalar);
    S.lt_last = acc;
    approx = acc;
    amax = fabs(acc);
    pending = 0;
  };
  for_each_window([&](float min_v, float vad, float vr) {
    const unsigned long long index = S.windows_done * fft;
    S.windows_done++;
    bool met;
    if (!lazy) {
      met = vadm_short(S, K, st, rb, B, min_v, vr);
      if (!met) {
        ra_push_long<kL>(lt, lts, K.n_lt, S.lt_widx, S.lt_count, S.lt_nw, K.init, S.lt_last, S.lt_has, S.lt_pre,
                     S.lt_pre_ok, min_v);
        lt_neg_push(S, n, min_v);
      }
    } else {
      const double st_avg = ra_push(st, B, K.n_st, S.st_widx, S.st_count, S.st_last, S.st_has, min_v);
      const double r_avg = ra_push(rb, B, K.n_r, S.r_widx, S.r_count, S.r_last, S.r_has, vr);
      met = false;
      if (r_avg > (double)K.ratio_thr) {  // else met is false whatever the long-term average
        if (pending == 0) {
          met = st_avg > S.lt_last * f;
          if (cnt) atomicAdd(cnt + kVcExact, 1ull);
        } else {
          // |approx - fold| <= E (fvad_exact.h lt_bound: the fold's (n-1) u,
          // twice, and 2u per estimate update, on the largest estimate)
          const int d = lt_decide(st_avg, approx, lt_bound(n, (unsigned)pending, amax, bscale), f);
          if (d >= 0) {
            met = d == 1;
            if (cnt) atomicAdd(cnt + kVcSettled, 1ull);
          } else {  // not settled by the bound: the exact fold
            fold();
            met = st_avg > S.lt_last * f;
            if (cnt) atomicAdd(cnt + kVcOpen, 1ull);
          }
        }
      }
      if (!met) {  // push min_v into the long-term buffer (ra_push_long's state, the fold deferred)
        const unsigned wi = S.lt_widx;
        const double t_old = (wi < S.lt_nw ? (double)lt[(size_t)wi * lts] : K.init) * scalar;
        lt[(size_t)wi * lts] = min_v;
        const double t_new = (double)min_v * scalar;
        fpre = S.lt_pre + t_new;  // the fold through index wi
        S.lt_widx = (wi + 1) % n;
        if (S.lt_nw < n) S.lt_nw++;
        S.lt_pre = S.lt_widx == 0 ? 0.0 : fpre;
        lt_estimate(approx, amax, t_new, t_old);
        pending++;
        lt_neg_push(S, n, min_v);
        if (S.lt_neg) bscale = __builtin_inf();
      }
    }
    vadm_fsm(S, K, index, met, vad, vr, seg, seg_cap, ev);
  });
  if (pending && (final || (unsigned)pending >= (defer_max ? defer_max : kLtDeferMax))) {
    fold();
    if (cnt) atomicAdd(cnt + kVcEndFold, 1ull);
  }
  S.lt_defer = (unsigned)pending;
  S.lt_approx = approx;
  S.lt_amax = amax;
  S.lt_fpre = fpre;
}

}  // namespace fvad
