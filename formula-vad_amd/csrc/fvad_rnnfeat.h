// What the recurrence kernels share beside their GRU arithmetic (k_rnn3 /
// k_rnn3f in fvad_rnn3.hip: f32 chains; k_gru16 / k_fused16 in fvad_gru16.hip:
// f16 MFMA tiles): the per-stream bookkeeping in LDS with its load from and
// write-back to the state block, the raw-feature fetch, and the feature and
// gain-smoothing steps around fvad_rnnfeat_core.h's formulas.  Each kernel
// keeps its wave plan (which lanes take which items in which phase), its GRU
// state layout, its spectral-variability lane layout and its pf depth.
#pragma once
#pragma clang fp contract(off)
#include "fvad_rnnfeat_core.h"
#include "fvad_staged_dev.h"

namespace fvad {

constexpr int kRawFeat = 30;  // raw feature words per stream and frame: Lyf[22], f34[7], silence

// streams [sb, sb + per_wg) of the push that exist: the ones a workgroup owns
__device__ __forceinline__ int own_streams(const StagedArgs &a, int sb, int per_wg) {
  return min(per_wg, a.n_streams - sb);
}

// S stream slots; slots >= n_own stay zero and inactive (nfs = 0)
template <int S>
struct RecurLds {
  float tt[204];
  float ceps[S][kCeps * kBands];
  float dist[S][kCeps * kCeps];
  float lastg[S][kBands];
  int act[8][S];  // frame f in slot f & 7: valid and not silent
  int memid[S], nfs[S];
  long long fbase[S];

  // (before the workgroup's first barrier)
  __device__ __forceinline__ void load(const StagedArgs &a, int sb, int n_own, int tid, int NT) {
    for (int i = tid; i < 201; i += NT) tt[i] = a.plan->tansig[i];
    for (int idx = tid; idx < S * kCeps * kBands; idx += NT) {
      const int s = idx / (kCeps * kBands), i = idx - s * (kCeps * kBands);
      ceps[s][i] = (s < n_own) ? a.state[(size_t)(sb + s) * st::kWords + st::kCepsMem + i] : 0.0f;
    }
    for (int idx = tid; idx < S * kCeps * kCeps; idx += NT) {
      const int s = idx / (kCeps * kCeps), i = idx - s * (kCeps * kCeps);
      dist[s][i] = (s < n_own) ? a.state[(size_t)(sb + s) * st::kWords + st::kCepsDist + i] : 0.0f;
    }
    for (int idx = tid; idx < S * kBands; idx += NT) {
      const int s = idx / kBands, i = idx - s * kBands;
      lastg[s][i] = (s < n_own) ? a.state[(size_t)(sb + s) * st::kWords + st::kLastG + i] : 0.0f;
    }
    if (tid < 8 * S) act[tid / S][tid % S] = 0;
    if (tid < S) {
      const int s = sb + tid;
      const bool ok = tid < n_own;
      memid[tid] = ok ? reinterpret_cast<const int *>(a.state)[(size_t)s * st::kWords + st::kMemId] : 0;
      nfs[tid] = ok ? ticks_of(a, s) * a.n_channels : 0;
      fbase[tid] = (long long)s * a.V;
    }
  }
  // a stream that ran at least one frame in this push writes its state back
  __device__ __forceinline__ bool ran(int s, int n_own) const { return s < n_own && nfs[s] > 0; }
  __device__ __forceinline__ void store(const StagedArgs &a, int sb, int n_own, int tid, int NT) const {
    for (int idx = tid; idx < S * kCeps * kBands; idx += NT) {
      const int s = idx / (kCeps * kBands), i = idx - s * (kCeps * kBands);
      if (ran(s, n_own)) a.state[(size_t)(sb + s) * st::kWords + st::kCepsMem + i] = ceps[s][i];
    }
    for (int idx = tid; idx < S * kCeps * kCeps; idx += NT) {
      const int s = idx / (kCeps * kCeps), i = idx - s * (kCeps * kCeps);
      if (ran(s, n_own)) a.state[(size_t)(sb + s) * st::kWords + st::kCepsDist + i] = dist[s][i];
    }
    for (int idx = tid; idx < S * kBands; idx += NT) {
      const int s = idx / kBands, i = idx - s * kBands;
      if (ran(s, n_own)) a.state[(size_t)(sb + s) * st::kWords + st::kLastG + i] = lastg[s][i];
    }
    if (tid < S && ran(tid, n_own))
      reinterpret_cast<int *>(a.state)[(size_t)(sb + tid) * st::kWords + st::kMemId] = memid[tid];
  }
  __device__ __forceinline__ int max_frames() const {
    int m = 0;
#pragma unroll
    for (int s = 0; s < S; s++) m = max(m, nfs[s]);
    return m;
  }
};

// raw feature word i of stream slot s, frame v: i < 22 Lyf, 22..28 f34, 29
// silence (the flag's bits, nonzero = silent: converting it here would wait
// for the load where it is issued).  Past the stream's end: silent (inactive).
template <int S>
__device__ __forceinline__ float raw_feature(const StagedArgs &a, const RecurLds<S> &R, int s, int i, int v) {
  if (v >= R.nfs[s]) return 1.0f;
  const long long f = R.fbase[s] + v;
  if (i < kBands) return a.Lyf[f * kBands + i];
  if (i < kBands + 7) return a.f34[f * 8 + (i - kBands)];
  return __int_as_float(a.silence[f]);
}

// Item idx = s * rnnfeat::kItems + i of frame f's features (cepstral memory,
// deltas, 34..40, the new distance row) from the raw rows c0[s]; put(s, k, v)
// takes feature k of stream s.  Item i == 0 records act(f).
template <int S, class Put>
__device__ __forceinline__ void feat_items(RecurLds<S> &R, const StagedArgs &a, int f, int idx,
                                           const float (*c0)[kRawFeat], Put put) {
  const int s = idx / rnnfeat::kItems, i = idx - s * rnnfeat::kItems;
  const bool valid = f < R.nfs[s];
  const bool on = valid && __float_as_int(c0[s][kRawFeat - 1]) == 0;
  if (i == 0) {
    R.act[f & 7][s] = on;
    if (valid && !on) a.vadf[R.fbase[s] + f] = 0;  // silent: X passes through, state untouched
  }
  if (!on) return;
  rnnfeat::feat_item(c0[s], R.ceps[s], R.dist[s], R.memid[s], i, [&](int k, float v) { put(s, k, v); });
}

// gain smoothing of band i of stream s, frame f, from denoise_output's gi
template <int S>
__device__ __forceinline__ void gains_of(RecurLds<S> &R, const StagedArgs &a, int f, int s, int i, float gi) {
  if (!R.act[f & 7][s]) return;
  const long long g = R.fbase[s] + f;
  const float gsm = rnnfeat::gain_smooth(gi, R.lastg[s][i]);
  R.lastg[s][i] = gsm;
  a.gr[g * kBands + i] = gi;
  a.gs[g * kBands + i] = gsm;
}

}  // namespace fvad
