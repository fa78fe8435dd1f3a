// The f32 recurrence of the staged pipeline: k_rnn3 (exact) and k_rnn3f
// (FVAD_MODE_F32_FAST, fused multiply-add terms), one body.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "fvad_device.h"
#include "fvad_internal.h"
#include "fvad_launch.h"
#include "fvad_rnnfeat.h"
#include "fvad_staged.h"
#include "fvad_staged_dev.h"

namespace fvad {

// ---------------------------------------------------------------------------
// GRU helpers of k_rnn3.  The whole GRU stack is resident in LDS as an int8
// image (rnnimg, 88 KB; int8 -> f32 is exact), so weights never come from L2
// per frame.  A matrix column = one neuron's C-order sum: lane (column, stream
// group) accumulates SL streams of that column with one weight fetch per term;
// per-stream vectors are stored [j][S] so the SL inputs of a term are one LDS
// read.  GRU inputs are read in place from their segments (no concatenation
// copies) and GRU states live in rings indexed by frame (no copy-back phase).
// ---------------------------------------------------------------------------

// acc[q] += w[j] * v[j][s0 + q] for the n terms of one segment, C order.  The
// segment's weights start 8-byte aligned: 8 terms = one 64-bit LDS read plus
// eight SL-float input reads, all issued before the arithmetic.
template <int SL>
struct VecT;
template <>
struct VecT<2> {
  typedef float2 T;
};
template <>
struct VecT<4> {
  typedef float4 T;
};
__device__ __forceinline__ float wbyte(uint2 w8, int u) {
  return (float)(signed char)((u < 4 ? w8.x : w8.y) >> (8 * (u & 3)));
}
// (FMA, through every helper below: k_rnn3f's form of a term, one fused
// multiply-add -- a single rounding -- where k_rnn3 multiplies, then adds)
template <int SL, bool FMA>
__device__ __forceinline__ void mac(float (&acc)[SL], float w, const typename VecT<SL>::T &v) {
  if constexpr (FMA) {
    acc[0] = __builtin_fmaf(w, v.x, acc[0]);
    acc[1] = __builtin_fmaf(w, v.y, acc[1]);
    if constexpr (SL == 4) {
      acc[2] = __builtin_fmaf(w, v.z, acc[2]);
      acc[3] = __builtin_fmaf(w, v.w, acc[3]);
    }
  } else {
    acc[0] = acc[0] + w * v.x;
    acc[1] = acc[1] + w * v.y;
    if constexpr (SL == 4) {
      acc[2] = acc[2] + w * v.z;
      acc[3] = acc[3] + w * v.w;
    }
  }
}
template <int SL, bool FMA>
__device__ __forceinline__ void mac_r(float (&acc)[SL], float w, const typename VecT<SL>::T &sv,
                                      const typename VecT<SL>::T &rv) {
  if constexpr (FMA) {
    acc[0] = __builtin_fmaf(w * sv.x, rv.x, acc[0]);
    acc[1] = __builtin_fmaf(w * sv.y, rv.y, acc[1]);
    if constexpr (SL == 4) {
      acc[2] = __builtin_fmaf(w * sv.z, rv.z, acc[2]);
      acc[3] = __builtin_fmaf(w * sv.w, rv.w, acc[3]);
    }
  } else {
    acc[0] = acc[0] + w * sv.x * rv.x;
    acc[1] = acc[1] + w * sv.y * rv.y;
    if constexpr (SL == 4) {
      acc[2] = acc[2] + w * sv.z * rv.z;
      acc[3] = acc[3] + w * sv.w * rv.w;
    }
  }
}

template <int n, int S, int SL, bool FMA>
__device__ __forceinline__ void mv_seg(const int8_t *__restrict__ wc, const float *vT, int s0, float (&acc)[SL]) {
  typedef typename VecT<SL>::T V;
  constexpr int nb = n / 8, r = n % 8;
#pragma unroll 1
  for (int jb = 0; jb < nb; jb++) {
    const uint2 w8 = *reinterpret_cast<const uint2 *>(wc + jb * 8);
    V v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = *reinterpret_cast<const V *>(vT + (jb * 8 + u) * S + s0);
#pragma unroll
    for (int u = 0; u < 8; u++) mac<SL, FMA>(acc, wbyte(w8, u), v[u]);
  }
  if (r) {
    const uint2 w8 = *reinterpret_cast<const uint2 *>(wc + nb * 8);
#pragma unroll
    for (int u = 0; u < r; u++) mac<SL, FMA>(acc, wbyte(w8, u), *reinterpret_cast<const V *>(vT + (nb * 8 + u) * S + s0));
  }
}

// GRU candidate recurrent segment: acc[q] += (w[j] * state[j][q]) * r[j][q]
template <int n, int S, int SL, bool FMA>
__device__ __forceinline__ void mv_seg_r(const int8_t *__restrict__ wc, const float *sT, const float *rT, int s0,
                                         float (&acc)[SL]) {
  typedef typename VecT<SL>::T V;
  static_assert(n % 8 == 0, "recurrent segment shape");
#pragma unroll 1
  for (int jb = 0; jb < n / 8; jb++) {
    const uint2 w8 = *reinterpret_cast<const uint2 *>(wc + jb * 8);
    V sv[8], rv[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      sv[u] = *reinterpret_cast<const V *>(sT + (jb * 8 + u) * S + s0);
      rv[u] = *reinterpret_cast<const V *>(rT + (jb * 8 + u) * S + s0);
    }
#pragma unroll
    for (int u = 0; u < 8; u++) mac_r<SL, FMA>(acc, wbyte(w8, u), sv[u], rv[u]);
  }
}

// Input of one matrix: its input-vector segments in concatenation order.
struct RnnIn {
  const float *v0, *v1, *v2;
};

template <int m, int S, int SL, bool FMA>
__device__ __forceinline__ void rnn_inputs(const int8_t *wc, const RnnIn &in, int s0, float (&acc)[SL]) {
  constexpr int n0 = rnnimg::kSegs[m][0];
  mv_seg<n0, S, SL, FMA>(wc, in.v0, s0, acc);
  if constexpr (m == 3 || m == 4 || m == 5 || m == 6) {
    constexpr int n1 = rnnimg::kSegs[m][1], n2 = rnnimg::kSegs[m][2];
    mv_seg<n1, S, SL, FMA>(wc + rnnimg::seg_off(m, 1), in.v1, s0, acc);
    mv_seg<n2, S, SL, FMA>(wc + rnnimg::seg_off(m, 2), in.v2, s0, acc);
  }
}

// input segments [G0, G1) of matrix m (a sum split across phases continues
// where the stored partial sum stopped: the same adds in the same order)
template <int m, int S, int SL, int G0, int G1, bool FMA>
__device__ __forceinline__ void rnn_segs(const int8_t *wc, const RnnIn &in, int s0, float (&acc)[SL]) {
  if constexpr (G0 <= 0 && G1 > 0) mv_seg<rnnimg::kSegs[m][0], S, SL, FMA>(wc, in.v0, s0, acc);
  if constexpr (m == 3 || m == 4 || m == 5 || m == 6) {
    if constexpr (G0 <= 1 && G1 > 1) mv_seg<rnnimg::kSegs[m][1], S, SL, FMA>(wc + rnnimg::seg_off(m, 1), in.v1, s0, acc);
    if constexpr (G0 <= 2 && G1 > 2) mv_seg<rnnimg::kSegs[m][2], S, SL, FMA>(wc + rnnimg::seg_off(m, 2), in.v2, s0, acc);
  }
}
template <int SL>
__device__ __forceinline__ void acc_load(float (&acc)[SL], const float *p) {
  const typename VecT<SL>::T v = *reinterpret_cast<const typename VecT<SL>::T *>(p);
  acc[0] = v.x;
  acc[1] = v.y;
  if constexpr (SL == 4) {
    acc[2] = v.z;
    acc[3] = v.w;
  }
}
template <int SL>
__device__ __forceinline__ void acc_store(const float (&acc)[SL], float *p) {
  typename VecT<SL>::T v;
  v.x = acc[0];
  v.y = acc[1];
  if constexpr (SL == 4) {
    v.z = acc[2];
    v.w = acc[3];
  }
  *reinterpret_cast<typename VecT<SL>::T *>(p) = v;
}

// dense layer / GRU z|r gates of image matrix m:
//   out[c][s] = act(kWs * (b[c] + sum_j w[c][j] * [in ; state][j][s]))
// (tasks t = tid, tid + NT, ...; NT = 0: the single task tid)
// (PART 3: b + input segment 0 only, stored to preT [c][S]; PART 5: from
// preT, the remaining input segments and the state)
template <bool FMA, int m, int S, int G, int NT, int PART = 0>
__device__ __forceinline__ void rnn_gates(const int8_t *W, const RnnIn &in, const float *stT, float *outT, int act,
                                          const float *tt, int tid, float *preT = nullptr) {
  constexpr int SL = S / G, cols = rnnimg::kCols[m];
  constexpr int ob = rnnimg::off_b(m), ow = rnnimg::off_w(m), ws = rnnimg::stride(m);
  constexpr int gst = (m == 1) ? 1 : (m == 3 || m == 5) ? 3 : -1;  // state segment of z|r matrices
  for (int t = tid; t < cols * G; t += (NT ? NT : cols * G)) {
    const int c = t / G, s0 = (t - c * G) * SL;
    const int8_t *wc = W + ow + c * ws;
    float acc[SL];
    if constexpr (PART == 5) {
      acc_load<SL>(acc, preT + c * S + s0);
      rnn_segs<m, S, SL, 1, 3, FMA>(wc, in, s0, acc);
    } else {
      const float b = (float)W[ob + c];
#pragma unroll
      for (int q = 0; q < SL; q++) acc[q] = b;
      if constexpr (PART == 3) {
        rnn_segs<m, S, SL, 0, 1, FMA>(wc, in, s0, acc);
        acc_store<SL>(acc, preT + c * S + s0);
        continue;
      } else {
        rnn_inputs<m, S, SL, FMA>(wc, in, s0, acc);
      }
    }
    if constexpr (gst >= 0) mv_seg<rnnimg::kSegs[m][gst], S, SL, FMA>(wc + rnnimg::seg_off(m, gst), stT, s0, acc);
#pragma unroll
    for (int q = 0; q < SL; q++) outT[c * S + s0 + q] = activate(tt, act, kWs * acc[q]);
  }
}

// GRU candidate of image matrix m: sum = b + sum_j w*in[j] + sum_j (w*state[j])*r[j];
// new[c][s] = z*state + (1-z)*act(kWs*sum) for active streams, state otherwise.
// The sum's input prefix (b + the input terms) does not depend on the reset
// gate, so it can run one phase early: PART 1 stores the prefix to preT
// ([c][S]) and returns, PART 2 starts from preT and adds the recurrent terms
// -- the same sequence of f32 adds as PART 0, split at a store.
template <bool FMA, int m, int S, int G, int NT, int PART = 0>
__device__ __forceinline__ void rnn_cand(const int8_t *W, const RnnIn &in, const float *stT, const float *zrT,
                                         float *newT, const int *actv, int act, const float *tt, int tid,
                                         float *preT = nullptr) {
  constexpr int SL = S / G, cols = rnnimg::kCols[m], N = cols;
  constexpr int ob = rnnimg::off_b(m), ow = rnnimg::off_w(m), ws = rnnimg::stride(m);
  constexpr int gst = (m == 2) ? 1 : 3;
  for (int t = tid; t < cols * G; t += (NT ? NT : cols * G)) {
    const int c = t / G, s0 = (t - c * G) * SL;
    const int8_t *wc = W + ow + c * ws;
    float acc[SL];
    if constexpr (PART == 2 || PART == 4) {
      acc_load<SL>(acc, preT + c * S + s0);
      if constexpr (PART == 4) rnn_segs<m, S, SL, 1, 3, FMA>(wc, in, s0, acc);
    } else {
      const float b = (float)W[ob + c];
#pragma unroll
      for (int q = 0; q < SL; q++) acc[q] = b;
      if constexpr (PART == 3)
        rnn_segs<m, S, SL, 0, 1, FMA>(wc, in, s0, acc);
      else
        rnn_inputs<m, S, SL, FMA>(wc, in, s0, acc);
    }
    if constexpr (PART == 1 || PART == 3 || PART == 4) {
      acc_store<SL>(acc, preT + c * S + s0);
      continue;
    }
    mv_seg_r<rnnimg::kSegs[m][gst], S, SL, FMA>(wc + rnnimg::seg_off(m, gst), stT, zrT + N * S, s0, acc);
#pragma unroll
    for (int q = 0; q < SL; q++) {
      const int o = c * S + s0 + q;
      const float sum = activate(tt, act, kWs * acc[q]);
      const float z = zrT[o];
      newT[o] = actv[s0 + q] ? z * stT[o] + (1 - z) * sum : stT[o];
    }
  }
}

// ---------------------------------------------------------------------------
// k_rnn3: the recurrence.  One workgroup owns 8 streams and walks their
// frames in lockstep, 4 streams per lane (G = 2: one column's 8 streams on two
// lanes), as a two-phase layer pipeline over frames: compute_rnn's GRUs
// depend on each other only within a frame (vad -> noise -> denoise) and on
// their own previous state, so one step runs different layers of different
// frames side by side.  A lane's inputs
// for one term are one 16-byte LDS read (ds_read_b128, full LDS rate; the
// float2 reads of G = 4 were paired into half-rate ds_read2_b64) and one
// int8 -> f32 conversion serves 4 streams.  Step t:
//   P1  z|r gates of vad(t-1), noise(t-2), denoise(t-3); the denoise
//       candidates' input prefixes of t-3; spectral variability of t; gain
//       smoothing of t-5
//   P2  candidates of vad(t-1), noise(t-2), denoise(t-3) (denoise: its 96
//       recurrent terms after the P1 prefix); dense(t); denoise_output(t-4);
//       vad_output(t-2); features of t+1 (cepstral memory, deltas, distance
//       row) -> LDS; the denoise z|r gates' and candidates' first segment
//       (b + the 24 vad-state terms) of frame t-2, continued by the next P1
// Two barriers per step.  Every term keeps its C order; buffers are rings
// indexed by frame (features 8, dense/vad state 4, noise/denoise state 2).
// ---------------------------------------------------------------------------

// P2 wave priorities (s_setprio while the role runs): bit 2 the noise h
// waves, bit 4 denoise_output (kept: k_rnn3 1.19 -> 1.16 ms; both are young
// waves that set P2's end), bit 128 the denoise candidates' vad-state
// segment wave 15 (kept: 1.141 -> 1.128 ms; the z|r segment waves 12-14
// raised lost, 1.17), bit 8 vad h + dense (no gain; nor vad_output or
// the feature waves raised: 1.17 -> 1.18 ms).  Raising P1's
// noise or vad z|r waves above the denoise waves lost (1.16 -> 1.19 / 1.21 ms),
// as did the denoise prefix waves (1.23 ms).
#ifndef FVAD_PRIO
#define FVAD_PRIO 134
#endif
constexpr int kR3S = 8, kR3G = 2, kR3NT = 1024;
// FMA = false: k_rnn3; true: k_rnn3f (FVAD_MODE_F32_FAST), the same plan with
// every GRU and dense term a fused multiply-add.  (a by value, as a kernel
// takes it: k_rnn3 then compiles to the instructions it had as a plain kernel)
template <bool FMA>
__device__ __forceinline__ void rnn3_body(StagedArgs a) {
  constexpr int S = kR3S, G = kR3G, NT = kR3NT;
  struct Lds {
    alignas(16) float featT[8][44 * S];  // frame f in slot f & 7
    alignas(16) float doutT[4][24 * S];
    alignas(16) float gvT[4][24 * S];
    alignas(16) float gnT[2][48 * S];
    alignas(16) float gdT[2][96 * S];
    alignas(16) float zrv[48 * S], zrn[96 * S], zrd[192 * S];
    alignas(16) float dhp[2][96 * S];  // denoise candidate input prefixes of frame f in slot f & 1
    alignas(16) float zpre[192 * S];  // denoise z|r: b + the vad-state segment of the frame P1 continues
    alignas(16) float gout[2][22 * S];  // denoise_output of frame f in slot f & 1
    alignas(16) float vo[S];  // vad_output of the frame P2 computed last
    RecurLds<S> R;           // tt, cepstral memory and distances, lastg, act, memid, nfs, fbase
    float pf[S][kRawFeat];   // raw features of the frame the next F-C stage reads
    alignas(16) int8_t W[rnnimg::kBytes];
  };
  __shared__ Lds L;
  const int tid = threadIdx.x;
  const int sb = blockIdx.x * S, n_own = own_streams(a, sb, S);
  auto &R = L.R;
  const int *ra = a.rnn_act;
  {
    const int4 *src = reinterpret_cast<const int4 *>(a.rnn_img);
    int4 *dst = reinterpret_cast<int4 *>(L.W);
    for (int i = tid; i < rnnimg::kBytes / 16; i += NT) dst[i] = src[i];
  }
  R.load(a, sb, n_own, tid, NT);
  // states before frame 0 = "frame -1": gv slot 3, gn / gd slot 1
  for (int idx = tid; idx < S * 96; idx += NT) {
    const int s = idx / 96, i = idx - s * 96;
    const bool ok = s < n_own;
    const float *stp = a.state + (size_t)(sb + s) * st::kWords;
    if (i < 24) L.gvT[3][i * S + s] = ok ? stp[st::kVadGru + i] : 0.0f;
    if (i < 48) L.gnT[1][i * S + s] = ok ? stp[st::kNoiseGru + i] : 0.0f;
    L.gdT[1][i * S + s] = ok ? stp[st::kDenGru + i] : 0.0f;
  }
  __syncthreads();
  const int maxnf = R.max_frames();
  // prefetch lane (s, i) of the raw features (raw_feature: the silence word
  // unconverted, or the lane would wait for the load at the top of every step,
  // before its P1 role)
  const int pfs = tid / kRawFeat, pfi = tid - pfs * kRawFeat;
  const bool pf_lane = tid < S * kRawFeat;
  auto fetch = [&](int v) -> float { return pf_lane ? raw_feature(a, R, pfs, pfi, v) : 1.0f; };
  // F-C: frame f's features from L.pf into featT slot f & 7; item (s, i), i < 37
  auto feat_c = [&](int f, int idx) {
    float *featT = L.featT[f & 7];
    feat_items(R, a, f, idx, L.pf, [&](int s, int k, float v) { featT[k * S + s] = v; });
  };
  // F-D: spectral variability of frame f, stream s
  auto feat_d = [&](int f, int s) {
    if (!R.act[f & 7][s]) return;
    float sv = 0;
    for (int i = 0; i < kCeps; i++) sv += rnnfeat::dist_row_min(R.dist[s], i);
    L.featT[f & 7][41 * S + s] = rnnfeat::spec_variability(sv);
    R.memid[s] = rnnfeat::memid_next(R.memid[s]);
  };
  // prologue: features of frame 0 (its spectral variability: P1 of step 0)
  if (pf_lane) L.pf[pfs][pfi] = fetch(0);
  __syncthreads();
  for (int idx = tid; idx < S * rnnfeat::kItems; idx += NT) feat_c(0, idx);
  __syncthreads();
  // P1 wave plan (w = tid >> 6).  Waves w, w+4, w+8, w+12 share a SIMD under
  // the cyclic wave placement, so the heavy roles are spread over the four
  // residue classes -- {den, den, pre}, {den, den, pre}, {den, noise, noise,
  // vad}, {den, noise, vad, pre} -- and no wave holds lanes of two roles (it
  // would run both branches one after the other): denoise z|r waves 0..5 (384
  // tasks), noise z|r waves 6, 7, 10 (192), vad z|r waves 11, 14 (96), the
  // denoise candidates' input prefixes (b + the 114 input terms, which do not
  // need the reset gate) waves 12, 13, 15 (192), gain smoothing + vad_output
  // store wave 8, spectral variability of frame t wave 9.  (The constants
  // name each role's first thread, for the stamps build.)  Measured and lost
  // (DESIGN §8 r3): the noise candidates' prefixes here too (on waves 8 / 9,
  // gains moved to P2: P1 16.0 -> 17.7 k cycles, P2 12.6 -> 10.9 k), and the
  // heavy roles on the oldest waves of each SIMD (the young vad waves starve).
  [[maybe_unused]] constexpr int kP1Den = 0, kP1Noise = 384, kP1Vad = 704, kP1Var = 576, kP1Gain = 512;
  // P2 wave plan, balanced over the residue classes the same way (a wave
  // holding lanes of two roles set the phase at 19.6 k cycles before): denoise
  // h waves 0..2 (192 tasks; the 96 recurrent terms from the P1 prefix),
  // noise h waves 3, 6 (96), denoise_output wave 4 (44), vad h wave 5 (48),
  // dense of frame t wave 7 (48), vad_output wave 8 (2 lanes), features of
  // frame t+1 waves 9..11 (296 items, two per lane on the first 104), the
  // denoise z|r first segments of frame t-2 waves 12..14 (384 tasks, two per
  // lane), the denoise candidates' wave 15 (192, three per lane).  (Denoise h with 2 streams per lane on
  // 6 waves shortened its chain to 11.1 k cycles but the extra waves
  // stretched the other roles: 15.3 vs 14.6 k per phase.)
  [[maybe_unused]] constexpr int kP2Den = 0, kP2Noise = 192, kP2Vad = 320, kP2Dense = 448, kP2Out = 256, kP2VadOut = 512,
                kP2Feat = 576;
  constexpr int kFeatItems = S * rnnfeat::kItems;
  static_assert(kP2Feat + kFeatItems <= 14 * 64 && 96 * kR3G == 192 && 48 * kR3G <= 128 && 22 * kR3G <= 64 &&
                    24 * kR3G <= 64,
                "P2 wave plan");
  STAMP_INIT();
  PHASE_INIT();  // a role's finish time: its first thread's busy cycles of the phase
  // gain smoothing (gains_of) of frame f5 on lanes i0, i0 + n, ...; reads
  // denoise_output slot f5 & 1
  auto gains = [&](int f5, int i0, int n) {
    for (int idx = i0; f5 >= 0 && idx < S * kBands; idx += n) {
      const int s = idx / kBands, i = idx - s * kBands;
      gains_of(R, a, f5, s, i, L.gout[f5 & 1][i * S + s]);
    }
  };
  for (int t = 0; t <= maxnf + 4; t++) {
    // per-step opaque thread id: the roles' per-thread offsets are recomputed
    // each step instead of hoisted out of the frame loop, where they spilled
    // (128 VGPRs + 34 spilled -> 112, no scratch: 1.27 -> 1.23-1.24 ms)
    int tq = tid;
    asm volatile("" : "+v"(tq));
    const int fv = t - 1, fn = t - 2, fd = t - 3;
    PHASE_BEGIN();
    // frame t+1's raw features, staged at the end of P1 for P2's feat_c:
    // issued here, so no load is outstanding across a step boundary (a
    // loop-carried register would make the step's last barrier wait for it)
    const float pf_now = fetch(t + 1);
    // ---- P1
    // (the wave index as a scalar, readfirstlane: measured neutral here,
    // 1.135-1.154 vs 1.126-1.155 ms interleaved; k_gru16 gains from it)
    const int wv = tq >> 6, ln = tq & 63;
    if (wv < 6) {
      if (fd >= 0 && fd < maxnf)
        rnn_gates<FMA, 5, S, G, 0, 5>(L.W, RnnIn{L.gvT[fd & 3], L.gnT[fd & 1], L.featT[fd & 7]}, L.gdT[(fd + 1) & 1],
                                 L.zrd, kActSigmoid, R.tt, tq, L.zpre);
    } else if (wv == 6 || wv == 7 || wv == 10) {
      if (fn >= 0 && fn < maxnf)
        rnn_gates<FMA, 3, S, G, 0>(L.W, RnnIn{L.doutT[fn & 3], L.gvT[fn & 3], L.featT[fn & 7]}, L.gnT[(fn + 1) & 1], L.zrn,
                              kActSigmoid, R.tt, (wv == 10 ? 128 : 64 * (wv - 6)) + ln);
    } else if (wv == 11 || wv == 14) {
      if (fv >= 0 && fv < maxnf)
        rnn_gates<FMA, 1, S, G, 0>(L.W, RnnIn{L.doutT[fv & 3], nullptr, nullptr}, L.gvT[(fv + 3) & 3], L.zrv, kActSigmoid,
                              R.tt, (wv == 14 ? 64 : 0) + ln);
    } else if (wv == 12 || wv == 13 || wv == 15) {
      // denoise candidate input prefixes of frame t-3
      if (fd >= 0 && fd < maxnf)
        rnn_cand<FMA, 6, S, G, 0, 4>(L.W, RnnIn{L.gvT[fd & 3], L.gnT[fd & 1], L.featT[fd & 7]}, nullptr, nullptr, nullptr,
                                nullptr, 0, nullptr, (wv == 15 ? 128 : 64 * (wv - 12)) + ln, L.dhp[fd & 1]);
    } else if (wv == 8 && ln < 48) {  // gain smoothing of frame t-5
      gains(t - 5, ln, 48);
    } else if (wv == 9 && ln < S) {  // spectral variability of frame t (features: P2 of step t-1)
      if (t < maxnf) feat_d(t, ln);
    } else if (wv == 8 && ln >= 48 && ln < 48 + S) {  // vad_output of frame t-3 (P2 of step t-1)
      const int s = ln - 48, fw = t - 3;
      if (fw >= 0 && fw < maxnf && R.act[fw & 7][s]) a.vadf[R.fbase[s] + fw] = L.vo[s];
    }
    PHASE_END(0);
    if (pf_lane) L.pf[pfs][pfi] = pf_now;
    lds_sync();
    RSTAMP(0);
    PHASE_BEGIN();
    // ---- P2
    const int fo = t - 4;
    if (wv < 3) {
      if (fd >= 0 && fd < maxnf)
        rnn_cand<FMA, 6, S, G, 0, 2>(L.W, RnnIn{nullptr, nullptr, nullptr}, L.gdT[(fd + 1) & 1], L.zrd, L.gdT[fd & 1],
                                R.act[fd & 7], ra[6], R.tt, tq, L.dhp[fd & 1]);
    } else if (wv == 3 || wv == 6) {
      if (FVAD_PRIO & 2) __builtin_amdgcn_s_setprio(3);
      if (fn >= 0 && fn < maxnf)
        rnn_cand<FMA, 4, S, G, 0>(L.W, RnnIn{L.doutT[fn & 3], L.gvT[fn & 3], L.featT[fn & 7]}, L.gnT[(fn + 1) & 1], L.zrn,
                             L.gnT[fn & 1], R.act[fn & 7], ra[4], R.tt, (wv == 6 ? 64 : 0) + ln);
      if (FVAD_PRIO & 2) __builtin_amdgcn_s_setprio(0);
    } else if (wv == 5) {
      if (FVAD_PRIO & 8) __builtin_amdgcn_s_setprio(2);
      if (fv >= 0 && fv < maxnf)
        rnn_cand<FMA, 2, S, G, 0>(L.W, RnnIn{L.doutT[fv & 3], nullptr, nullptr}, L.gvT[(fv + 3) & 3], L.zrv, L.gvT[fv & 3],
                             R.act[fv & 7], ra[2], R.tt, ln);
      if (FVAD_PRIO & 8) __builtin_amdgcn_s_setprio(0);
    } else if (wv == 7) {
      if (FVAD_PRIO & 8) __builtin_amdgcn_s_setprio(2);
      if (t < maxnf)
        rnn_gates<FMA, 0, S, G, 0>(L.W, RnnIn{L.featT[t & 7], nullptr, nullptr}, nullptr, L.doutT[t & 3], ra[0], R.tt, ln);
      if (FVAD_PRIO & 8) __builtin_amdgcn_s_setprio(0);
    } else if (wv == 4) {
      if (FVAD_PRIO & 4) __builtin_amdgcn_s_setprio(2);
      if (fo >= 0 && fo < maxnf)
        rnn_gates<FMA, 7, S, G, 0>(L.W, RnnIn{L.gdT[fo & 1], nullptr, nullptr}, nullptr, L.gout[fo & 1], ra[7], R.tt, ln);
      if (FVAD_PRIO & 4) __builtin_amdgcn_s_setprio(0);
    } else if (wv == 8 && ln < G) {
      // vad_output(t-2) -> L.vo, stored by the next step's P1
      if (fn >= 0 && fn < maxnf)
        rnn_gates<FMA, 8, S, G, 0>(L.W, RnnIn{L.gvT[fn & 3], nullptr, nullptr}, nullptr, L.vo, ra[8], R.tt, ln);
    } else if (tq >= kP2Feat && tq < kP2Feat + 192) {  // features of t+1 on waves 9..11
      for (int idx = tq - kP2Feat; t + 1 < maxnf && idx < kFeatItems; idx += 192) feat_c(t + 1, idx);
    } else if (wv >= 12 && wv <= 14) {  // denoise z|r of frame t-2: b + the vad-state segment
      const int fz = t - 2;
      if (fz >= 0 && fz < maxnf)
        rnn_gates<FMA, 5, S, G, 192, 3>(L.W, RnnIn{L.gvT[fz & 3], nullptr, nullptr}, nullptr, nullptr, kActSigmoid, R.tt,
                                   tq - 768, L.zpre);
    } else if (wv == 15) {  // denoise candidates of frame t-2: b + the vad-state segment
      const int fz = t - 2;
      if (FVAD_PRIO & 128) __builtin_amdgcn_s_setprio(2);
      if (fz >= 0 && fz < maxnf)
        rnn_cand<FMA, 6, S, G, 64, 3>(L.W, RnnIn{L.gvT[fz & 3], nullptr, nullptr}, nullptr, nullptr, nullptr, nullptr, 0,
                                 nullptr, ln, L.dhp[fz & 1]);
      if (FVAD_PRIO & 128) __builtin_amdgcn_s_setprio(0);
    }
    PHASE_END(1);
    lds_sync();
    RSTAMP(1);
  }
  STAMP_FLUSH(0, 2);
#ifdef FVAD_STAMPS
  // P1 roles -> stamps[2..6], P2 roles -> stamps[8..14] (tid 0 and 384 lead a
  // role in both phases)
  if (a.stamps) {
    const int p1[5] = {kP1Den, kP1Noise, kP1Vad, kP1Var, kP1Gain};
    const int p2[7] = {kP2Den, kP2Noise, kP2Vad, kP2Dense, kP2Out, kP2VadOut, kP2Feat};
    for (int i = 0; i < 5; i++)
      if (tid == p1[i]) atomicAdd(&a.stamps[2 + i], ph_acc[0]);
    for (int i = 0; i < 7; i++)
      if (tid == p2[i]) atomicAdd(&a.stamps[8 + i], ph_acc[1]);
  }
  // every wave's busy cycles per phase (lane 0): stamps[64 + w] P1, [80 + w] P2
  if (a.stamps && (tid & 63) == 0) {
    atomicAdd(&a.stamps[64 + (tid >> 6)], ph_acc[0]);
    atomicAdd(&a.stamps[80 + (tid >> 6)], ph_acc[1]);
  }
#endif
  const int fin = maxnf - 1;  // the slots of the latest states ("frame -1" if there were none)
  R.store(a, sb, n_own, tid, NT);
  for (int idx = tid; idx < S * 96; idx += NT) {
    const int s = idx / 96, i = idx - s * 96;
    if (!R.ran(s, n_own)) continue;
    float *stp = a.state + (size_t)(sb + s) * st::kWords;
    if (i < 24) stp[st::kVadGru + i] = L.gvT[fin & 3][i * S + s];
    if (i < 48) stp[st::kNoiseGru + i] = L.gnT[fin & 1][i * S + s];
    stp[st::kDenGru + i] = L.gdT[fin & 1][i * S + s];
  }
}
__global__ void __launch_bounds__(kR3NT) k_rnn3(StagedArgs a) { rnn3_body<false>(a); }
__global__ void __launch_bounds__(kR3NT) k_rnn3f(StagedArgs a) { rnn3_body<true>(a); }

hipError_t launch_rnn3(const StagedArgs &a, hipStream_t stream) {
  const dim3 grid((a.n_streams + kR3S - 1) / kR3S);
  if (a.fma)  // FVAD_MODE_F32_FAST
    FVAD_KERNEL_TRY(k_rnn3f, grid, dim3(kR3NT), 0, stream, a);
  else
    FVAD_KERNEL_TRY(k_rnn3, grid, dim3(kR3NT), 0, stream, a);
  return hipSuccess;
}

}  // namespace fvad
