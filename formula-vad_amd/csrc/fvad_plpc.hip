// The pitch front of the staged pipeline: k_plpc.  k_pcorr follows it
// (fvad_pitch.hip, built with other flags), then k_select (at the end of
// fvad_vadm.hip, where the compiler gives it the code it was measured with).
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
// Pitch analysis (pitch.c: pitch_downsample, pitch_search, remove_doubling up
// to its sequential selection), split by how each part parallelises:
//
//   k_plpc   lane per frame.  Every serial chain that depends only on the
//            frame itself and streams its pitch buffer: x_lp, the 5 autocorr
//            sums (860 terms each), LPC, the 5-tap FIR, the Syy recurrences of
//            both find_best_pitch calls and xx.  A wave owns a tile of 64
//            streams at one frame position (lane = stream), so all 64 lanes
//            walk a chain.  Writes xf and the sequences to the tile buffer.
//   k_pcorr  8 frames per workgroup, xf resident in LDS.  The inner products
//            (coarse xcorr: 147 lags x 240, fine xcorr at <= 10 lags, the
//            remove_doubling products), both find_best_pitch scans and the
//            yy_lookup recurrence (lane per frame) and the pitch record for
//            k_select (fvad_pitch.hip).
// Every C-order sum stays on one lane in its original order.
// ---------------------------------------------------------------------------

// pitch_downsample's LPC part (celt_lpc.c _celt_lpc, order 4) and the FIR
// coefficients lpc2 of celt_fir5, from the 5 autocorrelation values.
__device__ __forceinline__ void lpc_fir5_coeffs(float (&acv)[5], float (&lpc2)[5]) {
  acv[0] *= 1.0001f;
  for (int i = 1; i <= 4; i++) acv[i] -= acv[i] * (.008f * i) * (.008f * i);
  float lpc[4] = {0, 0, 0, 0};
  float error = acv[0];
  if (acv[0] != 0) {
    for (int i = 0; i < 4; i++) {
      float r_acc = 0;
      for (int j = 0; j < i; j++) r_acc += lpc[j] * acv[i - j];
      r_acc += acv[i + 1];
      const float r = -r_acc / error;
      lpc[i] = r;
      for (int j = 0; j < (i + 1) >> 1; j++) {
        const float tmp1 = lpc[j], tmp2 = lpc[i - 1 - j];
        lpc[j] = tmp1 + r * tmp2;
        lpc[i - 1 - j] = tmp2 + r * tmp1;
      }
      error = error - (r * r) * error;
      if (error < .001f * acv[0]) break;
    }
  }
  float tmp = 1.0f;
  for (int i = 0; i < 4; i++) {
    tmp = .9f * tmp;
    lpc[i] = lpc[i] * tmp;
  }
  const float c1 = .8f;
  lpc2[0] = lpc[0] + .8f;
  lpc2[1] = lpc[1] + c1 * lpc[0];
  lpc2[2] = lpc[2] + c1 * lpc[1];
  lpc2[3] = lpc[3] + c1 * lpc[2];
  lpc2[4] = c1 * lpc[3];
}

// ---------------------------------------------------------------------------
// k_plpc.  Both passes walk the frame's x_lp (pitch_downsample's 2:1
// decimation of the pitch buffer), read from the x_lp rows: every x_lp value
// of the push is computed once (k_prep3 for the history, k_fftAw for each
// frame's 240 new values) instead of from 1728 pitch-buffer samples per frame
// and pass, which halves this kernel's input bytes (0.88 -> 0.7x ms).  A
// tile's 64 rows are staged through LDS in chunks of 8 values: 16-byte
// coalesced loads of each stream's row, transposed to [value][stream] (row
// pitch 68: conflict-free for both the transposing writes and the column
// reads), the next chunk loading while one is summed.  x_lp[0] is the frame's
// own edge value (.5 * (.5 * x[1] + x[0])), from two pitch-buffer samples.
// Tile t = sb * Vr + v (Vr = frame positions of this push); the four waves of
// a workgroup take consecutive v of the same streams.
// ---------------------------------------------------------------------------
constexpr int kLpStep = 8;                // x_lp steps per chunk
constexpr int kLpRows = kLpStep;          // x_lp values of a stream per chunk (32 bytes)
constexpr int kLpPR = kLpRows / 4;        // float4 per stream row of a chunk (= loads per lane)
constexpr int kLpSPI = 64 / kLpPR;        // streams per load instruction
constexpr int kLpCols = 68;               // 4 * 68 = 16 (mod 32): the two float4 columns of a
                                          // half-wave's ds_write_b32 land on disjoint bank halves
constexpr int kLpChunks = kXlp / kLpStep;  // 108
static_assert(kXlp % kLpStep == 0 && kLpPR == 2, "x_lp chunking");

struct LpSrc {
  const float *p[kLpPR];  // per load slot: stream's x_lp row + 4 * (lane % kLpPR)
};

__device__ __forceinline__ void lp_fetch(const LpSrc &s, int c, float4 (&r)[kLpPR]) {
#pragma unroll
  for (int i = 0; i < kLpPR; i++) r[i] = *reinterpret_cast<const float4 *>(s.p[i] + kLpRows * c);
}

// chunk registers -> LDS [value][stream]
__device__ __forceinline__ void lp_stage(float *stg, int lane, const float4 (&r)[kLpPR]) {
  wave_sync();
  const int p = lane % kLpPR, s0 = lane / kLpPR;
#pragma unroll
  for (int i = 0; i < kLpPR; i++) {
    float *d = stg + (4 * p) * kLpCols + s0 + kLpSPI * i;
    d[0] = r[i].x;
    d[kLpCols] = r[i].y;
    d[2 * kLpCols] = r[i].z;
    d[3 * kLpCols] = r[i].w;
  }
  wave_sync();
}

// x_lp[n] for n = kLpStep * c + u from the staged column; the frame's x_lp[0]
// (pitch_downsample's edge value, .5 * (.5 * x[1] + x[0])) is not in the
// shared row and comes from the lane (x0)
template <bool First>
__device__ __forceinline__ float lp_value(const float *col, int u, float x0) {
  return (First && u == 0) ? x0 : col[u * kLpCols];
}

// pass-2 state of one lane (k_plpc)
struct Fir5State {
  float l[5];
  float m1 = 0, m2 = 0, m3 = 0, m4 = 0, m5 = 0;  // x_lp[n-1..n-5]
  float b1 = 0, b2 = 0, b3 = 0, b4 = 0, b5 = 0;  // x_lp[n-481..n-485]: the lagged filter (xf[n - 480])
  float x0 = 0;                                  // x_lp[0]
  float Sc = 1.0f, Sf = 1.0f, xx = 0.0f;
};

// celt_fir5 step: y = x + l0 x[n-1] + ... + l4 x[n-5] in C order, history shifted
__device__ __forceinline__ float fir5_step(const float (&l)[5], float x, float &m1, float &m2, float &m3, float &m4,
                                           float &m5) {
  float y = x;
  y = y + l[0] * m1;
  y = y + l[1] * m2;
  y = y + l[2] * m3;
  y = y + l[3] * m4;
  y = y + l[4] * m5;
  m5 = m4, m4 = m3, m3 = m2, m2 = m1, m1 = x;
  return y;
}

// Row stores of the tile buffer go through a per-wave LDS stage: a chunk's
// rows (one value per lane each) are written to LDS [row][lane], then each
// lane stores two float4 of its quarter's [row][16] block, so one store
// instruction writes 1 KB in four 256-byte runs instead of 256 bytes in four
// 64-byte pieces (measured: the per-step dword row stores cost k_plpc ~0.4 ms).
// xf itself is not stored (k_pcorr rebuilds it from x_lp and the coefficients):
// the Syy recurrences' xf[n - 480] comes from a second filter over the x_lp
// chunk 480 values back, staged like the current one.
struct OutStage {
  float sf[1][64];            // the fine Syy checkpoint of the chunk (i = n0 - 480, a multiple of 8)
  float sc[kLpStep / 2][64];  // coarse Syy rows
};
// rows row0 .. row0 + NR - 1 of the lane's quarter (qbase = its [row][16] block)
template <int NR>
__device__ __forceinline__ void flush_rows(float *qbase, int row0, const float (*ob)[64], int lane) {
  const int q = lane >> 4;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int j = (lane & 15) + 16 * k, u = j >> 2, c4 = j & 3;
    if (u < NR)
      *reinterpret_cast<float4 *>(qbase + (row0 + u) * ptile::kQuarter + 4 * c4) =
          *reinterpret_cast<const float4 *>(&ob[u][16 * q + 4 * c4]);
  }
}

// One chunk of pass 2.  Region R of n = n0 .. n0+7:
//   1 [0, 384)    Syy initial sums      2 [384, 480)  + xx
//   3 [480, 774)  xx + Syy recurrences  4 the chunk holding n = 773 (guarded)
//   5 [774, 864)  xx only
// bcol: the staged x_lp column of chunk n0 - 480 (regions 3, 4; LagFirst: it
// is chunk 0, whose x_lp[0] is the lane's x0)
template <bool First, int R, bool LagFirst>
__device__ __forceinline__ void fir5_chunk(Fir5State &f, const float *col, const float *bcol, float *qbase, int n0,
                                           OutStage &ob, int lane) {
  constexpr int kR4 = (480 + 294) % kLpStep;  // region 4 starts at a chunk boundary
#pragma unroll
  for (int u = 0; u < kLpStep; u++) {
    const float y = fir5_step(f.l, lp_value<First>(col, u, f.x0), f.m1, f.m2, f.m3, f.m4, f.m5);
    if (R <= 2) {
      if ((u & 1) == 0) f.Sc = f.Sc + y * y;  // n0 is a multiple of 8: n even <=> u even
      f.Sf = f.Sf + y * y;
    }
    if (R == 3 || (R == 4 && u < kR4)) {
      const float yb = fir5_step(f.l, lp_value<LagFirst>(bcol, u, f.x0), f.b1, f.b2, f.b3, f.b4, f.b5);
      if (u == 0) ob.sf[0][lane] = f.Sf;  // k_pcorr walks from here to the lags it needs
      f.Sf += y * y - yb * yb;
      f.Sf = (1 > f.Sf) ? 1 : f.Sf;
      if ((u & 1) == 0) {
        ob.sc[u >> 1][lane] = f.Sc;
        f.Sc += y * y - yb * yb;
        f.Sc = (1 > f.Sc) ? 1 : f.Sc;
      }
    }
    if (R >= 2) f.xx = f.xx + y * y;
  }
  if (R == 3 || R == 4) {
    wave_sync();
    flush_rows<1>(qbase, ptile::kSf + (n0 - 480) / kLpStep, ob.sf, lane);
    if (R == 3)
      flush_rows<kLpStep / 2>(qbase, ptile::kSc + (n0 - 480) / 2, ob.sc, lane);
    else
      flush_rows<(kR4 + 1) / 2>(qbase, ptile::kSc + (n0 - 480) / 2, ob.sc, lane);
    wave_sync();
  }
}
static_assert(384 % kLpStep == 0 && 480 % kLpStep == 0 && kLpStep % 2 == 0, "pass-2 regions");
static_assert(480 % kLpStep == 0, "the lagged chunk is a whole chunk");
static_assert(kLpStep == 8 && (294 + kLpStep - 1) / kLpStep == ptile::kSfCk, "fine Syy checkpoints every 8 lags");

// x_lp chunks in flight per pass (the ring depth)
#ifndef FVAD_PLPC_OCC
#define FVAD_PLPC_OCC 2
#endif
#ifndef FVAD_LP_PF
#define FVAD_LP_PF 4
#endif
constexpr int kLpPf = FVAD_LP_PF;
static_assert(kLpChunks % kLpPf == 0, "prefetch ring must divide the passes");

// pass-1 state of one lane (k_plpc): _celt_autocorr's 5 lag sums, the tail
// sums of lags 1..3 and the last 4 x_lp values
struct AcState {
  float acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0, acc4 = 0;
  float d0 = 0, d1 = 0, d2 = 0, d3 = 0;
  float h1 = 0, h2 = 0, h3 = 0, h4 = 0;
};
// One chunk of pass 1 (lag k: sum_{i<860} x[i] x[i+k], then the tail).
// Kind 0: the first chunk (x_lp[0] = x0, lags start at their first term),
// 1: a middle chunk, 2: the last (n = 856..863: term i = n - k belongs to the
// 860-term sum while i < 860, else (n >= 860 + k) to the tail sum of x[n] x[n-k])
template <int Kind>
__device__ __forceinline__ void ac_chunk(AcState &s, const float *col, float x0, int c) {
#pragma unroll
  for (int u = 0; u < kLpStep; u++) {
    const float x = lp_value<Kind == 0>(col, u, x0);
    if (Kind == 2) {
      const int n = c * kLpStep + u;
      if (n < 860) s.acc0 = s.acc0 + x * x; else s.d0 = s.d0 + x * x;
      if (n - 1 < 860) s.acc1 = s.acc1 + s.h1 * x; else s.d1 = s.d1 + x * s.h1;
      if (n - 2 < 860) s.acc2 = s.acc2 + s.h2 * x; else s.d2 = s.d2 + x * s.h2;
      if (n - 3 < 860) s.acc3 = s.acc3 + s.h3 * x; else s.d3 = s.d3 + x * s.h3;
      s.acc4 = s.acc4 + s.h4 * x;  // n - 4 <= 859
    } else {
      s.acc0 = s.acc0 + x * x;
      if (Kind == 1 || u >= 1) s.acc1 = s.acc1 + s.h1 * x;
      if (Kind == 1 || u >= 2) s.acc2 = s.acc2 + s.h2 * x;
      if (Kind == 1 || u >= 3) s.acc3 = s.acc3 + s.h3 * x;
      if (Kind == 1 || u >= 4) s.acc4 = s.acc4 + s.h4 * x;
    }
    s.h4 = s.h3, s.h3 = s.h2, s.h2 = s.h1, s.h1 = x;
  }
}
static_assert(kLpChunks * kLpStep == 864 && (kLpChunks - 1) * kLpStep == 856, "pass-1 tail chunk");

__global__ void __launch_bounds__(256, FVAD_PLPC_OCC) k_plpc(StagedArgs a) {
  __shared__ float stg_all[4][2][kLpRows * kLpCols];
  __shared__ __attribute__((aligned(16))) OutStage ost_all[4];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  float *stg = stg_all[w][0], *stgb = stg_all[w][1];
  OutStage &ob = ost_all[w];
  const float *col = stg + lane;
  const int Vr = a.n_ticks * a.n_channels;
  const int n_sb = (a.n_streams + 63) >> 6;
  const long long n_tiles = (long long)n_sb * Vr;
  // a workgroup takes 4 consecutive tiles (one per wave: neighbouring frame
  // positions of the same streams share pitch-buffer samples in L2)
  const long long n_quads = (n_tiles + 3) / 4;
  __shared__ long long gq;
  STAMP_INIT();
  if (tid == 0) gq = take_group(a, kWorkPlpc);
  __syncthreads();
  long long q = gq;
  while (q < n_quads) {
    const long long t = q * 4 + w;
    if (t >= n_tiles) {
      __syncthreads();
      if (tid == 0) gq = take_group(a, kWorkPlpc);
      __syncthreads();
      q = gq;
      continue;
    }
    const int sb = (int)(t / Vr), v = (int)(t - (long long)sb * Vr);
    LpSrc src;
#pragma unroll
    for (int i = 0; i < kLpPR; i++) {
      const int s = min(sb * 64 + lane / kLpPR + kLpSPI * i, a.n_streams - 1);
      src.p[i] = a.xlp + (size_t)s * a.LX + (size_t)v * (kFrame / 2) + 4 * (lane % kLpPR);
    }
    float x0;
    {
      const float *pb = a.xs + (size_t)min(sb * 64 + lane, a.n_streams - 1) * a.L + (size_t)v * kFrame;
      x0 = .5f * (.5f * (pb[1]) + pb[0]);
    }
    // lane's output column: quarter (lane >> 4) of tile t, [row][16]
    float *out = a.ptile + ((size_t)(t * 4 + (lane >> 4)) * ptile::kRows) * ptile::kQuarter + (lane & 15);
    float *qbase = out - (lane & 15);
    RSTAMP(3);

    // Both passes walk the x_lp chunks through a register ring: chunk c is
    // staged while the loads of chunks c + 1 .. c + kLpPf are in flight (the
    // chunk loops unrolled by the ring depth, so slots are static registers)
    float4 pf[kLpPf][kLpPR];
    // pass 1: x_lp -> _celt_autocorr
    AcState as;
#pragma unroll
    for (int d = 0; d < kLpPf; d++) lp_fetch(src, d, pf[d]);
    for (int c0 = 0; c0 < kLpChunks; c0 += kLpPf) {
#pragma unroll
      for (int dd = 0; dd < kLpPf; dd++) {
        const int c = c0 + dd;
        lp_stage(stg, lane, pf[dd]);
        if (c + kLpPf < kLpChunks) lp_fetch(src, c + kLpPf, pf[dd]);
        if (c == 0)
          ac_chunk<0>(as, col, x0, c);
        else if (c + 1 < kLpChunks)
          ac_chunk<1>(as, col, x0, c);
        else
          ac_chunk<2>(as, col, x0, c);
      }
    }
    RSTAMP(0);
    float acv[5] = {as.acc0 + as.d0, as.acc1 + as.d1, as.acc2 + as.d2, as.acc3 + as.d3, as.acc4 + 0.0f};
    float l[5];
    lpc_fir5_coeffs(acv, l);

    // pass 2: x_lp again -> celt_fir5 -> xf; Syy initial sums, xx; from
    // n = 480 on, the Syy recurrences with xf[n - 480] from a second filter
    // over the x_lp chunk 480 values back (a second ring, staged in the
    // wave's second column).  The chunk body is specialised per region of n,
    // so it has no branches.
    Fir5State fs;
    fs.x0 = x0;
#pragma unroll
    for (int i = 0; i < 5; i++) fs.l[i] = l[i];
    const float *bcol = stgb + lane;
    constexpr int kLag = 480 / kLpStep;  // chunks between a value and its lagged partner
    auto lagged = [](int c) { return c * kLpStep >= 480 && c * kLpStep < 480 + 294; };
    float4 bk[kLpPf][kLpPR];
#pragma unroll
    for (int d = 0; d < kLpPf; d++) lp_fetch(src, d, pf[d]);
    for (int c0 = 0; c0 < kLpChunks; c0 += kLpPf) {
#pragma unroll
      for (int dd = 0; dd < kLpPf; dd++) {
        const int c = c0 + dd, n0 = c * kLpStep;
        lp_stage(stg, lane, pf[dd]);
        if (c + kLpPf < kLpChunks) lp_fetch(src, c + kLpPf, pf[dd]);
        if (lagged(c)) lp_stage(stgb, lane, bk[dd]);
        if (lagged(c + kLpPf)) lp_fetch(src, c + kLpPf - kLag, bk[dd]);
        if (c == 0)
          fir5_chunk<true, 1, false>(fs, col, bcol, qbase, n0, ob, lane);
        else if (n0 < 384)
          fir5_chunk<false, 1, false>(fs, col, bcol, qbase, n0, ob, lane);
        else if (n0 < 480)
          fir5_chunk<false, 2, false>(fs, col, bcol, qbase, n0, ob, lane);
        else if (n0 == 480)
          fir5_chunk<false, 3, true>(fs, col, bcol, qbase, n0, ob, lane);
        else if (n0 + kLpStep <= 480 + 294)
          fir5_chunk<false, 3, false>(fs, col, bcol, qbase, n0, ob, lane);
        else if (n0 < 480 + 294)
          fir5_chunk<false, 4, false>(fs, col, bcol, qbase, n0, ob, lane);
        else
          fir5_chunk<false, 5, false>(fs, col, bcol, qbase, n0, ob, lane);
      }
    }
    RSTAMP(1);
    out[ptile::kXx * ptile::kQuarter] = fs.xx;
    // k_pcorr's xf: the FIR coefficients and x_lp[0]
#pragma unroll
    for (int i = 0; i < 5; i++) out[(ptile::kFir + i) * ptile::kQuarter] = l[i];
    out[(ptile::kFir + 5) * ptile::kQuarter] = x0;

    // yy_lookup (remove_doubling's energy recurrence from xx) is k_pcorr's:
    // it walks it on a wave its product phase leaves idle, from xf in LDS
    RSTAMP(2);
    __syncthreads();
    if (tid == 0) gq = take_group(a, kWorkPlpc);
    __syncthreads();
    q = gq;
  }
  STAMP_FLUSH(56, 4);
}

// k_plpc over `tiles` pitch tiles: a persistent grid of at most the resident
// capacity (blocks per CU from the occupancy calculator x CUs)
hipError_t launch_plpc(const StagedArgs &a, long long tiles, int n_cu, hipStream_t stream) {
  static const int p_plpc = resident_per_cu(k_plpc, 256);
  const int g_plpc = p_plpc * n_cu;
  // as many workgroups as give every one the same number of quads: 3 200
  // tiles on 2 048 wave slots run as 2 even rounds on 400 workgroups rather
  // than a full round and a 56 % one (0.90 -> 0.88 ms)
  const long long quads = (tiles + 3) / 4, rounds = (quads + g_plpc - 1) / g_plpc;
  const unsigned grid = (unsigned)std::min<long long>((quads + rounds - 1) / rounds, g_plpc);
  FVAD_KERNEL_TRY(k_plpc, dim3(grid), dim3(256), 0, stream, a);
  return hipSuccess;
}

}  // namespace fvad
