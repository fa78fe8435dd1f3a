// Per-stream lifecycle (fvad_engine_reset_streams / save_streams /
// restore_streams): argument blocks and launchers of the clear, gather and
// scatter kernels (fvad_lifecycle.hip), and the layout of one stream's record
// in a stream blob (include/fvad.h documents the blob's header).
//
// Everything a stream carries between pushes, all indexed by stream:
//   state  [s][st::kWords]            the rnnoise / re-block record
//   ring   [s][c][ring_len]           denoised samples awaiting FFT B
//   per machine m: VadmState [m][s], the long-term row [s][lt_pitch], the
//   short-term and ratio columns [i][s], the segment row [m][s][seg_cap],
//   and with per-stream configs the constant table's row [m][s]
//   (fvad_engine_set_stream_vadm: k_vadm_retarget; a blob does not carry it)
#pragma once
#include <hip/hip_runtime.h>

#include "fvad_staged.h"

namespace fvad {

// The listed streams reach the device as kernel arguments (no copy, nothing
// whose lifetime a later call could end): kListMax indices per launch, longer
// lists take several launches.
constexpr int kListMax = 256;
struct IdList {
  int n;
  int id[kListMax];
};

constexpr int kVadmStateWords = (int)(sizeof(VadmState) / 4);
constexpr int kVadmSegWords = (int)(sizeof(VadmSeg) / 4);
static_assert(sizeof(VadmState) % 16 == 0, "VadmState rows are copied as float4");
static_assert(sizeof(VadmSeg) % 4 == 0, "VadmSeg rows are copied as words");
static_assert(st::kWords % 64 == 0 && st::kPitch == 0 && kPitchBuf % 4 == 0 && st::kSyn % 4 == 0,
              "the state record's float4 parts");

// One stream's record in a blob, offsets in 32-bit words, every section a
// multiple of 4 words (16-byte accesses):
//   [0, kWords)                 the state record
//   o_ring + c * pend_pad       channel c's pending window part in sample order: the samples
//                               since the last completed window, pend = samples % fft_size of
//                               them (from the record's own counter), zeros after
//   o_mach[m]                   machine m: VadmState | long-term row [lt_pitch] |
//                               short-term [pad4(n_st)] | ratio [pad4(n_r)] |
//                               segments [pad4(6 * seg_cap)] (min(n_segs, seg_cap) stored, zeros after)
//   o_rs + c * rs_pad           a resampling engine only (rs_tail = K - 1 > 0): channel c's resampler
//                               tail, its last rs_tail input samples, zeros after
//                               (per-stream rates: rs_tail = rs::kMaxTail, the stream's own K - 1 at
//                               the front of each, and 4 words behind the last: the stream's rate,
//                               then zeros -- o_rate, written and read by the host)
//   o_ro + c * ro_pad           an engine with denoised_rate only (ro_tail = K - 1 > 0), behind the
//                               input tails: channel c's output resampler tail, its last ro_tail
//                               denoised samples, zeros after
//                               (per-stream denoised rates: ro_tail = rs::kMaxTailOut, the row's last
//                               287 48 kHz denoised samples as on the device, and 4 words behind the
//                               last: the stream's denoised rate, then zeros -- o_orate, written and
//                               read by the host)
struct BlobLayout {
  int n_channels, n_mach, seg_cap, fft_size, use_denoiser, rs_tail, ro_tail;
  long long pend_pad, o_ring, o_mach[kMaxBandCfg], rs_pad, o_rs, ro_pad, o_ro, words;
  long long o_rate;   // per-stream rates only (0 otherwise)
  long long o_orate;  // per-stream denoised rates only (0 otherwise)
};
constexpr long long pad4(long long x) { return (x + 3) & ~3LL; }
inline BlobLayout blob_layout(int n_channels, int fft_size, int use_denoiser, const VadmArgs &v, int seg_cap,
                              int rs_tail = 0, int ro_tail = 0, bool rs_rate = false, bool ro_rate = false) {
  BlobLayout L{};
  L.n_channels = n_channels;
  L.n_mach = v.n;
  L.seg_cap = seg_cap;
  L.fft_size = fft_size;
  L.use_denoiser = use_denoiser;
  L.pend_pad = pad4((long long)fft_size - 1);
  L.o_ring = st::kWords;
  long long o = L.o_ring + (long long)n_channels * L.pend_pad;
  for (int m = 0; m < v.n; m++) {
    L.o_mach[m] = o;
    o += kVadmStateWords + pad4(v.c[m].lt_pitch) + pad4(v.c[m].n_st) + pad4(v.c[m].n_r) +
         pad4((long long)kVadmSegWords * seg_cap);
  }
  L.rs_tail = rs_tail;
  L.rs_pad = pad4(rs_tail);
  L.o_rs = o;
  o += (long long)n_channels * L.rs_pad;
  if (rs_rate) {
    L.o_rate = o;
    o += 4;
  }
  L.ro_tail = ro_tail;
  L.ro_pad = pad4(ro_tail);
  L.o_ro = o;
  o += (long long)n_channels * L.ro_pad;
  if (ro_rate) {
    L.o_orate = o;
    o += 4;
  }
  L.words = o;
  return L;
}

// k_stream_clear: which words of the state record a launch clears
enum ClearMode {
  kClearAll = 0,   // the whole record and the ring rows (fused engines, use_denoiser = 0)
  kClearMain = 1,  // every word but st::kPitch / st::kHp, and the ring rows (the engine stream's kernels own them)
  kClearPrep = 2,  // st::kPitch and st::kHp only (k_prep3's, on the prep stream)
};
struct ClearArgs {
  float *state, *ring;
  int ring_len, n_channels, mode;
  IdList ids;
};
struct VClearArgs {
  VadmArgs vadm;
  int n_streams;
  VadmState init[kMaxBandCfg];  // a machine's state after fvad_engine_reset (with vadm.tab: a fresh
                                //   machine of the stream's own row instead, vadm_fresh)
  IdList ids;
};

// A freshly constructed machine of a row's config (fvad_vadm_derive's s0: the
// long-term RollingAverage full of the initial average when there is one),
// keeping what outlives the machine: the stream's window count, so window
// sample indices continue, and the segments emitted so far.
// (the row's has_init, n_lt and lt0 by value: a kernel reads them where the
// row lies, in the table or in its argument block, and keeps no copy of it)
__host__ __device__ inline VadmState vadm_fresh(int has_init, int n_lt, double lt0, unsigned long long windows_done,
                                                unsigned n_segs) {
  VadmState S{};
  S.windows_done = windows_done;
  S.n_segs = n_segs;
  if (has_init) {
    S.lt_count = (unsigned)n_lt;
    S.lt_last = lt0;
    S.lt_has = 1;
    S.lt_pre_ok = 1;
  }
  return S;
}

// k_vadm_retarget (fvad_engine_set_stream_vadm): machine `machine` of the
// listed streams becomes a fresh machine of row[i].  The rows travel in the
// argument block like the stream lists above: kRetargetMax per launch.
constexpr int kRetargetMax = 47;  // (48 rows of 80 bytes and their ids would be 4112 bytes)
struct RetargetArgs {
  VadmState *st;  // [m][stream]
  float *buf;
  VadmRow *tab;   // [m][stream]
  int n_streams, machine, n;
  int lt_pitch, n_st, n_r;  // the machine's room: what is cleared
  long long lt_off, st_off, r_off;
  int id[kRetargetMax];
  VadmRow row[kRetargetMax];
};
static_assert(sizeof(RetargetArgs) <= 4096, "kernel argument block");
struct XferArgs {
  float *state, *ring;
  int ring_len, n_streams;
  VadmArgs vadm;
  BlobLayout lay;
  float *blob;        // device staging: records of lay.words each
  float *rs_tails;    // [s][c][lay.rs_tail], a resampling engine's (fvad_resample.h)
  float *ro_tails;    // [s][c][lay.ro_tail], of an engine with denoised_rate (fvad_resample_out.h)
  IdList slots, recs;  // stream slots[i] <-> record recs[i]
};

hipError_t launch_stream_clear(const ClearArgs &a, hipStream_t stream);
hipError_t launch_stream_vclear(const VClearArgs &a, hipStream_t stream);
hipError_t launch_vadm_retarget(const RetargetArgs &a, hipStream_t stream);
hipError_t launch_stream_gather(const XferArgs &a, hipStream_t stream);
hipError_t launch_stream_scatter(const XferArgs &a, hipStream_t stream);

}  // namespace fvad
