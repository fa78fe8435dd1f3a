// The batched engine's private parts: struct fvad_engine and the functions its
// translation units share (fvad_engine.cpp, fvad_engine_create.cpp,
// fvad_engine_ingest.cpp, fvad_engine_rates.cpp, fvad_engine_vadm.cpp,
// fvad_engine_events.cpp, fvad_engine_lifecycle.cpp, fvad_capture_host.cpp).
// The engine's subsystems each have one owner, a struct of namespace eng:
// Capture, Resample / ResampleOut with their RatePlan, Vadm, EventFeed and
// Staged; their timing samples are Timers.
// Host code only: not installed, and no .hip file includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <deque>
#include <memory>
#include <string>
#include <vector>

#include "../../include/fvad.h"
#include "fvad_hip_own.h"
#include "fvad_capture.h"
#include "fvad_internal.h"
#include "fvad_kernels.h"
#include "fvad_lifecycle.h"
#include "fvad_machine.h"
#include "fvad_resample.h"
#include "fvad_resample_out.h"
#include "fvad_staged.h"

#define HIP_TRY(expr)                                                                                             \
  do {                                                                                                            \
    hipError_t e_ = (expr);                                                                                       \
    if (e_ != hipSuccess) return fvad::eng::fail(FVAD_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

namespace fvad {
namespace eng {

inline int fail(int code, const std::string &msg) { return set_error(code, msg); }
// the GRU stack on the matrix cores (configs[4]): split (k_pspecw + k_gru16) or fused (k_fused16)
inline bool fp16_mode(int mode) { return mode == FVAD_MODE_FP16 || mode == FVAD_MODE_FP16_FUSED; }
// want_denoised = 2 keeps the denoised rows on the device (for a capture of
// them): computed as with 1, never copied to the host, no pinned slot buffer
inline bool denoised_to_host(const fvad_engine_config &c) { return c.want_denoised && c.want_denoised != 2; }
// a cross-stream wait (skipping the ones already complete measured no gain:
// DESIGN §8 r4)
inline hipError_t wait_event(hipStream_t stream, hipEvent_t ev) { return hipStreamWaitEvent(stream, ev, 0); }

// A begin / end event pair round work on one stream, read without waiting:
// collect adds the sample once its end event has completed and leaves it
// pending otherwise.  A begin over an unread sample drops that sample.
struct EventTimer {
  event_ptr ev[2];
  bool pending = false;
  int create() {
    for (event_ptr &x : ev)
      if (!x)
        if (const int rc = make_event(x, true)) return rc;
    return FVAD_OK;
  }
  int begin(hipStream_t s) {
    pending = false;
    HIP_TRY(hipEventRecord(ev[0].get(), s));
    return FVAD_OK;
  }
  int end(hipStream_t s) {
    HIP_TRY(hipEventRecord(ev[1].get(), s));
    pending = true;
    return FVAD_OK;
  }
  int collect(double &ms_sum, int &n) {
    if (!pending || hipEventQuery(ev[1].get()) != hipSuccess) return FVAD_OK;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0].get(), ev[1].get()));
    ms_sum += ms;
    n++;
    pending = false;
    return FVAD_OK;
  }
};

// N EventTimers and the samples read from them, by kind: each of the K kinds
// has its own sum and count, and end() names the kind of the sample its slot
// brackets.  What becomes of a sample that is unread when its slot comes up
// again is the caller's: begin alone drops it, collect(slot) ahead of begin
// keeps it if it is complete.
template <int N, int K = 1>
struct Timers {
  EventTimer tm[N];
  int kind[N] = {};
  double ms_sum[K] = {};
  int n_timed[K] = {};
  // the events of n slots from slot `first` on (a slot that has them keeps them)
  int create(int first = 0, int n = N) {
    for (int i = first; i < first + n; i++)
      if (const int rc = tm[i].create()) return rc;
    return FVAD_OK;
  }
  int begin(int slot, hipStream_t s) { return tm[slot].begin(s); }
  int end(int slot, hipStream_t s, int k = 0) {
    kind[slot] = k;
    return tm[slot].end(s);
  }
  // never waits: a sample whose end event has not completed stays pending
  int collect(int slot) { return tm[slot].collect(ms_sum[kind[slot]], n_timed[kind[slot]]); }
  int collect() {
    for (int i = 0; i < N; i++)
      if (const int rc = collect(i)) return rc;
    return FVAD_OK;
  }
  // the round-robin use: the slot after `slot` keeps what it held if that is
  // complete, then begins
  int begin_next(int &slot, hipStream_t s) {
    slot = (slot + 1) % N;
    if (const int rc = collect(slot)) return rc;
    return begin(slot, s);
  }
  void drop() {
    for (EventTimer &t : tm) t.pending = false;
  }
  void read(int k, double *ms_avg, int *n_runs) const {
    *ms_avg = n_timed[k] ? ms_sum[k] / n_timed[k] : 0.0;
    if (n_runs) *n_runs = n_timed[k];
  }
  void clear() {
    for (int k = 0; k < K; k++) ms_sum[k] = 0, n_timed[k] = 0;
  }
};

// FNV-1a (64 bit), the hash of a stream blob's compatibility fields
constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull;
inline uint64_t fnv1a(uint64_t h, const void *p, size_t n) {
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
  return h;
}

}  // namespace eng
}  // namespace fvad

// Clip capture (fvad_engine_enable_capture; DESIGN.md section 7, "Clip
// capture"): everything it owns, made by the enabling call; an engine without
// capture has none of it.
namespace fvad {
namespace eng {
struct Capture {
  int machine = 0;
  // What is recorded and how it is delivered (fvad_capture_config).  A
  // capture of the denoised rows counts samples of the clip rate `rate` =
  // 48000 L / M everywhere below (history, H, the positions, the pool), has
  // `frame` = rate / 100 of them per tick, and appends on the engine stream.
  int source = FVAD_CLIP_SOURCE_INPUT, format = FVAD_CLIP_F32;
  int rate = 48000, frame = kFrame;
  unsigned L = 1, M = 1;
  unsigned long long history = 0, H = 0;
  size_t pool_cap = 0, desc_cap = 0;
  pinned_ptr<int16_t> pool16;         // the pool of an s16 capture (pool is null then)
  int16_t *dv_pool16 = nullptr;
  dev_ptr<float> hist;                // [s][c][H]
  dev_ptr<CapPos> pos, snap[2];       // the appending stream's positions; their value after the push of each parity
  dev_ptr<cap::Pend> pend;            // [s][cap::kQueue]
  dev_ptr<unsigned> pend_n;           // [s]
  dev_ptr<CapState> state;
  dev_ptr<CapWork> work;              // [cap::kQueue * n_streams]
  dev_ptr<unsigned char> flush;       // [s] fvad_engine_capture_flush's list
  pinned_ptr<float> pool;             // written by the device through dv_pool
  float *dv_pool = nullptr;
  pinned_ptr<fvad_clip> desc;
  CapClip *dv_desc = nullptr;
  // header slots: a push's pass writes slot pass % kEvHeaders (the event
  // feed's pass ordinal: events_retire reads both), a flush the last one
  pinned_ptr<CapHeader> hdr;
  CapHeader *dv_hdr = nullptr;
  // behind the capture pass of the push of each parity: the next append of
  // that parity waits for it (it rewrites the ring words and the snapshot
  // that pass read)
  event_ptr ev_pass[2];
  uint64_t desc_read = 0, desc_end = 0, pool_read = 0, pool_end = 0, lost = 0;
  // slots [0, 2): k_hist_append by push parity, kind kAppend; kPassSlot +
  // the machines' timer slot: the pass, kind kPass
  enum { kAppend = 0, kPass = 1, kPassSlot = 2 };
  Timers<4, 2> tm;
};

// Per-stream rates of either resampler (input_rate = FVAD_INPUT_RATE_PER_STREAM,
// denoised_rate = FVAD_DENOISED_RATE_PER_STREAM; DESIGN.md section 7,
// "Per-stream rates"): each stream's rate, the layout of a packed push and the
// device tables a push's launches read.  Empty (on() false) on a fixed-rate
// engine.  fvad_engine_rates.cpp.
struct RatePlan {
  int n_streams = 0, n_channels = 0, rate_max = 0;
  rs::Desc dr[rs::kPsRates]{};          // by rate index (48000: the identity)
  dev_ptr<float> taps_r[rs::kPsRates];  // the tables of the rates up to rate_max (none at 48000)
  // what the next submitted push uses: each stream's rate index, the layout
  // (fvad_input_layout) and the streams by rate; gen counts their changes
  std::vector<int> ridx, lists;
  std::vector<long long> offsets;  // [B + 1]
  int list_at[rs::kPsRates + 1] = {};
  uint64_t gen = 1;
  // The device tables, [offsets (B + 1) | rate_idx (B) | lists (B)] (the
  // latter two as int), in one or two copies -- the input side keeps one per
  // raw buffer parity, the output side one -- and the generation each holds.  A
  // push that finds its copy stale (sync) copies it from the next pinned
  // staging row on its stream, ahead of its launches: stream order keeps an
  // in-flight push's tables until its kernels are done.  stage_ev[i]: the
  // copy out of row i, waited for only should the ring come round to a row
  // whose copy has not run (more than kStage table copies queued: not with
  // submit / collect, FVAD_MAX_IN_FLIGHT pushes deep)
  static constexpr int kStage = 8;
  dev_ptr<long long> tab[2];
  uint64_t tab_gen[2] = {0, 0};
  pinned_ptr<long long> stage;
  event_ptr stage_ev[kStage];
  bool stage_used[kStage] = {};
  int stage_next = 0;

  bool on() const { return rate_max != 0; }
  size_t tab_words() const { return offsets.size() + (offsets.size() - 1); }  // (2 B ints are B words)
  int frame(int s) const { return dr[ridx[s]].n; }
  int rate(int s) const { return dr[ridx[s]].rate; }
  long long tick_len() const { return offsets.back(); }
  // fvad_engine_create's part: the descriptions and device tap tables of the
  // rates up to rate_max, every stream at rate_max, n_tab copies of the
  // device tables and the staging ring
  int make(rs::Dir dir, int n_streams, int n_channels, int rate_max, int n_tab);
  // the layout and the lists of the current ridx (gen advances)
  void relayout();
  // a change of rates in two steps, so that a caller can stand between them:
  // check that each of n rates is a listed rate or 48000 up to rate_max
  // (FVAD_ERATE with bad_rate otherwise), then streams[i] takes rates[i]
  int check(int n, const int *rates, const char *bad_rate) const;
  void apply(const int *streams, int n, const int *rates);
  // copy `copy` of the device tables follows the host's, on stream st
  int sync(int copy, hipStream_t st);
  // a push's tables: copy `copy` on the device, the rest by value
  void fill(PsTables &t, int copy) const;
  // a stream blob's rate word of a stream, and a restored one's rate index:
  // 0, 1 off the list, 2 above rate_max
  uint32_t save_rate(int stream) const { return (uint32_t)rate(stream); }
  int check_restored_rate(uint32_t word, int *ri) const;
};

// Input resampling (fvad_engine_config.input_rate; DESIGN.md section 7, "Input
// resampling"): everything it owns, made by fvad_engine_create; an engine of
// 48 kHz input has none of it.
struct Resample {
  rs::Desc d{};           // fixed rate; empty with per-stream rates, as taps
  dev_ptr<float> taps;    // [L][K]
  // [s][c][K - 1], per-stream rates: [s][c][rs::kMaxTail]; the prep stream's
  // (fused: the engine stream's)
  dev_ptr<float> tails;
  // the push as the host sent it, float or int16: the parity of d_pcm_b,
  // released by the same ev_in_free (recorded behind the reader of d_pcm,
  // which is behind k_resample)
  dev_ptr<float> raw[2];  // max_ticks * B * C * (rate or rate_max) / 100 words each
  bool in16 = false;      // the push being launched holds int16 samples
  Timers<2> tm;           // the resample launches of a push, taken in turn (tm_slot)
  int tm_slot = 0;
  RatePlan plan;          // per-stream rates; tables by raw buffer parity
};

// The denoised PCM at another rate (fvad_engine_config.denoised_rate;
// DESIGN.md section 7, "Output rate of the denoised PCM"): everything it owns,
// made by fvad_engine_create; an engine that returns the 48 kHz signal has
// none of it.  All of it is the engine stream's.
struct ResampleOut {
  rs::Desc d{};          // fixed rate; empty with per-stream rates, as taps
  dev_ptr<float> taps;   // [L][K]
  // [s][c][K - 1]; per-stream rates: [s][c][rs::kMaxTailOut], a row's last
  // 48 kHz denoised samples whatever its rate
  dev_ptr<float> tails;
  // d_den_out: [tick][s][c][n], max_ticks ticks; per-stream rates: packed
  // [tick][s][c][rate(s) / 100], max_ticks * B * C * rate_max / 100 words
  dev_ptr<float> out;
  Timers<4> tm;          // the launches of a push, taken in turn (tm_slot): three pushes in flight and their copies
  int tm_slot = 0;
  RatePlan plan;         // per-stream rates; one copy of the tables
  // a tick's length of the push launched last: what fetch and the D2H copies
  // of that push move (the layout may have changed since)
  long long pushed_len = 0;
};
// One set of a push's window outputs
struct WinOut {
  dev_ptr<int> flag;
  dev_ptr<float> ratio, vad, band;
};

// The device VADMachines (fvad_engine_attach_vadm / attach_vadm_ex; DESIGN.md
// section 7): everything they own, made by the attaching call in a local Vadm
// that is move-assigned into the engine once nothing can fail any more.  Held
// by value: args goes by value into every argument block, and the test hooks
// (par_serial_every, defer_max, always_par) may be set before the attach, which
// carries them over.  fvad_engine_vadm.cpp.
struct Vadm {
  VadmArgs args{};  // its pointers are views of the owners below (ev_stage / ev_count: the feed's)
  dev_ptr<VadmState> st;
  dev_ptr<float> buf;
  dev_ptr<VadmSeg> seg;
  dev_ptr<unsigned long long> count;  // FVAD_DEBUG_VADM_COUNT
  // Window outputs of push k in set k & 1: set 0 is the engine's own, set 1
  // exists with the machines (without them every push writes set 0).
  // k_vadm_hbm of push k reads set k & 1 in place, push k + 2 rewrites it
  // after that pass (ev_set_free).  vticks: the pass's copy of the push's ticks.
  WinOut set1;
  dev_ptr<int32_t> vticks[2];
  event_ptr ev_done, ev_set_free[2];  // behind the pass queued last; behind the last pass of each parity
  // The VADMachine of push k is enqueued when the next push is launched, as
  // k_vadm_hbm (32 waves, overlapping that push quietly: the 512-wave burst of
  // k_vadm_par beside the next push's k_fftAw cost more than it saved,
  // measured), or at a sync point with nothing else queued as k_vadm_par
  // (0.25 ms instead of 1.45: the drain of a job's last push).
  bool pend = false, pend_timed = false;
  int pend_b = 0;
  StagedArgs pend_args{};
  uint64_t pend_push = 0;  // the pending pass's push (fvad_engine::push_count)
  // a non-final k_vadm_hbm was queued last (its machines may owe their
  // long-term fold): a sync point with no push pending resolves it with a
  // resolve-only pass (owed_args: that launch's argument block)
  bool owed = false;
  StagedArgs owed_args{};
  // VADMachine timing never blocks the host (it would serialise the overlap):
  // two timers alternate (slot) and are read once complete.  By kernel: kind 0
  // k_vadm_hbm (steady state), kind 1 k_vadm_par (a push flushed at a sync point)
  Timers<2, 2> tm;
  int slot = 0;
  bool always_par = false;  // test hook FVAD_DEBUG_VADM_ALWAYS_PAR
  bool lt_full = false;     // test hook FVAD_DEBUG_VADM_LT_FULL
  std::vector<fvad_vadm_config> cfgs;  // the attached machines' configs (hashed into a stream blob's header)
  std::vector<VadmState> init;         // [m][stream] initial states
  size_t buf_len = 0;
  // Per-stream configs (fvad_engine_attach_vadm_ex): the
  // device table args.tab [m][stream] and its host mirror -- the rows, the
  // configs they came from, and init above, which then holds each stream's own
  // fresh machine.  args.c[m] carries the room's lengths (the buffers'
  // layout).  nopar: rows without an initial average; while there is one, sync
  // points run k_vadm_hbm_ps (launch_vadm).
  bool ps = false;
  dev_ptr<VadmRow> tab;
  std::vector<VadmRow> rows;
  std::vector<fvad_vadm_config> stream_cfgs;
  size_t nopar = 0;

  bool on() const { return args.n > 0; }
};

// Speech event feed (fvad_engine_enable_events):
// everything it owns, made by the enabling call in a local EventFeed and
// move-assigned like Vadm (chunk may be set before).  The machine kernels stage
// events per lane in HBM (stage), k_vadm_events packs them behind each pass
// into a ring in pinned host memory and writes the pass's header slot there;
// flight holds, oldest first, the passes whose `done` event (recorded behind
// k_vadm_events) has not been seen complete yet.  poll_events reads the ring
// only up to the end cursor of the last retired pass: the host never looks at
// ring or header bytes of a pass before its event has completed (an event's
// completion releases the kernel's stores to the system, whichever coherence
// the allocation has).  fvad_engine_events.cpp.
constexpr int kEvHeaders = 64;  // header slots: passes in flight at most (an older one is waited for)
struct EventFeed {
  struct Pass {
    uint64_t pass, push;
    event_ptr done;
  };
  dev_ptr<VadmEvRec> stage;            // Vadm::args.ev_stage
  dev_ptr<unsigned> count;             // Vadm::args.ev_count
  dev_ptr<unsigned long long> cursor;  // device: [0] write cursor, [1] lost
  pinned_ptr<fvad_event> ring;         // written by the device through dv_ring
  VadmEvent *dv_ring = nullptr;
  pinned_ptr<VadmEventHeader> hdr;  // [kEvHeaders], slot pass % kEvHeaders
  VadmEventHeader *dv_hdr = nullptr;
  size_t ring_cap = 0;
  uint64_t read = 0, end = 0, lost = 0;  // host read cursor; ring valid up to end; lost so far
  uint64_t pass_next = 0;
  uint64_t pushes_done = 0;  // pushes up to here have every event in the ring's valid part
  std::deque<Pass> flight;
  std::vector<event_ptr> pool;  // retired passes' events, re-used
  Timers<2> tm;                 // k_vadm_events' samples, by the machines' timer slot
  int chunk = 0;                // test hook FVAD_DEBUG_EVENTS_CHUNK

  bool on() const { return ring_cap > 0; }
};

// The staged pipeline (every mode but FVAD_MODE_FUSED): its intermediates,
// the double-buffered arrays and the events that order a push's parts, made by
// staged_make (fvad_engine_create.cpp); a fused engine has none of it.
struct Staged {
  int V = 0, L = 0, LX = 0, wmax = 0, grid_frames = 0;
  dev_ptr<float> d_X, d_P, d_Ex, d_Ep, d_Exp, d_Lyf, d_f34, d_rec, d_ptile, d_vadf, d_ys, d_gr, d_gs;
  dev_ptr<int> d_sil, d_pitch, d_wtick;
  dev_ptr<long long> d_wstart;
  dev_ptr<unsigned> d_work;  // persistent-kernel group counters
  // k_fftb's scratch (FFT B above kMaxFftB)
  dev_ptr<float2> d_fbwork;
  int fb_work_blocks = 0;
  long long fb_work_stride = 0;
  // xs / xlp / ratio / ticks are double-buffered: push k uses buffer k & 1,
  // reused once the push that used it last has finished (ev_buf_free[b]).
  // (ratio and ticks: fvad_engine::d_ratio_b / d_ticks_b, whose buffer 0 a
  // fused engine has too.)  d_xs: the buffer of the latest push (a view)
  dev_ptr<float> d_xs_b[2], d_xlp_b[2];
  float *d_xs = nullptr;
  event_ptr ev_prep_done[2], ev_buf_free[2];
  bool buf_busy[2] = {false, false};
  int next_buf = 0;
  // the last push's k_fftAw done: push k's k_prep3 starts once push k-1's
  // k_fftAw has finished, so it runs beside k_plpc / k_pcorr instead (measured:
  // k_fftAw 0.64 -> 0.57, k_plpc 0.48 -> 0.40, k_pcorr 1.18 -> 1.24 ms, push
  // 5.00 -> 4.90 ms; started after k_plpc it overruns into k_rnn3: 5.93 ms)
  event_ptr ev_fft_a;
  bool fft_a_rec = false;
  // push k's k_fftAw runs on pstream (after its k_prep3) once push k-1's
  // k_synthw, the last reader of what it writes, is done (ev_synth): beside
  // push k-1's k_olafb instead of after it (push 4.87 -> 4.78 ms)
  event_ptr ev_synth;
  bool synth_rec = false;
  hipEvent_t synth_wait = nullptr;  // the last push's k_synthw-end event: ev_synth, or ev[kEvSynthEnd] in a timed push (a view)
};
}  // namespace eng
}  // namespace fvad

struct fvad_engine {
  // Ownership: every allocation, event and stream has exactly one owning
  // member (fvad_hip_own.h); raw pointers beside them are views.  Members are
  // destroyed in reverse order of declaration, so the streams come first
  // here: every buffer and event is released before any stream, and the
  // engine stream goes last (fvad_engine_destroy synchronises them before).
  fvad::stream_ptr stream;
  // H2D copies of the streaming ingest, created on first use (ensure_slots)
  fvad::stream_ptr cstream;
  // staged mode: k_prep3 runs on pstream, so push k's prep overlaps push k-1's
  // kernels.  k_vadm_hbm runs on the side stream over one push's window
  // outputs, overlapped with the next push (it only depends on its own state).
  // Engines of one GPU may share either (fvad_engine_share_streams): the last
  // owner destroys the stream; pstream / side are the streams in use.
  std::shared_ptr<ihipStream_t> pstream_ref, side_ref;
  hipStream_t pstream = nullptr, side = nullptr;

  fvad_engine_config cfg{};
  int ring_len = 0;
  fvad::dev_ptr<fvad::Plan> d_plan;
  fvad::dev_ptr<float> d_weights;
  fvad::DevModel dmodel{};
  fvad::dev_ptr<fvad::DevModel> d_model;
  fvad::dev_ptr<float> d_state, d_ring, d_xbuf, d_vad, d_den;
  fvad::dev_ptr<int8_t> d_rnn_img;
  fvad::dev_ptr<uint16_t> d_gru16;  // FVAD_MODE_FP16: MFMA weight fragments (f16 bits)
  fvad::dev_ptr<float> d_gru16_bias;
  // ratio / ticks of a push: buffer 0, and on a staged engine buffer 1 for
  // the pushes of odd parity (eng::Staged).  d_ratio, d_ticks: the buffer of
  // the latest push (views)
  fvad::dev_ptr<float> d_ratio_b[2];
  fvad::dev_ptr<int> d_ticks_b[2];
  float *d_ratio = nullptr;
  int *d_ticks = nullptr;
  // the staged pipeline: null on a fused engine
  std::unique_ptr<fvad::eng::Staged> sg;
  // Window-output set 0 (set 1: eng::Vadm).  d_wflag / d_wratio / d_wvad /
  // d_band: the latest push's set (views).
  fvad::eng::WinOut wout0;
  int *d_wflag = nullptr;
  float *d_wratio = nullptr, *d_wvad = nullptr, *d_band = nullptr;
  // device VADMachines (fvad_engine_attach_vadm): vadm.on() once attached
  fvad::eng::Vadm vadm;
  // speech event feed (fvad_engine_enable_events): feed.on() once enabled
  fvad::eng::EventFeed feed;
  uint64_t push_count = 0;  // pushes launched since create / reset
  // test hook (fvad_engine_output_log): the per-tick outputs of the next
  // log_cap pushes, copied on the engine stream as each push ends
  fvad::dev_ptr<float> d_log;
  int log_cap = 0, log_n = 0;
  size_t log_stride = 0;
  std::vector<int> log_ticks;
  int rnn_act[fvad::rnnimg::kMats] = {};
  int wpt = 1;  // window slots per (tick, stream): windows_per_tick(fft_size)
  // FFT B above kMaxFftB: tables [tw | sup | hann | perm]
  fvad::dev_ptr<float> d_fbtab;
  // Window spectra (fvad_engine_config.want_spectrum; DESIGN.md section 7,
  // "Window spectra and band sweeps"): the last launched push's,
  // [max_ticks][streams][wpt][channels][n_spec]; null without the tap.
  // last_ticks: that push's ticks (what fvad_engine_fetch_spectrum may read)
  fvad::dev_ptr<float> d_spec;
  int n_spec = 0, last_ticks = 0;
  int resident_ticks = 0;
  int n_kernels = 0;
  fvad::StagedKernels kernels{};  // not fused: the kernels of a push and their timing events (n_kernels of them)
  // per-kernel timing events, two sets used alternately so the host reads
  // push k's events while push k+1 is already queued (no launch gap).  The
  // launchers take hipEvent_t *: evs holds the handles evs_own owns
  fvad::event_ptr evs_own[2][FVAD_MAX_TIMES];
  hipEvent_t evs[2][FVAD_MAX_TIMES] = {};
  hipEvent_t *ev = evs[0];
  int n_events = 0;    // timing events per launch
  int last_event = 0;  // the one recorded last (the launch's end)
  int ev_slot = 0;
  bool slot_pending[2] = {false, false};
  double ms_sum[FVAD_MAX_TIMES] = {};
  int n_timed = 0;
  int res_count = 0;  // run_resident calls since the last clear_times (event sampling)
  int raw_s16 = 0;    // rnnoise compat mode (s16-scaled I/O)
  fvad::dev_ptr<unsigned long long> d_stamps;  // diagnostic stamp buffer (FVAD_STAMPS builds)
  // Device inputs alternate by push (d_pcm: the current one, a view): the
  // input of push k+1 may be copied in while push k's k_prep3 still reads
  // its own.  ev_in_free[i]: buffer i's last reader (k_prep3 / k_prep) done.
  // run_resident reads d_pcm_b[0] (fvad_engine_load_synthetic).
  fvad::dev_ptr<float> d_pcm_b[2];
  float *d_pcm = nullptr;
  // fvad_engine_load_synthetic_ex with n_pushes > 1: [push][tick][stream][ch][480]
  fvad::dev_ptr<float> d_res;
  int res_pushes = 0, res_next = 0;
  fvad::event_ptr ev_in_free[2];
  bool in_busy[2] = {false, false};
  int in_next = 0;
  // Streaming ingest (fvad_engine_submit / collect): pinned host input slots
  // and output slots per in-flight push (kSlots = FVAD_MAX_IN_FLIGHT), H2D
  // copies on cstream.  Allocated on first use.  With three pushes in
  // flight the H2D of push k + 2 waits only for its device input buffer, free
  // once push k's k_prep3 has read it -- not for push k's outputs.
  struct Slot {
    fvad::pinned_ptr<float> in;       // [max_ticks][B][C][480]
    fvad::pinned_ptr<int16_t> in16;   // 16-bit input slot (fvad_engine_input_slot_i16; on first use)
    fvad::pinned_ptr<int32_t> ticks;  // [B]
    // outputs of the push that used this slot
    fvad::pinned_ptr<float> vad, ratio, wratio, wvad, band, den;
    fvad::pinned_ptr<int32_t> wflag;
    fvad::event_ptr h2d, done;
    bool h2d_busy = false, pending = false;
    int n_ticks = 0;
    size_t den_floats = 0;  // the denoised floats of the push in den (per-stream rates: in its own layout)
  } slots[FVAD_MAX_IN_FLIGHT];
  int sub_next = 0, col_next = 0;
  // device staging of a 16-bit submit that k_pcm16 converts into d_pcm: fused
  // and no-denoiser engines, and the rnnoise compat mode (raw_s16)
  fvad::dev_ptr<int16_t> d_pcm16;
  // this push's input is 16-bit samples in d_pcm's buffer, read by k_prep3
  // itself (staged engines with the denoiser: no d_pcm16, no k_pcm16)
  bool pcm16_push = false;
  // per-stream lifecycle (fvad_engine_reset_streams / save_streams / restore_streams)
  uint64_t model_hash = 0;      // of the model's int8 arrays (a blob's compatibility check)
  fvad::dev_ptr<float> d_blob;  // device staging of a save / restore, grown on demand
  size_t blob_cap = 0;          //   (bytes)
  // test hook FVAD_DEBUG_RESET_TIMES: timers round the launches of
  // fvad_engine_reset_streams (kind and slot within a call: 0 engine stream,
  // 1 prep stream, 2 side stream), kRtSlots calls deep (slot 3 * call + kind,
  // their events made on first use), read at fvad_engine_reset_times
  static constexpr int kRtSlots = 64;
  bool dbg_reset_times = false;
  fvad::eng::Timers<3 * kRtSlots, 3> rt;
  int rt_next = 0;
  // input resampling (input_rate set): null on an engine of 48 kHz input
  std::unique_ptr<fvad::eng::Resample> rs;
  // the denoised PCM at another rate (denoised_rate set): null otherwise
  std::unique_ptr<fvad::eng::ResampleOut> ro;
  // clip capture, last: released before everything it refers to
  std::unique_ptr<fvad::eng::Capture> cap;
};

namespace fvad {
namespace eng {

// fvad_engine.cpp
int launch(fvad_engine *e, int n_ticks, bool use_ticks, bool timed, bool use_tail = false);
int fetch(fvad_engine *e, int n_ticks, fvad_outputs *o);
void fill_bands(const fvad_engine_config &c, int *band_lo, int *band_hi, int *lo_all, int *hi_all);
void use_win_out(fvad_engine *e, int b);
// fvad_engine_create.cpp
int make_win_out(const fvad_engine *e, WinOut &w);
// fvad_engine_ingest.cpp: the device input buffers
hipStream_t input_reader(const fvad_engine *e);
int input_buffer(fvad_engine *e, hipStream_t cs);
int release_input(fvad_engine *e);
int check_ticks(const fvad_engine *e, const int32_t *ticks_valid, int n_ticks);
int tail_ticks(const fvad_engine *e, const int32_t *ticks_valid, const int32_t *last, int n_ticks,
               std::vector<int32_t> &tt);
// fvad_engine_rates.cpp: the two resamplers' host side.  Input: samples per
// tick and channel of a push, where its H2D copy goes, the stream that owns
// the tails, and the push's resample launches
int input_frame(const fvad_engine *e);
// per-stream rates: the largest frame (what the staging is sized by) and the
// samples of a push of n_ticks in the current layout
int input_frame_max(const fvad_engine *e);
size_t push_samples(const fvad_engine *e, int n_ticks);
void *input_target(const fvad_engine *e);
hipStream_t resample_stream(const fvad_engine *e);
int resample_make(fvad_engine *e, const rs::Desc &d, int rate_max);
int resample_push(fvad_engine *e, int n_ticks, const int *d_ticks);
// the denoised PCM at another rate: samples per tick and channel of the
// denoised rows the host receives, the device rows they are copied from, and
// the push's launches on the engine stream (behind its last writer of d_den)
int denoised_frame(const fvad_engine *e);
const float *denoised_source(const fvad_engine *e);
// per-stream denoised rates: the largest frame (what the slots are sized by)
// and the denoised floats of the push launched last (n_ticks of it)
int denoised_frame_max(const fvad_engine *e);
size_t denoised_floats(const fvad_engine *e, int n_ticks);
int resample_out_make(fvad_engine *e, const rs::Desc &d, int rate_max);
int resample_out_push(fvad_engine *e, int n_ticks, const int *d_ticks);
// words of a row's tail of either resampler: K - 1; rs::kMaxTail /
// rs::kMaxTailOut with per-stream rates
int resample_tail_words(const fvad_engine *e, rs::Dir dir);
// both resamplers' tails become zeros: every stream's on the engine stream
// (fvad_engine_reset), the listed streams' on the streams that own them
int resample_reset(fvad_engine *e);
int resample_reset_streams(fvad_engine *e, const IdList &ids);
// fvad_engine_vadm.cpp
int vadm_reset(fvad_engine *e);
int vadm_flush(fvad_engine *e, bool fast = true);
int collect_vadm_timing(fvad_engine *e);
// fvad_engine_events.cpp: k_vadm_events behind the machine pass just queued on
// the side stream, the feed as after enable, and the passes that have finished
int enqueue_events(fvad_engine *e, const VadmArgs &v, uint64_t push, int slot, bool timed);
int events_reset(fvad_engine *e);
int events_retire(fvad_engine *e, bool wait_oldest);
// fvad_capture_host.cpp
int capture_append(fvad_engine *e, const fvad::StagedArgs &a, int b, bool timed);
int capture_append_den(fvad_engine *e, const fvad::StagedArgs &a, int b, bool timed);
hipStream_t capture_appender(const fvad_engine *e);
int capture_pass(fvad_engine *e, const fvad::VadmArgs &v, uint64_t push, int b, int slot, bool timed);
int capture_retire(fvad_engine *e, uint64_t pass);
int capture_reset(fvad_engine *e);
int capture_set_streams(fvad_engine *e, const int32_t *streams, const uint64_t *samples, int n);
int capture_collect_timing(fvad_engine *e);
// fvad_engine_lifecycle.cpp: n distinct stream indices in range
int check_stream_list(const fvad_engine *e, const int32_t *streams, int n);

}  // namespace eng
}  // namespace fvad
