// Ownership of the batched engine's and the config sweep's GPU resources under
// allocation failure.
//
// Their real host translation units (fvad_engine*.cpp, fvad_sweep.cpp with
// fvad_machine.cpp, fvad_eval.cpp, fvad_model.cpp, fvad_plan.cpp,
// fvad_synth.cpp) linked against two stubs
// defined here, so the program needs no GPU:
//   - a HIP runtime on the heap: device and pinned memory from calloc, copies
//     are memcpy, events and streams are small heap objects, every query
//     succeeds, elapsed times are 0, one device.  It counts live device
//     allocations, pinned allocations, events and streams, refuses to release
//     what is not live, and can fail the k-th creating call;
//   - kernel launches: every fvad::launch_* and the host helpers the .hip
//     files define return at once, doing only what the host code reads back.
//
// One scenario walks every allocation site of an engine kind, the two
// resamplers' among them (a fixed-rate kind and a per-stream kind, whose rate
// plans, staging rings and tap tables it reaches).  Run without a
// failure it must leave nothing live and gives the number N of creating
// calls; then for every k < N the k-th creating call fails: the API call it
// fails in must report it, destroy must still release everything, and
// attach_vadm / enable_events must succeed when simply called again.  The
// sweep's scenario (run_sweep) does the same for a sweep.
//
// The scenario also pins two things the owners of the engine's subsystems must
// keep.  Test hooks set before attach_vadm / enable_events reach the launches
// after them: the launch stubs keep the last argument blocks they saw.  And
// every *_times entry point reports the runs it has (printed for the run
// without a failure; with every event query succeeding they are
// deterministic) and reads 0 after fvad_engine_clear_times.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../include/fvad.h"
#include "fvad_eval_core.h"
#include "fvad_lifecycle.h"
#include "fvad_kernels.h"
#include "fvad_machine.h"
#include "fvad_staged.h"
#include "fvad_sweep.h"

// ---------------------------------------------------------------------------
// stub HIP runtime
// ---------------------------------------------------------------------------
namespace {
std::set<void *> g_dev, g_pinned, g_events, g_streams;
long g_creates = 0;   // creating calls so far in this run
long g_fail_at = -1;  // the creating call to fail (-1: none)
int g_bad = 0;        // releases of something not live

bool refuse() { return g_creates++ == g_fail_at; }
hipError_t create(std::set<void *> &live, void **out, size_t bytes) {
  if (refuse()) return hipErrorOutOfMemory;
  *out = calloc(bytes ? bytes : 1, 1);
  live.insert(*out);
  return hipSuccess;
}
hipError_t release(std::set<void *> &live, void *p, const char *what) {
  if (!live.erase(p)) {
    std::printf("FAIL: %s of %p, which is not live\n", what, p);
    g_bad++;
    return hipErrorInvalidValue;
  }
  free(p);
  return hipSuccess;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t n) { return create(g_dev, p, n); }
hipError_t hipFree(void *p) { return p ? release(g_dev, p, "hipFree") : hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { return create(g_pinned, p, n); }
hipError_t hipHostFree(void *p) { return p ? release(g_pinned, p, "hipHostFree") : hipSuccess; }
hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned) {
  *dev = host;
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e) { return create(g_events, reinterpret_cast<void **>(e), 1); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) { return release(g_events, e, "hipEventDestroy"); }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { return g_events.count(e) ? hipSuccess : hipErrorInvalidHandle; }
hipError_t hipEventQuery(hipEvent_t e) { return g_events.count(e) ? hipSuccess : hipErrorInvalidHandle; }
hipError_t hipEventSynchronize(hipEvent_t e) { return hipEventQuery(e); }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b) {
  *ms = 0;
  return g_events.count(a) && g_events.count(b) ? hipSuccess : hipErrorInvalidHandle;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return create(g_streams, reinterpret_cast<void **>(s), 1); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned f, int) { return hipStreamCreateWithFlags(s, f); }
hipError_t hipStreamDestroy(hipStream_t s) { return release(g_streams, s, "hipStreamDestroy"); }
hipError_t hipStreamSynchronize(hipStream_t s) { return g_streams.count(s) ? hipSuccess : hipErrorInvalidHandle; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
  return g_streams.count(s) && g_events.count(e) ? hipSuccess : hipErrorInvalidHandle;
}
hipError_t hipDeviceGetStreamPriorityRange(int *lo, int *hi) {
  *lo = 0;
  *hi = -1;
  return hipSuccess;
}
hipError_t hipGetDeviceCount(int *n) {
  *n = 1;
  return hipSuccess;
}
hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : hipErrorInvalidDevice; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t *p, int) {
  std::memset(p, 0, sizeof(*p));
  p->multiProcessorCount = 4;
  return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory (injected)" : "stub error"; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) {
  std::memcpy(d, s, n);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t) { return hipMemcpy(d, s, n, k); }
hipError_t hipMemcpy2D(void *d, size_t dp, const void *s, size_t sp, size_t w, size_t h, hipMemcpyKind) {
  for (size_t r = 0; r < h; r++) std::memcpy(static_cast<char *>(d) + r * dp, static_cast<const char *>(s) + r * sp, w);
  return hipSuccess;
}
hipError_t hipMemset(void *d, int v, size_t n) {
  std::memset(d, v, n);
  return hipSuccess;
}
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { return hipMemset(d, v, n); }
}  // extern "C"

// ---------------------------------------------------------------------------
// stub kernel launches and the host helpers of the .hip files
// ---------------------------------------------------------------------------
namespace {
fvad::VadmArgs g_last_vadm{};             // what launch_vadm saw last
fvad::VadmEventArgs g_last_vadm_events{};  // what launch_vadm_events saw last
}  // namespace

namespace fvad {
hipError_t launch_prep(const PrepArgs &, hipStream_t) { return hipSuccess; }
hipError_t launch_frame(const FrameArgs &, hipStream_t) { return hipSuccess; }
hipError_t launch_prep(const StagedArgs &, hipStream_t, hipEvent_t *) { return hipSuccess; }
hipError_t launch_staged(const StagedArgs &, int, hipStream_t, hipEvent_t *, hipEvent_t, hipStream_t, hipEvent_t,
                         hipEvent_t) {
  return hipSuccess;
}
hipError_t launch_nodenoise(const StagedArgs &, int, hipStream_t) { return hipSuccess; }
hipError_t launch_pcm16(const int16_t *, float *, size_t, hipStream_t) { return hipSuccess; }
hipError_t launch_vadm(const StagedArgs &a, hipStream_t, bool fast, bool *ran_par) {
  g_last_vadm = a.vadm;
  if (ran_par) *ran_par = fast;
  return hipSuccess;
}
// the host reads the pass's header once the pass's event has completed
hipError_t launch_vadm_events(const VadmEventArgs &a, hipStream_t) {
  *a.header = VadmEventHeader{a.pass, 0, 0, 0};
  g_last_vadm_events = a;
  return hipSuccess;
}
// the sweep reads back every lane's state (left as uploaded: a fresh machine
// with no segments) and, scored, its status word and statistics
hipError_t launch_sweep_min(const SweepArgs &, hipStream_t) { return hipSuccess; }
hipError_t launch_vadm_sweep(const SweepArgs &, hipStream_t) { return hipSuccess; }
hipError_t launch_sweep_score(const ScoreArgs &a, hipStream_t) {
  for (int l = 0; l < a.n_streams * a.n_cfgs; l++) a.status[l] = kEvalScored;
  return hipSuccess;
}
hipError_t launch_stream_clear(const ClearArgs &, hipStream_t) { return hipSuccess; }
hipError_t launch_stream_vclear(const VClearArgs &, hipStream_t) { return hipSuccess; }
hipError_t launch_stream_gather(const XferArgs &, hipStream_t) { return hipSuccess; }  // (the staging is zeroed: a valid record)
hipError_t launch_stream_scatter(const XferArgs &, hipStream_t) { return hipSuccess; }
bool olafb_fused(const StagedArgs &a) { return a.nfft_b == 2048 && a.n_channels <= 4; }
bool fftb_generic(int) { return false; }
// scratch only above kMaxFftB, so that kind reaches the d_fbwork allocation
long long fftb_work_stride(int nfft_b, int, int, int) { return nfft_b > kMaxFftB ? nfft_b : 0; }
int gru16_frag_count() { return 1; }
int gru16_bias_rows() { return 1; }
void gru16_build(const int8_t *, uint16_t *, float *) {}
}  // namespace fvad

// ---------------------------------------------------------------------------
// the scenario
// ---------------------------------------------------------------------------
namespace {

struct Kind {
  const char *name;
  int mode, fft_size, use_denoiser;
  bool machines;  // fused engines refuse device VADMachines (and with them the event feed)
  // both resamplers: 0 for none, input_rate = denoised_rate = 16000, or
  // FVAD_INPUT_RATE_PER_STREAM (= FVAD_DENOISED_RATE_PER_STREAM) with both *_rate_max = 48000
  int rate;
};
const Kind kKinds[] = {{"staged", FVAD_MODE_STAGED, 2048, 1, true, 0},
                       {"staged, fft_size above kMaxFftB", FVAD_MODE_STAGED, 2 * fvad::kMaxFftB, 1, true, 0},
                       {"fused", FVAD_MODE_FUSED, 2048, 1, false, 0},
                       {"fp16", FVAD_MODE_FP16, 2048, 1, true, 0},
                       {"use_denoiser = 0", FVAD_MODE_STAGED, 2048, 0, true, 0},
                       {"staged, resampling at 16000", FVAD_MODE_STAGED, 2048, 1, true, 16000},
                       {"staged, per-stream rates", FVAD_MODE_STAGED, 2048, 1, true, FVAD_INPUT_RATE_PER_STREAM}};
static_assert(FVAD_INPUT_RATE_PER_STREAM == FVAD_DENOISED_RATE_PER_STREAM, "Kind::rate");

constexpr int kStreams = 2, kChannels = 1, kTicks = 2;
int g_fail = 0;
std::string g_note;  // what the run without a failure adds to its scenario's line
fvad_model *g_model = nullptr;

#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      std::printf("FAIL: ");        \
      std::printf(__VA_ARGS__);     \
      std::printf("\n");            \
      g_fail++;                     \
    }                               \
  } while (0)

bool all_released(const char *when, const char *name, long fail_at) {
  const bool ok = g_dev.empty() && g_pinned.empty() && g_events.empty() && g_streams.empty();
  CHECK(ok, "%s, failing call %ld, %s: live device %zu, pinned %zu, events %zu, streams %zu", name, fail_at, when,
        g_dev.size(), g_pinned.size(), g_events.size(), g_streams.size());
  return ok;
}

// One run of the scenario with creating call fail_at refused (-1: none).
// Returns the creating calls made, -1 after a failed check.
long run(const Kind &k, long fail_at) {
  g_creates = 0;
  g_fail_at = fail_at;
  const int fails_before = g_fail;
  fvad_engine *e = nullptr;
  bool over = false;  // the scenario ended at the injected failure
  // a step's status: negative only where the injected failure struck, and
  // then with a message; `again` (attach_vadm, enable_events) repeats the call
  auto step = [&](const char *what, auto call, bool again = false) {
    if (over || g_fail != fails_before) return;
    const long before = g_creates;
    const bool bad = call();
    const bool struck = fail_at >= before && fail_at < g_creates;
    if (!struck) {
      CHECK(!bad, "%s, failing call %ld: %s failed: %s", k.name, fail_at, what, fvad_last_error());
      return;
    }
    CHECK(bad, "%s: %s succeeded although its creating call %ld failed", k.name, what, fail_at);
    CHECK(fvad_last_error()[0] != 0, "%s: %s failed at creating call %ld without a message", k.name, what, fail_at);
    if (again)
      CHECK(!call(), "%s: %s repeated after its failed creating call %ld: %s", k.name, what, fail_at, fvad_last_error());
    else
      over = true;
  };

  fvad_engine_config cfg;
  fvad_engine_config_default(&cfg, kStreams, kChannels);
  cfg.mode = k.mode;
  cfg.fft_size = k.fft_size;
  cfg.use_denoiser = k.use_denoiser;
  cfg.max_ticks = kTicks;
  const bool per_stream = k.rate == FVAD_INPUT_RATE_PER_STREAM;
  if (k.rate) {
    cfg.input_rate = cfg.denoised_rate = k.rate;
    cfg.want_denoised = 1;
    if (per_stream) cfg.input_rate_max = cfg.denoised_rate_max = 48000;
  }
  fvad_vadm_config vc;
  fvad_vadm_config_default(&vc);
  // the machine's speech band as an engine band
  const fvad::VadmDerived d = fvad::vadm_derive(vc, cfg.sample_rate, cfg.fft_size);
  cfg.band_lo[0] = d.lo;
  cfg.band_hi[0] = d.hi;

  step("create", [&] { return fvad_engine_create(&cfg, g_model, &e) < 0; });
  if (!e) {  // create itself failed: nothing to destroy
    all_released("after the failed create", k.name, fail_at);
    return g_fail == fails_before ? g_creates : -1;
  }
  // a push's samples (a per-stream engine's streams start at *_rate_max: the largest push)
  int64_t offsets[kStreams + 1] = {};
  if (per_stream) {
    CHECK(fvad_engine_input_layout(e, offsets) == FVAD_OK, "%s: input_layout: %s", k.name, fvad_last_error());
  } else {
    offsets[kStreams] = (int64_t)kStreams * kChannels * fvad_engine_input_frame(e);
  }
  const size_t n_in = (size_t)kTicks * (size_t)offsets[kStreams];
  const int32_t stream0 = 0;
  constexpr int kDeferMax = 3, kSerialEvery = 5, kChunk = 7;
  if (k.machines) {
    // the machines' and the feed's hooks, set before either exists
    step("set_debug", [&] {
      return fvad_engine_set_debug(e, FVAD_DEBUG_VADM_DEFER_MAX, kDeferMax) < 0 ||
             fvad_engine_set_debug(e, FVAD_DEBUG_VADM_PAR_SERIAL_EVERY, kSerialEvery) < 0 ||
             fvad_engine_set_debug(e, FVAD_DEBUG_EVENTS_CHUNK, kChunk) < 0;
    });
    step("attach_vadm", [&] { return fvad_engine_attach_vadm(e, &vc, 1, 4) < 0; }, true);
    step("enable_events", [&] { return fvad_engine_enable_events(e, 16) < 0; }, true);
  }
  g_last_vadm = fvad::VadmArgs{};
  g_last_vadm_events = fvad::VadmEventArgs{};
  float *slot = nullptr;
  step("input_slot", [&] { return (slot = fvad_engine_input_slot(e)) == nullptr; });
  step("submit", [&] {
    std::memset(slot, 0, n_in * sizeof(float));
    return fvad_engine_submit(e, slot, kTicks, nullptr) < 0;
  });
  if (k.machines) {  // the first push's machine pass and event pass run at the sync
    step("sync", [&] { return fvad_engine_sync(e) < 0; });
    if (!over && g_fail == fails_before) {
      CHECK(g_last_vadm.n == 1 && g_last_vadm.defer_max == (unsigned)kDeferMax &&
                g_last_vadm.par_serial_every == kSerialEvery,
            "%s: hooks set before attach_vadm: launch_vadm saw n %d, defer_max %u, par_serial_every %d", k.name,
            g_last_vadm.n, g_last_vadm.defer_max, g_last_vadm.par_serial_every);
      CHECK(g_last_vadm_events.n_machines == 1 && g_last_vadm_events.chunk == kChunk,
            "%s: hook set before enable_events: launch_vadm_events saw n_machines %d, chunk %d", k.name,
            g_last_vadm_events.n_machines, g_last_vadm_events.chunk);
    }
  }
  if (per_stream) {  // between two pushes: the next one syncs both plans' tables a second time (a second staging row each)
    const int rate = 16000;
    step("set_stream_rates", [&] { return fvad_engine_set_stream_rates(e, &stream0, 1, &rate) < 0; });
    step("set_stream_denoised_rates", [&] { return fvad_engine_set_stream_denoised_rates(e, &stream0, 1, &rate) < 0; });
  }
  step("submit_i16", [&] {
    const std::vector<int16_t> pcm(n_in, 0);
    return fvad_engine_submit_i16(e, pcm.data(), kTicks, nullptr, nullptr) < 0;
  });
  for (int i = 0; i < 2; i++) step("collect", [&] { return fvad_engine_collect(e, nullptr, nullptr) < 0; });
  if (!k.rate) {  // (a resampling engine refuses both)
    step("load_synthetic_ex", [&] { return fvad_engine_load_synthetic_ex(e, kTicks, 2, 0) < 0; });
    for (int i = 0; i < 2; i++) step("run_resident", [&] { return fvad_engine_run_resident(e, kTicks) < 0; });
  }
  step("set_debug", [&] { return fvad_engine_set_debug(e, FVAD_DEBUG_RESET_TIMES, 1) < 0; });
  step("reset_streams", [&] { return fvad_engine_reset_streams(e, &stream0, 1) < 0; });
  std::vector<char> blob;
  step("save_streams", [&] {
    blob.resize(fvad_engine_save_size(e, 1));
    return fvad_engine_save_streams(e, &stream0, 1, blob.data(), blob.size()) < 0;
  });
  step("restore_streams", [&] { return fvad_engine_restore_streams(e, &stream0, 1, blob.data(), blob.size(), nullptr) < 0; });
  step("kernel_times", [&] {
    double ms[FVAD_MAX_TIMES];
    int n = 0;
    return fvad_engine_kernel_times(e, ms, &n) < 0;
  });
  // every timer's runs (0: a null pointer's place where the kind has no such timer), then cleared
  auto timing_runs = [&](int *n) {
    double ms[FVAD_MAX_TIMES];
    bool bad = fvad_engine_kernel_times(e, ms, &n[0]) < 0;
    if (k.machines) bad = bad || fvad_engine_event_times(e, ms, &n[1]) < 0;
    if (k.rate) bad = bad || fvad_engine_resample_times(e, ms, &n[2]) < 0 || fvad_engine_resample_out_times(e, ms, &n[3]) < 0;
    return bad || fvad_engine_reset_times(e, ms, &n[4]) < 0;
  };
  int runs[7] = {}, after[7] = {};
  step("timing runs", [&] { return timing_runs(runs); });
  step("clear_times", [&] { return fvad_engine_clear_times(e) < 0; });
  step("timing runs after clear_times", [&] { return timing_runs(after); });
  if (!over && g_fail == fails_before) {
    if (fail_at < 0) {
      char note[160];
      std::snprintf(note, sizeof(note), "; timed runs: kernels %d, event feed %d, resample %d, resample_out %d, reset %d/%d/%d",
                    runs[0], runs[1], runs[2], runs[3], runs[4], runs[5], runs[6]);
      g_note = note;
    }
    for (int i = 0; i < 7; i++) CHECK(after[i] == 0, "%s: timer %d reads %d runs after clear_times", k.name, i, after[i]);
  }
  fvad_engine_destroy(e);
  all_released("after destroy", k.name, fail_at);
  CHECK(fail_at < 0 || fail_at < g_creates, "%s: creating call %ld was never reached (%ld made)", k.name, fail_at,
        g_creates);
  return g_fail == fails_before ? g_creates : -1;
}

// The config sweep over the same stubs: create, the windows, fvad_sweep_run
// and fvad_sweep_run_score, three configs of growing buffer lengths one per
// chunk (FVAD_SWEEP_DEBUG_CHUNK = 1), so the machines' buffers grow between
// chunks.  The call a creating call fails in must report FVAD_ENOMEM or
// FVAD_EDEVICE and succeed when repeated.  Returns as run does.
long run_sweep(long fail_at) {
  const char *name = "sweep";
  g_creates = 0;
  g_fail_at = fail_at;
  const int fails_before = g_fail;
  auto step = [&](const char *what, auto call) {
    if (g_fail != fails_before) return;
    const long before = g_creates;
    const int rc = call();
    if (fail_at < before || fail_at >= g_creates) {
      CHECK(rc >= 0, "%s, failing call %ld: %s failed: %s", name, fail_at, what, fvad_last_error());
      return;
    }
    CHECK(rc == FVAD_ENOMEM || rc == FVAD_EDEVICE, "%s: %s returned %d although its creating call %ld failed", name,
          what, rc, fail_at);
    CHECK(fvad_last_error()[0] != 0, "%s: %s failed at creating call %ld without a message", name, what, fail_at);
    CHECK(call() >= 0, "%s: %s repeated after its failed creating call %ld: %s", name, what, fail_at, fvad_last_error());
  };

  fvad_vadm_config vc[3];
  fvad_sweep_config cfg{};
  cfg.n_streams = kStreams;
  cfg.n_channels = kChannels;
  cfg.sample_rate = 48000;
  cfg.fft_size = 2048;
  cfg.n_bands = 1;
  cfg.use_denoiser = 1;
  cfg.seg_capacity = 4;
  cfg.device = 0;
  for (int m = 0; m < 3; m++) {  // each config's three buffers outgrow the previous one's (and the 256-byte floor)
    fvad_vadm_config_default(&vc[m]);
    vc[m].long_term_speech_avg_sec += 20.0f * m;
    vc[m].short_term_speech_avg_sec = vc[m].channel_vol_ratio_avg_sec = m ? 2.0f * m : 0.2f;
  }
  const fvad::VadmDerived d = fvad::vadm_derive(vc[0], cfg.sample_rate, cfg.fft_size);
  cfg.band_lo[0] = d.lo;
  cfg.band_hi[0] = d.hi;
  const size_t n_win = 3;
  const std::vector<float> zeros(n_win * kChannels, 0.0f);
  const float label[2] = {0.0f, 1.0f};
  const float *refs[kStreams] = {label, label};
  const size_t n_ref[kStreams] = {1, 1};
  const fvad_stat_config stat{};
  fvad_aggregate_stats agg[3];

  fvad_sweep *sw = nullptr;
  step("sweep_create", [&] { return fvad_sweep_create(&cfg, &sw); });
  if (sw) {
    for (int s = 0; s < kStreams; s++)
      step("set_windows", [&] { return fvad_sweep_set_windows(sw, s, n_win, zeros.data(), zeros.data(), zeros.data()); });
    step("set_debug", [&] { return fvad_sweep_set_debug(sw, FVAD_SWEEP_DEBUG_CHUNK, 1); });
    step("sweep_run", [&] { return fvad_sweep_run(sw, vc, 3); });
    step("sweep_run_score", [&] { return fvad_sweep_run_score(sw, vc, 3, refs, n_ref, &stat, 1, agg, nullptr); });
    fvad_sweep_destroy(sw);
  } else {
    CHECK(false, "%s, failing call %ld: no sweep", name, fail_at);
  }
  all_released("after destroy", name, fail_at);
  CHECK(fail_at < g_creates, "%s: creating call %ld was never reached (%ld made)", name, fail_at, g_creates);
  return g_fail == fails_before ? g_creates : -1;
}

// The stage table (fvad_staged.h staged_kernels, the real function): the
// kernels of a push per pipeline variant, and that every list is a chain of
// timing events from the push's first to its last.
void check_stage_table() {
  using fvad::StagedVariant;
  struct Case {
    const char *what;
    StagedVariant v;  // fma, fp16, fuse16, olafb
    std::vector<std::string> names;
  };
  const std::vector<std::string> front = {"k_prep3", "k_fftAw", "k_plpc", "k_pcorr", "k_select"};
  auto with = [&](std::vector<std::string> rest) {
    std::vector<std::string> l = front;
    l.insert(l.end(), rest.begin(), rest.end());
    return l;
  };
  const Case cases[] = {
      {"staged, fused tail", {false, false, false, true}, with({"k_pspecw", "k_rnn3", "k_synthw", "k_olafb"})},
      {"f32_fast", {true, false, false, true}, with({"k_pspecw", "k_rnn3f", "k_synthw", "k_olafb"})},
      {"fp16", {false, true, false, true}, with({"k_pspecw", "k_gru16", "k_synthw", "k_olafb"})},
      {"fp16_fused", {false, true, true, true}, with({"k_fused16", "k_synthw", "k_olafb"})},
      {"three-kernel tail", {false, false, false, false},
       with({"k_pspecw", "k_rnn3", "k_synthw", "k_ola", "k_winmeta", "k_fftbw"})},
  };
  for (const Case &c : cases) {
    const fvad::StagedKernels l = fvad::staged_kernels(c.v);
    std::vector<std::string> got;
    for (int i = 0; i < l.n; i++) got.push_back(l.k[i].name);
    std::string joined;
    for (const std::string &s : got) joined += s + " ";
    CHECK(got == c.names, "stage table, %s: kernels %s", c.what, joined.c_str());
    CHECK(l.n >= 1 && l.n <= fvad::kStagedStages && l.n + 2 < FVAD_MAX_TIMES, "stage table, %s: %d kernels", c.what, l.n);
    for (int i = 0; i < l.n; i++) {
      CHECK(l.k[i].begin >= 0 && l.k[i].begin < fvad::kStagedEvents && l.k[i].end >= 0 &&
                l.k[i].end < fvad::kStagedEvents && l.k[i].begin != l.k[i].end,
            "stage table, %s: %s runs between events %d and %d", c.what, l.k[i].name, l.k[i].begin, l.k[i].end);
      CHECK(i == 0 || l.k[i].stage > l.k[i - 1].stage, "stage table, %s: %s out of pipeline order", c.what, l.k[i].name);
    }
    CHECK(l.k[0].begin == fvad::kStagedFirst, "stage table, %s: starts at event %d", c.what, l.k[0].begin);
    CHECK(l.k[l.n - 1].end == fvad::kStagedLast, "stage table, %s: ends at event %d", c.what, l.k[l.n - 1].end);
  }
  // the variant as launch_staged derives it from a push's arguments
  fvad::StagedArgs a{};
  a.nfft_b = 2048;
  a.n_channels = 2;
  a.fma = 1;
  StagedVariant v = fvad::staged_variant(a);
  CHECK(v.fma && !v.fp16 && !v.fuse16 && v.olafb, "staged_variant: f32_fast");
  a.gru16_frags = &a;  // the fp16 recurrence runs whatever a.fma says
  a.fuse16 = 1;
  a.nfft_b = 1000;
  v = fvad::staged_variant(a);
  CHECK(!v.fma && v.fp16 && v.fuse16 && !v.olafb, "staged_variant: fp16_fused, fft_size 1000");
  a.gru16_frags = nullptr;  // (fuse16 means nothing without the fp16 recurrence)
  a.fma = 0;
  v = fvad::staged_variant(a);
  CHECK(!v.fma && !v.fp16 && !v.fuse16 && !v.olafb, "staged_variant: staged, fft_size 1000");
  static_assert(fvad::kStagedEvents <= FVAD_MAX_TIMES && fvad::kStagedLast < fvad::kStagedEvents, "timing events");
}

}  // namespace

int main() {
  if (fvad_model_synthetic(1, &g_model) != FVAD_OK) {
    std::printf("FAIL: no synthetic model: %s\n", fvad_last_error());
    return 1;
  }
  check_stage_table();
  // a scenario without a failure, then with each of its creating calls failed in turn
  auto every_failure = [](const char *name, auto scenario) {
    const long n = scenario(-1);
    if (n < 0) return;
    long done = 0;
    for (long f = 0; f < n; f++)
      if (scenario(f) >= 0) done++;
    std::printf("%s: %ld creating calls, %ld of them failed in turn and survived%s\n", name, n, done, g_note.c_str());
    g_note.clear();
    CHECK(done == n, "%s: %ld of %ld failure runs passed", name, done, n);
  };
  for (const Kind &k : kKinds) every_failure(k.name, [&](long f) { return run(k, f); });
  every_failure("sweep", run_sweep);
  fvad_model_free(g_model);
  CHECK(g_bad == 0, "%d releases of something not live", g_bad);
  std::printf(g_fail ? "FAILED: %d checks\n" : "ok\n", g_fail);
  return g_fail ? 1 : 0;
}
