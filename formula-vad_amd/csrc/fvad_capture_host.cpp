// The batched engine's clip capture ("Clip capture"):
// enable, the append of each push on the input's reading stream, the capture
// pass behind each machine pass on the side stream, poll, flush, the
// lifecycle's part and the timers.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fvad_engine_impl.h"

using namespace fvad::eng;

static_assert(sizeof(fvad_clip) == 64 && sizeof(fvad::CapClip) == sizeof(fvad_clip), "fvad_clip is 64 bytes");
static_assert(offsetof(fvad_clip, push) == offsetof(fvad::CapClip, push) &&
                  offsetof(fvad_clip, first_sample) == offsetof(fvad::CapClip, first_sample) &&
                  offsetof(fvad_clip, reserved) == offsetof(fvad::CapClip, reserved),
              "the device's clip descriptor is fvad_clip");
static_assert(FVAD_CLIP_HEAD_SHORT == fvad::cap::kHeadShort && FVAD_CLIP_TAIL_SHORT == fvad::cap::kTailShort &&
                  FVAD_CLIP_NO_AUDIO == fvad::cap::kNoAudio,
              "the clip flags");
static_assert(sizeof(fvad::CapSetArgs) <= 4096 && sizeof(fvad::CapPassArgs) <= 4096, "kernel argument blocks");

namespace {

constexpr size_t kDefaultPool = (size_t)64 << 20;
constexpr int kFlushSlot = kEvHeaders;  // the header slot of a flush

fvad::CapPassArgs pass_args(const fvad_engine *e, const fvad::VadmArgs &v) {
  const Capture &c = *e->cap;
  fvad::CapPassArgs a{};
  a.stage = v.ev_stage;
  a.count = v.ev_count;
  a.ev_cap = v.ev_cap;
  a.n_machines = v.n;
  a.machine = c.machine;
  a.n_streams = e->cfg.n_streams;
  a.n_channels = e->cfg.n_channels;
  a.pend = c.pend.get();
  a.pend_n = c.pend_n.get();
  a.history = c.history;
  a.H = c.H;
  a.hist = c.hist.get();
  a.state = c.state.get();
  a.work = c.work.get();
  a.pool = c.dv_pool;
  a.pool16 = c.dv_pool16;
  a.L = c.L;
  a.M = c.M;
  a.reserved = c.source == FVAD_CLIP_SOURCE_INPUT && c.format == FVAD_CLIP_F32
                   ? 0ull
                   : (unsigned long long)c.rate | (unsigned long long)c.format << 32 | (unsigned long long)c.source << 40;
  a.pool_cap = c.pool_cap;
  a.desc = c.dv_desc;
  a.desc_cap = c.desc_cap;
  a.host_desc_read = c.desc_read;
  a.host_pool_read = c.pool_read;
  return a;
}

void take_header(Capture &c, const volatile fvad::CapHeader *h) {
  c.desc_end = h->desc_end;
  c.pool_end = h->pool_end;
  c.lost = h->lost;
}

}  // namespace

// k_hist_append of the push being launched, behind its k_prep3 on the prep
// stream (the stream that reads the push's device input) and before the
// push's ev_prep_done and ev_in_free are recorded.  The append rewrites ring
// words and the snapshot of parity b that the capture pass of the push two
// before read: it waits for that pass.
int fvad::eng::capture_append(fvad_engine *e, const fvad::StagedArgs &a, int b, bool timed) {
  Capture &c = *e->cap;
  const hipStream_t s = input_reader(e);
  HIP_TRY(wait_event(s, c.ev_pass[b].get()));
  fvad::CapAppendArgs p{};
  p.pcm = a.pcm;
  p.pcm16 = a.pcm16;
  p.ticks_valid = a.ticks_valid;
  p.n_ticks = a.n_ticks;
  p.n_streams = a.n_streams;
  p.n_channels = a.n_channels;
  p.hist = c.hist.get();
  p.H = c.H;
  p.pos = c.pos.get();
  p.snap = c.snap[b].get();
  p.frame = fvad::kFrame;
  int rc;
  if (timed && (rc = c.tm.begin(b, s))) return rc;
  HIP_TRY(fvad::launch_hist_append(p, s));
  if (timed && (rc = c.tm.end(b, s, Capture::kAppend))) return rc;
  return FVAD_OK;
}

// The stream that owns the positions and writes the ring: the input's reader,
// or the engine stream for a capture of the denoised rows
hipStream_t fvad::eng::capture_appender(const fvad_engine *e) {
  return e->cap->source == FVAD_CLIP_SOURCE_DENOISED ? e->stream.get() : input_reader(e);
}

// k_den_append of the push being launched (FVAD_CLIP_SOURCE_DENOISED), on
// the engine stream behind the push's last writer of the rows it reads --
// k_resample_out, or the tail kernels without an output rate -- and ahead of
// ev_buf_free[b]: it reads ticks buffer b, and the rows are single-buffered,
// rewritten by the next push on this stream.  It waits for the capture pass of
// the push two before, as capture_append does and for the same words.
int fvad::eng::capture_append_den(fvad_engine *e, const fvad::StagedArgs &a, int b, bool timed) {
  Capture &c = *e->cap;
  const hipStream_t s = e->stream.get();
  HIP_TRY(wait_event(s, c.ev_pass[b].get()));
  fvad::CapAppendArgs p{};
  p.den = denoised_source(e);
  p.frame = c.frame;
  p.ticks_valid = a.ticks_valid;
  p.n_ticks = a.n_ticks;
  p.n_streams = a.n_streams;
  p.n_channels = a.n_channels;
  p.hist = c.hist.get();
  p.H = c.H;
  p.pos = c.pos.get();
  p.snap = c.snap[b].get();
  // timed on every push without waiting, as the output resampler's launches
  // ahead of it are (a host-fed push is never a sampled one)
  (void)timed;
  int rc;
  if ((rc = c.tm.collect(b)) || (rc = c.tm.begin(b, s))) return rc;
  HIP_TRY(fvad::launch_hist_append(p, s));
  return c.tm.end(b, s, Capture::kAppend);
}

// The capture pass of push `push` (parity b) on the side stream, behind its
// machine pass and before its k_vadm_events, which clears the staged counts
// this pass reads and ends with the `done` event events_retire waits for: the
// pass's header slot is the event pass's.
int fvad::eng::capture_pass(fvad_engine *e, const fvad::VadmArgs &v, uint64_t push, int b, int slot, bool timed) {
  Capture &c = *e->cap;
  // the header slot is free: at most kEvHeaders passes in flight
  int rc = events_retire(e, false);
  if (!rc && e->feed.flight.size() >= (size_t)kEvHeaders) rc = events_retire(e, true);
  if (rc) return rc;
  fvad::CapPassArgs a = pass_args(e, v);
  a.flush_mode = 0;
  a.pos = c.snap[b].get();
  a.pass = e->feed.pass_next;
  a.push = push;
  a.header = c.dv_hdr + a.pass % kEvHeaders;
  if (timed && (rc = c.tm.begin(Capture::kPassSlot + slot, e->side))) return rc;
  HIP_TRY(fvad::launch_capture_pass(a, e->side));
  if (timed && (rc = c.tm.end(Capture::kPassSlot + slot, e->side, Capture::kPass))) return rc;
  HIP_TRY(hipEventRecord(c.ev_pass[b].get(), e->side));
  return FVAD_OK;
}

// events_retire saw the `done` event of pass `pass` complete
int fvad::eng::capture_retire(fvad_engine *e, uint64_t pass) {
  Capture &c = *e->cap;
  const volatile fvad::CapHeader *h = c.hdr.get() + pass % kEvHeaders;
  if (h->pass != pass) return fail(FVAD_EDEVICE, "clip capture: a finished pass left no header");
  take_header(c, h);
  return FVAD_OK;
}

// capture as after enable on fresh streams (every stream is idle)
int fvad::eng::capture_reset(fvad_engine *e) {
  Capture &c = *e->cap;
  const size_t B = e->cfg.n_streams;
  HIP_TRY(hipMemset(c.pos.get(), 0, B * sizeof(fvad::CapPos)));
  for (auto &sn : c.snap) HIP_TRY(hipMemset(sn.get(), 0, B * sizeof(fvad::CapPos)));
  HIP_TRY(hipMemset(c.pend_n.get(), 0, B * sizeof(unsigned)));
  HIP_TRY(hipMemset(c.state.get(), 0, sizeof(fvad::CapState)));
  std::memset(c.hdr.get(), 0xff, sizeof(fvad::CapHeader) * (kEvHeaders + 1));
  c.desc_read = c.desc_end = c.pool_read = c.pool_end = c.lost = 0;
  c.tm.drop();
  return FVAD_OK;
}

// fvad_engine_reset_streams / restore_streams: the listed streams' position
// and base to samples[i] (0 when null) on the appending stream, behind the
// appends already queued; their pending clips dropped on the side stream,
// behind the passes already queued.  No host wait.
int fvad::eng::capture_set_streams(fvad_engine *e, const int32_t *streams, const uint64_t *samples, int n) {
  Capture &c = *e->cap;
  fvad::CapSetArgs a{};
  a.pos = c.pos.get();
  a.pend_n = c.pend_n.get();
  for (int i0 = 0; i0 < n; i0 += fvad::kListMax) {
    a.ids.n = std::min(fvad::kListMax, n - i0);
    for (int i = 0; i < a.ids.n; i++) {
      a.ids.id[i] = streams[i0 + i];
      // (a 48 kHz sample count, a multiple of 480, in samples of the clip rate)
      a.value[i] = samples ? samples[i0 + i] / fvad::kFrame * (unsigned long long)c.frame : 0;
    }
    HIP_TRY(fvad::launch_capture_set_pos(a, capture_appender(e)));
    HIP_TRY(fvad::launch_capture_drop(a, e->side));
  }
  return FVAD_OK;
}

int fvad::eng::capture_collect_timing(fvad_engine *e) {
  return e->cap ? e->cap->tm.collect() : FVAD_OK;
}

// All or nothing, as fvad_engine_attach_vadm: everything is made in a local
// Capture that moves into the engine after the last step that can fail.
extern "C" void fvad_capture_config_default(fvad_capture_config *c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->machine = 0;
  c->history_sec = 10.0;
  c->pool_samples = 0;
  c->source = FVAD_CLIP_SOURCE_INPUT;
  c->format = FVAD_CLIP_F32;
}

extern "C" int fvad_engine_enable_capture(fvad_engine *e, int machine, double history_sec, size_t pool_samples) {
  fvad_capture_config c;
  fvad_capture_config_default(&c);
  c.machine = machine;
  c.history_sec = history_sec;
  c.pool_samples = pool_samples;
  return fvad_engine_enable_capture_ex(e, &c);
}

extern "C" int fvad_engine_enable_capture_ex(fvad_engine *e, const fvad_capture_config *cc) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  if (!cc) return fail(FVAD_EINVAL, "null capture config");
  const int machine = cc->machine;
  const double history_sec = cc->history_sec;
  size_t pool_samples = cc->pool_samples;
  if (cc->source != FVAD_CLIP_SOURCE_INPUT && cc->source != FVAD_CLIP_SOURCE_DENOISED)
    return fail(FVAD_EINVAL, "source must be FVAD_CLIP_SOURCE_INPUT or FVAD_CLIP_SOURCE_DENOISED");
  if (cc->format != FVAD_CLIP_F32 && cc->format != FVAD_CLIP_S16)
    return fail(FVAD_EINVAL, "format must be FVAD_CLIP_F32 or FVAD_CLIP_S16");
  const bool den = cc->source == FVAD_CLIP_SOURCE_DENOISED, s16 = cc->format == FVAD_CLIP_S16;
  if (den && !e->cfg.want_denoised)
    return fail(FVAD_EINVAL, "a capture of the denoised rows needs an engine created with want_denoised");
  if (den && e->ro && e->ro->plan.on())  // (clips at a stream's own rate: not built)
    return fail(FVAD_EINVAL, "a capture of the denoised rows is not available with per-stream denoised rates");
  if (!e->vadm.on() || !e->feed.on())
    return fail(FVAD_EINVAL, "clip capture needs fvad_engine_attach_vadm and fvad_engine_enable_events first");
  if (e->cap) return fail(FVAD_EINVAL, "capture already enabled");
  if (e->cfg.mode == FVAD_MODE_FUSED || !e->cfg.use_denoiser)
    return fail(FVAD_EINVAL, "clip capture needs a staged-family engine with the denoiser");
  if (machine < 0 || machine >= e->vadm.args.n) return fail(FVAD_EINVAL, "no such attached machine");
  if (!(history_sec >= 4.0) || !(history_sec <= 86400.0))
    return fail(FVAD_EINVAL, "history_sec must be at least 4 (two seconds of margin at each end)");
  for (const auto &sl : e->slots)
    if (sl.pending) return fail(FVAD_EINVAL, "submitted pushes not collected yet");
  if (pool_samples == 0) pool_samples = kDefaultPool;
  int rc = fvad_engine_sync(e);  // a pending machine pass runs now, without capture
  if (!rc) rc = events_retire(e, false);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t B = e->cfg.n_streams, C = e->cfg.n_channels;
  auto c = std::make_unique<Capture>();
  c->machine = machine;
  c->source = cc->source;
  c->format = cc->format;
  if (den && e->ro) {  // the engine's denoised_rate: the rows k_resample_out writes
    c->rate = e->ro->d.rate;
    c->frame = e->ro->d.n;
    c->L = (unsigned)e->ro->d.L;
    c->M = (unsigned)e->ro->d.M;
  }
  // the ring: history and a whole push, in samples of the clip rate
  c->history = (unsigned long long)std::floor((double)c->rate * history_sec);
  c->H = (c->history + (unsigned long long)e->cfg.max_ticks * c->frame + 3) & ~3ull;
  c->pool_cap = pool_samples;
  c->desc_cap = std::max<size_t>(1024, 8 * B);
  if ((rc = fvad::make_dev(c->hist, B * C * (size_t)c->H)) || (rc = fvad::make_dev(c->pos, B)) ||
      (rc = fvad::make_dev(c->snap[0], B)) || (rc = fvad::make_dev(c->snap[1], B)) ||
      (rc = fvad::make_dev(c->pend, B * fvad::cap::kQueue)) || (rc = fvad::make_dev(c->pend_n, B)) ||
      (rc = fvad::make_dev(c->state, 1)) || (rc = fvad::make_dev(c->work, B * fvad::cap::kQueue)) ||
      (rc = fvad::make_dev(c->flush, B)) ||
      (rc = s16 ? fvad::make_pinned(c->pool16, c->pool_cap) : fvad::make_pinned(c->pool, c->pool_cap)) ||
      (rc = fvad::make_pinned(c->desc, c->desc_cap)) ||
      (rc = fvad::make_pinned(c->hdr, (size_t)kEvHeaders + 1)) || (rc = fvad::make_event(c->ev_pass[0])) ||
      (rc = fvad::make_event(c->ev_pass[1])))
    return rc;
  if ((rc = c->tm.create())) return rc;
  void *dv_pool = nullptr, *dv_desc = nullptr, *dv_hdr = nullptr;
  if (hipHostGetDevicePointer(&dv_pool, s16 ? (void *)c->pool16.get() : (void *)c->pool.get(), 0) != hipSuccess ||
      hipHostGetDevicePointer(&dv_desc, c->desc.get(), 0) != hipSuccess ||
      hipHostGetDevicePointer(&dv_hdr, c->hdr.get(), 0) != hipSuccess) {
    (void)hipGetLastError();
    return fail(FVAD_EDEVICE, "hipHostGetDevicePointer failed (clip capture)");
  }
  if (s16)
    c->dv_pool16 = static_cast<int16_t *>(dv_pool);
  else
    c->dv_pool = static_cast<float *>(dv_pool);
  c->dv_desc = static_cast<fvad::CapClip *>(dv_desc);
  c->dv_hdr = static_cast<fvad::CapHeader *>(dv_hdr);
  // the streams' positions: what each has consumed so far (the state record's
  // tick counter; the engine is idle), nothing of it held
  std::vector<int> ticks(B);
  std::vector<fvad::CapPos> pos(B);
  if (hipMemcpy2D(ticks.data(), sizeof(int), e->d_state.get() + fvad::st::kFramesDone,
                  sizeof(float) * fvad::st::kWords, sizeof(int), B, hipMemcpyDeviceToHost) != hipSuccess) {
    (void)hipGetLastError();
    return fail(FVAD_EDEVICE, "reading the streams' tick counters failed (clip capture)");
  }
  for (size_t s = 0; s < B; s++) {
    pos[s] = fvad::CapPos{};
    pos[s].pos = pos[s].base = (unsigned long long)ticks[s] * c->frame;
  }
  if (hipMemcpy(c->pos.get(), pos.data(), B * sizeof(fvad::CapPos), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->snap[0].get(), pos.data(), B * sizeof(fvad::CapPos), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->snap[1].get(), pos.data(), B * sizeof(fvad::CapPos), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(c->pend_n.get(), 0, B * sizeof(unsigned)) != hipSuccess ||
      hipMemset(c->state.get(), 0, sizeof(fvad::CapState)) != hipSuccess ||
      hipEventRecord(c->ev_pass[0].get(), e->side) != hipSuccess ||
      hipEventRecord(c->ev_pass[1].get(), e->side) != hipSuccess) {
    (void)hipGetLastError();
    return fail(FVAD_EDEVICE, "initialising clip capture failed");
  }
  std::memset(c->hdr.get(), 0xff, sizeof(fvad::CapHeader) * (kEvHeaders + 1));
  // nothing below fails
  e->cap = std::move(c);
  return FVAD_OK;
}

namespace {

// fvad_engine_poll_clip / fvad_engine_poll_clip_s16: `pool` is the capture's
// pool of this sample type, null when the capture delivers the other one
template <typename Sample>
int poll_any(fvad_engine *e, fvad_clip *info, Sample *pcm, size_t cap_samples, uint64_t *lost) {
  if (!e || !info || (cap_samples > 0 && !pcm)) return fail(FVAD_EINVAL, "invalid argument");
  if (!e->cap) return fail(FVAD_EINVAL, "capture not enabled");
  const Sample *pool;
  if constexpr (sizeof(Sample) == 2)
    pool = e->cap->pool16.get();
  else
    pool = e->cap->pool.get();
  if (!pool)
    return fail(FVAD_EINVAL, "an s16 capture is read with fvad_engine_poll_clip_s16, an f32 capture with fvad_engine_poll_clip");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (const int rc = events_retire(e, false)) return rc;
  Capture &c = *e->cap;
  if (lost) *lost = c.lost;
  if (c.desc_read == c.desc_end) return 0;
  const fvad_clip d = c.desc.get()[c.desc_read % c.desc_cap];
  *info = d;
  if (d.n_samples > cap_samples) return fail(FVAD_EINVAL, "clip longer than the buffer (n_samples in *info)");
  if (d.n_samples > c.pool_end - c.pool_read) return fail(FVAD_EDEVICE, "clip capture: descriptor past the pool's end");
  const size_t n = (size_t)d.n_samples, at = (size_t)(c.pool_read % c.pool_cap), head = std::min(n, c.pool_cap - at);
  if (n) {
    std::memcpy(pcm, pool + at, head * sizeof(Sample));
    std::memcpy(pcm + head, pool, (n - head) * sizeof(Sample));
  }
  c.pool_read += n;
  c.desc_read++;
  return 1;
}

}  // namespace

extern "C" int fvad_engine_poll_clip(fvad_engine *e, fvad_clip *info, float *pcm, size_t cap_samples, uint64_t *lost) {
  return poll_any(e, info, pcm, cap_samples, lost);
}

extern "C" int fvad_engine_poll_clip_s16(fvad_engine *e, fvad_clip *info, int16_t *pcm, size_t cap_samples,
                                         uint64_t *lost) {
  return poll_any(e, info, pcm, cap_samples, lost);
}

extern "C" int fvad_engine_clip_rate(const fvad_engine *e) { return e && e->cap ? e->cap->rate : 0; }

extern "C" void fvad_pcm_f32_to_s16(const float *x, int16_t *q, size_t n) {
  for (size_t i = 0; i < n; i++) q[i] = fvad::cap::to_s16(x[i]);
}

extern "C" int fvad_clip_range(int rate, uint64_t from48, uint64_t to48, uint64_t *first, uint64_t *end) {
  unsigned L = 1, M = 1;
  if (rate != 48000) {
    fvad::rs::Desc d{};
    if (!fvad::rs::describe(rate, fvad::rs::Dir::kOut, d)) return fail(FVAD_ERATE, "rate must be 48000, 8000, 16000, 24000, 32000, 44100 or 96000");
    L = (unsigned)d.L;
    M = (unsigned)d.M;
  }
  if (to48 < from48) return fail(FVAD_EINVAL, "to48 < from48");
  if (first) *first = fvad::cap::to_rate(from48, L, M);
  if (end) *end = fvad::cap::to_rate(to48, L, M);
  return FVAD_OK;
}

extern "C" int fvad_engine_capture_flush(fvad_engine *e, const int32_t *streams, int n) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  if (!e->cap) return fail(FVAD_EINVAL, "capture not enabled");
  const size_t B = e->cfg.n_streams;
  std::vector<unsigned char> flags;
  if (streams) {
    if (n < 0) return fail(FVAD_EINVAL, "invalid stream list");
    flags.assign(B, 0);
    for (int i = 0; i < n; i++) {
      if (streams[i] < 0 || (size_t)streams[i] >= B) return fail(FVAD_EINVAL, "stream index out of range");
      flags[streams[i]] = 1;
    }
  }
  int rc = fvad_engine_sync(e);  // every queued push and its pass; the positions are final
  if (!rc) rc = events_retire(e, false);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device));
  Capture &c = *e->cap;
  if (streams) HIP_TRY(hipMemcpy(c.flush.get(), flags.data(), B, hipMemcpyHostToDevice));
  fvad::CapPassArgs a = pass_args(e, e->vadm.args);
  a.flush_mode = streams ? 1 : 2;
  a.flush = c.flush.get();
  a.pos = c.pos.get();
  a.pass = ~0ull - 1;  // (no push's pass has this ordinal)
  a.push = e->push_count ? e->push_count - 1 : 0;
  a.header = c.dv_hdr + kFlushSlot;
  HIP_TRY(fvad::launch_capture_pass(a, e->side));
  HIP_TRY(hipStreamSynchronize(e->side));
  const volatile fvad::CapHeader *h = c.hdr.get() + kFlushSlot;
  if (h->pass != a.pass) return fail(FVAD_EDEVICE, "clip capture: the flush left no header");
  take_header(c, h);
  c.hdr.get()[kFlushSlot].pass = ~0ull;
  return FVAD_OK;
}

extern "C" int fvad_engine_capture_times(fvad_engine *e, double *ms_avg, int *n_runs) {
  if (!e || !ms_avg) return fail(FVAD_EINVAL, "null argument");
  if (!e->cap) return fail(FVAD_EINVAL, "capture not enabled");
  if (const int rc = fvad_engine_sync(e)) return rc;
  const Capture &c = *e->cap;
  c.tm.read(Capture::kAppend, &ms_avg[0], nullptr);
  c.tm.read(Capture::kPass, &ms_avg[1], n_runs);
  return FVAD_OK;
}
