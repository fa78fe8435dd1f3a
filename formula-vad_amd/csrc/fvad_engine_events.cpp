// The batched engine's speech event feed (eng::EventFeed): enable, the
// k_vadm_events pass behind each machine pass, retiring finished passes, poll,
// progress and times.
#include <algorithm>
#include <cstring>
#include <string>

#include "fvad_engine_impl.h"

using namespace fvad::eng;

static_assert(sizeof(fvad_event) == 48 && sizeof(fvad::VadmEvent) == sizeof(fvad_event), "fvad_event is 48 bytes");
static_assert(offsetof(fvad_event, push) == offsetof(fvad::VadmEvent, push) &&
                  offsetof(fvad_event, sample_to) == offsetof(fvad::VadmEvent, sample_to) &&
                  offsetof(fvad_event, debug_avg_speech_vol_ratio) ==
                      offsetof(fvad::VadmEvent, debug_avg_speech_vol_ratio),
              "the device's event record is fvad_event");

// The passes whose `done` event has completed leave flight, the newest one's
// header giving the ring's valid end and the lost count (and, with clip
// capture, the capture pass's header the clips' valid ends).  Never blocks
// unless wait_oldest (the header slots are all taken).
int fvad::eng::events_retire(fvad_engine *e, bool wait_oldest) {
  EventFeed &f = e->feed;
  while (!f.flight.empty()) {
    EventFeed::Pass &p = f.flight.front();
    const hipError_t q = hipEventQuery(p.done.get());
    if (q == hipErrorNotReady) {
      (void)hipGetLastError();
      if (!wait_oldest) break;
      HIP_TRY(hipEventSynchronize(p.done.get()));
    } else if (q != hipSuccess) {
      return fail(FVAD_EDEVICE, std::string("hipEventQuery (event feed): ") + hipGetErrorString(q));
    }
    wait_oldest = false;
    const volatile fvad::VadmEventHeader *h = f.hdr.get() + p.pass % kEvHeaders;
    if (h->pass != p.pass) return fail(FVAD_EDEVICE, "event feed: a finished pass left no header");
    f.end = h->end;
    f.lost = h->lost;
    f.pushes_done = p.push + 1;
    if (e->cap)
      if (const int rc = capture_retire(e, p.pass)) return rc;
    f.pool.push_back(std::move(p.done));
    f.flight.pop_front();
  }
  return FVAD_OK;
}

// k_vadm_events behind the machine pass just queued on the side stream
int fvad::eng::enqueue_events(fvad_engine *e, const fvad::VadmArgs &v, uint64_t push, int slot, bool timed) {
  EventFeed &f = e->feed;
  int rc = events_retire(e, false);
  if (!rc && f.flight.size() >= (size_t)kEvHeaders) rc = events_retire(e, true);
  if (rc) return rc;
  // the pass's `done` event: a retired one, or a new one; it stays in the
  // pool until the pass is queued (so also when a call below fails)
  if (f.pool.empty()) {
    fvad::event_ptr fresh;
    if ((rc = fvad::make_event(fresh))) return rc;
    f.pool.push_back(std::move(fresh));
  }
  const hipEvent_t done = f.pool.back().get();
  fvad::VadmEventArgs a{};
  a.stage = v.ev_stage;
  a.count = v.ev_count;
  a.ev_cap = v.ev_cap;
  a.n_lanes = e->cfg.n_streams * v.n;
  a.n_machines = v.n;
  a.chunk = f.chunk;
  a.ring = f.dv_ring;
  a.ring_cap = f.ring_cap;
  a.cursor = f.cursor.get();
  a.pass = f.pass_next;
  a.header = f.dv_hdr + a.pass % kEvHeaders;
  a.push = push;
  a.host_read = f.read;
  if (timed && (rc = f.tm.begin(slot, e->side))) return rc;
  HIP_TRY(fvad::launch_vadm_events(a, e->side));
  if (timed && (rc = f.tm.end(slot, e->side))) return rc;
  HIP_TRY(hipEventRecord(done, e->side));
  f.flight.push_back({a.pass, push, std::move(f.pool.back())});
  f.pool.pop_back();
  f.pass_next++;
  return FVAD_OK;
}

// the feed as after enable: nothing queued, cursors, pass and lost counts zero
// (the side stream is idle)
int fvad::eng::events_reset(fvad_engine *e) {
  EventFeed &f = e->feed;
  for (auto &p : f.flight) f.pool.push_back(std::move(p.done));
  f.flight.clear();
  HIP_TRY(hipMemset(f.cursor.get(), 0, 2 * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(f.count.get(), 0, sizeof(unsigned) * (size_t)e->cfg.n_streams * e->vadm.args.n));
  std::memset(f.hdr.get(), 0xff, sizeof(fvad::VadmEventHeader) * kEvHeaders);
  f.read = f.end = f.lost = f.pass_next = f.pushes_done = 0;
  f.tm.drop();
  return e->cap ? capture_reset(e) : FVAD_OK;
}

// All or nothing, as fvad_engine_attach_vadm: the feed is made in a local and
// moves into the engine after the last step that can fail.
extern "C" int fvad_engine_enable_events(fvad_engine *e, size_t ring_capacity) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  if (!e->vadm.on()) return fail(FVAD_EINVAL, "no VADMachines attached");
  if (e->feed.on()) return fail(FVAD_EINVAL, "events already enabled");
  for (const auto &sl : e->slots)
    if (sl.pending) return fail(FVAD_EINVAL, "submitted pushes not collected yet");
  if (ring_capacity == 0) ring_capacity = 65536;
  if (ring_capacity > (size_t)1 << 26) return fail(FVAD_EINVAL, "ring_capacity above 2^26 events");
  HIP_TRY(hipSetDevice(e->cfg.device));
  // a push whose machine pass is still pending runs it now, without events
  if (e->vadm.pend)
    if (const int rc = vadm_flush(e, false)) return rc;
  const size_t lanes = (size_t)e->cfg.n_streams * e->vadm.args.n;
  const int ev_cap = e->sg->wmax;  // windows of one stream in a push at most (one event each at most)
  EventFeed f;
  f.chunk = e->feed.chunk;  // (the hook may have been set already)
  int rc;
  if ((rc = fvad::make_dev(f.stage, lanes * ev_cap)) || (rc = fvad::make_dev(f.count, lanes)) ||
      (rc = fvad::make_dev(f.cursor, 2)) || (rc = fvad::make_pinned(f.ring, ring_capacity)) ||
      (rc = fvad::make_pinned(f.hdr, kEvHeaders)))
    return rc;
  void *dv_ring = nullptr, *dv_hdr = nullptr;
  if (hipHostGetDevicePointer(&dv_ring, f.ring.get(), 0) != hipSuccess ||
      hipHostGetDevicePointer(&dv_hdr, f.hdr.get(), 0) != hipSuccess) {
    (void)hipGetLastError();
    return fail(FVAD_EDEVICE, "hipHostGetDevicePointer failed (event feed)");
  }
  f.dv_ring = static_cast<fvad::VadmEvent *>(dv_ring);
  f.dv_hdr = static_cast<fvad::VadmEventHeader *>(dv_hdr);
  if ((rc = f.tm.create())) return rc;
  if (hipMemset(f.count.get(), 0, lanes * sizeof(unsigned)) != hipSuccess ||
      hipMemset(f.cursor.get(), 0, 2 * sizeof(unsigned long long)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(FVAD_EDEVICE, "hipMemset failed (event feed)");
  }
  std::memset(f.hdr.get(), 0xff, sizeof(fvad::VadmEventHeader) * kEvHeaders);
  f.ring_cap = ring_capacity;
  // nothing below fails
  e->feed = std::move(f);
  e->vadm.args.ev_stage = e->feed.stage.get();
  e->vadm.args.ev_count = e->feed.count.get();
  e->vadm.args.ev_cap = ev_cap;
  return FVAD_OK;
}

extern "C" int fvad_engine_poll_events(fvad_engine *e, fvad_event *out, size_t cap, size_t *n, uint64_t *lost) {
  if (n) *n = 0;
  if (!e || !n || (cap > 0 && !out)) return fail(FVAD_EINVAL, "invalid argument");
  if (!e->feed.on()) return fail(FVAD_EINVAL, "events not enabled");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (const int rc = events_retire(e, false)) return rc;
  EventFeed &f = e->feed;
  const size_t k = (size_t)std::min<uint64_t>(cap, f.end - f.read);
  for (size_t i = 0; i < k; i++) out[i] = f.ring.get()[(f.read + i) % f.ring_cap];
  f.read += k;
  *n = k;
  if (lost) *lost = f.lost;
  return FVAD_OK;
}

extern "C" int fvad_engine_event_progress(fvad_engine *e, uint64_t *pushes_done) {
  if (!e || !pushes_done) return fail(FVAD_EINVAL, "null argument");
  if (!e->feed.on()) return fail(FVAD_EINVAL, "events not enabled");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (const int rc = events_retire(e, false)) return rc;
  *pushes_done = e->feed.pushes_done;
  return FVAD_OK;
}

// (fvad_engine_sync collects the feed's samples)
extern "C" int fvad_engine_event_times(fvad_engine *e, double *ms_avg, int *n_runs) {
  if (!e || !ms_avg) return fail(FVAD_EINVAL, "null argument");
  if (!e->feed.on()) return fail(FVAD_EINVAL, "events not enabled");
  if (const int rc = fvad_engine_sync(e)) return rc;
  e->feed.tm.read(0, ms_avg, n_runs);
  return FVAD_OK;
}
