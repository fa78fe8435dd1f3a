// The batched engine's device VADMachines: attach, the machine pass of each
// push on the side stream, segments and state readback, the speech event
// feed, and the machines' test hooks.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fvad_engine_impl.h"

using namespace fvad::eng;

// Event feed: the passes whose `done` event has completed leave ev_flight, the
// newest one's header giving the ring's valid end and the lost count (and,
// with clip capture, the capture pass's header the clips' valid ends).  Never
// blocks unless wait_oldest (the header slots are all taken).
int fvad::eng::events_retire(fvad_engine *e, bool wait_oldest) {
  while (!e->ev_flight.empty()) {
    fvad_engine::EvPass &p = e->ev_flight.front();
    const hipError_t q = hipEventQuery(p.done.get());
    if (q == hipErrorNotReady) {
      (void)hipGetLastError();
      if (!wait_oldest) break;
      HIP_TRY(hipEventSynchronize(p.done.get()));
    } else if (q != hipSuccess) {
      return fail(FVAD_EDEVICE, std::string("hipEventQuery (event feed): ") + hipGetErrorString(q));
    }
    wait_oldest = false;
    const volatile fvad::VadmEventHeader *h = e->h_ev_hdr.get() + p.pass % fvad_engine::kEvHeaders;
    if (h->pass != p.pass) return fail(FVAD_EDEVICE, "event feed: a finished pass left no header");
    e->ev_end = h->end;
    e->ev_lost = h->lost;
    e->ev_pushes_done = p.push + 1;
    if (e->cap)
      if (const int rc = capture_retire(e, p.pass)) return rc;
    e->ev_pool.push_back(std::move(p.done));
    e->ev_flight.pop_front();
  }
  return FVAD_OK;
}

namespace {

// k_vadm_events behind the machine pass just queued on the side stream
int enqueue_events(fvad_engine *e, const fvad::VadmArgs &v, uint64_t push, int slot, bool timed) {
  int rc = events_retire(e, false);
  if (!rc && e->ev_flight.size() >= (size_t)fvad_engine::kEvHeaders) rc = events_retire(e, true);
  if (rc) return rc;
  // the pass's `done` event: a retired one, or a new one; it stays in the
  // pool until the pass is queued (so also when a call below fails)
  if (e->ev_pool.empty()) {
    fvad::event_ptr fresh;
    if ((rc = fvad::make_event(fresh))) return rc;
    e->ev_pool.push_back(std::move(fresh));
  }
  const hipEvent_t done = e->ev_pool.back().get();
  fvad::VadmEventArgs a{};
  a.stage = v.ev_stage;
  a.count = v.ev_count;
  a.ev_cap = v.ev_cap;
  a.n_lanes = e->cfg.n_streams * v.n;
  a.n_machines = v.n;
  a.chunk = e->dbg_events_chunk;
  a.ring = e->dv_ev_ring;
  a.ring_cap = e->ev_ring_cap;
  a.cursor = e->d_ev_cursor.get();
  a.pass = e->ev_pass_next;
  a.header = e->dv_ev_hdr + a.pass % fvad_engine::kEvHeaders;
  a.push = push;
  a.host_read = e->ev_read;
  if (timed && (rc = e->et[slot].begin(e->side))) return rc;
  HIP_TRY(fvad::launch_vadm_events(a, e->side));
  if (timed && (rc = e->et[slot].end(e->side))) return rc;
  HIP_TRY(hipEventRecord(done, e->side));
  e->ev_flight.push_back({a.pass, push, std::move(e->ev_pool.back())});
  e->ev_pool.pop_back();
  e->ev_pass_next++;
  return FVAD_OK;
}

// k_vadm of one push on the side stream (its waits already queued), with
// its timer and the events later pushes wait for
int enqueue_vadm(fvad_engine *e, const fvad::StagedArgs &v, int b, bool timed, bool fast) {
  const int slot = e->vadm_slot ^= 1;
  int rc;
  if (timed && (rc = e->vt[slot].begin(e->side))) return rc;  // (an unread older sample in this slot is dropped)
  bool par = false;
  // a sync point's flush (or the test hook's every push) leaves every machine
  // exact; between sync points k_vadm_hbm may owe its long-term fold
  fvad::StagedArgs vf = v;
  vf.vadm.vfinal = (fast || e->dbg_always_par) ? 1 : 0;
  e->vowed = false;  // (a final pass resolves every machine, those without ticks included)
  // per-stream configs: k_vadm_par_ps only while every row has an initial
  // average (a machine whose long-term buffer is still filling folds it whole
  // at every push: k_vadm_hbm_ps' lane each, not a group's leader lane)
  const bool rows_par = !e->vadm_ps || e->vadm_nopar == 0;
  HIP_TRY(fvad::launch_vadm(vf, e->side, (fast || e->dbg_always_par) && rows_par, &par));
  if (!vf.vadm.vfinal) {
    e->vowed = true;
    e->vowed_args = vf;
  }
  if (timed) {
    if ((rc = e->vt[slot].end(e->side))) return rc;
    e->vadm_kind[slot] = par ? 1 : 0;
  }
  if (vf.vadm.ev_stage) {
    // the window outputs are free once the machines have read them: the
    // next push but one does not wait for the event pass
    HIP_TRY(hipEventRecord(e->ev_vadm_b[b].get(), e->side));
    // the capture pass reads the staged records before k_vadm_events clears
    // their counts, and becomes visible with that pass's `done` event
    if (e->cap && (rc = capture_pass(e, vf.vadm, e->vpend_push, b, slot, timed))) return rc;
    if ((rc = enqueue_events(e, vf.vadm, e->vpend_push, slot, timed))) return rc;
    HIP_TRY(hipEventRecord(e->ev_vadm.get(), e->side));
    return FVAD_OK;
  }
  HIP_TRY(hipEventRecord(e->ev_vadm.get(), e->side));
  HIP_TRY(hipEventRecord(e->ev_vadm_b[b].get(), e->side));
  return FVAD_OK;
}

}  // namespace

// the feed as after enable: nothing queued, cursors, pass and lost counts zero
// (the side stream is idle)
int fvad::eng::events_reset(fvad_engine *e) {
  for (auto &p : e->ev_flight) e->ev_pool.push_back(std::move(p.done));
  e->ev_flight.clear();
  HIP_TRY(hipMemset(e->d_ev_cursor.get(), 0, 2 * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(e->vadm.ev_count, 0, sizeof(unsigned) * (size_t)e->cfg.n_streams * e->vadm.n));
  std::memset(e->h_ev_hdr.get(), 0xff, sizeof(fvad::VadmEventHeader) * fvad_engine::kEvHeaders);
  e->ev_read = e->ev_end = e->ev_lost = e->ev_pass_next = e->ev_pushes_done = 0;
  for (EventTimer &t : e->et) t.pending = false;
  return e->cap ? capture_reset(e) : FVAD_OK;
}

// the last push's VADMachine, enqueued now (after its push's kernels);
// fast: nothing else is queued behind it (a sync point)
int fvad::eng::vadm_flush(fvad_engine *e, bool fast) {
  if (!e->vpend) {
    if (fast && e->vowed) {
      // folds owed with no push pending (a push whose launch failed after
      // the previous push's non-final pass was queued): k_vadm_hbm with no
      // ticks and vfinal = 1 only resolves them
      fvad::StagedArgs r = e->vowed_args;
      r.n_ticks = 0;
      r.ticks_valid = nullptr;
      r.vadm = e->vadm;
      r.vadm.vfinal = 1;
      e->vowed = false;
      HIP_TRY(fvad::launch_vadm(r, e->side, false, nullptr));
      HIP_TRY(hipEventRecord(e->ev_vadm.get(), e->side));
    }
    return FVAD_OK;
  }
  e->vpend = false;
  // the push's end: ev_buf_free of its parity (recorded after its kernels and
  // ticks copy; re-recorded only by the push after next)
  HIP_TRY(hipStreamWaitEvent(e->side, e->ev_buf_free[e->vpend_b].get(), 0));
  // a flush at a sync point (k_vadm_par, the job's drain) is always timed:
  // its event pair sits on the side stream, after everything else
  return enqueue_vadm(e, e->vpend_args, e->vpend_b, e->vpend_timed || fast, fast);
}

// VADMachine and k_vadm_events samples whose end event has completed
// (non-blocking), the former by kernel
int fvad::eng::collect_vadm_timing(fvad_engine *e) {
  int rc;
  for (int k = 0; k < 2; k++)
    if ((rc = e->vt[k].collect(e->vadm_ms_sum[e->vadm_kind[k]], e->vadm_timed[e->vadm_kind[k]]))) return rc;
  for (EventTimer &t : e->et)
    if ((rc = t.collect(e->et_ms_sum, e->et_timed))) return rc;
  return capture_collect_timing(e);
}

// ---------------------------------------------------------------------------
// Device VADMachines (VADMachine.zig:126-230 on the GPU)
// ---------------------------------------------------------------------------
namespace {
// a fresh machine's state and rolling buffers into the device arrays of v
int vadm_upload(const fvad_engine *e, const fvad::VadmArgs &v, const std::vector<fvad::VadmState> &init,
                size_t buf_len) {
  std::vector<fvad::VadmState> st = init;
  if (!e->dbg_lt_full) {
    // every entry 0.0f (initial entries are K.init, tracked by lt_nw): a device
    // memset, no host image of the buffers (hundreds of MB at 2048 streams)
    HIP_TRY(hipMemset(v.buf, 0, buf_len * sizeof(float)));
  } else {
    std::vector<float> buf(buf_len, 0.0f);
    // test hook FVAD_DEBUG_VADM_LT_FULL: every long-term entry counts as pushed
    // (holding (float)init), the state of a stream past its first
    // long_term_speech_avg_sec -- timing only, not the reference's values
    const int B = e->cfg.n_streams;
    for (int m = 0; m < v.n; m++) {
      const fvad::VadmConst &K = v.c[m];
      for (int s = 0; s < B; s++) {
        // (per-stream configs: the stream's own length and initial average)
        const fvad::VadmRow *row = e->vadm_ps ? &e->vadm_rows[(size_t)m * B + s] : nullptr;
        const int n_lt = row ? row->n_lt : K.n_lt;
        const float init = (float)(row ? row->init : K.init);
        for (int i = 0; i < n_lt; i++) buf[K.lt_off + (size_t)s * K.lt_pitch + i] = init;
        st[(size_t)m * B + s].lt_nw = (unsigned)n_lt;
      }
    }
    HIP_TRY(hipMemcpy(v.buf, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(v.st, st.data(), st.size() * sizeof(fvad::VadmState), hipMemcpyHostToDevice));
  return FVAD_OK;
}
}  // namespace

int fvad::eng::vadm_reset(fvad_engine *e) { return vadm_upload(e, e->vadm, e->vadm_init, e->vadm_buf_len); }

namespace {
// All or nothing: every buffer, the side stream, the events and the initial
// state upload are made into locals, and move into the engine after the last
// step that can fail.  A failed call leaves the engine unattached.
// ps (fvad_engine_attach_vadm_ex): a constant table row per (machine, stream),
// every stream starting on cfgs[m]; the rolling buffers are laid out for the
// room, each of a machine's three lengths the maximum over cfgs[m] and room[].
int attach(fvad_engine *e, const fvad_vadm_config *cfgs, int n, int seg_capacity, bool ps,
           const fvad_vadm_config *room, int n_room) {
  if (!e || !cfgs || n < 1 || n > FVAD_MAX_BANDS || seg_capacity < 1 || n_room < 0 || (n_room > 0 && !room))
    return fail(FVAD_EINVAL, "invalid argument");
  if (e->cfg.mode == FVAD_MODE_FUSED) return fail(FVAD_EINVAL, "device VADMachines need the staged engine");
  if (e->vadm.n > 0) return fail(FVAD_EINVAL, "VADMachines already attached");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int B = e->cfg.n_streams;
  fvad::VadmArgs v{};
  v.n = n;
  v.seg_cap = seg_capacity;
  v.bound_scale = 1.0;
  v.negate_at = -1;
  long long off = 0;
  std::vector<fvad::VadmState> init((size_t)n * B);
  std::vector<fvad::VadmRow> rows(ps ? (size_t)n * B : 0);
  size_t nopar = 0;
  for (int m = 0; m < n; m++) {
    const fvad::VadmDerived d = fvad::vadm_derive(cfgs[m], e->cfg.sample_rate, e->cfg.fft_size);
    fvad::VadmConst &K = v.c[m] = d.K;
    K.slot = fvad::band_slot(e->cfg.band_lo, e->cfg.band_hi, e->cfg.n_bands, d.lo, d.hi);
    if (K.slot < 0) return fail(FVAD_EINVAL, "no engine band matches the machine's speech band");
    if (ps) {
      for (int s = 0; s < B; s++) rows[(size_t)m * B + s] = fvad::vadm_row(d, K.slot);
      if (!K.has_init) nopar += (size_t)B;
      for (int i = 0; i < n_room; i++) {
        const fvad::VadmConst R = fvad::vadm_derive(room[i], e->cfg.sample_rate, e->cfg.fft_size).K;
        K.n_lt = std::max(K.n_lt, R.n_lt);
        K.n_st = std::max(K.n_st, R.n_st);
        K.n_r = std::max(K.n_r, R.n_r);
      }
      K.lt_pitch = (K.n_lt + 3) & ~3;
    }
    off = (off + 3) & ~3LL;  // (the long-term rows start 16-byte aligned)
    K.lt_off = off;
    off += (long long)K.lt_pitch * B;
    K.st_off = off;
    off += (long long)K.n_st * B;
    K.r_off = off;
    off += (long long)K.n_r * B;
    for (int s = 0; s < B; s++) init[(size_t)m * B + s] = d.s0;
  }
  fvad::dev_ptr<fvad::VadmState> st;
  fvad::dev_ptr<float> buf;
  fvad::dev_ptr<fvad::VadmSeg> seg;
  fvad::dev_ptr<fvad::VadmRow> tab;
  fvad_engine::WinOut set1;  // the second window-output set (push parity 1); set 0 is the engine's own
  fvad::dev_ptr<int32_t> vticks0;
  fvad::stream_ptr side;
  fvad::event_ptr ev_vadm, ev_vadm_b[2];
  EventTimer vt[2];
  int rc;
  if (ps && (rc = fvad::make_dev(tab, rows.size()))) return rc;
  if ((rc = fvad::make_dev(st, init.size())) || (rc = fvad::make_dev(buf, (size_t)off)) ||
      (rc = fvad::make_dev(seg, (size_t)n * B * seg_capacity)) || (rc = make_win_out(e, set1)) ||
      (rc = fvad::make_dev(vticks0, (size_t)B)) || (rc = fvad::make_dev(set1.vticks, (size_t)B)) ||
      (rc = fvad::make_stream(side)) || (rc = fvad::make_event(ev_vadm)) || (rc = vt[0].create()) ||
      (rc = vt[1].create()) || (rc = fvad::make_event(ev_vadm_b[0])) || (rc = fvad::make_event(ev_vadm_b[1])))
    return rc;
  HIP_TRY(hipEventRecord(ev_vadm.get(), side.get()));
  HIP_TRY(hipEventRecord(ev_vadm_b[0].get(), side.get()));
  HIP_TRY(hipEventRecord(ev_vadm_b[1].get(), side.get()));
  v.st = st.get();
  v.buf = buf.get();
  v.seg = seg.get();
  v.tab = tab.get();
  if ((rc = vadm_upload(e, v, init, (size_t)off))) return rc;
  if (ps) HIP_TRY(hipMemcpy(v.tab, rows.data(), rows.size() * sizeof(fvad::VadmRow), hipMemcpyHostToDevice));
  // nothing below fails
  e->vadm = v;
  e->vadm_st = std::move(st);
  e->vadm_buf = std::move(buf);
  e->vadm_seg = std::move(seg);
  e->vadm_init = std::move(init);
  e->vadm_cfgs.assign(cfgs, cfgs + n);
  e->vadm_buf_len = (size_t)off;
  e->vadm_ps = ps;
  e->vadm_tab = std::move(tab);
  e->vadm_rows = std::move(rows);
  e->vadm_nopar = nopar;
  if (ps) {
    e->vadm_stream_cfgs.resize((size_t)n * B);
    for (int m = 0; m < n; m++) std::fill_n(e->vadm_stream_cfgs.begin() + (size_t)m * B, (size_t)B, cfgs[m]);
  }
  e->wout[0].vticks = std::move(vticks0);
  e->wout[1] = std::move(set1);
  e->side_ref = std::move(side);
  e->side = e->side_ref.get();
  e->ev_vadm = std::move(ev_vadm);
  for (int k = 0; k < 2; k++) {
    e->ev_vadm_b[k] = std::move(ev_vadm_b[k]);
    e->vt[k] = std::move(vt[k]);
  }
  return FVAD_OK;
}
}  // namespace

extern "C" int fvad_engine_attach_vadm(fvad_engine *e, const fvad_vadm_config *cfgs, int n, int seg_capacity) {
  return attach(e, cfgs, n, seg_capacity, false, nullptr, 0);
}

extern "C" int fvad_engine_attach_vadm_ex(fvad_engine *e, const fvad_vadm_config *cfgs, int n, int seg_capacity,
                                          const fvad_vadm_config *room, int n_room) {
  return attach(e, cfgs, n, seg_capacity, true, room, n_room);
}

// Everything is checked and every row derived before the first launch; the
// launches then go on the side stream behind the pending machine pass, the
// rows in their argument blocks (kRetargetMax per launch), and the host mirror
// follows each launch that was queued.
extern "C" int fvad_engine_set_stream_vadm(fvad_engine *e, const int32_t *streams, int n, int machine,
                                           const fvad_vadm_config *cfgs) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  if (!e->vadm_ps)
    return fail(FVAD_EINVAL, "fvad_engine_set_stream_vadm needs an engine attached with fvad_engine_attach_vadm_ex");
  if (const int rc = check_stream_list(e, streams, n)) return rc;
  if (machine < 0 || machine >= e->vadm.n) return fail(FVAD_EINVAL, "no such attached machine");
  if (n == 0) return FVAD_OK;
  if (!cfgs) return fail(FVAD_EINVAL, "null configs");
  if (e->dbg_lt_full)
    return fail(FVAD_EINVAL, "fvad_engine_set_stream_vadm is not available under FVAD_DEBUG_VADM_LT_FULL");
  const int B = e->cfg.n_streams;
  const fvad::VadmConst &K = e->vadm.c[machine];  // the room
  std::vector<fvad::VadmRow> rows((size_t)n);
  std::vector<fvad::VadmState> fresh((size_t)n);
  for (int i = 0; i < n; i++) {
    const fvad::VadmDerived d = fvad::vadm_derive(cfgs[i], e->cfg.sample_rate, e->cfg.fft_size);
    const int slot = fvad::band_slot(e->cfg.band_lo, e->cfg.band_hi, e->cfg.n_bands, d.lo, d.hi);
    if (slot < 0)
      return fail(FVAD_EINVAL, "stream " + std::to_string(streams[i]) + ": no engine band matches the config's speech band");
    const int len[3] = {d.K.n_lt, d.K.n_st, d.K.n_r}, cap[3] = {K.n_lt, K.n_st, K.n_r};
    static const char *const name[3] = {"long-term", "short-term", "volume ratio"};
    for (int k = 0; k < 3; k++)
      if (len[k] > cap[k])
        return fail(FVAD_EINVAL, "stream " + std::to_string(streams[i]) + ": " + name[k] + " length " +
                                     std::to_string(len[k]) + " exceeds the attached room of " + std::to_string(cap[k]));
    rows[i] = fvad::vadm_row(d, slot);
    fresh[i] = d.s0;
  }
  HIP_TRY(hipSetDevice(e->cfg.device));
  // the previous push's machine pass sees the old configs: queued first
  if (e->vpend)
    if (const int rc = vadm_flush(e, false)) return rc;
  fvad::RetargetArgs a{};
  a.st = e->vadm.st;
  a.buf = e->vadm.buf;
  a.tab = e->vadm.tab;
  a.n_streams = B;
  a.machine = machine;
  a.lt_pitch = K.lt_pitch;
  a.n_st = K.n_st;
  a.n_r = K.n_r;
  a.lt_off = K.lt_off;
  a.st_off = K.st_off;
  a.r_off = K.r_off;
  for (int i0 = 0; i0 < n; i0 += fvad::kRetargetMax) {
    a.n = std::min(fvad::kRetargetMax, n - i0);
    for (int i = 0; i < a.n; i++) {
      a.id[i] = streams[i0 + i];
      a.row[i] = rows[i0 + i];
    }
    HIP_TRY(fvad::launch_vadm_retarget(a, e->side));
    for (int i = 0; i < a.n; i++) {
      const size_t idx = (size_t)machine * B + streams[i0 + i];
      e->vadm_nopar += (size_t)!rows[i0 + i].has_init;
      e->vadm_nopar -= (size_t)!e->vadm_rows[idx].has_init;
      e->vadm_rows[idx] = rows[i0 + i];
      e->vadm_stream_cfgs[idx] = cfgs[i0 + i];
      e->vadm_init[idx] = fresh[i0 + i];
    }
  }
  return FVAD_OK;
}

extern "C" int fvad_engine_stream_vadm_config(const fvad_engine *e, int stream, int machine, fvad_vadm_config *out) {
  if (!e || !out || e->vadm.n == 0 || stream < 0 || stream >= e->cfg.n_streams || machine < 0 || machine >= e->vadm.n)
    return fail(FVAD_EINVAL, "no such attached machine");
  *out = e->vadm_ps ? e->vadm_stream_cfgs[(size_t)machine * e->cfg.n_streams + stream] : e->vadm_cfgs[machine];
  return FVAD_OK;
}

extern "C" size_t fvad_engine_segments(fvad_engine *e, int stream, int machine, fvad_segment *out, size_t cap) {
  return fvad_engine_segments_range(e, stream, machine, 0, out, cap);
}

extern "C" int fvad_engine_vadm_state(fvad_engine *e, int stream, int machine, int *speech_state,
                                      uint64_t *speech_start, uint64_t *speech_end) {
  if (!e || e->vadm.n == 0 || stream < 0 || stream >= e->cfg.n_streams || machine < 0 || machine >= e->vadm.n)
    return fail(FVAD_EINVAL, "no such attached machine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream.get()));
  if (const int rf = vadm_flush(e, true)) return rf;
  HIP_TRY(hipStreamSynchronize(e->side));
  fvad::VadmState st;
  HIP_TRY(hipMemcpy(&st, e->vadm.st + (size_t)machine * e->cfg.n_streams + stream, sizeof(st),
                    hipMemcpyDeviceToHost));
  if (speech_state) *speech_state = st.state;
  if (speech_start) *speech_start = st.speech_start;
  if (speech_end) *speech_end = st.speech_end;
  return FVAD_OK;
}

extern "C" size_t fvad_engine_segments_range(fvad_engine *e, int stream, int machine, size_t first,
                                             fvad_segment *out, size_t cap) {
  if (!e || e->vadm.n == 0 || stream < 0 || stream >= e->cfg.n_streams || machine < 0 || machine >= e->vadm.n)
    return 0;
  if (hipSetDevice(e->cfg.device) != hipSuccess || vadm_flush(e, true) != FVAD_OK ||
      hipStreamSynchronize(e->stream.get()) != hipSuccess || hipStreamSynchronize(e->side) != hipSuccess)
    return 0;
  const size_t idx = (size_t)machine * e->cfg.n_streams + stream;
  fvad::VadmState st;
  if (hipMemcpy(&st, e->vadm.st + idx, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  const size_t n = std::min<size_t>(st.n_segs, (size_t)e->vadm.seg_cap);
  const size_t k = first < n ? std::min(n - first, cap) : 0;
  // (a VadmSeg is an fvad_segment: fvad_machine.h)
  if (out && k &&
      hipMemcpy(out, e->vadm.seg + idx * e->vadm.seg_cap + first, k * sizeof(fvad_segment), hipMemcpyDeviceToHost) !=
          hipSuccess)
    return 0;
  return st.n_segs;
}

// ---------------------------------------------------------------------------
// Speech event feed
// ---------------------------------------------------------------------------
static_assert(sizeof(fvad_event) == 48 && sizeof(fvad::VadmEvent) == sizeof(fvad_event), "fvad_event is 48 bytes");
static_assert(offsetof(fvad_event, push) == offsetof(fvad::VadmEvent, push) &&
                  offsetof(fvad_event, sample_to) == offsetof(fvad::VadmEvent, sample_to) &&
                  offsetof(fvad_event, debug_avg_speech_vol_ratio) ==
                      offsetof(fvad::VadmEvent, debug_avg_speech_vol_ratio),
              "the device's event record is fvad_event");

extern "C" int fvad_engine_enable_events(fvad_engine *e, size_t ring_capacity) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  if (e->vadm.n == 0) return fail(FVAD_EINVAL, "no VADMachines attached");
  if (e->events_on) return fail(FVAD_EINVAL, "events already enabled");
  for (const auto &sl : e->slots)
    if (sl.pending) return fail(FVAD_EINVAL, "submitted pushes not collected yet");
  if (ring_capacity == 0) ring_capacity = 65536;
  if (ring_capacity > (size_t)1 << 26) return fail(FVAD_EINVAL, "ring_capacity above 2^26 events");
  HIP_TRY(hipSetDevice(e->cfg.device));
  // a push whose machine pass is still pending runs it now, without events
  if (e->vpend)
    if (const int rc = vadm_flush(e, false)) return rc;
  const size_t lanes = (size_t)e->cfg.n_streams * e->vadm.n;
  const int ev_cap = e->wmax;  // windows of one stream in a push at most (one event each at most)
  // all or nothing, as fvad_engine_attach_vadm: locals first
  fvad::dev_ptr<fvad::VadmEvRec> stage;
  fvad::dev_ptr<unsigned> count;
  fvad::dev_ptr<unsigned long long> cursor;
  fvad::pinned_ptr<fvad_event> ring;
  fvad::pinned_ptr<fvad::VadmEventHeader> hdr;
  EventTimer et[2];
  int rc;
  if ((rc = fvad::make_dev(stage, lanes * ev_cap)) || (rc = fvad::make_dev(count, lanes)) ||
      (rc = fvad::make_dev(cursor, 2)) || (rc = fvad::make_pinned(ring, ring_capacity)) ||
      (rc = fvad::make_pinned(hdr, fvad_engine::kEvHeaders)))
    return rc;
  void *dv_ring = nullptr, *dv_hdr = nullptr;
  if (hipHostGetDevicePointer(&dv_ring, ring.get(), 0) != hipSuccess ||
      hipHostGetDevicePointer(&dv_hdr, hdr.get(), 0) != hipSuccess) {
    (void)hipGetLastError();
    return fail(FVAD_EDEVICE, "hipHostGetDevicePointer failed (event feed)");
  }
  if ((rc = et[0].create()) || (rc = et[1].create())) return rc;
  if (hipMemset(count.get(), 0, lanes * sizeof(unsigned)) != hipSuccess ||
      hipMemset(cursor.get(), 0, 2 * sizeof(unsigned long long)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(FVAD_EDEVICE, "hipMemset failed (event feed)");
  }
  std::memset(hdr.get(), 0xff, sizeof(fvad::VadmEventHeader) * fvad_engine::kEvHeaders);
  // nothing below fails
  e->ev_stage = std::move(stage);
  e->ev_count = std::move(count);
  e->vadm.ev_stage = e->ev_stage.get();
  e->vadm.ev_count = e->ev_count.get();
  e->vadm.ev_cap = ev_cap;
  e->d_ev_cursor = std::move(cursor);
  e->h_ev_ring = std::move(ring);
  e->dv_ev_ring = static_cast<fvad::VadmEvent *>(dv_ring);
  e->h_ev_hdr = std::move(hdr);
  e->dv_ev_hdr = static_cast<fvad::VadmEventHeader *>(dv_hdr);
  e->ev_ring_cap = ring_capacity;
  e->ev_read = e->ev_end = e->ev_lost = e->ev_pass_next = 0;
  for (int k = 0; k < 2; k++) e->et[k] = std::move(et[k]);
  e->events_on = true;
  return FVAD_OK;
}

extern "C" int fvad_engine_poll_events(fvad_engine *e, fvad_event *out, size_t cap, size_t *n, uint64_t *lost) {
  if (n) *n = 0;
  if (!e || !n || (cap > 0 && !out)) return fail(FVAD_EINVAL, "invalid argument");
  if (!e->events_on) return fail(FVAD_EINVAL, "events not enabled");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (const int rc = events_retire(e, false)) return rc;
  const size_t k = (size_t)std::min<uint64_t>(cap, e->ev_end - e->ev_read);
  for (size_t i = 0; i < k; i++) out[i] = e->h_ev_ring.get()[(e->ev_read + i) % e->ev_ring_cap];
  e->ev_read += k;
  *n = k;
  if (lost) *lost = e->ev_lost;
  return FVAD_OK;
}

extern "C" int fvad_engine_event_progress(fvad_engine *e, uint64_t *pushes_done) {
  if (!e || !pushes_done) return fail(FVAD_EINVAL, "null argument");
  if (!e->events_on) return fail(FVAD_EINVAL, "events not enabled");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (const int rc = events_retire(e, false)) return rc;
  *pushes_done = e->ev_pushes_done;
  return FVAD_OK;
}

extern "C" int fvad_engine_event_times(fvad_engine *e, double *ms_avg, int *n_runs) {
  if (!e || !ms_avg) return fail(FVAD_EINVAL, "null argument");
  if (!e->events_on) return fail(FVAD_EINVAL, "events not enabled");
  if (const int rc = fvad_engine_sync(e)) return rc;
  *ms_avg = e->et_timed ? e->et_ms_sum / e->et_timed : 0.0;
  if (n_runs) *n_runs = e->et_timed;
  return FVAD_OK;
}

// ---------------------------------------------------------------------------
// Checker access: the whole device machine state and the test hooks
// ---------------------------------------------------------------------------
namespace {
int vadm_read_state(fvad_engine *e, int stream, int machine, fvad::VadmState *st) {
  if (!e || e->vadm.n == 0 || stream < 0 || stream >= e->cfg.n_streams || machine < 0 || machine >= e->vadm.n)
    return fail(FVAD_EINVAL, "no such attached machine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (const int rc = fvad_engine_sync(e)) return rc;
  HIP_TRY(hipMemcpy(st, e->vadm.st + (size_t)machine * e->cfg.n_streams + stream, sizeof(*st),
                    hipMemcpyDeviceToHost));
  return FVAD_OK;
}
}  // namespace

extern "C" int fvad_engine_vadm_snapshot(fvad_engine *e, int stream, int machine, fvad_vadm_snapshot *out) {
  if (!out) return fail(FVAD_EINVAL, "null argument");
  fvad::VadmState st;
  if (const int rc = vadm_read_state(e, stream, machine, &st)) return rc;
  fvad::vadm_snapshot_of(st, out);
  return FVAD_OK;
}

extern "C" long fvad_engine_vadm_rolling(fvad_engine *e, int stream, int machine, int which, double *out, size_t cap) {
  if (which < 0 || which > 2) return fail(FVAD_EINVAL, "which: 0 long-term, 1 short-term, 2 volume ratio");
  fvad::VadmState st;
  if (const int rc = vadm_read_state(e, stream, machine, &st)) return rc;
  const fvad::VadmConst &K = e->vadm.c[machine];
  const size_t B = e->cfg.n_streams;
  // per-stream configs: the stream's own lengths and initial average inside the room's layout
  const fvad::VadmRow *row = e->vadm_ps ? &e->vadm_rows[(size_t)machine * B + stream] : nullptr;
  const int n = row ? (which == 0 ? row->n_lt : which == 1 ? row->n_st : row->n_r)
                    : (which == 0 ? K.n_lt : which == 1 ? K.n_st : K.n_r);
  const int has_init = row ? row->has_init : K.has_init;
  const double init = row ? row->init : K.init;
  const long long off = which == 0 ? K.lt_off : which == 1 ? K.st_off : K.r_off;
  const size_t k = std::min<size_t>((size_t)n, cap);
  if (out && k) {
    // long-term entries: the stream's row; the others [i][stream]: a strided 2D copy of its column
    std::vector<float> col(k);
    if (which == 0)
      HIP_TRY(hipMemcpy(col.data(), e->vadm.buf + off + (size_t)stream * K.lt_pitch, k * sizeof(float),
                        hipMemcpyDeviceToHost));
    else
      HIP_TRY(hipMemcpy2D(col.data(), sizeof(float), e->vadm.buf + off + stream, B * sizeof(float), sizeof(float), k,
                          hipMemcpyDeviceToHost));
    for (size_t i = 0; i < k; i++)
      // long-term entries never written since the machine started hold the
      // initial average, a double (RollingAverage.zig:16-32; lt_nw counts the written)
      out[i] = (which == 0 && has_init && i >= st.lt_nw) ? init : (double)col[i];
  }
  return n;
}

extern "C" int fvad_engine_set_debug(fvad_engine *e, int key, int value) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  switch (key) {
    case FVAD_DEBUG_VADM_PAR_SERIAL_EVERY:
      if (value < 0) return fail(FVAD_EINVAL, "value >= 0 required");
      e->vadm.par_serial_every = value;
      return FVAD_OK;
    case FVAD_DEBUG_VADM_ALWAYS_PAR:
      e->dbg_always_par = value != 0;
      return FVAD_OK;
    case FVAD_DEBUG_VADM_DEFER_MAX:
      if (value < 0) return fail(FVAD_EINVAL, "value >= 0 required");
      e->vadm.defer_max = (unsigned)value;
      return FVAD_OK;
    case FVAD_DEBUG_VADM_BOUND_SCALE:
      if (e->vadm.n == 0) return fail(FVAD_EINVAL, "no VADMachines attached");
      if (value < -1) return fail(FVAD_EINVAL, "value >= -1 required");
      if (const int rc = fvad_engine_sync(e)) return rc;  // a queued k_vadm_hbm reads the argument block's copy
      e->vadm.bound_scale = value == -1 ? HUGE_VAL : (value == 0 ? 1.0 : (double)value);
      return FVAD_OK;
    case FVAD_DEBUG_VADM_NEGATE_AT:
      if (e->vadm.n == 0) return fail(FVAD_EINVAL, "no VADMachines attached");
      if (value < -1) return fail(FVAD_EINVAL, "value >= -1 required");
      if (const int rc = fvad_engine_sync(e)) return rc;
      e->vadm.negate_at = value;
      return FVAD_OK;
    case FVAD_DEBUG_VADM_COUNT:
      if (e->vadm.n == 0) return fail(FVAD_EINVAL, "no VADMachines attached");
      if (const int rc = fvad_engine_sync(e)) return rc;
      if (value && !e->vadm_count)
        if (const int rc = fvad::make_dev(e->vadm_count, fvad::kVadmCounts)) return rc;
      if (!value) e->vadm_count.reset();
      e->vadm.count = e->vadm_count.get();
      if (e->vadm.count) HIP_TRY(hipMemset(e->vadm.count, 0, fvad::kVadmCounts * sizeof(unsigned long long)));
      return FVAD_OK;
    case FVAD_DEBUG_VADM_LT_FULL:
      if (e->vadm.n == 0) return fail(FVAD_EINVAL, "no VADMachines attached");
      e->dbg_lt_full = value != 0;
      if (const int rc = fvad_engine_sync(e)) return rc;
      return vadm_reset(e);
    case FVAD_DEBUG_RESET_TIMES:
      e->dbg_reset_times = value != 0;
      return FVAD_OK;
    case FVAD_DEBUG_EVENTS_CHUNK:
      if (value < 0) return fail(FVAD_EINVAL, "value >= 0 required");
      e->dbg_events_chunk = value;
      return FVAD_OK;
    default:
      return fail(FVAD_EINVAL, "unknown debug key");
  }
}

extern "C" int fvad_engine_debug_counts(fvad_engine *e, unsigned long long *out, int n) {
  if (!e || !out || n < 1) return fail(FVAD_EINVAL, "invalid argument");
  if (!e->vadm.count) return fail(FVAD_EINVAL, "FVAD_DEBUG_VADM_COUNT is not set");
  if (const int rc = fvad_engine_sync(e)) return rc;
  unsigned long long c[fvad::kVadmCounts];
  HIP_TRY(hipMemcpy(c, e->vadm.count, sizeof(c), hipMemcpyDeviceToHost));
  const int k = std::min(n, (int)fvad::kVadmCounts);
  for (int i = 0; i < k; i++) out[i] = c[i];
  return k;
}
