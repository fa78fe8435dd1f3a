// The batched engine's device VADMachines (eng::Vadm): attach, the machine
// pass of each push on the side stream, segments and state readback, and the
// machines' and the feed's test hooks.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fvad_engine_impl.h"

using namespace fvad::eng;

namespace {

// k_vadm of one push on the side stream (its waits already queued), with
// its timer and the events later pushes wait for
int enqueue_vadm(fvad_engine *e, const fvad::StagedArgs &v, int b, bool timed, bool fast) {
  const int slot = e->vadm.slot ^= 1;
  int rc;
  if (timed && (rc = e->vadm.tm.begin(slot, e->side))) return rc;  // (an unread older sample in this slot is dropped)
  bool par = false;
  // a sync point's flush (or the test hook's every push) leaves every machine
  // exact; between sync points k_vadm_hbm may owe its long-term fold
  fvad::StagedArgs vf = v;
  vf.vadm.vfinal = (fast || e->vadm.always_par) ? 1 : 0;
  e->vadm.owed = false;  // (a final pass resolves every machine, those without ticks included)
  // per-stream configs: k_vadm_par_ps only while every row has an initial
  // average (a machine whose long-term buffer is still filling folds it whole
  // at every push: k_vadm_hbm_ps' lane each, not a group's leader lane)
  const bool rows_par = !e->vadm.ps || e->vadm.nopar == 0;
  HIP_TRY(fvad::launch_vadm(vf, e->side, (fast || e->vadm.always_par) && rows_par, &par));
  if (!vf.vadm.vfinal) {
    e->vadm.owed = true;
    e->vadm.owed_args = vf;
  }
  if (timed && (rc = e->vadm.tm.end(slot, e->side, par ? 1 : 0))) return rc;
  if (vf.vadm.ev_stage) {
    // the window outputs are free once the machines have read them: the
    // next push but one does not wait for the event pass
    HIP_TRY(hipEventRecord(e->vadm.ev_set_free[b].get(), e->side));
    // the capture pass reads the staged records before k_vadm_events clears
    // their counts, and becomes visible with that pass's `done` event
    if (e->cap && (rc = capture_pass(e, vf.vadm, e->vadm.pend_push, b, slot, timed))) return rc;
    if ((rc = enqueue_events(e, vf.vadm, e->vadm.pend_push, slot, timed))) return rc;
    HIP_TRY(hipEventRecord(e->vadm.ev_done.get(), e->side));
    return FVAD_OK;
  }
  HIP_TRY(hipEventRecord(e->vadm.ev_done.get(), e->side));
  HIP_TRY(hipEventRecord(e->vadm.ev_set_free[b].get(), e->side));
  return FVAD_OK;
}

}  // namespace

// the last push's VADMachine, enqueued now (after its push's kernels);
// fast: nothing else is queued behind it (a sync point)
int fvad::eng::vadm_flush(fvad_engine *e, bool fast) {
  if (!e->vadm.pend) {
    if (fast && e->vadm.owed) {
      // folds owed with no push pending (a push whose launch failed after
      // the previous push's non-final pass was queued): k_vadm_hbm with no
      // ticks and vfinal = 1 only resolves them
      fvad::StagedArgs r = e->vadm.owed_args;
      r.n_ticks = 0;
      r.ticks_valid = nullptr;
      r.vadm = e->vadm.args;
      r.vadm.vfinal = 1;
      e->vadm.owed = false;
      HIP_TRY(fvad::launch_vadm(r, e->side, false, nullptr));
      HIP_TRY(hipEventRecord(e->vadm.ev_done.get(), e->side));
    }
    return FVAD_OK;
  }
  e->vadm.pend = false;
  // the push's end: ev_buf_free of its parity (recorded after its kernels and
  // ticks copy; re-recorded only by the push after next)
  HIP_TRY(hipStreamWaitEvent(e->side, e->sg->ev_buf_free[e->vadm.pend_b].get(), 0));
  // a flush at a sync point (k_vadm_par, the job's drain) is always timed:
  // its event pair sits on the side stream, after everything else
  return enqueue_vadm(e, e->vadm.pend_args, e->vadm.pend_b, e->vadm.pend_timed || fast, fast);
}

// VADMachine and k_vadm_events samples whose end event has completed
// (non-blocking), the former by kernel
int fvad::eng::collect_vadm_timing(fvad_engine *e) {
  int rc = e->vadm.tm.collect();
  if (!rc) rc = e->feed.tm.collect();
  return rc ? rc : capture_collect_timing(e);
}

// ---------------------------------------------------------------------------
// Device VADMachines (VADMachine.zig:126-230 on the GPU)
// ---------------------------------------------------------------------------
namespace {
// a fresh machine's state and rolling buffers into the device arrays of m
int vadm_upload(const fvad_engine *e, const Vadm &m) {
  const fvad::VadmArgs &v = m.args;
  std::vector<fvad::VadmState> st = m.init;
  if (!m.lt_full) {
    // every entry 0.0f (initial entries are K.init, tracked by lt_nw): a device
    // memset, no host image of the buffers (hundreds of MB at 2048 streams)
    HIP_TRY(hipMemset(v.buf, 0, m.buf_len * sizeof(float)));
  } else {
    std::vector<float> buf(m.buf_len, 0.0f);
    // test hook FVAD_DEBUG_VADM_LT_FULL: every long-term entry counts as pushed
    // (holding (float)init), the state of a stream past its first
    // long_term_speech_avg_sec -- timing only, not the reference's values
    const int B = e->cfg.n_streams;
    for (int k = 0; k < v.n; k++) {
      const fvad::VadmConst &K = v.c[k];
      for (int s = 0; s < B; s++) {
        // (per-stream configs: the stream's own length and initial average)
        const fvad::VadmRow *row = m.ps ? &m.rows[(size_t)k * B + s] : nullptr;
        const int n_lt = row ? row->n_lt : K.n_lt;
        const float init = (float)(row ? row->init : K.init);
        for (int i = 0; i < n_lt; i++) buf[K.lt_off + (size_t)s * K.lt_pitch + i] = init;
        st[(size_t)k * B + s].lt_nw = (unsigned)n_lt;
      }
    }
    HIP_TRY(hipMemcpy(v.buf, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(v.st, st.data(), st.size() * sizeof(fvad::VadmState), hipMemcpyHostToDevice));
  return FVAD_OK;
}
}  // namespace

int fvad::eng::vadm_reset(fvad_engine *e) { return vadm_upload(e, e->vadm); }

namespace {
// All or nothing: every buffer, the events and the initial state upload are
// made in a local Vadm (the side stream beside it), which moves into the
// engine after the last step that can fail.  A failed call leaves the engine
// unattached.  The test hooks set before the call are carried over.
// ps (fvad_engine_attach_vadm_ex): a constant table row per (machine, stream),
// every stream starting on cfgs[m]; the rolling buffers are laid out for the
// room, each of a machine's three lengths the maximum over cfgs[m] and room[].
int attach(fvad_engine *e, const fvad_vadm_config *cfgs, int n, int seg_capacity, bool ps,
           const fvad_vadm_config *room, int n_room) {
  if (!e || !cfgs || n < 1 || n > FVAD_MAX_BANDS || seg_capacity < 1 || n_room < 0 || (n_room > 0 && !room))
    return fail(FVAD_EINVAL, "invalid argument");
  if (e->cfg.mode == FVAD_MODE_FUSED) return fail(FVAD_EINVAL, "device VADMachines need the staged engine");
  if (e->vadm.on()) return fail(FVAD_EINVAL, "VADMachines already attached");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int B = e->cfg.n_streams;
  fvad::stream_ptr side;  // (ahead of m: released after the events made on it)
  Vadm m;
  fvad::VadmArgs &v = m.args;
  v.par_serial_every = e->vadm.args.par_serial_every;
  v.defer_max = e->vadm.args.defer_max;
  m.always_par = e->vadm.always_par;
  v.n = n;
  v.seg_cap = seg_capacity;
  v.bound_scale = 1.0;
  v.negate_at = -1;
  long long off = 0;
  m.ps = ps;
  m.cfgs.assign(cfgs, cfgs + n);
  m.init.resize((size_t)n * B);
  m.rows.resize(ps ? (size_t)n * B : 0);
  m.stream_cfgs.resize(ps ? (size_t)n * B : 0);
  for (int k = 0; k < n; k++) {
    const fvad::VadmDerived d = fvad::vadm_derive(cfgs[k], e->cfg.sample_rate, e->cfg.fft_size);
    fvad::VadmConst &K = v.c[k] = d.K;
    K.slot = fvad::band_slot(e->cfg.band_lo, e->cfg.band_hi, e->cfg.n_bands, d.lo, d.hi);
    if (K.slot < 0) return fail(FVAD_EINVAL, "no engine band matches the machine's speech band");
    if (ps) {
      std::fill_n(m.rows.begin() + (size_t)k * B, (size_t)B, fvad::vadm_row(d, K.slot));
      std::fill_n(m.stream_cfgs.begin() + (size_t)k * B, (size_t)B, cfgs[k]);
      if (!K.has_init) m.nopar += (size_t)B;
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
    std::fill_n(m.init.begin() + (size_t)k * B, (size_t)B, d.s0);
  }
  m.buf_len = (size_t)off;
  int rc;
  if (ps && (rc = fvad::make_dev(m.tab, m.rows.size()))) return rc;
  if ((rc = fvad::make_dev(m.st, m.init.size())) || (rc = fvad::make_dev(m.buf, m.buf_len)) ||
      (rc = fvad::make_dev(m.seg, (size_t)n * B * seg_capacity)) || (rc = make_win_out(e, m.set1)) ||
      (rc = fvad::make_dev(m.vticks[0], (size_t)B)) || (rc = fvad::make_dev(m.vticks[1], (size_t)B)) ||
      (rc = fvad::make_stream(side)) || (rc = fvad::make_event(m.ev_done)) || (rc = m.tm.create()) ||
      (rc = fvad::make_event(m.ev_set_free[0])) || (rc = fvad::make_event(m.ev_set_free[1])))
    return rc;
  HIP_TRY(hipEventRecord(m.ev_done.get(), side.get()));
  HIP_TRY(hipEventRecord(m.ev_set_free[0].get(), side.get()));
  HIP_TRY(hipEventRecord(m.ev_set_free[1].get(), side.get()));
  v.st = m.st.get();
  v.buf = m.buf.get();
  v.seg = m.seg.get();
  v.tab = m.tab.get();
  if ((rc = vadm_upload(e, m))) return rc;
  if (ps) HIP_TRY(hipMemcpy(v.tab, m.rows.data(), m.rows.size() * sizeof(fvad::VadmRow), hipMemcpyHostToDevice));
  // nothing below fails
  e->vadm = std::move(m);
  e->side_ref = std::move(side);
  e->side = e->side_ref.get();
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
  if (!e->vadm.ps)
    return fail(FVAD_EINVAL, "fvad_engine_set_stream_vadm needs an engine attached with fvad_engine_attach_vadm_ex");
  if (const int rc = check_stream_list(e, streams, n)) return rc;
  if (machine < 0 || machine >= e->vadm.args.n) return fail(FVAD_EINVAL, "no such attached machine");
  if (n == 0) return FVAD_OK;
  if (!cfgs) return fail(FVAD_EINVAL, "null configs");
  if (e->vadm.lt_full)
    return fail(FVAD_EINVAL, "fvad_engine_set_stream_vadm is not available under FVAD_DEBUG_VADM_LT_FULL");
  const int B = e->cfg.n_streams;
  const fvad::VadmConst &K = e->vadm.args.c[machine];  // the room
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
  if (e->vadm.pend)
    if (const int rc = vadm_flush(e, false)) return rc;
  fvad::RetargetArgs a{};
  a.st = e->vadm.args.st;
  a.buf = e->vadm.args.buf;
  a.tab = e->vadm.args.tab;
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
      e->vadm.nopar += (size_t)!rows[i0 + i].has_init;
      e->vadm.nopar -= (size_t)!e->vadm.rows[idx].has_init;
      e->vadm.rows[idx] = rows[i0 + i];
      e->vadm.stream_cfgs[idx] = cfgs[i0 + i];
      e->vadm.init[idx] = fresh[i0 + i];
    }
  }
  return FVAD_OK;
}

extern "C" int fvad_engine_stream_vadm_config(const fvad_engine *e, int stream, int machine, fvad_vadm_config *out) {
  if (!e || !out || !e->vadm.on() || stream < 0 || stream >= e->cfg.n_streams || machine < 0 || machine >= e->vadm.args.n)
    return fail(FVAD_EINVAL, "no such attached machine");
  *out = e->vadm.ps ? e->vadm.stream_cfgs[(size_t)machine * e->cfg.n_streams + stream] : e->vadm.cfgs[machine];
  return FVAD_OK;
}

extern "C" size_t fvad_engine_segments(fvad_engine *e, int stream, int machine, fvad_segment *out, size_t cap) {
  return fvad_engine_segments_range(e, stream, machine, 0, out, cap);
}

extern "C" int fvad_engine_vadm_state(fvad_engine *e, int stream, int machine, int *speech_state,
                                      uint64_t *speech_start, uint64_t *speech_end) {
  if (!e || !e->vadm.on() || stream < 0 || stream >= e->cfg.n_streams || machine < 0 || machine >= e->vadm.args.n)
    return fail(FVAD_EINVAL, "no such attached machine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream.get()));
  if (const int rf = vadm_flush(e, true)) return rf;
  HIP_TRY(hipStreamSynchronize(e->side));
  fvad::VadmState st;
  HIP_TRY(hipMemcpy(&st, e->vadm.args.st + (size_t)machine * e->cfg.n_streams + stream, sizeof(st),
                    hipMemcpyDeviceToHost));
  if (speech_state) *speech_state = st.state;
  if (speech_start) *speech_start = st.speech_start;
  if (speech_end) *speech_end = st.speech_end;
  return FVAD_OK;
}

extern "C" size_t fvad_engine_segments_range(fvad_engine *e, int stream, int machine, size_t first,
                                             fvad_segment *out, size_t cap) {
  if (!e || !e->vadm.on() || stream < 0 || stream >= e->cfg.n_streams || machine < 0 || machine >= e->vadm.args.n)
    return 0;
  if (hipSetDevice(e->cfg.device) != hipSuccess || vadm_flush(e, true) != FVAD_OK ||
      hipStreamSynchronize(e->stream.get()) != hipSuccess || hipStreamSynchronize(e->side) != hipSuccess)
    return 0;
  const size_t idx = (size_t)machine * e->cfg.n_streams + stream;
  fvad::VadmState st;
  if (hipMemcpy(&st, e->vadm.args.st + idx, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  const size_t n = std::min<size_t>(st.n_segs, (size_t)e->vadm.args.seg_cap);
  const size_t k = first < n ? std::min(n - first, cap) : 0;
  // (a VadmSeg is an fvad_segment: fvad_machine.h)
  if (out && k &&
      hipMemcpy(out, e->vadm.args.seg + idx * e->vadm.args.seg_cap + first, k * sizeof(fvad_segment), hipMemcpyDeviceToHost) !=
          hipSuccess)
    return 0;
  return st.n_segs;
}

// ---------------------------------------------------------------------------
// Checker access: the whole device machine state and the test hooks
// ---------------------------------------------------------------------------
namespace {
int vadm_read_state(fvad_engine *e, int stream, int machine, fvad::VadmState *st) {
  if (!e || !e->vadm.on() || stream < 0 || stream >= e->cfg.n_streams || machine < 0 || machine >= e->vadm.args.n)
    return fail(FVAD_EINVAL, "no such attached machine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (const int rc = fvad_engine_sync(e)) return rc;
  HIP_TRY(hipMemcpy(st, e->vadm.args.st + (size_t)machine * e->cfg.n_streams + stream, sizeof(*st),
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
  const fvad::VadmConst &K = e->vadm.args.c[machine];
  const size_t B = e->cfg.n_streams;
  // per-stream configs: the stream's own lengths and initial average inside the room's layout
  const fvad::VadmRow *row = e->vadm.ps ? &e->vadm.rows[(size_t)machine * B + stream] : nullptr;
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
      HIP_TRY(hipMemcpy(col.data(), e->vadm.args.buf + off + (size_t)stream * K.lt_pitch, k * sizeof(float),
                        hipMemcpyDeviceToHost));
    else
      HIP_TRY(hipMemcpy2D(col.data(), sizeof(float), e->vadm.args.buf + off + stream, B * sizeof(float), sizeof(float), k,
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
      e->vadm.args.par_serial_every = value;
      return FVAD_OK;
    case FVAD_DEBUG_VADM_ALWAYS_PAR:
      e->vadm.always_par = value != 0;
      return FVAD_OK;
    case FVAD_DEBUG_VADM_DEFER_MAX:
      if (value < 0) return fail(FVAD_EINVAL, "value >= 0 required");
      e->vadm.args.defer_max = (unsigned)value;
      return FVAD_OK;
    case FVAD_DEBUG_VADM_BOUND_SCALE:
      if (!e->vadm.on()) return fail(FVAD_EINVAL, "no VADMachines attached");
      if (value < -1) return fail(FVAD_EINVAL, "value >= -1 required");
      if (const int rc = fvad_engine_sync(e)) return rc;  // a queued k_vadm_hbm reads the argument block's copy
      e->vadm.args.bound_scale = value == -1 ? HUGE_VAL : (value == 0 ? 1.0 : (double)value);
      return FVAD_OK;
    case FVAD_DEBUG_VADM_NEGATE_AT:
      if (!e->vadm.on()) return fail(FVAD_EINVAL, "no VADMachines attached");
      if (value < -1) return fail(FVAD_EINVAL, "value >= -1 required");
      if (const int rc = fvad_engine_sync(e)) return rc;
      e->vadm.args.negate_at = value;
      return FVAD_OK;
    case FVAD_DEBUG_VADM_COUNT:
      if (!e->vadm.on()) return fail(FVAD_EINVAL, "no VADMachines attached");
      if (const int rc = fvad_engine_sync(e)) return rc;
      if (value && !e->vadm.count)
        if (const int rc = fvad::make_dev(e->vadm.count, fvad::kVadmCounts)) return rc;
      if (!value) e->vadm.count.reset();
      e->vadm.args.count = e->vadm.count.get();
      if (e->vadm.args.count) HIP_TRY(hipMemset(e->vadm.args.count, 0, fvad::kVadmCounts * sizeof(unsigned long long)));
      return FVAD_OK;
    case FVAD_DEBUG_VADM_LT_FULL:
      if (!e->vadm.on()) return fail(FVAD_EINVAL, "no VADMachines attached");
      e->vadm.lt_full = value != 0;
      if (const int rc = fvad_engine_sync(e)) return rc;
      return vadm_reset(e);
    case FVAD_DEBUG_RESET_TIMES:
      e->dbg_reset_times = value != 0;
      return FVAD_OK;
    case FVAD_DEBUG_EVENTS_CHUNK:
      if (value < 0) return fail(FVAD_EINVAL, "value >= 0 required");
      e->feed.chunk = value;
      return FVAD_OK;
    default:
      return fail(FVAD_EINVAL, "unknown debug key");
  }
}

extern "C" int fvad_engine_debug_counts(fvad_engine *e, unsigned long long *out, int n) {
  if (!e || !out || n < 1) return fail(FVAD_EINVAL, "invalid argument");
  if (!e->vadm.args.count) return fail(FVAD_EINVAL, "FVAD_DEBUG_VADM_COUNT is not set");
  if (const int rc = fvad_engine_sync(e)) return rc;
  unsigned long long c[fvad::kVadmCounts];
  HIP_TRY(hipMemcpy(c, e->vadm.args.count, sizeof(c), hipMemcpyDeviceToHost));
  const int k = std::min(n, (int)fvad::kVadmCounts);
  for (int i = 0; i < k; i++) out[i] = c[i];
  return k;
}
