// The batched engine's two resamplers, host side (fvad_resample.h: input_rate,
// the raw push to 48 kHz; fvad_resample_out.h: denoised_rate, the denoised PCM
// from 48 kHz): what fvad_engine_create makes for them, a push's launches, and
// per-stream rates, whose plan (eng::RatePlan) both directions share.
#include <algorithm>
#include <cstring>
#include <vector>

#include "fvad_engine_impl.h"

using namespace fvad::eng;
namespace rs = fvad::rs;

// ---------------------------------------------------------------------------
// The per-stream plan
// ---------------------------------------------------------------------------
namespace {
// fvad_input_layout's arithmetic over rates or rate indices
template <typename Offset, typename RateOf>
void layout(int n_streams, int n_channels, Offset *offsets, RateOf rate_of) {
  Offset o = 0;
  for (int s = 0; s < n_streams; s++) {
    offsets[s] = o;
    o += (Offset)n_channels * (rate_of(s) / 100);
  }
  offsets[n_streams] = o;
}

// samples per tick and channel at a resampler's rate (480 without one); at_max:
// with per-stream rates the largest, rate_max's (no single frame otherwise)
template <typename R>
int frame_of(const std::unique_ptr<R> &r, bool at_max) {
  if (!r) return fvad::kFrame;
  return at_max && r->plan.on() ? r->plan.rate_max / 100 : r->d.n;
}

int upload_taps(fvad::dev_ptr<float> &dst, rs::Dir dir, const rs::Desc &d) {
  const std::vector<float> &taps = fvad::resample_table(dir, d);
  if (const int rc = fvad::make_dev(dst, taps.size())) return rc;
  HIP_TRY(hipMemcpy(dst.get(), taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice));
  return FVAD_OK;
}
}  // namespace

int RatePlan::make(rs::Dir dir, int n_streams_, int n_channels_, int rate_max_, int n_tab) {
  n_streams = n_streams_;
  n_channels = n_channels_;
  rate_max = rate_max_;
  int rc;
  for (int i = 0; i < rs::kPsRates; i++) {
    rs::describe_ps(rs::index_rate(i), dir, dr[i]);
    if (i == rs::kPsIndex48 || dr[i].rate > rate_max) continue;  // (48000: no filter, the copy kernels)
    if ((rc = upload_taps(taps_r[i], dir, dr[i]))) return rc;
  }
  ridx.assign((size_t)n_streams, rs::rate_index(rate_max));
  lists.resize((size_t)n_streams);
  offsets.resize((size_t)n_streams + 1);
  relayout();
  for (int i = 0; i < n_tab; i++)
    if ((rc = fvad::make_dev(tab[i], tab_words()))) return rc;
  if ((rc = fvad::make_pinned(stage, (size_t)kStage * tab_words()))) return rc;
  for (fvad::event_ptr &ev : stage_ev)
    if ((rc = fvad::make_event(ev))) return rc;
  return FVAD_OK;
}

void RatePlan::relayout() {
  layout(n_streams, n_channels, offsets.data(), [&](int s) { return rate(s); });
  int n = 0;
  for (int i = 0; i < rs::kPsRates; i++) {
    list_at[i] = n;
    for (int s = 0; s < n_streams; s++)
      if (ridx[s] == i) lists[n++] = s;
  }
  list_at[rs::kPsRates] = n;
  gen++;
}

int RatePlan::check(int n, const int *rates, const char *bad_rate) const {
  for (int i = 0; i < n; i++)
    if (rs::rate_index(rates[i]) < 0 || rates[i] > rate_max) return fail(FVAD_ERATE, bad_rate);
  return FVAD_OK;
}

void RatePlan::apply(const int *streams, int n, const int *rates) {
  for (int i = 0; i < n; i++) ridx[streams[i]] = rs::rate_index(rates[i]);
  relayout();
}

int RatePlan::sync(int copy, hipStream_t st) {
  if (tab_gen[copy] == gen) return FVAD_OK;
  const int B = n_streams, i = stage_next;
  stage_next = (i + 1) % kStage;
  if (stage_used[i]) HIP_TRY(hipEventSynchronize(stage_ev[i].get()));  // (complete long ago: see RatePlan)
  long long *row = stage.get() + (size_t)i * tab_words();
  std::memcpy(row, offsets.data(), sizeof(long long) * (size_t)(B + 1));
  int *ints = reinterpret_cast<int *>(row + B + 1);
  std::memcpy(ints, ridx.data(), sizeof(int) * (size_t)B);
  std::memcpy(ints + B, lists.data(), sizeof(int) * (size_t)B);
  HIP_TRY(hipMemcpyAsync(tab[copy].get(), row, tab_words() * sizeof(long long), hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(stage_ev[i].get(), st));
  stage_used[i] = true;
  tab_gen[copy] = gen;
  return FVAD_OK;
}

void RatePlan::fill(fvad::PsTables &t, int copy) const {
  t.offsets = tab[copy].get();
  t.rate_idx = reinterpret_cast<const int *>(tab[copy].get() + n_streams + 1);
  t.lists = t.rate_idx + n_streams;
  t.tick_len = tick_len();
  std::copy(list_at, list_at + rs::kPsRates + 1, t.list_at);
  for (int i = 0; i < rs::kPsRates; i++) {
    t.taps[i] = taps_r[i].get();
    t.d[i] = dr[i];
  }
}

int RatePlan::check_restored_rate(uint32_t word, int *ri) const {
  *ri = word <= 96000u ? rs::rate_index((int)word) : -1;
  return *ri < 0 ? 1 : (int)word > rate_max ? 2 : 0;
}

// ---------------------------------------------------------------------------
// Input resampling (input_rate set): the host's copies go to the raw buffer of
// d_pcm's parity, k_resample writes d_pcm from it
// ---------------------------------------------------------------------------
int fvad::eng::input_frame(const fvad_engine *e) { return frame_of(e->rs, false); }
int fvad::eng::input_frame_max(const fvad_engine *e) { return frame_of(e->rs, true); }

size_t fvad::eng::push_samples(const fvad_engine *e, int n_ticks) {
  if (e->rs && e->rs->plan.on()) return (size_t)n_ticks * (size_t)e->rs->plan.tick_len();
  return (size_t)n_ticks * e->cfg.n_streams * e->cfg.n_channels * input_frame(e);
}

// where the H2D copy of the push about to launch goes (after input_buffer)
void *fvad::eng::input_target(const fvad_engine *e) {
  return e->rs ? static_cast<void *>(e->rs->raw[e->in_next].get()) : static_cast<void *>(e->d_pcm);
}

// the tails' owner: k_resample runs there, ahead of the push's first reader
// of d_pcm (staged: the prep stream, with and without the denoiser)
hipStream_t fvad::eng::resample_stream(const fvad_engine *e) {
  return e->cfg.mode != FVAD_MODE_FUSED ? e->pstream : e->stream.get();
}

// fvad_engine_create's part: the tap table or the plan (rate_max set), the
// tails (zeroed by the reset that follows), the raw staging, the timers
int fvad::eng::resample_make(fvad_engine *e, const rs::Desc &d, int rate_max) {
  const fvad_engine_config &c = e->cfg;
  e->rs.reset(new Resample());
  Resample &r = *e->rs;
  r.d = d;
  int rc;
  if ((rc = rate_max ? r.plan.make(rs::Dir::kIn, c.n_streams, c.n_channels, rate_max, 2) : upload_taps(r.taps, rs::Dir::kIn, d)))
    return rc;
  const size_t rows = (size_t)c.n_streams * c.n_channels, raw = (size_t)c.max_ticks * rows * input_frame_max(e);
  if ((rc = fvad::make_dev(r.tails, rows * resample_tail_words(e, rs::Dir::kIn))) || (rc = fvad::make_dev(r.raw[0], raw)) ||
      (rc = fvad::make_dev(r.raw[1], raw)))
    return rc;
  return r.tm.create();
}

// the resample launches of the push about to launch, timed without waiting
int fvad::eng::resample_push(fvad_engine *e, int n_ticks, const int *d_ticks) {
  Resample &r = *e->rs;
  const int ib = e->in_next;
  hipStream_t st = resample_stream(e);
  fvad::ResamplePsPush p{};
  p.r.raw = r.raw[ib].get();
  p.r.taps = r.taps.get();
  p.r.tails = r.tails.get();
  p.r.ticks_valid = d_ticks;
  p.r.out = e->d_pcm;
  p.r.n_streams = e->cfg.n_streams;
  p.r.n_channels = e->cfg.n_channels;
  p.r.n_ticks = n_ticks;
  p.r.in16 = r.in16;
  p.r.d = r.d;
  int rc;
  if (r.plan.on()) {
    if ((rc = r.plan.sync(ib, st))) return rc;
    r.plan.fill(p.ps, ib);
  }
  if ((rc = r.tm.begin_next(r.tm_slot, st))) return rc;
  HIP_TRY(r.plan.on() ? fvad::launch_resample_ps(p, st) : fvad::launch_resample(p.r, st));
  return r.tm.end(r.tm_slot, st);
}

// ---------------------------------------------------------------------------
// The denoised PCM at another rate (denoised_rate set): k_resample_out writes
// d_den_out from d_den on the engine stream, and every copy of denoised rows to
// the host reads d_den_out
// ---------------------------------------------------------------------------
int fvad::eng::denoised_frame(const fvad_engine *e) { return frame_of(e->ro, false); }
int fvad::eng::denoised_frame_max(const fvad_engine *e) { return frame_of(e->ro, true); }

const float *fvad::eng::denoised_source(const fvad_engine *e) { return e->ro ? e->ro->out.get() : e->d_den.get(); }

size_t fvad::eng::denoised_floats(const fvad_engine *e, int n_ticks) {
  if (e->ro && e->ro->plan.on()) return (size_t)n_ticks * (size_t)e->ro->pushed_len;
  return (size_t)n_ticks * e->cfg.n_streams * e->cfg.n_channels * denoised_frame(e);
}

// fvad_engine_create's part: the tap table or the plan (rate_max set), the
// tails (zeroed by the reset that follows), the output rows, the timers
int fvad::eng::resample_out_make(fvad_engine *e, const rs::Desc &d, int rate_max) {
  const fvad_engine_config &c = e->cfg;
  e->ro.reset(new ResampleOut());
  ResampleOut &r = *e->ro;
  r.d = d;
  int rc;
  if ((rc = rate_max ? r.plan.make(rs::Dir::kOut, c.n_streams, c.n_channels, rate_max, 1) : upload_taps(r.taps, rs::Dir::kOut, d)))
    return rc;
  const size_t rows = (size_t)c.n_streams * c.n_channels;
  if ((rc = fvad::make_dev(r.tails, rows * resample_tail_words(e, rs::Dir::kOut))) ||
      (rc = fvad::make_dev(r.out, (size_t)c.max_ticks * rows * denoised_frame_max(e))))
    return rc;
  return r.tm.create();
}

// the launches of the push being launched, on the engine stream behind its
// last writer of d_den, timed without waiting (as resample_push)
int fvad::eng::resample_out_push(fvad_engine *e, int n_ticks, const int *d_ticks) {
  ResampleOut &r = *e->ro;
  hipStream_t st = e->stream.get();
  fvad::ResampleOutPsPush p{};
  p.r.den = e->d_den.get();
  p.r.taps = r.taps.get();
  p.r.tails = r.tails.get();
  p.r.ticks_valid = d_ticks;
  p.r.out = r.out.get();
  p.r.n_streams = e->cfg.n_streams;
  p.r.n_channels = e->cfg.n_channels;
  p.r.n_ticks = n_ticks;
  p.r.d = r.d;
  int rc;
  if (r.plan.on()) {
    if ((rc = r.plan.sync(0, st))) return rc;
    r.plan.fill(p.ps, 0);
    r.pushed_len = r.plan.tick_len();
  }
  if ((rc = r.tm.begin_next(r.tm_slot, st))) return rc;
  HIP_TRY(r.plan.on() ? fvad::launch_resample_out_ps(p, st) : fvad::launch_resample_out(p.r, st));
  return r.tm.end(r.tm_slot, st);
}

// ---------------------------------------------------------------------------
// Both: the tails
// ---------------------------------------------------------------------------
int fvad::eng::resample_tail_words(const fvad_engine *e, rs::Dir dir) {
  if (dir == rs::Dir::kIn) return e->rs->plan.on() ? rs::kMaxTail : e->rs->d.K - 1;
  return e->ro->plan.on() ? rs::kMaxTailOut : e->ro->d.K - 1;
}

namespace {
int zero_tails(fvad_engine *e, float *tails, rs::Dir dir) {
  HIP_TRY(hipMemsetAsync(tails, 0, sizeof(float) * (size_t)resample_tail_words(e, dir) * e->cfg.n_channels * e->cfg.n_streams,
                         e->stream.get()));
  return FVAD_OK;
}

// the n <= kListMax listed streams' tails become zeros, on the stream that owns them
int clear_tails(fvad_engine *e, float *tails, rs::Dir dir, const int *ids, int n, hipStream_t st) {
  fvad::ResampleClearArgs ra{};
  ra.tails = tails;
  ra.row_words = e->cfg.n_channels * resample_tail_words(e, dir);
  ra.ids.n = n;
  std::memcpy(ra.ids.id, ids, sizeof(int) * (size_t)n);
  HIP_TRY(fvad::launch_resample_clear(ra, st));
  return FVAD_OK;
}
}  // namespace

// (the input tails' owner, the prep stream, is idle: fvad_engine_reset has synchronised it)
int fvad::eng::resample_reset(fvad_engine *e) {
  int rc;
  if (e->rs && (rc = zero_tails(e, e->rs->tails.get(), rs::Dir::kIn))) return rc;
  if (e->ro && (rc = zero_tails(e, e->ro->tails.get(), rs::Dir::kOut))) return rc;
  return FVAD_OK;
}

// the input tails on the stream k_resample runs on, the output tails on the
// engine stream, where k_resample_out runs
int fvad::eng::resample_reset_streams(fvad_engine *e, const fvad::IdList &ids) {
  int rc;
  if (e->rs && (rc = clear_tails(e, e->rs->tails.get(), rs::Dir::kIn, ids.id, ids.n, resample_stream(e)))) return rc;
  if (e->ro && (rc = clear_tails(e, e->ro->tails.get(), rs::Dir::kOut, ids.id, ids.n, e->stream.get()))) return rc;
  return FVAD_OK;
}

// ---------------------------------------------------------------------------
// The C API of both directions
// ---------------------------------------------------------------------------
namespace {
const char *const kNotPsIn = "not a per-stream engine (FVAD_INPUT_RATE_PER_STREAM)";
const char *const kNotPsOut = "not an engine of per-stream denoised rates (FVAD_DENOISED_RATE_PER_STREAM)";

RatePlan *in_plan(const fvad_engine *e) { return e && e->rs && e->rs->plan.on() ? &e->rs->plan : nullptr; }
RatePlan *out_plan(const fvad_engine *e) { return e && e->ro && e->ro->plan.on() ? &e->ro->plan : nullptr; }

int get_rates(const fvad_engine *e, const RatePlan *p, int *rates, const char *not_ps) {
  if (!e || !rates) return fail(FVAD_EINVAL, "null argument");
  if (!p) return fail(FVAD_EINVAL, not_ps);
  for (int s = 0; s < p->n_streams; s++) rates[s] = p->rate(s);
  return FVAD_OK;
}

int get_layout(const fvad_engine *e, const RatePlan *p, int64_t *offsets, const char *not_ps) {
  if (!e || !offsets) return fail(FVAD_EINVAL, "null argument");
  if (!p) return fail(FVAD_EINVAL, not_ps);
  std::copy(p->offsets.begin(), p->offsets.end(), offsets);
  return FVAD_OK;
}

// 1: nothing listed, nothing to do.  device: the caller has device work behind
// the change (the device is selected once the rates are known to be good)
int set_rates(fvad_engine *e, RatePlan *p, const int *streams, int n, const int *rates, const char *not_ps,
              const char *bad_rate, bool device) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  if (!p) return fail(FVAD_EINVAL, not_ps);
  if (const int rc = check_stream_list(e, streams, n)) return rc;
  if (n == 0) return 1;
  if (!rates) return fail(FVAD_EINVAL, "null rates");
  if (const int rc = p->check(n, rates, bad_rate)) return rc;
  if (device) HIP_TRY(hipSetDevice(e->cfg.device));
  p->apply(streams, n, rates);
  return FVAD_OK;
}

// (after a sync: every pending sample is complete)
template <int N>
int times(fvad_engine *e, Timers<N> *tm, double *ms_avg, int *n_runs, const char *none) {
  if (!e || !ms_avg) return fail(FVAD_EINVAL, "null argument");
  if (!tm) return fail(FVAD_EINVAL, none);
  int rc = fvad_engine_sync(e);
  if (!rc) rc = tm->collect();
  if (!rc) tm->read(0, ms_avg, n_runs);
  return rc;
}
}  // namespace

extern "C" int fvad_engine_input_frame(const fvad_engine *e) {
  if (!e) return FVAD_EINVAL;
  if (in_plan(e)) return fail(FVAD_EINVAL, "a per-stream engine has no single frame: fvad_engine_input_layout");
  return input_frame(e);
}

extern "C" int fvad_engine_denoised_frame(const fvad_engine *e) {
  if (!e) return FVAD_EINVAL;
  if (out_plan(e))
    return fail(FVAD_EINVAL, "an engine of per-stream denoised rates has no single frame: fvad_engine_denoised_layout");
  return denoised_frame(e);
}

extern "C" int fvad_input_layout(const int *rates, int n_streams, int n_channels, int64_t *offsets) {
  if (!rates || !offsets || n_streams < 1 || n_channels < 1 || n_channels > FVAD_MAX_CHANNELS)
    return fail(FVAD_EINVAL, "fvad_input_layout: rates, offsets, n_streams >= 1 and 1 <= n_channels <= 8 required");
  for (int s = 0; s < n_streams; s++)
    if (rs::rate_index(rates[s]) < 0)
      return fail(FVAD_ERATE, "a stream's rate must be 8000, 16000, 24000, 32000, 44100, 48000 or 96000");
  layout(n_streams, n_channels, offsets, [&](int s) { return rates[s]; });
  return FVAD_OK;
}

extern "C" int fvad_denoised_layout(const int *rates, int n_streams, int n_channels, int64_t *offsets) {
  return fvad_input_layout(rates, n_streams, n_channels, offsets);  // (the same arithmetic, the same refusals)
}

extern "C" int fvad_engine_stream_rates(const fvad_engine *e, int *rates) {
  return get_rates(e, in_plan(e), rates, kNotPsIn);
}

extern "C" int fvad_engine_stream_denoised_rates(const fvad_engine *e, int *rates) {
  return get_rates(e, out_plan(e), rates, kNotPsOut);
}

extern "C" int fvad_engine_input_layout(const fvad_engine *e, int64_t *offsets) {
  return get_layout(e, in_plan(e), offsets, kNotPsIn);
}

extern "C" int fvad_engine_denoised_layout(const fvad_engine *e, int64_t *offsets) {
  return get_layout(e, out_plan(e), offsets, kNotPsOut);
}

// The host's rates and layout change here; the device tables follow ahead of
// the next push (RatePlan::sync), and the listed tails are cleared on the
// resample stream, behind the pushes already queued.  Nothing waits.
extern "C" int fvad_engine_set_stream_rates(fvad_engine *e, const int *streams, int n, const int *rates) {
  if (const int rc = set_rates(e, in_plan(e), streams, n, rates, kNotPsIn,
                               "a stream's rate must be a listed rate or 48000, at most input_rate_max", true))
    return rc < 0 ? rc : FVAD_OK;
  for (int i0 = 0; i0 < n; i0 += fvad::kListMax)
    if (const int rc = clear_tails(e, e->rs->tails.get(), rs::Dir::kIn, streams + i0, std::min(fvad::kListMax, n - i0),
                                   resample_stream(e)))
      return rc;
  return FVAD_OK;
}

// Only the host's rates and layout change here: the device tables follow ahead
// of the next push, and the history, which does not depend on a row's rate, is
// left alone.  No device call at all.
extern "C" int fvad_engine_set_stream_denoised_rates(fvad_engine *e, const int *streams, int n, const int *rates) {
  const int rc = set_rates(e, out_plan(e), streams, n, rates, kNotPsOut,
                           "a stream's denoised rate must be a listed rate or 48000, at most denoised_rate_max", false);
  return rc < 0 ? rc : FVAD_OK;
}

extern "C" int fvad_engine_fetch_input(fvad_engine *e, int n_ticks, float *pcm48) {
  if (!e || !pcm48) return fail(FVAD_EINVAL, "null argument");
  if (!e->rs) return fail(FVAD_EINVAL, "fvad_engine_fetch_input reads a resampling engine (input_rate)");
  if (n_ticks < 1 || n_ticks > e->cfg.max_ticks) return fail(FVAD_EINVAL, "n_ticks out of range");
  if (const int rc = fvad_engine_sync(e)) return rc;
  HIP_TRY(hipMemcpy(pcm48, e->d_pcm, (size_t)n_ticks * e->cfg.n_streams * e->cfg.n_channels * fvad::kFrame * sizeof(float),
                    hipMemcpyDeviceToHost));
  return FVAD_OK;
}

extern "C" int fvad_engine_resample_times(fvad_engine *e, double *ms_avg, int *n_runs) {
  return times(e, e && e->rs ? &e->rs->tm : nullptr, ms_avg, n_runs,
               "fvad_engine_resample_times reads a resampling engine (input_rate)");
}

extern "C" int fvad_engine_resample_out_times(fvad_engine *e, double *ms_avg, int *n_runs) {
  return times(e, e && e->ro ? &e->ro->tm : nullptr, ms_avg, n_runs,
               "fvad_engine_resample_out_times reads an engine with denoised_rate set");
}
