// The batched engine's input side: the device input buffers, the pinned
// slots of the streaming ingest, submit / collect.
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "fvad_engine_impl.h"

using namespace fvad::eng;

// the stream whose kernel reads the device input: k_prep3 on the prep stream
// (staged), k_prep / k_ndring on the engine stream (fused, no denoiser)
hipStream_t fvad::eng::input_reader(const fvad_engine *e) {
  return (e->cfg.mode != FVAD_MODE_FUSED && e->cfg.use_denoiser) ? e->pstream : e->stream.get();
}

// the input of the push about to launch goes to device buffer in_next; its
// previous reader (the k_prep3 of the push two before) must be done
int fvad::eng::input_buffer(fvad_engine *e, hipStream_t cs) {
  const int ib = e->in_next;
  if (e->in_busy[ib]) HIP_TRY(hipStreamWaitEvent(cs, e->ev_in_free[ib].get(), 0));
  e->d_pcm = e->d_pcm_b[ib].get();
  return FVAD_OK;
}

// after the launch: the buffer is free again once this push's prep read it
int fvad::eng::release_input(fvad_engine *e) {
  const int ib = e->in_next;
  HIP_TRY(hipEventRecord(e->ev_in_free[ib].get(), input_reader(e)));
  e->in_busy[ib] = true;
  e->in_next = ib ^ 1;
  e->resident_ticks = 0;
  return FVAD_OK;
}

// ---------------------------------------------------------------------------
// Input resampling (input_rate set; fvad_resample.h): the host's copies go to
// the raw buffer of d_pcm's parity, k_resample writes d_pcm from it
// ---------------------------------------------------------------------------
int fvad::eng::input_frame(const fvad_engine *e) { return e->rs ? e->rs->d.n_in : fvad::kFrame; }

int fvad::eng::input_frame_max(const fvad_engine *e) {
  return e->rs && e->rs->ps ? e->rs->rate_max / 100 : input_frame(e);
}

size_t fvad::eng::push_samples(const fvad_engine *e, int n_ticks) {
  if (e->rs && e->rs->ps) return (size_t)n_ticks * (size_t)e->rs->tick_len();
  return (size_t)n_ticks * e->cfg.n_streams * e->cfg.n_channels * input_frame(e);
}

int fvad::eng::resample_tail_words(const fvad_engine *e) { return e->rs->ps ? fvad::rs::kMaxTail : e->rs->d.K - 1; }

// fvad_input_layout over rate indices (all valid)
static void layout_of_indices(const int *ridx, int n_streams, int n_channels, long long *offsets) {
  long long o = 0;
  for (int s = 0; s < n_streams; s++) {
    offsets[s] = o;
    o += (long long)n_channels * (fvad::rs::index_rate(ridx[s]) / 100);
  }
  offsets[n_streams] = o;
}

void fvad::eng::resample_relayout(fvad_engine *e) {
  Resample &r = *e->rs;
  const int B = e->cfg.n_streams;
  layout_of_indices(r.ridx.data(), B, e->cfg.n_channels, r.offsets.data());
  int n = 0;
  for (int i = 0; i < fvad::rs::kPsRates; i++) {
    r.list_at[i] = n;
    for (int s = 0; s < B; s++)
      if (r.ridx[s] == i) r.lists[n++] = s;
  }
  r.list_at[fvad::rs::kPsRates] = n;
  r.gen++;
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

// fvad_engine_create's part: the table, the tails (zeroed by the reset that
// follows) and the raw staging
int fvad::eng::resample_make(fvad_engine *e) {
  Resample &r = *e->rs;
  const fvad_engine_config &c = e->cfg;
  if (r.ps) {
    // the tables of every rate up to rate_max, each stream at rate_max, the
    // raw staging and the slots sized by it
    const size_t B = c.n_streams, rows = B * c.n_channels, raw = (size_t)c.max_ticks * rows * (r.rate_max / 100);
    int rc;
    for (int i = 0; i < fvad::rs::kPsRates; i++) {
      fvad::rs::describe_ps(fvad::rs::index_rate(i), r.dr[i]);
      if (i == fvad::rs::kPsIndex48 || r.dr[i].rate > r.rate_max) continue;
      const std::vector<float> &taps = fvad::resample_table(r.dr[i]);
      if ((rc = fvad::make_dev(r.taps_r[i], taps.size()))) return rc;
      HIP_TRY(hipMemcpy(r.taps_r[i].get(), taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    r.ridx.assign(B, fvad::rs::rate_index(r.rate_max));
    r.lists.resize(B);
    r.offsets.resize(B + 1);
    resample_relayout(e);
    if ((rc = fvad::make_dev(r.tails, rows * fvad::rs::kMaxTail)) || (rc = fvad::make_dev(r.raw[0], raw)) ||
        (rc = fvad::make_dev(r.raw[1], raw)) || (rc = fvad::make_dev(r.tab[0], r.tab_words())) ||
        (rc = fvad::make_dev(r.tab[1], r.tab_words())) ||
        (rc = fvad::make_pinned(r.stage, (size_t)Resample::kStage * r.tab_words())) || (rc = r.tm[0].create()) ||
        (rc = r.tm[1].create()))
      return rc;
    for (fvad::event_ptr &ev : r.stage_ev)
      if ((rc = fvad::make_event(ev))) return rc;
    return FVAD_OK;
  }
  const std::vector<float> &taps = fvad::resample_table(r.d);
  const size_t rows = (size_t)c.n_streams * c.n_channels;
  int rc;
  if ((rc = fvad::make_dev(r.taps, taps.size())) || (rc = fvad::make_dev(r.tails, rows * (r.d.K - 1))) ||
      (rc = fvad::make_dev(r.raw[0], (size_t)c.max_ticks * rows * r.d.n_in)) ||
      (rc = fvad::make_dev(r.raw[1], (size_t)c.max_ticks * rows * r.d.n_in)) || (rc = r.tm[0].create()) ||
      (rc = r.tm[1].create()))
    return rc;
  HIP_TRY(hipMemcpy(r.taps.get(), taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice));
  return FVAD_OK;
}

// the resample launches of the push about to launch, timed without waiting
// (a sample still running when its timer comes round again is dropped)
namespace {
// the tables of the push's parity, when a change of rates has overtaken them
int resample_tables(fvad_engine *e, int ib, hipStream_t st) {
  Resample &r = *e->rs;
  if (r.tab_gen[ib] == r.gen) return FVAD_OK;
  const int B = e->cfg.n_streams, i = r.stage_next;
  r.stage_next = (i + 1) % Resample::kStage;
  if (r.stage_used[i]) HIP_TRY(hipEventSynchronize(r.stage_ev[i].get()));  // (complete long ago: see Resample)
  long long *row = r.stage.get() + (size_t)i * r.tab_words();
  std::memcpy(row, r.offsets.data(), sizeof(long long) * (size_t)(B + 1));
  int *ints = reinterpret_cast<int *>(row + B + 1);
  std::memcpy(ints, r.ridx.data(), sizeof(int) * (size_t)B);
  std::memcpy(ints + B, r.lists.data(), sizeof(int) * (size_t)B);
  HIP_TRY(hipMemcpyAsync(r.tab[ib].get(), row, r.tab_words() * sizeof(long long), hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(r.stage_ev[i].get(), st));
  r.stage_used[i] = true;
  r.tab_gen[ib] = r.gen;
  return FVAD_OK;
}

int resample_push_ps(fvad_engine *e, int n_ticks, const int *d_ticks) {
  Resample &r = *e->rs;
  const int ib = e->in_next, B = e->cfg.n_streams;
  hipStream_t st = resample_stream(e);
  int rc;
  if ((rc = resample_tables(e, ib, st))) return rc;
  fvad::ResamplePsPush p{};
  p.raw = r.raw[ib].get();
  p.tails = r.tails.get();
  p.ticks_valid = d_ticks;
  p.out = e->d_pcm;
  p.n_streams = B;
  p.n_channels = e->cfg.n_channels;
  p.n_ticks = n_ticks;
  p.in16 = r.in16;
  p.offsets = r.tab[ib].get();
  p.rate_idx = reinterpret_cast<const int *>(r.tab[ib].get() + B + 1);
  p.lists = p.rate_idx + B;
  p.tick_len = r.tick_len();
  for (int i = 0; i <= fvad::rs::kPsRates; i++) p.list_at[i] = r.list_at[i];
  for (int i = 0; i < fvad::rs::kPsRates; i++) {
    p.taps[i] = r.taps_r[i].get();
    p.d[i] = r.dr[i];
  }
  EventTimer &tm = r.tm[r.slot ^= 1];
  if ((rc = tm.collect(r.ms_sum, r.n_timed)) || (rc = tm.begin(st))) return rc;
  HIP_TRY(fvad::launch_resample_ps(p, st));
  return tm.end(st);
}
}  // namespace

int fvad::eng::resample_push(fvad_engine *e, int n_ticks, const int *d_ticks) {
  Resample &r = *e->rs;
  if (r.ps) return resample_push_ps(e, n_ticks, d_ticks);
  fvad::ResampleArgs a{};
  a.raw = r.raw[e->in_next].get();
  a.taps = r.taps.get();
  a.tails = r.tails.get();
  a.ticks_valid = d_ticks;
  a.out = e->d_pcm;
  a.n_streams = e->cfg.n_streams;
  a.n_channels = e->cfg.n_channels;
  a.n_ticks = n_ticks;
  a.in16 = r.in16;
  a.d = r.d;
  hipStream_t st = resample_stream(e);
  EventTimer &tm = r.tm[r.slot ^= 1];
  int rc;
  if ((rc = tm.collect(r.ms_sum, r.n_timed)) || (rc = tm.begin(st))) return rc;
  HIP_TRY(fvad::launch_resample(a, st));
  return tm.end(st);
}

extern "C" int fvad_engine_input_frame(const fvad_engine *e) {
  if (!e) return FVAD_EINVAL;
  if (e->rs && e->rs->ps) return fail(FVAD_EINVAL, "a per-stream engine has no single frame: fvad_engine_input_layout");
  return input_frame(e);
}

// ---------------------------------------------------------------------------
// Per-stream rates (FVAD_INPUT_RATE_PER_STREAM)
// ---------------------------------------------------------------------------
extern "C" int fvad_input_layout(const int *rates, int n_streams, int n_channels, int64_t *offsets) {
  if (!rates || !offsets || n_streams < 1 || n_channels < 1 || n_channels > FVAD_MAX_CHANNELS)
    return fail(FVAD_EINVAL, "fvad_input_layout: rates, offsets, n_streams >= 1 and 1 <= n_channels <= 8 required");
  for (int s = 0; s < n_streams; s++)
    if (fvad::rs::rate_index(rates[s]) < 0)
      return fail(FVAD_ERATE, "a stream's rate must be 8000, 16000, 24000, 32000, 44100, 48000 or 96000");
  int64_t o = 0;
  for (int s = 0; s < n_streams; s++) {
    offsets[s] = o;
    o += (int64_t)n_channels * (rates[s] / 100);
  }
  offsets[n_streams] = o;
  return FVAD_OK;
}

extern "C" int fvad_engine_stream_rates(const fvad_engine *e, int *rates) {
  if (!e || !rates) return fail(FVAD_EINVAL, "null argument");
  if (!e->rs || !e->rs->ps) return fail(FVAD_EINVAL, "not a per-stream engine (FVAD_INPUT_RATE_PER_STREAM)");
  for (int s = 0; s < e->cfg.n_streams; s++) rates[s] = fvad::rs::index_rate(e->rs->ridx[s]);
  return FVAD_OK;
}

extern "C" int fvad_engine_input_layout(const fvad_engine *e, int64_t *offsets) {
  if (!e || !offsets) return fail(FVAD_EINVAL, "null argument");
  if (!e->rs || !e->rs->ps) return fail(FVAD_EINVAL, "not a per-stream engine (FVAD_INPUT_RATE_PER_STREAM)");
  for (size_t i = 0; i < e->rs->offsets.size(); i++) offsets[i] = e->rs->offsets[i];
  return FVAD_OK;
}

// The host's rates and layout change here; the device tables follow ahead of
// the next push (resample_tables), and the listed tails are cleared on the
// resample stream, behind the pushes already queued.  Nothing waits.
extern "C" int fvad_engine_set_stream_rates(fvad_engine *e, const int *streams, int n, const int *rates) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  if (!e->rs || !e->rs->ps) return fail(FVAD_EINVAL, "not a per-stream engine (FVAD_INPUT_RATE_PER_STREAM)");
  if (const int rc = check_stream_list(e, streams, n)) return rc;
  if (n == 0) return FVAD_OK;
  if (!rates) return fail(FVAD_EINVAL, "null rates");
  Resample &r = *e->rs;
  for (int i = 0; i < n; i++)
    if (fvad::rs::rate_index(rates[i]) < 0 || rates[i] > r.rate_max)
      return fail(FVAD_ERATE, "a stream's rate must be a listed rate or 48000, at most input_rate_max");
  HIP_TRY(hipSetDevice(e->cfg.device));
  for (int i = 0; i < n; i++) r.ridx[streams[i]] = fvad::rs::rate_index(rates[i]);
  resample_relayout(e);
  fvad::ResampleClearArgs ra{};
  ra.tails = r.tails.get();
  ra.row_words = e->cfg.n_channels * fvad::rs::kMaxTail;
  for (int i0 = 0; i0 < n; i0 += fvad::kListMax) {
    ra.ids.n = std::min(fvad::kListMax, n - i0);
    std::memcpy(ra.ids.id, streams + i0, sizeof(int) * (size_t)ra.ids.n);
    HIP_TRY(fvad::launch_resample_clear(ra, resample_stream(e)));
  }
  return FVAD_OK;
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
  if (!e || !ms_avg) return fail(FVAD_EINVAL, "null argument");
  if (!e->rs) return fail(FVAD_EINVAL, "fvad_engine_resample_times reads a resampling engine (input_rate)");
  if (const int rc = fvad_engine_sync(e)) return rc;
  Resample &r = *e->rs;
  for (EventTimer &tm : r.tm)
    if (const int rc = tm.collect(r.ms_sum, r.n_timed)) return rc;
  *ms_avg = r.n_timed ? r.ms_sum / r.n_timed : 0.0;
  if (n_runs) *n_runs = r.n_timed;
  return FVAD_OK;
}

// ---------------------------------------------------------------------------
// The denoised PCM at another rate (denoised_rate set; fvad_resample_out.h):
// k_resample_out writes d_den_out from d_den on the engine stream, and every
// copy of denoised rows to the host reads d_den_out
// ---------------------------------------------------------------------------
int fvad::eng::denoised_frame(const fvad_engine *e) { return e->ro ? e->ro->d.n_out : fvad::kFrame; }

const float *fvad::eng::denoised_source(const fvad_engine *e) { return e->ro ? e->ro->out.get() : e->d_den.get(); }

int fvad::eng::denoised_frame_max(const fvad_engine *e) {
  return e->ro && e->ro->ps ? e->ro->rate_max / 100 : denoised_frame(e);
}

size_t fvad::eng::denoised_floats(const fvad_engine *e, int n_ticks) {
  if (e->ro && e->ro->ps) return (size_t)n_ticks * (size_t)e->ro->pushed_len;
  return (size_t)n_ticks * e->cfg.n_streams * e->cfg.n_channels * denoised_frame(e);
}

int fvad::eng::resample_out_tail_words(const fvad_engine *e) {
  return e->ro->ps ? fvad::rs::kMaxTailOut : e->ro->d.K - 1;
}

void fvad::eng::resample_out_relayout(fvad_engine *e) {
  ResampleOut &r = *e->ro;
  const int B = e->cfg.n_streams;
  layout_of_indices(r.ridx.data(), B, e->cfg.n_channels, r.offsets.data());
  int n = 0;
  for (int i = 0; i < fvad::rs::kPsRates; i++) {
    r.list_at[i] = n;
    for (int s = 0; s < B; s++)
      if (r.ridx[s] == i) r.lists[n++] = s;
  }
  r.list_at[fvad::rs::kPsRates] = n;
  r.gen++;
}

// fvad_engine_create's part: the table, the tails (zeroed by the reset that
// follows) and the output rows
int fvad::eng::resample_out_make(fvad_engine *e) {
  ResampleOut &r = *e->ro;
  const fvad_engine_config &c = e->cfg;
  if (r.ps) {
    // the tables of every listed rate up to rate_max, each stream at rate_max,
    // the output rows sized by it
    const size_t B = c.n_streams, rows = B * c.n_channels;
    int rc;
    for (int i = 0; i < fvad::rs::kPsRates; i++) {
      const int rate = fvad::rs::index_rate(i);
      if (i == fvad::rs::kPsIndex48) {  // (no filter: k_resample_out_copy)
        r.dr[i].rate = rate;
        r.dr[i].L = r.dr[i].M = r.dr[i].K = 1;
        r.dr[i].n_out = fvad::rs::kIn;
        continue;
      }
      fvad::rs::describe_out(rate, r.dr[i]);
      if (rate > r.rate_max) continue;
      const std::vector<float> &taps = fvad::resample_out_table(r.dr[i]);
      if ((rc = fvad::make_dev(r.taps_r[i], taps.size()))) return rc;
      HIP_TRY(hipMemcpy(r.taps_r[i].get(), taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    r.ridx.assign(B, fvad::rs::rate_index(r.rate_max));
    r.lists.resize(B);
    r.offsets.resize(B + 1);
    resample_out_relayout(e);
    if ((rc = fvad::make_dev(r.tails, rows * fvad::rs::kMaxTailOut)) ||
        (rc = fvad::make_dev(r.out, (size_t)c.max_ticks * rows * (r.rate_max / 100))) ||
        (rc = fvad::make_dev(r.tab, r.tab_words())) ||
        (rc = fvad::make_pinned(r.stage, (size_t)ResampleOut::kStage * r.tab_words())))
      return rc;
    for (EventTimer &tm : r.tm)
      if ((rc = tm.create())) return rc;
    for (fvad::event_ptr &ev : r.stage_ev)
      if ((rc = fvad::make_event(ev))) return rc;
    return FVAD_OK;
  }
  const std::vector<float> &taps = fvad::resample_out_table(r.d);
  const size_t rows = (size_t)c.n_streams * c.n_channels;
  int rc;
  if ((rc = fvad::make_dev(r.taps, taps.size())) || (rc = fvad::make_dev(r.tails, rows * (r.d.K - 1))) ||
      (rc = fvad::make_dev(r.out, (size_t)c.max_ticks * rows * r.d.n_out)))
    return rc;
  for (EventTimer &tm : r.tm)
    if ((rc = tm.create())) return rc;
  HIP_TRY(hipMemcpy(r.taps.get(), taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice));
  return FVAD_OK;
}

namespace {
// the device tables, when a change of rates has overtaken them: queued on the
// engine stream, so behind the launches of every push before this one
int resample_out_tables(fvad_engine *e, hipStream_t st) {
  ResampleOut &r = *e->ro;
  if (r.tab_gen == r.gen) return FVAD_OK;
  const int B = e->cfg.n_streams, i = r.stage_next;
  r.stage_next = (i + 1) % ResampleOut::kStage;
  if (r.stage_used[i]) HIP_TRY(hipEventSynchronize(r.stage_ev[i].get()));  // (complete long ago: see ResampleOut)
  long long *row = r.stage.get() + (size_t)i * r.tab_words();
  std::memcpy(row, r.offsets.data(), sizeof(long long) * (size_t)(B + 1));
  std::memcpy(row + B + 1, r.lists.data(), sizeof(int) * (size_t)B);
  HIP_TRY(hipMemcpyAsync(r.tab.get(), row, r.tab_words() * sizeof(long long), hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(r.stage_ev[i].get(), st));
  r.stage_used[i] = true;
  r.tab_gen = r.gen;
  return FVAD_OK;
}

int resample_out_push_ps(fvad_engine *e, int n_ticks, const int *d_ticks) {
  ResampleOut &r = *e->ro;
  const int B = e->cfg.n_streams;
  hipStream_t st = e->stream.get();
  int rc;
  if ((rc = resample_out_tables(e, st))) return rc;
  fvad::ResampleOutPsPush p{};
  p.den = e->d_den.get();
  p.tails = r.tails.get();
  p.ticks_valid = d_ticks;
  p.out = r.out.get();
  p.n_streams = B;
  p.n_channels = e->cfg.n_channels;
  p.n_ticks = n_ticks;
  p.offsets = r.tab.get();
  p.lists = reinterpret_cast<const int *>(r.tab.get() + B + 1);
  p.tick_len = r.tick_len();
  for (int i = 0; i <= fvad::rs::kPsRates; i++) p.list_at[i] = r.list_at[i];
  for (int i = 0; i < fvad::rs::kPsRates; i++) {
    p.taps[i] = r.taps_r[i].get();
    p.d[i] = r.dr[i];
  }
  r.pushed_len = r.tick_len();
  EventTimer &tm = r.tm[r.slot = (r.slot + 1) % 4];
  if ((rc = tm.collect(r.ms_sum, r.n_timed)) || (rc = tm.begin(st))) return rc;
  HIP_TRY(fvad::launch_resample_out_ps(p, st));
  return tm.end(st);
}
}  // namespace

// the two launches of the push being launched, on the engine stream behind
// its last writer of d_den, timed without waiting (as resample_push)
int fvad::eng::resample_out_push(fvad_engine *e, int n_ticks, const int *d_ticks) {
  ResampleOut &r = *e->ro;
  if (r.ps) return resample_out_push_ps(e, n_ticks, d_ticks);
  fvad::ResampleOutArgs a{};
  a.den = e->d_den.get();
  a.taps = r.taps.get();
  a.tails = r.tails.get();
  a.ticks_valid = d_ticks;
  a.out = r.out.get();
  a.n_streams = e->cfg.n_streams;
  a.n_channels = e->cfg.n_channels;
  a.n_ticks = n_ticks;
  a.d = r.d;
  hipStream_t st = e->stream.get();
  EventTimer &tm = r.tm[r.slot = (r.slot + 1) % 4];
  int rc;
  if ((rc = tm.collect(r.ms_sum, r.n_timed)) || (rc = tm.begin(st))) return rc;
  HIP_TRY(fvad::launch_resample_out(a, st));
  return tm.end(st);
}

extern "C" int fvad_engine_denoised_frame(const fvad_engine *e) {
  if (!e) return FVAD_EINVAL;
  if (e->ro && e->ro->ps)
    return fail(FVAD_EINVAL, "an engine of per-stream denoised rates has no single frame: fvad_engine_denoised_layout");
  return denoised_frame(e);
}

// ---------------------------------------------------------------------------
// Per-stream denoised rates (FVAD_DENOISED_RATE_PER_STREAM)
// ---------------------------------------------------------------------------
extern "C" int fvad_denoised_layout(const int *rates, int n_streams, int n_channels, int64_t *offsets) {
  return fvad_input_layout(rates, n_streams, n_channels, offsets);  // (the same arithmetic, the same refusals)
}

extern "C" int fvad_engine_stream_denoised_rates(const fvad_engine *e, int *rates) {
  if (!e || !rates) return fail(FVAD_EINVAL, "null argument");
  if (!e->ro || !e->ro->ps) return fail(FVAD_EINVAL, "not an engine of per-stream denoised rates (FVAD_DENOISED_RATE_PER_STREAM)");
  for (int s = 0; s < e->cfg.n_streams; s++) rates[s] = fvad::rs::index_rate(e->ro->ridx[s]);
  return FVAD_OK;
}

extern "C" int fvad_engine_denoised_layout(const fvad_engine *e, int64_t *offsets) {
  if (!e || !offsets) return fail(FVAD_EINVAL, "null argument");
  if (!e->ro || !e->ro->ps) return fail(FVAD_EINVAL, "not an engine of per-stream denoised rates (FVAD_DENOISED_RATE_PER_STREAM)");
  for (size_t i = 0; i < e->ro->offsets.size(); i++) offsets[i] = e->ro->offsets[i];
  return FVAD_OK;
}

// Only the host's rates and layout change here: the device tables follow ahead
// of the next push (resample_out_tables), and the history, which does not
// depend on a row's rate, is left alone.  No device call at all.
extern "C" int fvad_engine_set_stream_denoised_rates(fvad_engine *e, const int *streams, int n, const int *rates) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  if (!e->ro || !e->ro->ps) return fail(FVAD_EINVAL, "not an engine of per-stream denoised rates (FVAD_DENOISED_RATE_PER_STREAM)");
  if (const int rc = check_stream_list(e, streams, n)) return rc;
  if (n == 0) return FVAD_OK;
  if (!rates) return fail(FVAD_EINVAL, "null rates");
  ResampleOut &r = *e->ro;
  for (int i = 0; i < n; i++)
    if (fvad::rs::rate_index(rates[i]) < 0 || rates[i] > r.rate_max)
      return fail(FVAD_ERATE, "a stream's denoised rate must be a listed rate or 48000, at most denoised_rate_max");
  for (int i = 0; i < n; i++) r.ridx[streams[i]] = fvad::rs::rate_index(rates[i]);
  resample_out_relayout(e);
  return FVAD_OK;
}

extern "C" int fvad_engine_resample_out_times(fvad_engine *e, double *ms_avg, int *n_runs) {
  if (!e || !ms_avg) return fail(FVAD_EINVAL, "null argument");
  if (!e->ro) return fail(FVAD_EINVAL, "fvad_engine_resample_out_times reads an engine with denoised_rate set");
  if (const int rc = fvad_engine_sync(e)) return rc;
  ResampleOut &r = *e->ro;
  for (EventTimer &tm : r.tm)
    if (const int rc = tm.collect(r.ms_sum, r.n_timed)) return rc;
  *ms_avg = r.n_timed ? r.ms_sum / r.n_timed : 0.0;
  if (n_runs) *n_runs = r.n_timed;
  return FVAD_OK;
}

int fvad::eng::check_ticks(const fvad_engine *e, const int32_t *ticks_valid, int n_ticks) {
  if (ticks_valid)
    for (int s = 0; s < e->cfg.n_streams; s++)
      if (ticks_valid[s] < 0 || ticks_valid[s] > n_ticks) return fail(FVAD_EINVAL, "ticks_valid out of range");
  return FVAD_OK;
}

// last_tick_samples (nullable): real samples in each stream's last valid tick.
// Only the no-denoiser path consumes a partial tick (it reads fft_size frames,
// VAD.zig:206-220); with the denoiser a frame needs all 480 samples.  Fills
// tt = [ticks_valid (n_ticks where NULL) | tails] when tails are in use.
int fvad::eng::tail_ticks(const fvad_engine *e, const int32_t *ticks_valid, const int32_t *last, int n_ticks,
               std::vector<int32_t> &tt) {
  tt.clear();
  if (!last) return FVAD_OK;
  const int B = e->cfg.n_streams;
  if (e->rs) {  // whole ticks only: the resampler's phase restarts with every tick
    for (int s = 0; s < B; s++)
      if (last[s] != (e->rs->ps ? e->rs->frame(s) : e->rs->d.n_in))
        return fail(FVAD_EINVAL, "a resampling engine consumes whole ticks only");
    return FVAD_OK;
  }
  bool partial = false;
  for (int s = 0; s < B; s++) {
    if (last[s] < 1 || last[s] > fvad::kFrame) return fail(FVAD_EINVAL, "last_tick_samples out of range [1, 480]");
    partial |= last[s] != fvad::kFrame;
  }
  if (!partial) return FVAD_OK;
  if (e->cfg.use_denoiser || e->cfg.mode == FVAD_MODE_FUSED)
    return fail(FVAD_EINVAL, "a partial tick is only consumed with use_denoiser = 0 (VAD.zig:206-220)");
  tt.resize(2 * (size_t)B);
  for (int s = 0; s < B; s++) {
    tt[s] = ticks_valid ? ticks_valid[s] : n_ticks;
    tt[B + s] = last[s];
  }
  return FVAD_OK;
}

namespace {

// host copy into a pinned slot, split over threads for large inputs
void par_copy(void *dst, const void *src, size_t bytes) {
  constexpr size_t kChunk = 8u << 20;
  unsigned nthr = std::thread::hardware_concurrency();
  nthr = std::max(1u, std::min(nthr, 16u));
  const size_t parts = std::min<size_t>(nthr, (bytes + kChunk - 1) / kChunk);
  if (parts <= 1) {
    std::memcpy(dst, src, bytes);
    return;
  }
  std::vector<std::thread> pool;
  for (size_t i = 0; i < parts; i++) {
    const size_t a = bytes * i / parts, b = bytes * (i + 1) / parts;
    pool.emplace_back([=]() { std::memcpy((char *)dst + a, (const char *)src + a, b - a); });
  }
  for (auto &t : pool) t.join();
}

// The copy stream, and slot i's pinned buffers on first use: a caller that
// keeps k pushes in flight pins k slots, not FVAD_MAX_IN_FLIGHT
int ensure_slots(fvad_engine *e, int i) {
  const fvad_engine_config &c = e->cfg;
  const size_t B = c.n_streams, C = c.n_channels, T = c.max_ticks;
  const size_t TB = T * B, TBW = TB * e->wpt, frames = TB * C * fvad::kFrame;
  {
    // a streaming slot pins one push of input and outputs (fvad_engine_submit,
    // up to FVAD_MAX_IN_FLIGHT of them); the window outputs grow with W =
    // windows_per_tick (up to 240 at fft_size 2): refuse configurations whose
    // slot would not be a sane pinned allocation (the streaming API only:
    // resident and push-from-host engines never allocate a slot)
    const double slot = 4.0 * ((double)frames + (denoised_to_host(c) ? (double)TB * C * denoised_frame_max(e) : 0.0) + 3.0 * TB +
                               2.0 * TBW +
                               (double)TBW * C * c.n_bands);
    if (slot > 16.0 * (1ull << 30))
      return fail(FVAD_ENOMEM, "a push of max_ticks x n_streams needs > 16 GiB of pinned slot memory "
                               "(outputs scale with windows_per_tick): lower max_ticks or n_streams");
  }
  if (!e->cstream) {
    // the copy stream at the highest priority: its own hardware queue, so the
    // 16-bit ingest's k_pcm16 does not queue behind a long kernel of a stream
    // sharing its queue (it waited for k_vadm_hbm at the default priority)
    int lo_prio = 0, hi_prio = 0;
    hipStream_t cs = nullptr;
    if (hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio) != hipSuccess ||
        hipStreamCreateWithPriority(&cs, hipStreamNonBlocking, hi_prio) != hipSuccess)
      return fail(FVAD_EDEVICE, "copy stream creation failed");
    e->cstream.reset(cs);
  }
  auto &sl = e->slots[i];
  if (sl.done) return FVAD_OK;  // allocated (the events come last)
  // what an earlier, partly failed call allocated is kept and reused
  auto host = [](auto &p, size_t count) { return p ? FVAD_OK : fvad::make_pinned(p, count); };
  int rc;
  if ((rc = host(sl.in, TB * C * input_frame_max(e))) || (rc = host(sl.ticks, 2 * B)) || (rc = host(sl.vad, TB)) ||
      (rc = host(sl.ratio, TB)) || (rc = host(sl.wflag, TB)) || (rc = host(sl.wratio, TBW)) ||
      (rc = host(sl.wvad, TBW)) || (rc = host(sl.band, TBW * C * c.n_bands)) ||
      (denoised_to_host(c) && (rc = host(sl.den, TB * C * denoised_frame_max(e)))))
    return rc;
  if ((!sl.h2d && (rc = fvad::make_event(sl.h2d))) || (rc = fvad::make_event(sl.done))) return rc;
  return FVAD_OK;
}

// slot i's pinned 16-bit input and the device staging buffer, on first use
// (a resampling engine has its raw buffers instead of the staging buffer)
int ensure_slots16(fvad_engine *e, int i) {
  const fvad_engine_config &c = e->cfg;
  const size_t n = (size_t)c.max_ticks * c.n_streams * c.n_channels * input_frame_max(e);
  auto &sl = e->slots[i];
  int rc;
  if ((!sl.in16 && (rc = fvad::make_pinned(sl.in16, n))) ||
      (!e->rs && !e->d_pcm16 && (rc = fvad::make_dev(e->d_pcm16, n))))
    return rc;
  return FVAD_OK;
}

}  // namespace

extern "C" float *fvad_engine_input_slot(fvad_engine *e) {
  if (!e) {
    fail(FVAD_EINVAL, "null engine");
    return nullptr;
  }
  if (hipSetDevice(e->cfg.device) != hipSuccess || ensure_slots(e, e->sub_next)) return nullptr;
  auto &sl = e->slots[e->sub_next];
  if (sl.h2d_busy) {
    if (hipEventSynchronize(sl.h2d.get()) != hipSuccess) {
      fail(FVAD_EDEVICE, "hipEventSynchronize failed");
      return nullptr;
    }
    sl.h2d_busy = false;
  }
  return sl.in.get();
}

extern "C" int fvad_engine_submit(fvad_engine *e, const float *pcm, int n_ticks, const int32_t *ticks_valid) {
  return fvad_engine_submit_ex(e, pcm, n_ticks, ticks_valid, nullptr);
}

namespace {

// fvad_engine_submit_ex / fvad_engine_submit_i16: pcm is float or int16_t
// (16-bit samples k, pushed as k / 32768.0f -- libsndfile's short -> float
// normalisation, exact in f32: half the host-to-device bytes, converted by
// k_pcm16 on the copy stream right after the copy)
template <typename Sample>
int submit_any(fvad_engine *e, const Sample *pcm, int n_ticks, const int32_t *ticks_valid,
               const int32_t *last_tick_samples) {
  constexpr bool k16 = sizeof(Sample) == 2;
  if (!e || !pcm) return fail(FVAD_EINVAL, "null argument");
  const fvad_engine_config &c = e->cfg;
  if (n_ticks < 1 || n_ticks > c.max_ticks) return fail(FVAD_EINVAL, "n_ticks out of range [1, max_ticks]");
  int rc = check_ticks(e, ticks_valid, n_ticks);
  if (rc) return rc;
  std::vector<int32_t> tt;
  if ((rc = tail_ticks(e, ticks_valid, last_tick_samples, n_ticks, tt))) return rc;
  HIP_TRY(hipSetDevice(c.device));
  const int si = e->sub_next;
  if ((rc = ensure_slots(e, si))) return rc;
  if constexpr (k16)
    if ((rc = ensure_slots16(e, si))) return rc;
  auto &sl = e->slots[si];
  if (sl.pending) return fail(FVAD_EINVAL, "FVAD_MAX_IN_FLIGHT pushes in flight: collect the oldest one first");
  const size_t B = c.n_streams, TB = (size_t)n_ticks * B, TBW = TB * e->wpt;
  // (n_samples: the input's, at the engine's input rate)
  const size_t n_samples = push_samples(e, n_ticks);
  Sample *slot_in;
  if constexpr (k16)
    slot_in = sl.in16.get();
  else
    slot_in = sl.in.get();
  if (pcm != slot_in) {  // otherwise the producer wrote into the slot (fvad_engine_input_slot[_i16])
    if (sl.h2d_busy) HIP_TRY(hipEventSynchronize(sl.h2d.get()));
    par_copy(slot_in, pcm, n_samples * sizeof(Sample));
  }
  if (!tt.empty())
    std::memcpy(sl.ticks.get(), tt.data(), tt.size() * sizeof(int32_t));
  else if (ticks_valid)
    std::memcpy(sl.ticks.get(), ticks_valid, B * sizeof(int32_t));
  const bool use_ticks = ticks_valid != nullptr || !tt.empty();
  // staged: copies on the copy stream, overlapping the previous push's
  // kernels; the prep stream waits for them.  Fused: everything in order on
  // the engine stream (its kernels read d_ticks in place).
  const bool staged = c.mode != FVAD_MODE_FUSED;
  hipStream_t cs = staged ? e->cstream.get() : e->stream.get();
  if ((rc = input_buffer(e, cs))) return rc;
  // staged with the denoiser: k_prep3 reads the 16-bit samples straight from
  // the input buffer (half its input bytes; the copy stream carries only the
  // H2D copy, and no conversion kernel takes a slot beside the pushes)
  const bool direct16 = k16 && staged && c.use_denoiser && !e->raw_s16 && !e->rs;
  if (e->rs) {
    // a resampling engine: the samples as they are into the raw buffer;
    // k_resample (launch) converts and writes d_pcm as f32
    HIP_TRY(hipMemcpyAsync(input_target(e), slot_in, n_samples * sizeof(Sample), hipMemcpyHostToDevice, cs));
    e->rs->in16 = k16;
  } else if constexpr (k16) {
    if (direct16) {
      HIP_TRY(hipMemcpyAsync(e->d_pcm, sl.in16.get(), n_samples * sizeof(int16_t), hipMemcpyHostToDevice, cs));
    } else {
      // d_pcm16 is overwritten by the next 16-bit submit only after this
      // conversion read it (both on cs, in order)
      HIP_TRY(hipMemcpyAsync(e->d_pcm16.get(), sl.in16.get(), n_samples * sizeof(int16_t), hipMemcpyHostToDevice, cs));
      HIP_TRY(fvad::launch_pcm16(e->d_pcm16.get(), e->d_pcm, n_samples, cs));
    }
  } else {
    HIP_TRY(hipMemcpyAsync(e->d_pcm, sl.in.get(), n_samples * sizeof(float), hipMemcpyHostToDevice, cs));
  }
  if (use_ticks) {
    int *dticks = e->d_ticks;
    if (staged) {
      const int b = e->next_buf;
      if (e->buf_busy[b]) HIP_TRY(hipStreamWaitEvent(cs, e->ev_buf_free[b].get(), 0));
      dticks = e->d_ticks_b[b].get();
    }
    HIP_TRY(hipMemcpyAsync(dticks, sl.ticks.get(), (tt.empty() ? B : 2 * B) * sizeof(int32_t), hipMemcpyHostToDevice, cs));
  }
  HIP_TRY(hipEventRecord(sl.h2d.get(), cs));
  sl.h2d_busy = true;
  if (staged) HIP_TRY(hipStreamWaitEvent(e->pstream, sl.h2d.get(), 0));
  e->pcm16_push = direct16;
  rc = launch(e, n_ticks, use_ticks, false, !tt.empty());
  e->pcm16_push = false;
  if (rc) return rc;
  if ((rc = release_input(e))) return rc;
  // the denoised output's floats: this push's (per-stream rates: in the layout it was launched with)
  sl.den_floats = denoised_floats(e, n_ticks);
  // outputs into the slot's pinned buffers, after the kernels on the engine
  // stream (the next push's kernels queue behind these copies)
  auto d2h = [&](void *dst, const void *src, size_t n) -> int {
    HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, e->stream.get()));
    return FVAD_OK;
  };
  if ((rc = d2h(sl.vad.get(), e->d_vad.get(), TB * 4)) || (rc = d2h(sl.ratio.get(), e->d_ratio, TB * 4)) ||
      (rc = d2h(sl.wflag.get(), e->d_wflag, TB * 4)) || (rc = d2h(sl.wratio.get(), e->d_wratio, TBW * 4)) ||
      (rc = d2h(sl.wvad.get(), e->d_wvad, TBW * 4)) || (rc = d2h(sl.band.get(), e->d_band, TBW * c.n_channels * c.n_bands * 4)) ||
      (denoised_to_host(c) && (rc = d2h(sl.den.get(), denoised_source(e), sl.den_floats * sizeof(float)))))
    return rc;
  HIP_TRY(hipEventRecord(sl.done.get(), e->stream.get()));
  sl.pending = true;
  sl.n_ticks = n_ticks;
  e->sub_next = (si + 1) % FVAD_MAX_IN_FLIGHT;
  return FVAD_OK;
}

}  // namespace

extern "C" int fvad_engine_submit_ex(fvad_engine *e, const float *pcm, int n_ticks, const int32_t *ticks_valid,
                                     const int32_t *last_tick_samples) {
  return submit_any(e, pcm, n_ticks, ticks_valid, last_tick_samples);
}

extern "C" int16_t *fvad_engine_input_slot_i16(fvad_engine *e) {
  if (!e) {
    fail(FVAD_EINVAL, "null engine");
    return nullptr;
  }
  if (hipSetDevice(e->cfg.device) != hipSuccess || ensure_slots(e, e->sub_next) || ensure_slots16(e, e->sub_next))
    return nullptr;
  auto &sl = e->slots[e->sub_next];
  if (sl.h2d_busy) {
    if (hipEventSynchronize(sl.h2d.get()) != hipSuccess) {
      fail(FVAD_EDEVICE, "hipEventSynchronize failed");
      return nullptr;
    }
    sl.h2d_busy = false;
  }
  return sl.in16.get();
}

extern "C" int fvad_engine_submit_i16(fvad_engine *e, const int16_t *pcm, int n_ticks, const int32_t *ticks_valid,
                                      const int32_t *last_tick_samples) {
  return submit_any(e, pcm, n_ticks, ticks_valid, last_tick_samples);
}

extern "C" int fvad_engine_collect(fvad_engine *e, fvad_outputs *out, int *n_ticks) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  auto &sl = e->slots[e->col_next];
  if (!sl.pending) return fail(FVAD_EINVAL, "no submitted push to collect");
  const fvad_engine_config &c = e->cfg;
  HIP_TRY(hipSetDevice(c.device));
  HIP_TRY(hipEventSynchronize(sl.done.get()));
  const size_t TB = (size_t)sl.n_ticks * c.n_streams, TBW = TB * e->wpt;
  if (out) {
    if (out->denoised && !denoised_to_host(c))
      return fail(FVAD_EINVAL, c.want_denoised ? "want_denoised = 2 keeps the denoised rows on the device"
                                               : "engine created without want_denoised");
    auto cp = [](void *dst, const void *src, size_t n) {
      if (dst) std::memcpy(dst, src, n);
    };
    cp(out->vad, sl.vad.get(), TB * 4);
    cp(out->ratio, sl.ratio.get(), TB * 4);
    cp(out->win_flag, sl.wflag.get(), TB * 4);
    cp(out->win_ratio, sl.wratio.get(), TBW * 4);
    cp(out->win_vad, sl.wvad.get(), TBW * 4);
    cp(out->band, sl.band.get(), TBW * c.n_channels * c.n_bands * 4);
    if (out->denoised) par_copy(out->denoised, sl.den.get(), sl.den_floats * 4);
  }
  if (n_ticks) *n_ticks = sl.n_ticks;
  sl.pending = false;
  e->col_next = (e->col_next + 1) % FVAD_MAX_IN_FLIGHT;
  return FVAD_OK;
}
