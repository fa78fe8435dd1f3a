// Batched multi-stream engine (C ABI in include/fvad.h): the push path, fetch
// and the timing reads (construction: fvad_engine_create.cpp).
//
// One engine owns one GPU and a partition of streams.  Device memory layout
// (all HBM, sized for thousands of streams; 288 GB per MI355X leaves room for
// hundreds of ticks of input per push):
//   state   [streams][st::kWords]        persistent rnnoise + re-block state
//   ring    [streams][channels][ring]    denoised samples awaiting FFT B
//   pcm     [max_ticks][streams][ch][480] input staging (or resident synthetic)
//   xbuf    [max_ticks][streams][ch][480] high-passed s16-scale frames (k_prep)
//   ratio / outputs [max_ticks][streams] (+ channels, bands)
// staged mode (default, fvad_staged.hip) adds per-frame intermediates,
// frame f = s * V + tick * C + c with V = max_ticks * C:
//   xs [streams][1248 + V*480]  high-passed samples with pitch history
//   X, P [f][481] complex; Ex/Ep/Exp/Lyf [f][22]; f34 [f][8]; rec [f][144];
//   ys [f][960]; silence / pitch / vad [f]
// fused mode (fvad_kernels.hip): xbuf [max_ticks][streams][ch][480] and one
// k_frame workgroup per stream.  Both run on the engine's HIP stream and give
// identical results.
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fvad_engine_impl.h"

using namespace fvad::eng;

namespace {
thread_local std::string g_err;
}  // namespace

extern "C" const char *fvad_last_error(void) { return g_err.c_str(); }
int fvad::set_error(int code, const std::string &msg) {
  g_err = msg;
  return code;
}
extern "C" const char *fvad_version(void) { return "fvad-mi355x 0.1 (gfx950)"; }

// (the rnnoise compat path is 48 kHz only: ignored on a resampling engine)
void fvad_engine_set_raw_s16(fvad_engine *e, int raw) {
  if (!e->rs) e->raw_s16 = raw;
}

namespace {
using fvad::make_dev;
}  // namespace

extern "C" int fvad_engine_reset(fvad_engine *e) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (e->cstream) HIP_TRY(hipStreamSynchronize(e->cstream.get()));
  if (e->pstream) HIP_TRY(hipStreamSynchronize(e->pstream));
  if (e->vadm.on()) {
    e->vadm.pend = false;  // the pending push's machine state is wiped below: not run
    e->vadm.owed = false;
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    HIP_TRY(hipStreamSynchronize(e->side));
    int rc = vadm_reset(e);
    if (!rc && e->feed.on()) rc = events_reset(e);
    if (rc) return rc;
  }
  e->push_count = 0;
  HIP_TRY(hipMemsetAsync(e->d_state.get(), 0, sizeof(float) * fvad::st::kWords * (size_t)e->cfg.n_streams, e->stream.get()));
  e->res_next = 0;  // fresh streams start at the resident cycle's first push (t = 0)
  if (e->sg) HIP_TRY(hipMemsetAsync(e->sg->d_work.get(), 0, sizeof(unsigned) * fvad::kWorkCounters, e->stream.get()));
  HIP_TRY(hipMemsetAsync(e->d_ring.get(), 0,
                         sizeof(float) * (size_t)e->ring_len * e->cfg.n_channels * e->cfg.n_streams, e->stream.get()));
  if (const int rc = resample_reset(e)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream.get()));
  return FVAD_OK;
}

// a config's bands as the argument blocks carry them, and the bins they span
void fvad::eng::fill_bands(const fvad_engine_config &c, int *band_lo, int *band_hi, int *lo_all, int *hi_all) {
  int lo = 1 << 30, hi = -1;
  for (int b = 0; b < fvad::kMaxBandCfg; b++) {
    band_lo[b] = b < c.n_bands ? c.band_lo[b] : 0;
    band_hi[b] = b < c.n_bands ? c.band_hi[b] : -1;
    if (b < c.n_bands) {
      lo = std::min(lo, c.band_lo[b]);
      hi = std::max(hi, c.band_hi[b]);
    }
  }
  *lo_all = lo;
  *hi_all = hi;
}

// the push about to launch writes window-output set b
void fvad::eng::use_win_out(fvad_engine *e, int b) {
  const WinOut &w = b && e->vadm.on() ? e->vadm.set1 : e->wout0;
  e->d_wflag = w.flag.get();
  e->d_wratio = w.ratio.get();
  e->d_wvad = w.vad.get();
  e->d_band = w.band.get();
}

namespace {

int run_fused(fvad_engine *e, int n_ticks, bool use_ticks, bool timed) {
  const fvad_engine_config &c = e->cfg;
  fvad::PrepArgs pa;
  pa.n_streams = c.n_streams;
  pa.n_channels = c.n_channels;
  pa.n_ticks = n_ticks;
  pa.ticks_valid = use_ticks ? e->d_ticks : nullptr;
  pa.pcm = e->d_pcm;
  pa.xbuf = e->d_xbuf.get();
  pa.ratio = e->d_ratio;
  pa.state = e->d_state.get();
  pa.raw_s16 = e->raw_s16;
  fvad::FrameArgs fa;
  fa.n_streams = c.n_streams;
  fa.n_channels = c.n_channels;
  fa.n_ticks = n_ticks;
  fa.ticks_valid = pa.ticks_valid;
  fa.xbuf = e->d_xbuf.get();
  fa.ratio = e->d_ratio;
  fa.state = e->d_state.get();
  fa.ring = e->d_ring.get();
  fa.ring_len = e->ring_len;
  fa.plan = e->d_plan.get();
  fa.model = e->d_model.get();
  fa.n_bands = c.n_bands;
  fill_bands(c, fa.band_lo, fa.band_hi, &fa.bin_lo_all, &fa.bin_hi_all);
  fa.out_vad = e->d_vad.get();
  fa.out_win_ratio = e->d_wratio;
  fa.out_win_vad = e->d_wvad;
  fa.out_band = e->d_band;
  fa.out_den = e->d_den.get();
  fa.out_win_flag = e->d_wflag;
  fa.raw_s16 = e->raw_s16;
  fa.stamps = e->d_stamps.get();
  if (timed) HIP_TRY(hipEventRecord(e->ev[0], e->stream.get()));
  HIP_TRY(fvad::launch_prep(pa, e->stream.get()));
  if (timed) HIP_TRY(hipEventRecord(e->ev[1], e->stream.get()));
  HIP_TRY(fvad::launch_frame(fa, e->stream.get()));
  if (timed) HIP_TRY(hipEventRecord(e->ev[2], e->stream.get()));
  // the denoised rows at denoised_rate, behind k_frame, their writer
  if (e->ro)
    if (const int rr = resample_out_push(e, n_ticks, pa.ticks_valid)) return rr;
  return FVAD_OK;
}

}  // namespace

namespace {

// The argument block's part that no push changes: sizes, the buffers that are
// not double-buffered, the tables, the model and the machines as attached
// (with their test hooks' current values)
fvad::StagedArgs staged_fixed(const fvad_engine *e) {
  const fvad_engine_config &c = e->cfg;
  const Staged &g = *e->sg;
  fvad::StagedArgs a{};
  a.n_streams = c.n_streams;
  a.n_channels = c.n_channels;
  a.V = g.V;
  a.L = g.L;
  a.LX = g.LX;
  a.state = e->d_state.get();
  a.X = reinterpret_cast<float2 *>(g.d_X.get());
  a.P = reinterpret_cast<float2 *>(g.d_P.get());
  a.Ex = g.d_Ex.get();
  a.Ep = g.d_Ep.get();
  a.Exp = g.d_Exp.get();
  a.Lyf = g.d_Lyf.get();
  a.f34 = g.d_f34.get();
  a.silence = g.d_sil.get();
  a.rec = g.d_rec.get();
  a.ptile = g.d_ptile.get();
  a.work = g.d_work.get();
  a.pitch = g.d_pitch.get();
  a.vadf = g.d_vadf.get();
  a.gr = g.d_gr.get();
  a.gs = g.d_gs.get();
  a.rnn_img = e->d_rnn_img.get();
  a.gru16_frags = e->d_gru16.get();
  a.gru16_bias = e->d_gru16_bias.get();
  a.fuse16 = e->cfg.mode == FVAD_MODE_FP16_FUSED;
  a.fma = e->cfg.mode == FVAD_MODE_F32_FAST;
  for (int m = 0; m < fvad::rnnimg::kMats; m++) a.rnn_act[m] = e->rnn_act[m];
  a.ys = g.d_ys.get();
  a.ring = e->d_ring.get();
  a.ring_len = e->ring_len;
  a.win_tick = g.d_wtick.get();
  a.win_start = g.d_wstart.get();
  a.wmax = g.wmax;
  a.wpt = e->wpt;
  if (e->d_fbtab) {  // fft_size > kMaxFftB: [tw | sup | hann | perm] (fvad_engine_create)
    const size_t n = c.fft_size;
    a.fb_tw = reinterpret_cast<const float2 *>(e->d_fbtab.get());
    a.fb_sup = reinterpret_cast<const float2 *>(e->d_fbtab.get() + n);
    a.fb_hann = e->d_fbtab.get() + n + n / 2;
    a.fb_perm = reinterpret_cast<const int *>(e->d_fbtab.get() + n + n / 2 + n);
  } else {  // the plan's own tables (device addresses inside d_plan)
    const char *pb = reinterpret_cast<const char *>(e->d_plan.get());
    a.fb_tw = reinterpret_cast<const float2 *>(pb + offsetof(fvad::Plan, twb));
    a.fb_sup = reinterpret_cast<const float2 *>(pb + offsetof(fvad::Plan, superb));
    a.fb_hann = reinterpret_cast<const float *>(pb + offsetof(fvad::Plan, hannb));
    a.fb_perm = reinterpret_cast<const int *>(pb + offsetof(fvad::Plan, permb));
  }
  a.fb_work = g.d_fbwork.get();
  a.fb_work_blocks = g.fb_work_blocks;
  a.fb_work_stride = g.fb_work_stride;
  a.plan = e->d_plan.get();
  a.model = e->d_model.get();
  a.n_bands = c.n_bands;
  fill_bands(c, a.band_lo, a.band_hi, &a.bin_lo_all, &a.bin_hi_all);
  a.nfft_b = c.fft_size;
  a.use_denoiser = c.use_denoiser;
  a.out_vad = e->d_vad.get();
  a.out_den = e->d_den.get();
  a.raw_s16 = e->raw_s16;
  a.vadm = e->vadm.args;
  a.stamps = e->d_stamps.get();
  a.spec = e->d_spec.get();
  a.spec_lo = c.spec_lo;
  a.spec_hi = c.spec_hi;
  return a;
}

int run_staged(fvad_engine *e, int n_ticks, bool use_ticks, bool use_tail, bool timed) {
  const fvad_engine_config &c = e->cfg;
  Staged &g = *e->sg;
  // the previous push's VADMachine (after that push's ev_buf_free)
  if (e->vadm.pend)
    if (const int rf = vadm_flush(e, false)) return rf;
  // push k uses buffer b = k & 1 of xs / ratio / ticks; its k_prep3 waits
  // (on pstream) until push k-2 released b, then runs beside push k-1
  const int b = g.next_buf;
  if (g.buf_busy[b]) HIP_TRY(wait_event(e->pstream, g.ev_buf_free[b].get()));
  if (g.fft_a_rec) HIP_TRY(wait_event(e->pstream, g.ev_fft_a.get()));
  g.d_xs = g.d_xs_b[b].get();
  e->d_ratio = e->d_ratio_b[b].get();
  e->d_ticks = e->d_ticks_b[b].get();
  use_win_out(e, b);
  // the part that follows the push and its buffer parity
  fvad::StagedArgs a = staged_fixed(e);
  a.n_ticks = n_ticks;
  a.ticks_valid = use_ticks ? e->d_ticks : nullptr;
  a.tail = use_tail ? e->d_ticks + c.n_streams : nullptr;  // [B..2B) of the ticks buffer
  a.pcm = e->d_pcm;
  a.pcm16 = e->pcm16_push ? reinterpret_cast<const int16_t *>(e->d_pcm) : nullptr;
  a.xs = g.d_xs;
  a.xlp = g.d_xlp_b[b].get();
  a.ratio = e->d_ratio;
  a.out_win_ratio = e->d_wratio;
  a.out_win_vad = e->d_wvad;
  a.out_band = e->d_band;
  a.out_win_flag = e->d_wflag;
  // window spectra: the push's slots read 0 wherever FFT B writes no window
  // (behind the previous push's FFT B on the engine stream, ahead of this one's)
  if (e->d_spec)
    HIP_TRY(hipMemsetAsync(e->d_spec.get(), 0,
                           sizeof(float) * (size_t)n_ticks * c.n_streams * e->wpt * c.n_channels * e->n_spec,
                           e->stream.get()));
  if (c.use_denoiser) {
    HIP_TRY(fvad::launch_prep(a, e->pstream, timed ? e->ev : nullptr));
    // clip capture: the push's input into the history ring, by the stream that
    // reads it, before ev_prep_done (and the caller's ev_in_free) are recorded
    if (e->cap && e->cap->source == FVAD_CLIP_SOURCE_INPUT)
      if (const int rc = capture_append(e, a, b, timed)) return rc;
    HIP_TRY(hipEventRecord(g.ev_prep_done[b].get(), e->pstream));
    HIP_TRY(wait_event(e->stream.get(), g.ev_prep_done[b].get()));
    // window output set b is free once push k-2's k_vadm_hbm has read it
    if (e->vadm.on()) HIP_TRY(wait_event(e->stream.get(), e->vadm.ev_set_free[b].get()));
    // k_fftAw runs on the prep stream only while this engine owns it: on a
    // shared one (FVAD_SHARE_PREP) it would queue behind the other engine's
    // waits and couple the two pipelines, so it stays on the engine stream
    const bool own_prep = e->pstream_ref.use_count() <= 1;
    HIP_TRY(fvad::launch_staged(a, g.grid_frames, e->stream.get(), timed ? e->ev : nullptr, g.ev_fft_a.get(),
                                own_prep ? e->pstream : nullptr, g.synth_rec ? g.synth_wait : nullptr,
                                g.ev_synth.get()));
    // (launch_staged records the timing event in ev_synth's place when timed)
    g.synth_wait = timed ? e->ev[fvad::kEvSynthEnd] : g.ev_synth.get();
    g.synth_rec = true;
    g.fft_a_rec = true;
  } else {
    // no denoiser: raw input frames to the ring, windows, FFT B, all on the
    // engine stream after the input copy (queued on the prep stream)
    HIP_TRY(hipEventRecord(g.ev_prep_done[b].get(), e->pstream));
    HIP_TRY(wait_event(e->stream.get(), g.ev_prep_done[b].get()));
    if (e->vadm.on()) HIP_TRY(wait_event(e->stream.get(), e->vadm.ev_set_free[b].get()));
    HIP_TRY(fvad::launch_nodenoise(a, g.grid_frames, e->stream.get()));
  }
  if (e->vadm.on()) {
    // the ticks copy of parity b may be overwritten once push k - 2's
    // VADMachine has read it (ev_set_free[b], waited for above)
    if (use_ticks)
      HIP_TRY(hipMemcpyAsync(e->vadm.vticks[b].get(), e->d_ticks, (size_t)c.n_streams * 4, hipMemcpyDeviceToDevice,
                             e->stream.get()));
    fvad::StagedArgs v = a;
    v.ticks_valid = use_ticks ? e->vadm.vticks[b].get() : nullptr;
    e->vadm.pend = true;
    e->vadm.pend_args = v;
    e->vadm.pend_b = b;
    e->vadm.pend_timed = timed;
    e->vadm.pend_push = e->push_count;
  }
  e->push_count++;
  if (e->log_n < e->log_cap) {  // test hook: this push's outputs into the log (read after a sync)
    const size_t B = c.n_streams, TB = (size_t)n_ticks * B, TBW = TB * e->wpt, MT = (size_t)c.max_ticks * B,
                 MW = MT * e->wpt;
    float *L = e->d_log.get() + e->log_stride * (size_t)e->log_n;
    const void *src[6] = {e->d_vad.get(), e->d_ratio, e->d_wflag, e->d_wratio, e->d_wvad, e->d_band};
    const size_t off[6] = {0, MT, 2 * MT, 3 * MT, 3 * MT + MW, 3 * MT + 2 * MW};
    const size_t n[6] = {TB, TB, TB, TBW, TBW, TBW * c.n_channels * c.n_bands};
    for (int i = 0; i < 6; i++)
      HIP_TRY(hipMemcpyAsync(L + off[i], src[i], n[i] * 4, hipMemcpyDeviceToDevice, e->stream.get()));
    e->log_ticks[e->log_n++] = n_ticks;
  }
  // the denoised rows at denoised_rate, behind the tail kernels, the push's
  // last writers of d_den (it reads ticks buffer b: ahead of ev_buf_free)
  if (e->ro)
    if (const int rr = resample_out_push(e, n_ticks, a.ticks_valid)) return rr;
  // clip capture of the denoised rows: into the history ring behind their last
  // writer (k_resample_out above, or the tail kernels), by the stream that
  // owns them, ahead of ev_buf_free (it reads ticks buffer b)
  if (e->cap && e->cap->source == FVAD_CLIP_SOURCE_DENOISED)
    if (const int rc = capture_append_den(e, a, b, timed)) return rc;
  // every reader of buffer b (incl. the copy of ticks for k_vadm_hbm) is queued
  HIP_TRY(hipEventRecord(g.ev_buf_free[b].get(), e->stream.get()));
  g.buf_busy[b] = true;
  g.next_buf = b ^ 1;
  return FVAD_OK;
}

}  // namespace

int fvad::eng::launch(fvad_engine *e, int n_ticks, bool use_ticks, bool timed, bool use_tail) {
  if (!e->cfg.use_denoiser) timed = false;  // the no-denoiser pipeline records no kernel events
  if (e->rs) {
    // the push's first kernel: the raw input to 48 kHz, on the stream that
    // owns the tails, behind the copies of the input and of ticks_valid
    const int *tv = !use_ticks ? nullptr
                    : e->cfg.mode != FVAD_MODE_FUSED ? e->d_ticks_b[e->sg->next_buf].get() : e->d_ticks;
    if (const int rr = resample_push(e, n_ticks, tv)) return rr;
  }
  const int rc = e->cfg.mode == FVAD_MODE_FUSED ? run_fused(e, n_ticks, use_ticks, timed)
                                                 : run_staged(e, n_ticks, use_ticks, use_tail, timed);
  if (!rc && timed) e->slot_pending[e->ev_slot] = true;
  if (!rc) e->last_ticks = n_ticks;
  return rc;
}

namespace {

int collect_slot(fvad_engine *e, int slot) {
  if (!e->slot_pending[slot]) return FVAD_OK;
  hipEvent_t *ev = e->evs[slot];
  const bool staged = e->cfg.mode != FVAD_MODE_FUSED;
  HIP_TRY(hipEventSynchronize(ev[e->last_event]));
  for (int i = 0; i < e->n_kernels; i++) {
    float ms = 0;
    const int b = staged ? e->kernels.k[i].begin : i, en = staged ? e->kernels.k[i].end : i + 1;
    HIP_TRY(hipEventElapsedTime(&ms, ev[b], ev[en]));
    e->ms_sum[1 + i] += ms;
  }
  float total = 0;  // GPU time of the launch (kernels may overlap)
  HIP_TRY(hipEventElapsedTime(&total, ev[0], ev[e->last_event]));
  e->ms_sum[0] += total;
  e->n_timed++;
  e->slot_pending[slot] = false;
  return FVAD_OK;
}

int collect_timing(fvad_engine *e) {
  int rc = collect_slot(e, e->ev_slot ^ 1);
  if (!rc) rc = collect_slot(e, e->ev_slot);
  return rc;
}

}  // namespace

int fvad::eng::fetch(fvad_engine *e, int n_ticks, fvad_outputs *o) {
  if (!o) return FVAD_OK;
  const fvad_engine_config &c = e->cfg;
  const size_t TB = (size_t)n_ticks * c.n_streams, TBW = TB * e->wpt;
  auto cp = [&](void *dst, const void *src, size_t bytes) -> int {
    if (!dst) return FVAD_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream.get()));
    return FVAD_OK;
  };
  int rc;
  if ((rc = cp(o->vad, e->d_vad.get(), TB * 4)) || (rc = cp(o->ratio, e->d_ratio, TB * 4)) ||
      (rc = cp(o->win_flag, e->d_wflag, TB * 4)) || (rc = cp(o->win_ratio, e->d_wratio, TBW * 4)) ||
      (rc = cp(o->win_vad, e->d_wvad, TBW * 4)) || (rc = cp(o->band, e->d_band, TBW * c.n_channels * c.n_bands * 4)))
    return rc;
  if (o->denoised) {
    if (!e->d_den) return fail(FVAD_EINVAL, "engine created without want_denoised");
    if (!denoised_to_host(c)) return fail(FVAD_EINVAL, "want_denoised = 2 keeps the denoised rows on the device");
    if ((rc = cp(o->denoised, denoised_source(e), denoised_floats(e, n_ticks) * 4))) return rc;
  }
  HIP_TRY(hipStreamSynchronize(e->stream.get()));
  return FVAD_OK;
}

extern "C" int fvad_engine_push(fvad_engine *e, const float *pcm, int n_ticks, const int32_t *ticks_valid,
                                fvad_outputs *out) {
  return fvad_engine_push_ex(e, pcm, n_ticks, ticks_valid, nullptr, out);
}

extern "C" int fvad_engine_push_ex(fvad_engine *e, const float *pcm, int n_ticks, const int32_t *ticks_valid,
                                   const int32_t *last_tick_samples, fvad_outputs *out) {
  if (!e || !pcm) return fail(FVAD_EINVAL, "null argument");
  const fvad_engine_config &c = e->cfg;
  if (n_ticks < 0 || n_ticks > c.max_ticks) return fail(FVAD_EINVAL, "n_ticks out of range [0, max_ticks]");
  if (out && out->denoised && c.want_denoised == 2)  // (before anything is launched)
    return fail(FVAD_EINVAL, "want_denoised = 2 keeps the denoised rows on the device");
  if (n_ticks == 0) return FVAD_OK;
  int rc = check_ticks(e, ticks_valid, n_ticks);
  if (rc) return rc;
  std::vector<int32_t> tt;
  if ((rc = tail_ticks(e, ticks_valid, last_tick_samples, n_ticks, tt))) return rc;
  HIP_TRY(hipSetDevice(c.device));
  const size_t bytes = push_samples(e, n_ticks) * sizeof(float);
  // staged: the inputs go through the prep stream (ticks buffer b is free
  // once push k-2 finished)
  hipStream_t cs = e->stream.get();
  int *dticks = e->d_ticks;
  if (e->cfg.mode != FVAD_MODE_FUSED) {
    const int b = e->sg->next_buf;
    if (e->sg->buf_busy[b]) HIP_TRY(hipStreamWaitEvent(e->pstream, e->sg->ev_buf_free[b].get(), 0));
    cs = e->pstream;
    dticks = e->d_ticks_b[b].get();
  }
  if ((rc = input_buffer(e, cs))) return rc;
  HIP_TRY(hipMemcpyAsync(input_target(e), pcm, bytes, hipMemcpyHostToDevice, cs));
  if (e->rs) e->rs->in16 = false;
  if (!tt.empty()) {  // ticks and tails, [2 * B] (synchronous copy: tt is a local)
    HIP_TRY(hipMemcpyAsync(dticks, tt.data(), sizeof(int32_t) * tt.size(), hipMemcpyHostToDevice, cs));
    HIP_TRY(hipStreamSynchronize(cs));
  } else if (ticks_valid) {
    HIP_TRY(hipMemcpyAsync(dticks, ticks_valid, sizeof(int32_t) * c.n_streams, hipMemcpyHostToDevice, cs));
  }
  if ((rc = launch(e, n_ticks, ticks_valid != nullptr || !tt.empty(), false, !tt.empty()))) return rc;
  if ((rc = release_input(e))) return rc;
  return fetch(e, n_ticks, out);
}

extern "C" int fvad_engine_load_synthetic(fvad_engine *e, int n_ticks, uint32_t base) {
  return fvad_engine_load_synthetic_ex(e, n_ticks, 1, base);
}

// n_pushes distinct pushes of n_ticks resident in HBM: stream s's first
// n_pushes * n_ticks ticks of fvad_synth_stream(base + s) (generated at that
// length).  One push lives in the input buffer d_pcm_b[0]; more get their own
// [push][tick][stream][ch][480] buffer, and run_resident cycles through them.
// Host memory stays bounded: groups of kGroup streams are generated and copied
// (one strided copy per group: a group's rows of every tick), never the whole
// block.
extern "C" int fvad_engine_load_synthetic_ex(fvad_engine *e, int n_ticks, int n_pushes, uint32_t base) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  if (e->rs) return fail(FVAD_EINVAL, "the synthetic generator is 48 kHz: not available on a resampling engine");
  const fvad_engine_config &c = e->cfg;
  if (n_ticks < 1 || n_ticks > c.max_ticks) return fail(FVAD_EINVAL, "n_ticks out of range");
  if (n_pushes < 1 || (long long)n_ticks * n_pushes > (1LL << 30))
    return fail(FVAD_EINVAL, "1 <= n_pushes and n_ticks * n_pushes <= 2^30 required");
  HIP_TRY(hipSetDevice(c.device));
  const size_t row = (size_t)c.n_channels * fvad::kFrame;  // floats of one (tick, stream)
  const size_t per_push = (size_t)n_ticks * c.n_streams * row;
  const int total = n_ticks * n_pushes;
  constexpr int kGroup = 64;
  const int gs = std::min(kGroup, c.n_streams);
  std::vector<float> host;
  try {
    host.resize((size_t)total * gs * row);
  } catch (...) {
    return fail(FVAD_ENOMEM, "host buffer for the synthetic input");
  }
  // buffer 0 (or the resident set) may still be read by an in-flight push
  int rc = fvad_engine_sync(e);
  if (rc) return rc;
  e->d_res.reset();
  e->res_pushes = 0;
  if (n_pushes > 1 && (rc = make_dev(e->d_res, per_push * n_pushes))) return rc;
  // [push][tick][stream] rows are [global tick][stream] rows: tick g = k * n_ticks + t
  float *dst = n_pushes == 1 ? e->d_pcm_b[0].get() : e->d_res.get();
  for (int s0 = 0; s0 < c.n_streams; s0 += gs) {
    const int ns = std::min(gs, c.n_streams - s0);
    if ((rc = fvad_synth_group(base, s0, ns, c.n_channels, total, 0, total, host.data(), (size_t)ns)))
      return fail(rc, "synthetic input generation failed");
    HIP_TRY(hipMemcpy2D(dst + (size_t)s0 * row, (size_t)c.n_streams * row * sizeof(float), host.data(),
                        (size_t)ns * row * sizeof(float), (size_t)ns * row * sizeof(float), (size_t)total,
                        hipMemcpyHostToDevice));
  }
  if (n_pushes > 1) e->res_pushes = n_pushes;
  e->res_next = 0;
  e->resident_ticks = n_ticks;
  return FVAD_OK;
}

extern "C" int fvad_engine_resident_seek(fvad_engine *e, int push) {
  if (!e || e->resident_ticks < 1) return fail(FVAD_EINVAL, "no resident input");
  if (push < 0 || push >= std::max(1, e->res_pushes)) return fail(FVAD_EINVAL, "push index out of range");
  e->res_next = push;
  return FVAD_OK;
}

extern "C" int fvad_engine_run_resident(fvad_engine *e, int n_ticks) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  if (e->rs) return fail(FVAD_EINVAL, "no resident input on a resampling engine");
  if (n_ticks < 1 || n_ticks > e->resident_ticks) return fail(FVAD_EINVAL, "n_ticks exceeds resident input");
  HIP_TRY(hipSetDevice(e->cfg.device));
  // the set this push will record into was used two pushes ago: read it (it
  // is long finished) before reusing it; the previous push keeps running
  e->ev_slot ^= 1;
  e->ev = e->evs[e->ev_slot];
  int rc = collect_slot(e, e->ev_slot);
  if (rc) return rc;
  if (e->res_pushes > 1) {  // the next of the resident pushes, cyclically
    const size_t per_push = (size_t)e->resident_ticks * e->cfg.n_streams * e->cfg.n_channels * fvad::kFrame;
    e->d_pcm = e->d_res.get() + per_push * (size_t)e->res_next;
    e->res_next = (e->res_next + 1) % e->res_pushes;
  } else {
    e->d_pcm = e->d_pcm_b[0].get();
  }
  // Timing events on every FVAD_EVENT_EVERY-th push (default 4: the 15
  // event markers of a push cost it ~1 %, measured); FVAD_NO_EVENTS=1: none
  static const bool no_events = [] {
    const char *v = getenv("FVAD_NO_EVENTS");
    return v && atoi(v) == 1;
  }();
  static const int every = [] {
    const char *v = getenv("FVAD_EVENT_EVERY");
    const int n = v ? atoi(v) : 4;
    return n < 1 ? 1 : n;
  }();
  const bool timed = !no_events && e->res_count++ % every == 0;
  if ((rc = launch(e, n_ticks, false, timed))) return rc;
  // a later submit / push must not overwrite buffer 0 under this run's prep
  if (e->res_pushes <= 1) {
    HIP_TRY(hipEventRecord(e->ev_in_free[0].get(), input_reader(e)));
    e->in_busy[0] = true;
  }
  return FVAD_OK;
}

extern "C" int fvad_engine_sync(fvad_engine *e) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (e->cstream) HIP_TRY(hipStreamSynchronize(e->cstream.get()));
  if (e->pstream) HIP_TRY(hipStreamSynchronize(e->pstream));
  if (e->side)
    if (const int rf = vadm_flush(e, true)) return rf;
  HIP_TRY(hipStreamSynchronize(e->stream.get()));
  if (e->side) {
    HIP_TRY(hipStreamSynchronize(e->side));
    const int rc = collect_vadm_timing(e);
    if (rc) return rc;
  }
  return collect_timing(e);
}

extern "C" int fvad_engine_kernel_times(fvad_engine *e, double *ms_avg, int *n_runs) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  int rc = fvad_engine_sync(e);
  if (rc) return rc;
  for (int i = 0; i < FVAD_MAX_TIMES; i++)
    ms_avg[i] = (e->n_timed && i <= e->n_kernels) ? e->ms_sum[i] / e->n_timed : 0.0;
  // the VADMachine (side stream, overlapped with the next push): reported after
  // the pipeline kernels, not part of [0]; k_vadm_hbm (steady state) and
  // k_vadm_par (the push flushed at a sync point) separately
  for (int k = 0; k < 2; k++)
    if (e->vadm.on() && e->n_kernels + 1 + k < FVAD_MAX_TIMES) e->vadm.tm.read(k, &ms_avg[e->n_kernels + 1 + k], nullptr);
  if (n_runs) *n_runs = e->n_timed;
  return FVAD_OK;
}

extern "C" int fvad_engine_clear_times(fvad_engine *e) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  int rc = fvad_engine_sync(e);
  if (rc) return rc;
  for (double &v : e->ms_sum) v = 0;
  e->vadm.tm.clear();
  e->feed.tm.clear();
  if (e->rs) e->rs->tm.clear();
  if (e->ro) e->ro->tm.clear();
  if (e->cap) e->cap->tm.clear();
  e->n_timed = 0;
  e->res_count = 0;
  return FVAD_OK;
}

extern "C" int fvad_engine_fetch(fvad_engine *e, int n_ticks, fvad_outputs *out) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  if (n_ticks < 1 || n_ticks > e->cfg.max_ticks) return fail(FVAD_EINVAL, "n_ticks out of range");
  HIP_TRY(hipSetDevice(e->cfg.device));
  return fetch(e, n_ticks, out);
}

extern "C" int fvad_engine_spectrum_bins(const fvad_engine *e, int *lo, int *hi) {
  if (!e || !e->d_spec) return 0;
  if (lo) *lo = e->cfg.spec_lo;
  if (hi) *hi = e->cfg.spec_hi;
  return e->n_spec;
}

extern "C" int fvad_engine_fetch_spectrum(fvad_engine *e, int n_ticks, float *out) {
  if (!e || !out) return fail(FVAD_EINVAL, "null argument");
  if (!e->d_spec) return fail(FVAD_EINVAL, "engine created without want_spectrum");
  for (const fvad_engine::Slot &sl : e->slots)
    if (sl.pending) return fail(FVAD_EINVAL, "a submitted push is uncollected: the spectra are the last launched push's");
  if (n_ticks < 1 || n_ticks > e->last_ticks)
    return fail(FVAD_EINVAL, "n_ticks out of range [1, the last push's ticks]");
  if (const int rc = fvad_engine_sync(e)) return rc;
  const fvad_engine_config &c = e->cfg;
  HIP_TRY(hipMemcpy(out, e->d_spec.get(), sizeof(float) * (size_t)n_ticks * c.n_streams * e->wpt * c.n_channels * e->n_spec,
                    hipMemcpyDeviceToHost));
  return FVAD_OK;
}

extern "C" int fvad_engine_windows_per_tick(const fvad_engine *e) { return e ? e->wpt : FVAD_EINVAL; }

extern "C" const char *fvad_engine_kernel_name(const fvad_engine *e, int i) {
  // (per-stream configs run the _ps kernels, reported in the same two slots)
  if (e && i == e->n_kernels && e->vadm.on()) return e->vadm.ps ? "k_vadm_hbm_ps" : "k_vadm_hbm";
  if (e && i == e->n_kernels + 1 && e->vadm.on()) return e->vadm.ps ? "k_vadm_par_ps" : "k_vadm_par";
  if (!e || i < 0 || i >= e->n_kernels) return nullptr;
  if (e->cfg.mode == FVAD_MODE_FUSED) return i == 0 ? "k_prep" : "k_frame";
  return e->kernels.k[i].name;
}

extern "C" int fvad_engine_output_log(fvad_engine *e, int n_pushes) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  if (e->cfg.mode == FVAD_MODE_FUSED || !e->cfg.use_denoiser)
    return fail(FVAD_EINVAL, "the output log records staged / fp16 engines with the denoiser");
  if (n_pushes < 0) return fail(FVAD_EINVAL, "n_pushes >= 0 required");
  if (const int rc = fvad_engine_sync(e)) return rc;
  e->d_log.reset();
  const fvad_engine_config &c = e->cfg;
  const size_t MT = (size_t)c.max_ticks * c.n_streams, MW = MT * e->wpt;
  e->log_stride = 3 * MT + 2 * MW + MW * c.n_channels * c.n_bands;
  e->log_cap = e->log_n = 0;
  e->log_ticks.assign((size_t)n_pushes, 0);
  if (n_pushes > 0) {
    if (const int rc = make_dev(e->d_log, e->log_stride * (size_t)n_pushes)) return rc;
    e->log_cap = n_pushes;
  }
  return FVAD_OK;
}

extern "C" int fvad_engine_output_log_read(fvad_engine *e, int push, fvad_outputs *out, int *n_ticks) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  if (push < 0 || push >= e->log_n) return fail(FVAD_EINVAL, "push not in the log");
  if (const int rc = fvad_engine_sync(e)) return rc;
  const fvad_engine_config &c = e->cfg;
  const int T = e->log_ticks[push];
  const size_t MT = (size_t)c.max_ticks * c.n_streams, MW = MT * e->wpt;
  const size_t TB = (size_t)T * c.n_streams, TBW = TB * e->wpt;
  const float *L = e->d_log.get() + e->log_stride * (size_t)push;
  if (n_ticks) *n_ticks = T;
  if (!out) return FVAD_OK;
  void *dst[6] = {out->vad, out->ratio, out->win_flag, out->win_ratio, out->win_vad, out->band};
  const size_t off[6] = {0, MT, 2 * MT, 3 * MT, 3 * MT + MW, 3 * MT + 2 * MW};
  const size_t n[6] = {TB, TB, TB, TBW, TBW, TBW * c.n_channels * c.n_bands};
  for (int i = 0; i < 6; i++)
    if (dst[i]) HIP_TRY(hipMemcpy(dst[i], L + off[i], n[i] * 4, hipMemcpyDeviceToHost));
  return FVAD_OK;
}
