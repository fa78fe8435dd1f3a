// Batched multi-stream engine (C ABI in include/fvad.h).
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

const fvad::HostModel *fvad_model_host(const fvad_model *m);

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

extern "C" void fvad_engine_config_default(fvad_engine_config *c, int n_streams, int n_channels) {
  std::memset(c, 0, sizeof(*c));
  c->n_streams = n_streams;
  c->n_channels = n_channels;
  c->device = 0;
  c->sample_rate = 48000;
  c->fft_size = 2048;
  c->max_ticks = 100;
  c->n_bands = 1;
  // VADMachine defaults: freqToBin(100) .. freqToBin(1500) at 48 kHz / 2048 (FFT.zig:120-131)
  c->band_lo[0] = 4;
  c->band_hi[0] = 64;
  c->want_denoised = 0;
  c->use_denoiser = 1;
  c->denoised_rate_max = 0;
  c->input_rate_max = 0;
  c->denoised_rate = 0;
  c->input_rate = 0;
  c->want_spectrum = 0;
  c->spec_lo = 0;
  c->spec_hi = 1024;
}

namespace {

using fvad::make_dev;
using fvad::make_event;

// int8 GRU-stack image for k_rnn3 (layout: fvad_internal.h rnnimg).  Term j of
// a column's C-order sum lives in segment g at seg_off(g) + (j - start of g).
void build_rnn_image(const fvad::HostModel &hm, std::vector<int8_t> &img, int *act) {
  namespace R = fvad::rnnimg;
  img.assign(R::kBytes, 0);
  const int8_t *b = hm.blob;
  auto put = [&](int m, int c, int j, int8_t v) {
    int g = 0, base = 0;
    while (j >= base + R::kSegs[m][g]) base += R::kSegs[m][g++];
    img[R::off_w(m) + c * R::stride(m) + R::seg_off(m, g) + (j - base)] = v;
  };
  auto dense = [&](int m, int l) {
    const fvad::HostLayer &L = hm.layers[l];
    for (int c = 0; c < L.nout; c++) {
      img[R::off_b(m) + c] = b[L.off_b + c];
      for (int j = 0; j < L.nin; j++) put(m, c, j, b[L.off_w + (size_t)j * L.nout + c]);
    }
    act[m] = L.act;
  };
  auto gru = [&](int mg, int mh, int l) {
    const fvad::HostLayer &L = hm.layers[l];
    const int N = L.nout, M = L.nin, S3 = 3 * N;
    for (int col = 0; col < S3; col++) {
      const int m = col < 2 * N ? mg : mh, c = col < 2 * N ? col : col - 2 * N;
      img[R::off_b(m) + c] = b[L.off_b + col];
      for (int j = 0; j < M; j++) put(m, c, j, b[L.off_w + (size_t)j * S3 + col]);
      for (int j = 0; j < N; j++) put(m, c, M + j, b[L.off_r + (size_t)j * S3 + col]);
    }
    act[mg] = fvad::kActSigmoid;
    act[mh] = L.act;
  };
  dense(0, 0);
  gru(1, 2, 1);
  gru(3, 4, 2);
  gru(5, 6, 3);
  dense(7, 4);
  dense(8, 5);
}

// every int8 array of the model (what fvad_model_blob returns)
uint64_t model_hash_of(const fvad::HostModel &hm) { return fnv1a(kFnvBasis, hm.blob, hm.blob_size); }

int upload_model(fvad_engine *e, const fvad::HostModel &hm) {
  std::vector<float> w(hm.blob_size);
  for (size_t i = 0; i < hm.blob_size; i++) w[i] = (float)hm.blob[i];
  int rc = make_dev(e->d_weights, w.size());
  if (rc) return rc;
  HIP_TRY(hipMemcpy(e->d_weights.get(), w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
  auto dense = [&](int l) {
    const fvad::HostLayer &L = hm.layers[l];
    fvad::DevDense d;
    d.nin = L.nin;
    d.nout = L.nout;
    d.act = L.act;
    d.w = e->d_weights.get() + L.off_w;
    d.b = e->d_weights.get() + L.off_b;
    return d;
  };
  auto gru = [&](int l) {
    const fvad::HostLayer &L = hm.layers[l];
    fvad::DevGru g;
    g.nin = L.nin;
    g.nout = L.nout;
    g.act = L.act;
    g.win = e->d_weights.get() + L.off_w;
    g.wrec = e->d_weights.get() + L.off_r;
    g.b = e->d_weights.get() + L.off_b;
    return g;
  };
  for (int l = 0; l < 6; l++) {
    const fvad::HostLayer &L = hm.layers[l];
    const int m = l == 0 ? 0 : l == 1 ? 1 : l == 2 ? 3 : l == 3 ? 5 : l == 4 ? 7 : 8;
    if (L.nin != fvad::rnnimg::kKin[m] || (l >= 1 && l <= 3 ? 2 * L.nout : L.nout) != fvad::rnnimg::kCols[m])
      return fail(FVAD_EFORMAT, "model layer shapes differ from the rnnoise classic model");
  }
  {
    std::vector<int8_t> img;
    build_rnn_image(hm, img, e->rnn_act);
    rc = make_dev(e->d_rnn_img, img.size());
    if (rc) return rc;
    HIP_TRY(hipMemcpy(e->d_rnn_img.get(), img.data(), img.size(), hipMemcpyHostToDevice));
    if (fp16_mode(e->cfg.mode)) {  // MFMA fragments of the same image (fvad_gru16.hip)
      std::vector<uint16_t> frags((size_t)fvad::gru16_frag_count() * 64 * 8);
      std::vector<float> bias(fvad::gru16_bias_rows());
      fvad::gru16_build(img.data(), frags.data(), bias.data());
      if ((rc = make_dev(e->d_gru16, frags.size())) || (rc = make_dev(e->d_gru16_bias, bias.size()))) return rc;
      HIP_TRY(hipMemcpy(e->d_gru16.get(), frags.data(), frags.size() * 2, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(e->d_gru16_bias.get(), bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
    }
  }
  e->dmodel.in_dense = dense(0);
  e->dmodel.vad = gru(1);
  e->dmodel.noise = gru(2);
  e->dmodel.den = gru(3);
  e->dmodel.den_out = dense(4);
  e->dmodel.vad_out = dense(5);
  rc = make_dev(e->d_model, 1);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(e->d_model.get(), &e->dmodel, sizeof(fvad::DevModel), hipMemcpyHostToDevice));
  return FVAD_OK;
}

}  // namespace

extern "C" int fvad_engine_reset(fvad_engine *e) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (e->cstream) HIP_TRY(hipStreamSynchronize(e->cstream.get()));
  if (e->pstream) HIP_TRY(hipStreamSynchronize(e->pstream));
  if (e->vadm.n > 0) {
    e->vpend = false;  // the pending push's machine state is wiped below: not run
    e->vowed = false;
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    HIP_TRY(hipStreamSynchronize(e->side));
    int rc = vadm_reset(e);
    if (!rc && e->events_on) rc = events_reset(e);
    if (rc) return rc;
  }
  e->push_count = 0;
  HIP_TRY(hipMemsetAsync(e->d_state.get(), 0, sizeof(float) * fvad::st::kWords * (size_t)e->cfg.n_streams, e->stream.get()));
  e->res_next = 0;  // fresh streams start at the resident cycle's first push (t = 0)
  if (e->d_work) HIP_TRY(hipMemsetAsync(e->d_work.get(), 0, sizeof(unsigned) * fvad::kWorkCounters, e->stream.get()));
  HIP_TRY(hipMemsetAsync(e->d_ring.get(), 0,
                         sizeof(float) * (size_t)e->ring_len * e->cfg.n_channels * e->cfg.n_streams, e->stream.get()));
  if (const int rc = resample_reset(e)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream.get()));
  return FVAD_OK;
}

namespace {
void fill_bands(const fvad_engine_config &c, int *band_lo, int *band_hi, int *lo_all, int *hi_all) {
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

// fvad_engine_create's check of input_rate / denoised_rate and its *_rate_max:
// per-stream, rate_max is a listed rate or 48000; otherwise rate_max is 0 and
// the rate, when it is not 0 or 48000, a listed one, described in d
struct RateTexts {
  const char *max_off_list, *max_unread, *rate_off_list;
};
int check_rate(int rate, int rate_max, bool per_stream, fvad::rs::Dir dir, fvad::rs::Desc &d, const RateTexts &t) {
  if (per_stream) return fvad::rs::rate_index(rate_max) < 0 ? fail(FVAD_ERATE, t.max_off_list) : FVAD_OK;
  if (rate_max != 0) return fail(FVAD_ERATE, t.max_unread);
  if (rate != 0 && rate != 48000 && !fvad::rs::describe(rate, dir, d)) return fail(FVAD_ERATE, t.rate_off_list);
  return FVAD_OK;
}

}  // namespace

// one set of window outputs (the pass's ticks copy is attach_vadm's)
int fvad::eng::make_win_out(const fvad_engine *e, fvad_engine::WinOut &w) {
  const fvad_engine_config &c = e->cfg;
  const size_t TB = (size_t)c.max_ticks * c.n_streams, TBW = TB * e->wpt;  // window slots
  int rc;
  if ((rc = make_dev(w.ratio, TBW)) || (rc = make_dev(w.vad, TBW)) || (rc = make_dev(w.flag, TB)) ||
      (rc = make_dev(w.band, TBW * c.n_channels * c.n_bands)))
    return rc;
  return FVAD_OK;
}

// the push about to launch writes window-output set b
void fvad::eng::use_win_out(fvad_engine *e, int b) {
  const fvad_engine::WinOut &w = e->wout[e->wout[1].flag ? b : 0];
  e->d_wflag = w.flag.get();
  e->d_wratio = w.ratio.get();
  e->d_wvad = w.vad.get();
  e->d_band = w.band.get();
}

extern "C" int fvad_engine_create(const fvad_engine_config *cfg, const fvad_model *model, fvad_engine **out) {
  if (!cfg || !model || !out) return fail(FVAD_EINVAL, "null argument");
  const fvad_engine_config &c = *cfg;
  if (c.sample_rate != 48000) return fail(FVAD_ERATE, "only 48 kHz is supported (VAD.zig:101-104)");
  // input_rate: 0 or 48000 for none, or a rate k_resample brings to 48 kHz;
  // FVAD_INPUT_RATE_PER_STREAM: every stream its own rate, up to input_rate_max
  const bool resample = c.input_rate != 0 && c.input_rate != 48000;
  const bool per_stream = c.input_rate == FVAD_INPUT_RATE_PER_STREAM;
  fvad::rs::Desc rd{};
  if (const int rc = check_rate(c.input_rate, c.input_rate_max, per_stream, fvad::rs::Dir::kIn, rd,
                                {"input_rate_max must be 8000, 16000, 24000, 32000, 44100, 48000 or 96000",
                                 "input_rate_max is read only with input_rate = FVAD_INPUT_RATE_PER_STREAM",
                                 "input_rate must be 0, 48000, 8000, 16000, 24000, 32000, 44100 or 96000"}))
    return rc;
  // denoised_rate: 0 or 48000 for the 48 kHz signal, or a rate k_resample_out brings it to;
  // FVAD_DENOISED_RATE_PER_STREAM: every stream its own rate, up to denoised_rate_max
  const bool resample_out = c.denoised_rate != 0 && c.denoised_rate != 48000;
  const bool per_stream_out = c.denoised_rate == FVAD_DENOISED_RATE_PER_STREAM;
  fvad::rs::Desc od{};
  if (const int rc = check_rate(c.denoised_rate, c.denoised_rate_max, per_stream_out, fvad::rs::Dir::kOut, od,
                                {"denoised_rate_max must be 8000, 16000, 24000, 32000, 44100, 48000 or 96000",
                                 "denoised_rate_max is read only with denoised_rate = FVAD_DENOISED_RATE_PER_STREAM",
                                 "denoised_rate must be 0, 48000, 8000, 16000, 24000, 32000, 44100 or 96000"}))
    return rc;
  if (per_stream_out) {
    if (c.want_denoised != 1 || !c.use_denoiser)
      return fail(FVAD_EINVAL, "per-stream denoised rates need want_denoised = 1 and use_denoiser = 1");
    if (c.max_ticks > 65535) return fail(FVAD_EINVAL, "per-stream denoised rates: max_ticks <= 65535 (a grid dimension)");
  }
  if (resample_out && !per_stream_out && (!c.want_denoised || !c.use_denoiser))
    return fail(FVAD_EINVAL, "denoised_rate needs want_denoised = 1 and use_denoiser = 1");
  if (c.n_streams < 1 || c.n_channels < 1 || c.n_channels > FVAD_MAX_CHANNELS)
    return fail(FVAD_EINVAL, "n_streams >= 1 and 1 <= n_channels <= 8 required");
  // FFT.zig:29-31: any even, non-zero size.  fft_size < 480 completes several
  // windows per tick (VAD.zig:307-347; fvad_engine_windows_per_tick slots per
  // tick in the window outputs); kMaxFftSize keeps window indices in 32 bits
  if (c.fft_size < 2 || (c.fft_size & 1) || c.fft_size > fvad::kMaxFftSize)
    return fail(FVAD_EINVAL, "fft_size must be even, 2 <= fft_size <= 4194304 (FFT.zig:29-31)");
  if (c.mode == FVAD_MODE_FUSED) {
    int n = c.fft_size / 2;
    for (int p : {4, 2, 3, 5})
      while (n % p == 0) n /= p;
    if (n != 1 || c.fft_size > 2048 || c.fft_size < fvad::kFrame)
      return fail(FVAD_EINVAL, "fused mode: 480 <= fft_size <= 2048 with radices 2, 3, 4, 5 (use the staged mode)");
  }
  if (!c.use_denoiser && c.mode == FVAD_MODE_FUSED)
    return fail(FVAD_EINVAL, "use_denoiser = 0 runs on the staged engine");
  if (c.max_ticks < 1) return fail(FVAD_EINVAL, "max_ticks must be >= 1");
  if (c.n_bands < 1 || c.n_bands > FVAD_MAX_BANDS) return fail(FVAD_EINVAL, "1 <= n_bands <= 4");
  int lo = 1 << 30, hi = -1;
  for (int b = 0; b < c.n_bands; b++) {
    if (c.band_lo[b] < 0 || c.band_hi[b] < c.band_lo[b] || c.band_hi[b] > c.fft_size / 2)
      return fail(FVAD_EINVAL, "invalid band range");
    lo = std::min(lo, c.band_lo[b]);
    hi = std::max(hi, c.band_hi[b]);
  }
  if (hi - lo + 1 > 256 && (c.mode == FVAD_MODE_FUSED || c.fft_size == 2048))
    return fail(FVAD_EINVAL, "reported bins must span <= 256");
  if (c.mode != FVAD_MODE_STAGED && c.mode != FVAD_MODE_FUSED && !fp16_mode(c.mode) && c.mode != FVAD_MODE_F32_FAST)
    return fail(FVAD_EINVAL, "unknown engine mode");
  if (c.want_spectrum) {
    if (c.mode == FVAD_MODE_FUSED) return fail(FVAD_EINVAL, "want_spectrum runs on the staged engines (k_frame has no tap)");
    if (c.spec_lo < 0 || c.spec_hi < c.spec_lo || c.spec_hi > c.fft_size / 2)
      return fail(FVAD_EINVAL, "invalid spectrum range: 0 <= spec_lo <= spec_hi <= fft_size / 2 required");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(FVAD_EDEVICE, "no HIP device available");
  if (c.device < 0 || c.device >= ndev) return fail(FVAD_EDEVICE, "device ordinal out of range");

  fvad_engine *e = new fvad_engine();
  e->cfg = c;
  if (!resample) e->cfg.input_rate = 0;
  if (!resample_out) e->cfg.denoised_rate = 0;
  // the staged path writes every tick of a push before FFT B reads its
  // windows, so the ring holds one window plus a whole push
  // the re-block ring holds a window plus a push; a multiple of 4 so a
  // frame's float4 writes never straddle its end (k_ola, k_ndring)
  e->ring_len = (c.fft_size + c.max_ticks * fvad::kFrame + 3) & ~3;
  e->n_kernels = 2;  // fused: k_prep, k_frame
  if (c.mode != FVAD_MODE_FUSED) {
    // the kernels of this engine's pushes (launch_staged's variant: run_staged
    // sets a.fma, a.gru16_frags and a.fuse16 from the mode)
    fvad::StagedArgs probe{};
    probe.nfft_b = c.fft_size;
    probe.n_channels = c.n_channels;
    const bool olafb = c.use_denoiser && fvad::olafb_fused(probe);
    e->kernels = fvad::staged_kernels({c.mode == FVAD_MODE_F32_FAST && c.use_denoiser, fp16_mode(c.mode),
                                       c.mode == FVAD_MODE_FP16_FUSED, olafb});
    e->n_kernels = e->kernels.n;
    if (c.want_spectrum && c.fft_size == 2048)  // the tap twins' names in the FFT-B slot (fvad_wave.hip)
      for (int i = 0; i < e->kernels.n; i++) {
        fvad::StagedKernel &k = e->kernels.k[i];
        if (k.stage == fvad::kStageOla && olafb) k.name = "k_olafb_spec";
        if (k.stage == fvad::kStageFftB) k.name = "k_fftbw_spec";
      }
  }
  e->n_events = c.mode != FVAD_MODE_FUSED ? fvad::kStagedEvents : 3;
  e->last_event = c.mode != FVAD_MODE_FUSED ? fvad::kStagedLast : 2;
  static_assert(fvad::kStagedEvents <= FVAD_MAX_TIMES, "timing events");
  auto bail = [&](int rc) {
    delete e;
    return rc;
  };
  if (hipSetDevice(c.device) != hipSuccess) return bail(fail(FVAD_EDEVICE, "hipSetDevice failed"));
  int rc = fvad::make_stream(e->stream);
  if (rc) return bail(rc);
  if (c.mode != FVAD_MODE_FUSED) {
    fvad::stream_ptr prep;
    if ((rc = fvad::make_stream(prep)) || (rc = make_event(e->ev_prep_done[0])) ||
        (rc = make_event(e->ev_prep_done[1])) || (rc = make_event(e->ev_buf_free[0])) ||
        (rc = make_event(e->ev_buf_free[1])) || (rc = make_event(e->ev_fft_a)) || (rc = make_event(e->ev_synth)))
      return bail(rc);
    e->pstream_ref = std::move(prep);
    e->pstream = e->pstream_ref.get();
  }
  for (int i = 0; i < e->n_events; i++)
    for (int k = 0; k < 2; k++) {
      if ((rc = make_event(e->evs_own[k][i], true))) return bail(rc);
      e->evs[k][i] = e->evs_own[k][i].get();
    }
  fvad::Plan *plan = new fvad::Plan();
  fvad::build_plan(plan, c.fft_size);
  e->wpt = fvad::windows_per_tick(c.fft_size);
  if (c.fft_size > fvad::kMaxFftB) {  // FFT B's tables outside the plan: [tw | sup | hann | perm]
    const size_t n = c.fft_size;
    std::vector<float> tab(n + n / 2 + n + n / 2);
    int *perm = reinterpret_cast<int *>(tab.data() + n + n / 2 + n);
    plan->norm_b = fvad::build_fftb_tables(c.fft_size, plan->fac_b, tab.data(), tab.data() + n, perm,
                                           tab.data() + n + n / 2);
    rc = make_dev(e->d_fbtab, tab.size());
    if (!rc && hipMemcpy(e->d_fbtab.get(), tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(FVAD_EDEVICE, "FFT-B table upload failed");
  }
  if (!rc) rc = make_dev(e->d_plan, 1);
  if (!rc && hipMemcpy(e->d_plan.get(), plan, sizeof(fvad::Plan), hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(FVAD_EDEVICE, "plan upload failed");
  delete plan;
  if (rc) return bail(rc);
  if ((rc = upload_model(e, *fvad_model_host(model)))) return bail(rc);
  e->model_hash = model_hash_of(*fvad_model_host(model));
  const size_t B = c.n_streams, C = c.n_channels, T = c.max_ticks;
  const size_t frames = T * B * C * fvad::kFrame;
  if ((rc = make_dev(e->d_state, B * fvad::st::kWords)) || (rc = make_dev(e->d_ring, B * C * e->ring_len)) ||
      (rc = make_dev(e->d_pcm_b[0], frames)) || (rc = make_dev(e->d_pcm_b[1], frames)) ||
      (rc = make_dev(e->d_ratio_b[0], T * B)) ||
      (rc = make_dev(e->d_vad, T * B)) || (rc = make_win_out(e, e->wout[0])) ||
      (rc = make_dev(e->d_ticks_b[0], 2 * B)) || (c.want_denoised && (rc = make_dev(e->d_den, frames))))
    return bail(rc);
  e->d_pcm = e->d_pcm_b[0].get();
  if ((rc = make_event(e->ev_in_free[0])) || (rc = make_event(e->ev_in_free[1]))) return bail(rc);
  e->d_ratio = e->d_ratio_b[0].get();
  e->d_ticks = e->d_ticks_b[0].get();
  use_win_out(e, 0);
  if (c.mode == FVAD_MODE_FUSED) {
    if ((rc = make_dev(e->d_xbuf, frames))) return bail(rc);
  } else {
    e->V = (int)(T * C);
    e->L = (fvad::kPitchBuf - fvad::kFrame) + e->V * fvad::kFrame;
    e->LX = e->L / 2;
    e->wmax = (int)(T * fvad::kFrame / c.fft_size) + 2;
    const size_t F = B * e->V;
    if ((rc = make_dev(e->d_xs_b[0], B * e->L)) || (rc = make_dev(e->d_xs_b[1], B * e->L)) ||
        (rc = make_dev(e->d_xlp_b[0], B * e->LX)) || (rc = make_dev(e->d_xlp_b[1], B * e->LX)) ||
        (rc = make_dev(e->d_ratio_b[1], T * B)) || (rc = make_dev(e->d_ticks_b[1], 2 * B)) || (rc = make_dev(e->d_X, F * fvad::kFreq * 2)) ||
        (rc = make_dev(e->d_P, F * fvad::kFreq * 2)) || (rc = make_dev(e->d_Ex, F * fvad::kBands)) ||
        (rc = make_dev(e->d_Ep, F * fvad::kBands)) || (rc = make_dev(e->d_Exp, F * fvad::kBands)) ||
        (rc = make_dev(e->d_Lyf, F * fvad::kBands)) || (rc = make_dev(e->d_f34, F * 8)) ||
        (rc = make_dev(e->d_rec, F * fvad::kPitchRecord)) || (rc = make_dev(e->d_work, (size_t)fvad::kWorkCounters)) ||
        (rc = make_dev(e->d_ptile, (B + fvad::ptile::kTile - 1) / fvad::ptile::kTile * e->V * fvad::ptile::kTile *
                                      fvad::ptile::kRows)) || (rc = make_dev(e->d_vadf, F)) ||
        (rc = make_dev(e->d_ys, F * fvad::kWin)) || (rc = make_dev(e->d_sil, F)) || (rc = make_dev(e->d_pitch, F)) ||
        (rc = make_dev(e->d_wtick, B * e->wmax)) || (rc = make_dev(e->d_wstart, B * e->wmax)) ||
        (rc = make_dev(e->d_gr, F * fvad::kBands)) || (rc = make_dev(e->d_gs, F * fvad::kBands)))
      return bail(rc);
    e->d_xs = e->d_xs_b[0].get();
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c.device) != hipSuccess) return bail(fail(FVAD_EDEVICE, "device query failed"));
    // CUs; persistent grids are sized per kernel
    e->grid_frames = prop.multiProcessorCount;
    // k_fftb's device scratch when a transform does not fit in LDS: a slice per
    // workgroup, at most two per CU and 1 GiB
    int lo = 0, hi = 0, band_lo[fvad::kMaxBandCfg], band_hi[fvad::kMaxBandCfg];
    fill_bands(c, band_lo, band_hi, &lo, &hi);
    e->fb_work_stride = fvad::fftb_work_stride(c.fft_size, lo, hi, fvad::fftb_generic(c.fft_size / 2));
    if (e->fb_work_stride > 0) {
      const long long per = e->fb_work_stride * (long long)sizeof(float2);
      const long long units = (long long)B * e->wmax;
      e->fb_work_blocks = (int)std::max<long long>(
          1, std::min<long long>({units, 2LL * e->grid_frames, (1LL << 30) / per}));
      if ((rc = make_dev(e->d_fbwork, (size_t)e->fb_work_blocks * e->fb_work_stride))) return bail(rc);
    }
  }
  if (c.want_spectrum) {
    e->n_spec = c.spec_hi - c.spec_lo + 1;
    if ((rc = make_dev(e->d_spec, T * B * e->wpt * C * (size_t)e->n_spec))) return bail(rc);
  }
  if (resample && (rc = resample_make(e, rd, c.input_rate_max))) return bail(rc);
  if (resample_out && (rc = resample_out_make(e, od, c.denoised_rate_max))) return bail(rc);
  if ((rc = fvad_engine_reset(e))) return bail(rc);
  *out = e;
  return FVAD_OK;
}

extern "C" void fvad_engine_destroy(fvad_engine *e) {
  if (!e) return;
  (void)hipSetDevice(e->cfg.device);
  if (e->cstream) (void)hipStreamSynchronize(e->cstream.get());
  if (e->pstream) (void)hipStreamSynchronize(e->pstream);
  e->vpend = false;  // the last push's machine would only update state that is freed
  if (e->stream) (void)hipStreamSynchronize(e->stream.get());
  if (e->side) (void)hipStreamSynchronize(e->side);
  delete e;
}

// e runs its k_prep3 (which & FVAD_SHARE_PREP) and / or its VADMachine
// kernels (which & FVAD_SHARE_SIDE) on other's streams from now on.  Both
// engines idle (synchronised here); every dependency stays an event, so
// sharing only adds order between the engines' side work.  An engine whose
// prep stream is shared runs k_fftAw on its own stream (launch_staged), so
// the main pipelines stay independent.
extern "C" int fvad_engine_share_streams(fvad_engine *e, fvad_engine *other, int which) {
  if (!e || !other || e == other || (which & ~(FVAD_SHARE_PREP | FVAD_SHARE_SIDE)) || !which)
    return fail(FVAD_EINVAL, "invalid argument");
  if (e->cfg.device != other->cfg.device) return fail(FVAD_EINVAL, "engines on different devices");
  if ((which & FVAD_SHARE_PREP) && (!e->pstream || !other->pstream))
    return fail(FVAD_EINVAL, "FVAD_SHARE_PREP needs two staged engines");
  if ((which & FVAD_SHARE_SIDE) && (!e->side || !other->side))
    return fail(FVAD_EINVAL, "FVAD_SHARE_SIDE needs device VADMachines attached to both engines");
  int rc;
  if ((rc = fvad_engine_sync(e)) || (rc = fvad_engine_sync(other))) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (which & FVAD_SHARE_PREP) {
    e->pstream_ref = other->pstream_ref;
    e->pstream = other->pstream;
  }
  if (which & FVAD_SHARE_SIDE) {
    e->side_ref = other->side_ref;
    e->side = other->side;
  }
  return FVAD_OK;
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
  fvad::StagedArgs a{};
  a.n_streams = c.n_streams;
  a.n_channels = c.n_channels;
  a.V = e->V;
  a.L = e->L;
  a.LX = e->LX;
  a.state = e->d_state.get();
  a.X = reinterpret_cast<float2 *>(e->d_X.get());
  a.P = reinterpret_cast<float2 *>(e->d_P.get());
  a.Ex = e->d_Ex.get();
  a.Ep = e->d_Ep.get();
  a.Exp = e->d_Exp.get();
  a.Lyf = e->d_Lyf.get();
  a.f34 = e->d_f34.get();
  a.silence = e->d_sil.get();
  a.rec = e->d_rec.get();
  a.ptile = e->d_ptile.get();
  a.work = e->d_work.get();
  a.pitch = e->d_pitch.get();
  a.vadf = e->d_vadf.get();
  a.gr = e->d_gr.get();
  a.gs = e->d_gs.get();
  a.rnn_img = e->d_rnn_img.get();
  a.gru16_frags = e->d_gru16.get();
  a.gru16_bias = e->d_gru16_bias.get();
  a.fuse16 = e->cfg.mode == FVAD_MODE_FP16_FUSED;
  a.fma = e->cfg.mode == FVAD_MODE_F32_FAST;
  for (int m = 0; m < fvad::rnnimg::kMats; m++) a.rnn_act[m] = e->rnn_act[m];
  a.ys = e->d_ys.get();
  a.ring = e->d_ring.get();
  a.ring_len = e->ring_len;
  a.win_tick = e->d_wtick.get();
  a.win_start = e->d_wstart.get();
  a.wmax = e->wmax;
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
  a.fb_work = e->d_fbwork.get();
  a.fb_work_blocks = e->fb_work_blocks;
  a.fb_work_stride = e->fb_work_stride;
  a.plan = e->d_plan.get();
  a.model = e->d_model.get();
  a.n_bands = c.n_bands;
  fill_bands(c, a.band_lo, a.band_hi, &a.bin_lo_all, &a.bin_hi_all);
  a.nfft_b = c.fft_size;
  a.use_denoiser = c.use_denoiser;
  a.out_vad = e->d_vad.get();
  a.out_den = e->d_den.get();
  a.raw_s16 = e->raw_s16;
  a.vadm = e->vadm;
  a.stamps = e->d_stamps.get();
  a.spec = e->d_spec.get();
  a.spec_lo = c.spec_lo;
  a.spec_hi = c.spec_hi;
  return a;
}

int run_staged(fvad_engine *e, int n_ticks, bool use_ticks, bool use_tail, bool timed) {
  const fvad_engine_config &c = e->cfg;
  // the previous push's VADMachine (after that push's ev_buf_free)
  if (e->vpend)
    if (const int rf = vadm_flush(e, false)) return rf;
  // push k uses buffer b = k & 1 of xs / ratio / ticks; its k_prep3 waits
  // (on pstream) until push k-2 released b, then runs beside push k-1
  const int b = e->next_buf;
  if (e->buf_busy[b]) HIP_TRY(wait_event(e->pstream, e->ev_buf_free[b].get()));
  if (e->fft_a_rec) HIP_TRY(wait_event(e->pstream, e->ev_fft_a.get()));
  e->d_xs = e->d_xs_b[b].get();
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
  a.xs = e->d_xs;
  a.xlp = e->d_xlp_b[b].get();
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
    HIP_TRY(hipEventRecord(e->ev_prep_done[b].get(), e->pstream));
    HIP_TRY(wait_event(e->stream.get(), e->ev_prep_done[b].get()));
    // window output set b is free once push k-2's k_vadm_hbm has read it
    if (e->vadm.n > 0) HIP_TRY(wait_event(e->stream.get(), e->ev_vadm_b[b].get()));
    // k_fftAw runs on the prep stream only while this engine owns it: on a
    // shared one (FVAD_SHARE_PREP) it would queue behind the other engine's
    // waits and couple the two pipelines, so it stays on the engine stream
    const bool own_prep = e->pstream_ref.use_count() <= 1;
    HIP_TRY(fvad::launch_staged(a, e->grid_frames, e->stream.get(), timed ? e->ev : nullptr, e->ev_fft_a.get(),
                                own_prep ? e->pstream : nullptr, e->synth_rec ? e->synth_wait : nullptr,
                                e->ev_synth.get()));
    // (launch_staged records the timing event in ev_synth's place when timed)
    e->synth_wait = timed ? e->ev[fvad::kEvSynthEnd] : e->ev_synth.get();
    e->synth_rec = true;
    e->fft_a_rec = true;
  } else {
    // no denoiser: raw input frames to the ring, windows, FFT B, all on the
    // engine stream after the input copy (queued on the prep stream)
    HIP_TRY(hipEventRecord(e->ev_prep_done[b].get(), e->pstream));
    HIP_TRY(wait_event(e->stream.get(), e->ev_prep_done[b].get()));
    if (e->vadm.n > 0) HIP_TRY(wait_event(e->stream.get(), e->ev_vadm_b[b].get()));
    HIP_TRY(fvad::launch_nodenoise(a, e->grid_frames, e->stream.get()));
  }
  if (e->vadm.n > 0) {
    // the ticks copy of parity b may be overwritten once push k - 2's
    // VADMachine has read it (ev_vadm_b[b], waited for above)
    if (use_ticks)
      HIP_TRY(hipMemcpyAsync(e->wout[b].vticks.get(), e->d_ticks, (size_t)c.n_streams * 4, hipMemcpyDeviceToDevice,
                             e->stream.get()));
    fvad::StagedArgs v = a;
    v.ticks_valid = use_ticks ? e->wout[b].vticks.get() : nullptr;
    e->vpend = true;
    e->vpend_args = v;
    e->vpend_b = b;
    e->vpend_timed = timed;
    e->vpend_push = e->push_count;
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
  HIP_TRY(hipEventRecord(e->ev_buf_free[b].get(), e->stream.get()));
  e->buf_busy[b] = true;
  e->next_buf = b ^ 1;
  return FVAD_OK;
}

}  // namespace

int fvad::eng::launch(fvad_engine *e, int n_ticks, bool use_ticks, bool timed, bool use_tail) {
  if (!e->cfg.use_denoiser) timed = false;  // the no-denoiser pipeline records no kernel events
  if (e->rs) {
    // the push's first kernel: the raw input to 48 kHz, on the stream that
    // owns the tails, behind the copies of the input and of ticks_valid
    const int *tv = !use_ticks ? nullptr
                    : e->cfg.mode != FVAD_MODE_FUSED ? e->d_ticks_b[e->next_buf].get() : e->d_ticks;
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
    const int b = e->next_buf;
    if (e->buf_busy[b]) HIP_TRY(hipStreamWaitEvent(e->pstream, e->ev_buf_free[b].get(), 0));
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
    if (e->vadm.n > 0 && e->n_kernels + 1 + k < FVAD_MAX_TIMES)
      ms_avg[e->n_kernels + 1 + k] = e->vadm_timed[k] ? e->vadm_ms_sum[k] / e->vadm_timed[k] : 0.0;
  if (n_runs) *n_runs = e->n_timed;
  return FVAD_OK;
}

extern "C" int fvad_engine_clear_times(fvad_engine *e) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  int rc = fvad_engine_sync(e);
  if (rc) return rc;
  for (double &v : e->ms_sum) v = 0;
  for (int k = 0; k < 2; k++) {
    e->vadm_ms_sum[k] = 0;
    e->vadm_timed[k] = 0;
  }
  e->et_ms_sum = 0;
  e->et_timed = 0;
  if (e->rs) e->rs->tm.clear();
  if (e->ro) e->ro->tm.clear();
  if (e->cap)
    for (int k = 0; k < 2; k++) {
      e->cap->ms_sum[k] = 0;
      e->cap->n_timed[k] = 0;
    }
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
  if (e && i == e->n_kernels && e->vadm.n > 0) return e->vadm_ps ? "k_vadm_hbm_ps" : "k_vadm_hbm";
  if (e && i == e->n_kernels + 1 && e->vadm.n > 0) return e->vadm_ps ? "k_vadm_par_ps" : "k_vadm_par";
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
