// The batched engine's construction (C ABI in include/fvad.h): the config
// check, the kernel table, the plan and the model upload, the buffers of both
// engine kinds (staged_make for the staged pipeline's), destroy and the sharing
// of streams.  The device memory layout: fvad_engine.cpp.
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "fvad_engine_impl.h"

const fvad::HostModel *fvad_model_host(const fvad_model *m);

using namespace fvad::eng;

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
int fvad::eng::make_win_out(const fvad_engine *e, WinOut &w) {
  const fvad_engine_config &c = e->cfg;
  const size_t TB = (size_t)c.max_ticks * c.n_streams, TBW = TB * e->wpt;  // window slots
  int rc;
  if ((rc = make_dev(w.ratio, TBW)) || (rc = make_dev(w.vad, TBW)) || (rc = make_dev(w.flag, TB)) ||
      (rc = make_dev(w.band, TBW * c.n_channels * c.n_bands)))
    return rc;
  return FVAD_OK;
}

namespace {

// What the config check settles for the steps after it: which resamplers the
// engine has, and the fixed rates' descriptions
struct Rates {
  bool in = false, out = false;
  fvad::rs::Desc in_d{}, out_d{};
};

// fvad_engine_create's check of the config: calls no HIP function
int check_config(const fvad_engine_config &c, Rates &r) {
  if (c.sample_rate != 48000) return fail(FVAD_ERATE, "only 48 kHz is supported (VAD.zig:101-104)");
  // input_rate: 0 or 48000 for none, or a rate k_resample brings to 48 kHz;
  // FVAD_INPUT_RATE_PER_STREAM: every stream its own rate, up to input_rate_max
  r.in = c.input_rate != 0 && c.input_rate != 48000;
  const bool per_stream = c.input_rate == FVAD_INPUT_RATE_PER_STREAM;
  if (const int rc = check_rate(c.input_rate, c.input_rate_max, per_stream, fvad::rs::Dir::kIn, r.in_d,
                                {"input_rate_max must be 8000, 16000, 24000, 32000, 44100, 48000 or 96000",
                                 "input_rate_max is read only with input_rate = FVAD_INPUT_RATE_PER_STREAM",
                                 "input_rate must be 0, 48000, 8000, 16000, 24000, 32000, 44100 or 96000"}))
    return rc;
  // denoised_rate: 0 or 48000 for the 48 kHz signal, or a rate k_resample_out brings it to;
  // FVAD_DENOISED_RATE_PER_STREAM: every stream its own rate, up to denoised_rate_max
  r.out = c.denoised_rate != 0 && c.denoised_rate != 48000;
  const bool per_stream_out = c.denoised_rate == FVAD_DENOISED_RATE_PER_STREAM;
  if (const int rc = check_rate(c.denoised_rate, c.denoised_rate_max, per_stream_out, fvad::rs::Dir::kOut, r.out_d,
                                {"denoised_rate_max must be 8000, 16000, 24000, 32000, 44100, 48000 or 96000",
                                 "denoised_rate_max is read only with denoised_rate = FVAD_DENOISED_RATE_PER_STREAM",
                                 "denoised_rate must be 0, 48000, 8000, 16000, 24000, 32000, 44100 or 96000"}))
    return rc;
  if (per_stream_out) {
    if (c.want_denoised != 1 || !c.use_denoiser)
      return fail(FVAD_EINVAL, "per-stream denoised rates need want_denoised = 1 and use_denoiser = 1");
    if (c.max_ticks > 65535) return fail(FVAD_EINVAL, "per-stream denoised rates: max_ticks <= 65535 (a grid dimension)");
  }
  if (r.out && !per_stream_out && (!c.want_denoised || !c.use_denoiser))
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
  return FVAD_OK;
}

// The kernels of this engine's pushes and their timing events, two sets
int make_kernel_table(fvad_engine *e) {
  const fvad_engine_config &c = e->cfg;
  const bool staged = c.mode != FVAD_MODE_FUSED;
  e->n_kernels = 2;  // fused: k_prep, k_frame
  if (staged) {
    // launch_staged's variant: run_staged sets a.fma, a.gru16_frags and
    // a.fuse16 from the mode
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
  e->n_events = staged ? fvad::kStagedEvents : 3;
  e->last_event = staged ? fvad::kStagedLast : 2;
  static_assert(fvad::kStagedEvents <= FVAD_MAX_TIMES, "timing events");
  for (int i = 0; i < e->n_events; i++)
    for (int k = 0; k < 2; k++) {
      if (const int rc = make_event(e->evs_own[k][i], true)) return rc;
      e->evs[k][i] = e->evs_own[k][i].get();
    }
  return FVAD_OK;
}

// The plan, FFT B's tables where they lie outside it, and the model
int make_plan_and_tables(fvad_engine *e, const fvad_model *model) {
  const fvad_engine_config &c = e->cfg;
  e->wpt = fvad::windows_per_tick(c.fft_size);
  int rc = FVAD_OK;
  const std::unique_ptr<fvad::Plan> plan(new fvad::Plan());
  fvad::build_plan(plan.get(), c.fft_size);
  if (c.fft_size > fvad::kMaxFftB) {  // FFT B's tables outside the plan: [tw | sup | hann | perm]
    const size_t n = c.fft_size;
    std::vector<float> tab(n + n / 2 + n + n / 2);
    int *perm = reinterpret_cast<int *>(tab.data() + n + n / 2 + n);
    plan->norm_b = fvad::build_fftb_tables(c.fft_size, plan->fac_b, tab.data(), tab.data() + n, perm,
                                           tab.data() + n + n / 2);
    if ((rc = make_dev(e->d_fbtab, tab.size()))) return rc;
    if (hipMemcpy(e->d_fbtab.get(), tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
      return fail(FVAD_EDEVICE, "FFT-B table upload failed");
  }
  if ((rc = make_dev(e->d_plan, 1))) return rc;
  if (hipMemcpy(e->d_plan.get(), plan.get(), sizeof(fvad::Plan), hipMemcpyHostToDevice) != hipSuccess)
    return fail(FVAD_EDEVICE, "plan upload failed");
  if ((rc = upload_model(e, *fvad_model_host(model)))) return rc;
  e->model_hash = model_hash_of(*fvad_model_host(model));
  return FVAD_OK;
}

// The buffers every engine kind has: state, ring, the two inputs, buffer 0 of
// ratio / ticks, the outputs and window-output set 0
int make_common(fvad_engine *e) {
  const fvad_engine_config &c = e->cfg;
  const size_t B = c.n_streams, C = c.n_channels, T = c.max_ticks;
  const size_t frames = T * B * C * fvad::kFrame;
  // the re-block ring holds a window plus a push (the staged path writes
  // every tick of a push before FFT B reads its windows); a multiple of 4 so
  // a frame's float4 writes never straddle its end (k_ola, k_ndring)
  e->ring_len = (c.fft_size + c.max_ticks * fvad::kFrame + 3) & ~3;
  int rc;
  if ((rc = make_dev(e->d_state, B * fvad::st::kWords)) || (rc = make_dev(e->d_ring, B * C * e->ring_len)) ||
      (rc = make_dev(e->d_pcm_b[0], frames)) || (rc = make_dev(e->d_pcm_b[1], frames)) ||
      (rc = make_dev(e->d_ratio_b[0], T * B)) || (rc = make_dev(e->d_vad, T * B)) ||
      (rc = make_win_out(e, e->wout0)) || (rc = make_dev(e->d_ticks_b[0], 2 * B)) ||
      (c.want_denoised && (rc = make_dev(e->d_den, frames))) || (rc = make_event(e->ev_in_free[0])) ||
      (rc = make_event(e->ev_in_free[1])))
    return rc;
  if (c.want_spectrum) {
    e->n_spec = c.spec_hi - c.spec_lo + 1;
    if ((rc = make_dev(e->d_spec, T * B * e->wpt * C * (size_t)e->n_spec))) return rc;
  }
  e->d_pcm = e->d_pcm_b[0].get();
  e->d_ratio = e->d_ratio_b[0].get();
  e->d_ticks = e->d_ticks_b[0].get();
  use_win_out(e, 0);
  return FVAD_OK;
}

// The staged pipeline's own: the prep stream, eng::Staged, and buffer 1 of
// ratio / ticks
int staged_make(fvad_engine *e) {
  const fvad_engine_config &c = e->cfg;
  const size_t B = c.n_streams, C = c.n_channels, T = c.max_ticks;
  int rc;
  fvad::stream_ptr prep;
  if ((rc = fvad::make_stream(prep))) return rc;
  e->pstream_ref = std::move(prep);
  e->pstream = e->pstream_ref.get();
  e->sg.reset(new Staged());
  Staged &g = *e->sg;
  g.V = (int)(T * C);
  g.L = (fvad::kPitchBuf - fvad::kFrame) + g.V * fvad::kFrame;
  g.LX = g.L / 2;
  g.wmax = (int)(T * fvad::kFrame / c.fft_size) + 2;
  const size_t F = B * g.V, W = B * g.wmax;
  const size_t ptile = (B + fvad::ptile::kTile - 1) / fvad::ptile::kTile * g.V * fvad::ptile::kTile * fvad::ptile::kRows;
  for (fvad::event_ptr *ev : {&g.ev_prep_done[0], &g.ev_prep_done[1], &g.ev_buf_free[0], &g.ev_buf_free[1], &g.ev_fft_a,
                              &g.ev_synth})
    if ((rc = make_event(*ev))) return rc;
  const size_t FB = F * fvad::kBands;
  const struct {
    fvad::dev_ptr<float> &p;
    size_t n;
  } floats[] = {{g.d_xs_b[0], B * g.L},  {g.d_xs_b[1], B * g.L},  {g.d_xlp_b[0], B * g.LX}, {g.d_xlp_b[1], B * g.LX},
                {e->d_ratio_b[1], T * B}, {g.d_X, F * fvad::kFreq * 2}, {g.d_P, F * fvad::kFreq * 2},
                {g.d_Ex, FB}, {g.d_Ep, FB}, {g.d_Exp, FB}, {g.d_Lyf, FB}, {g.d_gr, FB}, {g.d_gs, FB},
                {g.d_f34, F * 8}, {g.d_rec, F * fvad::kPitchRecord}, {g.d_ptile, ptile}, {g.d_vadf, F},
                {g.d_ys, F * fvad::kWin}};
  for (const auto &f : floats)
    if ((rc = make_dev(f.p, f.n))) return rc;
  if ((rc = make_dev(e->d_ticks_b[1], 2 * B)) || (rc = make_dev(g.d_work, (size_t)fvad::kWorkCounters)) ||
      (rc = make_dev(g.d_sil, F)) || (rc = make_dev(g.d_pitch, F)) || (rc = make_dev(g.d_wtick, W)) ||
      (rc = make_dev(g.d_wstart, W)))
    return rc;
  g.d_xs = g.d_xs_b[0].get();
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, c.device) != hipSuccess) return fail(FVAD_EDEVICE, "device query failed");
  // CUs; persistent grids are sized per kernel
  g.grid_frames = prop.multiProcessorCount;
  // k_fftb's device scratch when a transform does not fit in LDS: a slice per
  // workgroup, at most two per CU and 1 GiB
  int lo = 0, hi = 0, band_lo[fvad::kMaxBandCfg], band_hi[fvad::kMaxBandCfg];
  fill_bands(c, band_lo, band_hi, &lo, &hi);
  g.fb_work_stride = fvad::fftb_work_stride(c.fft_size, lo, hi, fvad::fftb_generic(c.fft_size / 2));
  if (g.fb_work_stride > 0) {
    const long long per = g.fb_work_stride * (long long)sizeof(float2);
    g.fb_work_blocks = (int)std::max<long long>(1, std::min<long long>({(long long)W, 2LL * g.grid_frames, (1LL << 30) / per}));
    if ((rc = make_dev(g.d_fbwork, (size_t)g.fb_work_blocks * g.fb_work_stride))) return rc;
  }
  return FVAD_OK;
}

}  // namespace

extern "C" int fvad_engine_create(const fvad_engine_config *cfg, const fvad_model *model, fvad_engine **out) {
  if (!cfg || !model || !out) return fail(FVAD_EINVAL, "null argument");
  const fvad_engine_config &c = *cfg;
  Rates rates;
  if (const int rc = check_config(c, rates)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(FVAD_EDEVICE, "no HIP device available");
  if (c.device < 0 || c.device >= ndev) return fail(FVAD_EDEVICE, "device ordinal out of range");
  if (hipSetDevice(c.device) != hipSuccess) return fail(FVAD_EDEVICE, "hipSetDevice failed");

  std::unique_ptr<fvad_engine> e(new fvad_engine());  // (a failed step releases everything made so far)
  e->cfg = c;
  if (!rates.in) e->cfg.input_rate = 0;
  if (!rates.out) e->cfg.denoised_rate = 0;
  const bool staged = c.mode != FVAD_MODE_FUSED;
  const size_t frames = (size_t)c.max_ticks * c.n_streams * c.n_channels * fvad::kFrame;
  int rc;
  if ((rc = fvad::make_stream(e->stream)) || (rc = make_kernel_table(e.get())) ||
      (rc = make_plan_and_tables(e.get(), model)) || (rc = make_common(e.get())) ||
      (rc = staged ? staged_make(e.get()) : make_dev(e->d_xbuf, frames)) ||
      (rates.in && (rc = resample_make(e.get(), rates.in_d, c.input_rate_max))) ||
      (rates.out && (rc = resample_out_make(e.get(), rates.out_d, c.denoised_rate_max))) ||
      (rc = fvad_engine_reset(e.get())))
    return rc;
  *out = e.release();
  return FVAD_OK;
}

extern "C" void fvad_engine_destroy(fvad_engine *e) {
  if (!e) return;
  (void)hipSetDevice(e->cfg.device);
  if (e->cstream) (void)hipStreamSynchronize(e->cstream.get());
  if (e->pstream) (void)hipStreamSynchronize(e->pstream);
  e->vadm.pend = false;  // the last push's machine would only update state that is freed
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
