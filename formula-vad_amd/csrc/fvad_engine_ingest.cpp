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
      if (last[s] != (e->rs->plan.on() ? e->rs->plan.frame(s) : e->rs->d.n))
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
      const int b = e->sg->next_buf;
      if (e->sg->buf_busy[b]) HIP_TRY(hipStreamWaitEvent(cs, e->sg->ev_buf_free[b].get(), 0));
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
