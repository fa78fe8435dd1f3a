// The VADMachine's host side (fvad_machine.h):
//   the derivation            (VADMachine.zig:75-100, FFT.freqToBin)
//   RollingAverage            (structures/RollingAverage.zig:1-56)
//   VADMachine                (AudioPipeline/VADMachine.zig:18-310)
// The host machine is the plain restatement the device's lazy walk is tested
// against: every average is recomputed in f64 over the whole buffer in array
// order at every push.  It shares with the device only the derivation.
#include "fvad_machine.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

// RollingAverage(count, init) initial state (RollingAverage.zig:16-32)
double initial_avg(size_t n, double init) {
  double a = 0.0;
  const double scalar = 1.0 / (double)n;
  for (size_t i = 0; i < n; i++) a += init * scalar;
  return a;
}

}  // namespace

fvad::VadmDerived fvad::vadm_derive(const fvad_vadm_config &c, int sample_rate, int fft_size) {
  const float sr = (float)sample_rate;
  const float eval_per_sec = sr / (float)fft_size;
  auto len_of = [&](float sec) { return (int)std::max<size_t>(1, (size_t)(eval_per_sec * sec)); };
  // Zig @round: half away from zero
  auto freq_to_bin = [&](float f) { return (int)std::round(f / (sr / (float)fft_size)); };
  VadmDerived d{};
  d.lo = freq_to_bin(c.speech_min_freq);
  d.hi = freq_to_bin(c.speech_max_freq);
  VadmConst &K = d.K;
  K.n_lt = len_of(c.long_term_speech_avg_sec);
  K.n_st = len_of(c.short_term_speech_avg_sec);
  K.n_r = len_of(c.channel_vol_ratio_avg_sec);
  K.slot = -1;
  K.lt_pitch = (K.n_lt + 3) & ~3;  // 16-byte rows
  K.min_open = (unsigned long long)(size_t)(sr * c.min_consecutive_sec_to_open);
  K.max_gap = (unsigned long long)(size_t)(sr * c.max_speech_gap_sec);
  K.rec_pad = (unsigned long long)(sr * 2);
  K.thr_factor = c.speech_threshold_factor;
  K.ratio_thr = c.channel_vol_ratio_threshold;
  K.min_dur = c.min_vad_duration_sec;
  K.sr = sr;
  K.has_init = c.has_initial_long_term_avg != 0;
  K.init = c.initial_long_term_avg;
  if (K.has_init) {
    // RollingAverage(initial_avg): data = init (a double, VADMachine.zig:89-94)
    d.s0.lt_count = (unsigned)K.n_lt;
    d.s0.lt_last = initial_avg((size_t)K.n_lt, K.init);
    d.s0.lt_has = 1;
    d.s0.lt_pre_ok = 1;  // next write is at 0: the next pass starts from 0.0
    d.s0.lt_pre = 0.0;
  }
  return d;
}

fvad::VadmRow fvad::vadm_row(const VadmDerived &d, int slot) {
  const VadmConst &K = d.K;
  VadmRow r{};
  r.n_lt = K.n_lt;
  r.n_st = K.n_st;
  r.n_r = K.n_r;
  r.slot = slot;
  r.min_open = K.min_open;
  r.max_gap = K.max_gap;
  r.rec_pad = K.rec_pad;
  r.init = K.init;
  r.thr_factor = K.thr_factor;
  r.ratio_thr = K.ratio_thr;
  r.min_dur = K.min_dur;
  r.sr = K.sr;
  r.lt0 = d.s0.lt_last;
  r.has_init = K.has_init;
  return r;
}

extern "C" int fvad_vadm_lengths(const fvad_vadm_config *cfg, int sample_rate, int fft_size, int out[3]) {
  if (!cfg || !out || sample_rate <= 0 || fft_size <= 0) return FVAD_EINVAL;
  const fvad::VadmConst K = fvad::vadm_derive(*cfg, sample_rate, fft_size).K;
  out[0] = K.n_lt;
  out[1] = K.n_st;
  out[2] = K.n_r;
  return FVAD_OK;
}

int fvad::band_slot(const int *band_lo, const int *band_hi, int n_bands, int lo, int hi) {
  int slot = -1;
  for (int b = 0; b < n_bands; b++)
    if (band_lo[b] == lo && band_hi[b] == hi) slot = b;
  return slot;
}

void fvad::vadm_snapshot_of(const VadmState &st, fvad_vadm_snapshot *out) {
  std::memset(out, 0, sizeof(*out));
  out->speech_state = st.state;
  out->speech_start = st.speech_start;
  out->speech_end = st.speech_end;
  out->windows = st.windows_done;
  out->avg[0] = st.lt_last;
  out->avg[1] = st.st_last;
  out->avg[2] = st.r_last;
  out->write_idx[0] = st.lt_widx;
  out->write_idx[1] = st.st_widx;
  out->write_idx[2] = st.r_widx;
  out->written[0] = st.lt_count;
  out->written[1] = st.st_count;
  out->written[2] = st.r_count;
  out->speech_rnn_vad = st.rnn_vad;
  out->speech_vol_ratio = st.vol_ratio;
  out->speech_rnn_vad_count = st.rnn_vad_count;
  out->speech_vol_ratio_count = st.vol_ratio_count;
  out->n_segments = st.n_segs;
}

namespace {

// ---------------- RollingAverage ----------------
struct RollingAverage {
  std::vector<double> data;
  bool has_last = false;
  double last_avg = 0;
  size_t write_idx = 0, written_count = 0;
  RollingAverage(size_t count, bool has_init, double init) : data(count, 0.0) {
    if (has_init) {
      for (size_t i = 0; i < count; i++) data[i] = init;
      written_count = count;
      avg();
    }
  }
  double avg() {
    double a = 0.0;
    const double scalar = 1.0 / (double)written_count;
    for (size_t i = 0; i < written_count; i++) a += data[i] * scalar;
    last_avg = a;
    has_last = true;
    return a;
  }
  double push(float sample) {
    data[write_idx] = (double)sample;
    write_idx = (write_idx + 1) % data.size();
    if (written_count < data.size()) written_count++;
    return avg();
  }
};

// ---------------- VADMachine ----------------
struct VADMachine {
  enum State { kClosed, kOpening, kOpen, kClosing };
  fvad_vadm_config cfg;
  fvad::VadmDerived d;  // lengths, bins, thresholds in samples
  State state = kClosed;
  RollingAverage long_term, short_term, ratio;
  uint64_t speech_start = 0, speech_end = 0;
  float rnn_vad = 0;
  size_t rnn_vad_count = 0;
  float vol_ratio = 0;
  size_t vol_ratio_count = 0;
  std::vector<fvad_segment> segments;

  VADMachine(const fvad_vadm_config &c, int sr, int fft)
      : cfg(c),
        d(fvad::vadm_derive(c, sr, fft)),
        long_term((size_t)d.K.n_lt, c.has_initial_long_term_avg != 0, c.initial_long_term_avg),
        short_term((size_t)d.K.n_st, false, 0),
        ratio((size_t)d.K.n_r, false, 0) {
    segments.reserve(100);
  }
  uint64_t rec_start(uint64_t from) const {
    const uint64_t sb = d.K.rec_pad;
    return sb > from ? 0 : from - sb;
  }
  uint64_t rec_end(uint64_t to) const { return to + d.K.rec_pad; }
  void track(float vad, float vr, State from, State to) {
    if (from == kClosed && to == kOpening) {
      rnn_vad = vad;
      rnn_vad_count = 1;
      vol_ratio = vr;
      vol_ratio_count = 1;
    } else if (from == kOpening || from == kOpen) {
      rnn_vad += vad;
      rnn_vad_count += 1;
      vol_ratio += vr;
      vol_ratio_count += 1;
    }
  }
  void on_speech_end() {
    const uint64_t len = speech_end - speech_start;
    const float len_rt = (float)len / d.K.sr;
    if (len_rt >= cfg.min_vad_duration_sec) {
      fvad_segment s;
      s.sample_from = rec_start(speech_start);
      s.sample_to = rec_end(speech_end);
      s.debug_rnn_vad = rnn_vad / (float)rnn_vad_count;
      s.debug_avg_speech_vol_ratio = vol_ratio / (float)vol_ratio_count;
      segments.push_back(s);
    }
  }
  // VADMachine.run: channel band sums of this window, window vad (has_vad) and ratio
  void run(uint64_t index, const float *band_per_channel, int n_ch, int band_stride, float vad, float vr) {
    float min_v = 999, max_v = 0;
    for (int c = 0; c < n_ch; c++) {
      const float v = band_per_channel[c * band_stride];
      if (v < min_v) min_v = v;
      if (v > max_v) max_v = v;
    }
    const size_t min_open = (size_t)d.K.min_open;
    const size_t max_gap = (size_t)d.K.max_gap;
    const double st_avg = short_term.push(min_v);
    const double r_avg = ratio.push(vr);
    double base;
    if (long_term.has_last)
      base = long_term.last_avg;
    else if (cfg.has_initial_long_term_avg)
      base = cfg.initial_long_term_avg;
    else
      base = st_avg;
    const double threshold = base * (double)cfg.speech_threshold_factor;
    const bool met = st_avg > threshold && r_avg > (double)cfg.channel_vol_ratio_threshold;
    if (!met) long_term.push(min_v);
    switch (state) {
      case kClosed:
        if (met) {
          state = kOpening;
          speech_start = index;
        }
        track(vad, vr, kClosed, state);
        break;
      case kOpening:
        if (met && index - speech_start >= min_open)
          state = kOpen;
        else if (!met)
          state = kClosed;
        track(vad, vr, kOpening, state);
        break;
      case kOpen:
        if (!met) {
          state = kClosing;
          speech_end = index;
        }
        track(vad, vr, kOpen, state);
        break;
      case kClosing:
        if (met)
          state = kOpen;
        else if (index - speech_end >= max_gap) {
          state = kClosed;
          on_speech_end();
        }
        track(vad, vr, kClosing, state);
        break;
    }
  }
};

}  // namespace

extern "C" void fvad_vadm_config_default(fvad_vadm_config *c) {
  c->speech_min_freq = 100;
  c->speech_max_freq = 1500;
  c->long_term_speech_avg_sec = 180;
  c->has_initial_long_term_avg = 1;
  c->initial_long_term_avg = 0.005;
  c->short_term_speech_avg_sec = 0.2f;
  c->speech_threshold_factor = 18;
  c->channel_vol_ratio_avg_sec = 0.5f;
  c->channel_vol_ratio_threshold = 0.5f;
  c->min_consecutive_sec_to_open = 0.2f;
  c->max_speech_gap_sec = 2;
  c->min_vad_duration_sec = 0.7f;
}

// The sweep's host path (fvad_sweep.cpp): one fresh machine over a recorded
// window sequence, its final state in the device snapshot's terms.
void fvad::host_vadm_lane(const fvad_vadm_config &c, int sample_rate, int fft_size, int n_channels, int n_bands,
                          int slot, size_t n_windows, const float *band, const float *vad, const float *vol_ratio,
                          fvad_vadm_snapshot *snap, std::vector<fvad_segment> *segs) {
  VADMachine m(c, sample_rate, fft_size);
  for (size_t w = 0; w < n_windows; w++)
    m.run((uint64_t)w * (uint64_t)fft_size, band + w * (size_t)n_channels * n_bands + slot, n_channels, n_bands,
          vad[w], vol_ratio[w]);
  if (snap) {
    std::memset(snap, 0, sizeof(*snap));
    snap->speech_state = (int)m.state;
    snap->speech_start = m.speech_start;
    snap->speech_end = m.speech_end;
    snap->windows = n_windows;
    const RollingAverage *ra[3] = {&m.long_term, &m.short_term, &m.ratio};
    for (int k = 0; k < 3; k++) {
      snap->avg[k] = ra[k]->last_avg;
      snap->write_idx[k] = ra[k]->write_idx;
      snap->written[k] = ra[k]->written_count;
    }
    snap->speech_rnn_vad = m.rnn_vad;
    snap->speech_vol_ratio = m.vol_ratio;
    snap->speech_rnn_vad_count = m.rnn_vad_count;
    snap->speech_vol_ratio_count = m.vol_ratio_count;
    snap->n_segments = m.segments.size();
  }
  if (segs) *segs = std::move(m.segments);
}

// ---------------------------------------------------------------------------
// Standalone VADMachine (host decision logic; testable without a GPU)
// ---------------------------------------------------------------------------
struct fvad_vadm {
  VADMachine m;
  int n_channels;
  fvad_vadm(const fvad_vadm_config &c, int sr, int fft, int ch) : m(c, sr, fft), n_channels(ch) {}
};

extern "C" int fvad_vadm_create(const fvad_vadm_config *cfg, int sample_rate, int fft_size, int n_channels,
                                fvad_vadm **out) {
  if (!out || n_channels < 1 || fft_size <= 0 || sample_rate <= 0) return FVAD_EINVAL;
  fvad_vadm_config def;
  fvad_vadm_config_default(&def);
  *out = new fvad_vadm(cfg ? *cfg : def, sample_rate, fft_size, n_channels);
  return FVAD_OK;
}

extern "C" void fvad_vadm_destroy(fvad_vadm *v) { delete v; }

extern "C" void fvad_vadm_bins(const fvad_vadm *v, int *lo, int *hi) {
  if (lo) *lo = v->m.d.lo;
  if (hi) *hi = v->m.d.hi;
}

extern "C" int fvad_vadm_run(fvad_vadm *v, uint64_t index, const float *band_per_channel, float vad,
                             float vol_ratio) {
  if (!v || !band_per_channel) return FVAD_EINVAL;
  v->m.run(index, band_per_channel, v->n_channels, 1, vad, vol_ratio);
  return FVAD_OK;
}

extern "C" size_t fvad_vadm_segments(const fvad_vadm *v, fvad_segment *out, size_t cap) {
  const auto &segs = v->m.segments;
  for (size_t i = 0; i < segs.size() && i < cap; i++) out[i] = segs[i];
  return segs.size();
}

extern "C" int fvad_vadm_state(const fvad_vadm *v, int *speech_state, uint64_t *speech_start, uint64_t *speech_end) {
  if (!v) return FVAD_EINVAL;
  if (speech_state) *speech_state = (int)v->m.state;
  if (speech_start) *speech_start = v->m.speech_start;
  if (speech_end) *speech_end = v->m.speech_end;
  return FVAD_OK;
}
