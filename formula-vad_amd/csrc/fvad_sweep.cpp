// Config sweep (include/fvad.h: fvad_sweep_*): the recorded windows, the
// validation, the device run in chunks (k_vadm_sweep, fvad_sweep.hip; with
// fvad_sweep_run_score each chunk's k_sweep_score behind it,
// fvad_sweep_score.hip), the host run (the host VADMachine, fvad_host.cpp) and
// the scores (fvad_sweep_score: the host evaluator; fvad_sweep_run_score: the
// shared core, fvad_eval_core.h).  Everything but fvad_sweep_run and
// fvad_sweep_run_score on a device sweep is host code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/fvad.h"
#include "fvad_eval_core.h"
#include "fvad_hip_own.h"
#include "fvad_internal.h"
#include "fvad_sweep.h"

using fvad::set_error;

#define HIP_TRY(expr)                                                                                          \
  do {                                                                                                         \
    hipError_t e_ = (expr);                                                                                    \
    if (e_ != hipSuccess) return set_error(FVAD_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

namespace {
constexpr size_t kSweepBudget = (size_t)4 << 30;  // device bytes of one chunk's machines

struct Windows {  // one stream's recorded sequence
  std::vector<float> band, vad, vr;
  size_t n() const { return vr.size(); }
};
struct Lane {  // results of (stream, config)
  fvad_vadm_snapshot snap{};
  std::vector<fvad_segment> segs;  // the first min(total, seg_capacity)
};
struct DevBuf {  // device bytes, grown on demand (ensure)
  fvad::dev_ptr<char> p;
  size_t cap = 0;
};
struct Score {  // one fvad_sweep_run_score call: what the lanes are scored against, and their scores
  std::vector<float> lab;      // every stream's (from, to), each stream's stably sorted by start
  std::vector<long long> off;  // [n_streams + 1] first label of a stream
  const fvad_stat_config *stat = nullptr;
  size_t n_stat = 0;  // 1 or n_cfgs
  std::vector<fvad_single_stats> single;  // [stream][cfg]
  std::vector<unsigned> status;           // [stream][cfg] fvad::kEval*
};
}  // namespace

struct fvad_sweep {
  fvad_sweep_config cfg{};
  std::vector<Windows> win;
  bool dirty = true;  // the device copy of the windows is stale
  size_t n_cfgs = 0;
  std::vector<Lane> lanes;  // [stream][cfg]
  bool kept = true;         // the last run kept its segments (fvad_sweep_run_score does not)
  size_t bytes_back = 0;    // device-to-host bytes of the last run
  bool have_counts = false;
  unsigned long long counts[fvad::kVadmCounts] = {};
  // test hooks
  double bound_scale = 1.0;
  unsigned defer_max = 0;
  size_t chunk = 0;
  bool count_on = false;
  // device (the stream first: it is destroyed after the buffers)
  fvad::stream_ptr stream;
  DevBuf d_band, d_wmin, d_wvad, d_wvr, d_off, d_nwin, d_K, d_st, d_lt, d_sbuf, d_rbuf, d_seg, d_count;
  DevBuf d_lab, d_lab_off, d_stat, d_single, d_status;  // fvad_sweep_run_score
  long long n_windows = 0;
};

namespace {
int ensure(DevBuf &b, size_t bytes) {
  if (bytes <= b.cap) return FVAD_OK;
  b.p.reset();
  b.cap = 0;
  if (const int rc = fvad::make_dev(b.p, std::max<size_t>(bytes, 256))) return rc;
  b.cap = std::max<size_t>(bytes, 256);
  return FVAD_OK;
}

int check_config(const fvad_sweep_config &c) {
  if (c.sample_rate != 48000) return set_error(FVAD_ERATE, "only 48 kHz is supported (VAD.zig:101-104)");
  if (c.n_streams < 1 || c.n_streams > 65535 || c.n_channels < 1 || c.n_channels > FVAD_MAX_CHANNELS)
    return set_error(FVAD_EINVAL, "1 <= n_streams <= 65535 and 1 <= n_channels <= 8 required");
  if (c.fft_size < 2 || c.fft_size > fvad::kMaxFftSize || (c.fft_size & 1))
    return set_error(FVAD_EINVAL, "fft_size must be even, 2 <= fft_size <= 4194304 (FFT.zig:29-31)");
  if (c.n_bands < 1 || c.n_bands > FVAD_MAX_BANDS) return set_error(FVAD_EINVAL, "1 <= n_bands <= 4");
  for (int b = 0; b < c.n_bands; b++)
    if (c.band_lo[b] < 0 || c.band_hi[b] < c.band_lo[b] || c.band_hi[b] > c.fft_size / 2)
      return set_error(FVAD_EINVAL, "invalid band range");
  if (c.seg_capacity < 1) return set_error(FVAD_EINVAL, "seg_capacity must be >= 1");
  return FVAD_OK;
}

// every config's constants, initial state and band slot; FVAD_EINVAL naming
// the first config whose speech band is none of the sweep's
int prepare(const fvad_sweep_config &c, const fvad_vadm_config *cfgs, size_t n, std::vector<fvad::VadmConst> *K,
            std::vector<fvad::VadmState> *s0) {
  K->resize(n);
  s0->resize(n);
  for (size_t m = 0; m < n; m++) {
    int lo, hi;
    fvad::vadm_fill_const(cfgs[m], c.sample_rate, c.fft_size, &(*K)[m], &(*s0)[m], &lo, &hi);
    int slot = -1;
    for (int b = 0; b < c.n_bands; b++)
      if (c.band_lo[b] == lo && c.band_hi[b] == hi) slot = b;
    if (slot < 0)
      return set_error(FVAD_EINVAL, "config " + std::to_string(m) + ": its speech band (bins " + std::to_string(lo) +
                                        ".." + std::to_string(hi) + ") is none of the sweep's bands");
    (*K)[m].slot = slot;
    (*K)[m].lt_pitch = ((*K)[m].n_lt + 3) & ~3;  // 16-byte rows
  }
  return FVAD_OK;
}

// device bytes of the machines of configs [c0, c1) over B streams
size_t chunk_bytes(const fvad_sweep_config &c, const std::vector<fvad::VadmConst> &K, size_t c0, size_t c1) {
  const size_t B = (size_t)c.n_streams, lanes = B * (c1 - c0);
  size_t lt = 0, max_st = 0, max_r = 0;
  for (size_t m = c0; m < c1; m++) {
    lt += (size_t)K[m].lt_pitch * B;
    max_st = std::max(max_st, (size_t)K[m].n_st);
    max_r = std::max(max_r, (size_t)K[m].n_r);
  }
  return (lt + (max_st + max_r) * lanes) * sizeof(float) + lanes * sizeof(fvad::VadmState) +
         lanes * (size_t)c.seg_capacity * sizeof(fvad::VadmSeg) + (c1 - c0) * sizeof(fvad::VadmConst);
}

int check_run(const fvad_sweep *sw, const fvad_vadm_config *cfgs, size_t n_cfgs) {
  if (!sw || !cfgs || n_cfgs < 1) return set_error(FVAD_EINVAL, "invalid argument");
  if (n_cfgs > ((size_t)1 << 24)) return set_error(FVAD_EINVAL, "n_cfgs above 2^24");
  return FVAD_OK;
}

int upload_windows(fvad_sweep *sw) {
  const fvad_sweep_config &c = sw->cfg;
  const size_t B = (size_t)c.n_streams, per = (size_t)c.n_channels * c.n_bands;
  std::vector<long long> off(B);
  std::vector<int> nwin(B);
  size_t total = 0;
  for (size_t s = 0; s < B; s++) {
    off[s] = (long long)total;
    nwin[s] = (int)sw->win[s].n();
    total += sw->win[s].n();
  }
  std::vector<float> band(total * per), vad(total), vr(total);
  for (size_t s = 0; s < B; s++) {
    const Windows &w = sw->win[s];
    std::copy(w.band.begin(), w.band.end(), band.begin() + (size_t)off[s] * per);
    std::copy(w.vad.begin(), w.vad.end(), vad.begin() + off[s]);
    std::copy(w.vr.begin(), w.vr.end(), vr.begin() + off[s]);
  }
  int rc;
  if ((rc = ensure(sw->d_band, band.size() * sizeof(float))) || (rc = ensure(sw->d_wvad, total * sizeof(float))) ||
      (rc = ensure(sw->d_wvr, total * sizeof(float))) ||
      (rc = ensure(sw->d_wmin, total * c.n_bands * sizeof(float))) || (rc = ensure(sw->d_off, B * sizeof(long long))) ||
      (rc = ensure(sw->d_nwin, B * sizeof(int))))
    return rc;
  if (total) {
    HIP_TRY(hipMemcpy(sw->d_band.p.get(), band.data(), band.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(sw->d_wvad.p.get(), vad.data(), total * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(sw->d_wvr.p.get(), vr.data(), total * sizeof(float), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(sw->d_off.p.get(), off.data(), B * sizeof(long long), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(sw->d_nwin.p.get(), nwin.data(), B * sizeof(int), hipMemcpyHostToDevice));
  sw->n_windows = (long long)total;
  fvad::SweepArgs a{};
  a.n_channels = c.n_channels;
  a.n_bands = c.n_bands;
  a.n_windows = sw->n_windows;
  a.band = reinterpret_cast<const float *>(sw->d_band.p.get());
  a.wmin = reinterpret_cast<float *>(sw->d_wmin.p.get());
  HIP_TRY(fvad::launch_sweep_min(a, sw->stream.get()));
  HIP_TRY(hipStreamSynchronize(sw->stream.get()));
  sw->dirty = false;
  return FVAD_OK;
}

void lane_from_device(const fvad::VadmState &st, const fvad::VadmSeg *seg, int seg_cap, Lane *l) {
  fvad::vadm_snapshot_of(st, &l->snap);
  const size_t k = std::min<size_t>(st.n_segs, (size_t)seg_cap);
  l->segs.resize(k);
  for (size_t i = 0; i < k; i++) {
    l->segs[i].sample_from = seg[i].sample_from;
    l->segs[i].sample_to = seg[i].sample_to;
    l->segs[i].debug_rnn_vad = seg[i].debug_rnn_vad;
    l->segs[i].debug_avg_speech_vol_ratio = seg[i].debug_avg_speech_vol_ratio;
  }
}

// sc: null (the segments come back), or the lanes are scored on the device and
// their statistics and status words come back instead
int run_device(fvad_sweep *sw, std::vector<fvad::VadmConst> &K, const std::vector<fvad::VadmState> &s0, Score *sc) {
  const fvad_sweep_config &c = sw->cfg;
  const size_t B = (size_t)c.n_streams, n = K.size();
  HIP_TRY(hipSetDevice(c.device));
  if (sw->dirty)
    if (const int rc = upload_windows(sw)) return rc;
  int rc;
  if (sw->count_on) {
    if ((rc = ensure(sw->d_count, fvad::kVadmCounts * sizeof(unsigned long long)))) return rc;
    HIP_TRY(hipMemsetAsync(sw->d_count.p.get(), 0, fvad::kVadmCounts * sizeof(unsigned long long), sw->stream.get()));
  }
  if (sc) {  // the labels and the stat configs, once per call
    if ((rc = ensure(sw->d_lab, sc->lab.size() * sizeof(float))) ||
        (rc = ensure(sw->d_lab_off, sc->off.size() * sizeof(long long))) ||
        (rc = ensure(sw->d_stat, sc->n_stat * sizeof(fvad_stat_config))))
      return rc;
    const auto up = [&](DevBuf &d, const void *src, size_t bytes) {
      return bytes ? hipMemcpyAsync(d.p.get(), src, bytes, hipMemcpyHostToDevice, sw->stream.get()) : hipSuccess;
    };
    HIP_TRY(up(sw->d_lab, sc->lab.data(), sc->lab.size() * sizeof(float)));
    HIP_TRY(up(sw->d_lab_off, sc->off.data(), sc->off.size() * sizeof(long long)));
    HIP_TRY(up(sw->d_stat, sc->stat, sc->n_stat * sizeof(fvad_stat_config)));
  }
  std::vector<Lane> lanes(B * n);
  std::vector<fvad::VadmState> st;
  std::vector<fvad::VadmSeg> seg;
  std::vector<fvad_single_stats> single;
  std::vector<unsigned> status;
  size_t bytes_back = 0;
  for (size_t c0 = 0; c0 < n;) {
    // the chunk: configs [c0, c1), by the test hook or as many as the budget holds (one at least)
    size_t c1 = c0 + 1;
    if (sw->chunk)
      c1 = std::min(n, c0 + sw->chunk);
    else
      while (c1 < n && chunk_bytes(c, K, c0, c1 + 1) <= kSweepBudget) c1++;
    const size_t nc = c1 - c0, nl = B * nc;
    size_t lt = 0, max_st = 0, max_r = 0;
    for (size_t m = c0; m < c1; m++) {
      K[m].lt_off = (long long)lt;
      lt += (size_t)K[m].lt_pitch * B;
      max_st = std::max(max_st, (size_t)K[m].n_st);
      max_r = std::max(max_r, (size_t)K[m].n_r);
    }
    if ((rc = ensure(sw->d_K, nc * sizeof(fvad::VadmConst))) || (rc = ensure(sw->d_st, nl * sizeof(fvad::VadmState))) ||
        (rc = ensure(sw->d_lt, lt * sizeof(float))) || (rc = ensure(sw->d_sbuf, max_st * nl * sizeof(float))) ||
        (rc = ensure(sw->d_rbuf, max_r * nl * sizeof(float))) ||
        (rc = ensure(sw->d_seg, nl * (size_t)c.seg_capacity * sizeof(fvad::VadmSeg))))
      return rc;
    if (sc && ((rc = ensure(sw->d_single, nl * sizeof(fvad_single_stats))) ||
               (rc = ensure(sw->d_status, nl * sizeof(unsigned)))))
      return rc;
    st.resize(nl);
    for (size_t s = 0; s < B; s++)
      for (size_t m = 0; m < nc; m++) st[s * nc + m] = s0[c0 + m];
    HIP_TRY(hipMemcpyAsync(sw->d_K.p.get(), K.data() + c0, nc * sizeof(fvad::VadmConst), hipMemcpyHostToDevice, sw->stream.get()));
    HIP_TRY(hipMemcpyAsync(sw->d_st.p.get(), st.data(), nl * sizeof(fvad::VadmState), hipMemcpyHostToDevice, sw->stream.get()));
    // entries never pushed are never read (lt_nw, the counts); zeroed all the same
    HIP_TRY(hipMemsetAsync(sw->d_lt.p.get(), 0, lt * sizeof(float), sw->stream.get()));
    HIP_TRY(hipMemsetAsync(sw->d_sbuf.p.get(), 0, max_st * nl * sizeof(float), sw->stream.get()));
    HIP_TRY(hipMemsetAsync(sw->d_rbuf.p.get(), 0, max_r * nl * sizeof(float), sw->stream.get()));
    fvad::SweepArgs a{};
    a.n_streams = c.n_streams;
    a.n_cfgs = (int)nc;
    a.n_channels = c.n_channels;
    a.n_bands = c.n_bands;
    a.seg_cap = c.seg_capacity;
    a.K = reinterpret_cast<const fvad::VadmConst *>(sw->d_K.p.get());
    a.st = reinterpret_cast<fvad::VadmState *>(sw->d_st.p.get());
    a.lt = reinterpret_cast<float *>(sw->d_lt.p.get());
    a.sbuf = reinterpret_cast<float *>(sw->d_sbuf.p.get());
    a.rbuf = reinterpret_cast<float *>(sw->d_rbuf.p.get());
    a.seg = reinterpret_cast<fvad::VadmSeg *>(sw->d_seg.p.get());
    a.win_off = reinterpret_cast<const long long *>(sw->d_off.p.get());
    a.n_win = reinterpret_cast<const int *>(sw->d_nwin.p.get());
    a.band = reinterpret_cast<const float *>(sw->d_band.p.get());
    a.wmin = reinterpret_cast<float *>(sw->d_wmin.p.get());
    a.wvad = reinterpret_cast<const float *>(sw->d_wvad.p.get());
    a.wvr = reinterpret_cast<const float *>(sw->d_wvr.p.get());
    a.n_windows = sw->n_windows;
    a.fft = (unsigned long long)c.fft_size;
    a.bound_scale = sw->bound_scale;
    a.defer_max = sw->defer_max;
    a.count = sw->count_on ? reinterpret_cast<unsigned long long *>(sw->d_count.p.get()) : nullptr;
    HIP_TRY(fvad::launch_vadm_sweep(a, sw->stream.get()));
    if (sc) {
      fvad::ScoreArgs b{};
      b.n_streams = c.n_streams;
      b.n_cfgs = (int)nc;
      b.seg_cap = c.seg_capacity;
      b.st = a.st;
      b.seg = a.seg;
      b.lab = reinterpret_cast<const float *>(sw->d_lab.p.get());
      b.lab_off = reinterpret_cast<const long long *>(sw->d_lab_off.p.get());
      b.stat_stride = sc->n_stat == 1 ? 0 : 1;
      b.stat = reinterpret_cast<const fvad_stat_config *>(sw->d_stat.p.get()) + c0 * (size_t)b.stat_stride;
      b.single = reinterpret_cast<fvad_single_stats *>(sw->d_single.p.get());
      b.status = reinterpret_cast<unsigned *>(sw->d_status.p.get());
      HIP_TRY(fvad::launch_sweep_score(b, sw->stream.get()));
    }
    HIP_TRY(hipStreamSynchronize(sw->stream.get()));
    HIP_TRY(hipMemcpy(st.data(), sw->d_st.p.get(), nl * sizeof(fvad::VadmState), hipMemcpyDeviceToHost));
    bytes_back += nl * sizeof(fvad::VadmState);
    if (sc) {
      single.resize(nl);
      status.resize(nl);
      HIP_TRY(hipMemcpy(single.data(), sw->d_single.p.get(), nl * sizeof(fvad_single_stats), hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(status.data(), sw->d_status.p.get(), nl * sizeof(unsigned), hipMemcpyDeviceToHost));
      bytes_back += nl * (sizeof(fvad_single_stats) + sizeof(unsigned));
      for (size_t s = 0; s < B; s++)
        for (size_t m = 0; m < nc; m++) {
          fvad::vadm_snapshot_of(st[s * nc + m], &lanes[s * n + c0 + m].snap);
          sc->status[s * n + c0 + m] = status[s * nc + m];
          sc->single[s * n + c0 + m] = single[s * nc + m];
        }
    } else {
      seg.resize(nl * (size_t)c.seg_capacity);
      HIP_TRY(hipMemcpy(seg.data(), sw->d_seg.p.get(), seg.size() * sizeof(fvad::VadmSeg), hipMemcpyDeviceToHost));
      bytes_back += seg.size() * sizeof(fvad::VadmSeg);
      for (size_t s = 0; s < B; s++)
        for (size_t m = 0; m < nc; m++)
          lane_from_device(st[s * nc + m], seg.data() + (s * nc + m) * (size_t)c.seg_capacity, c.seg_capacity,
                           &lanes[s * n + c0 + m]);
    }
    c0 = c1;
  }
  if (sw->count_on)
    HIP_TRY(hipMemcpy(sw->counts, sw->d_count.p.get(), sizeof(sw->counts), hipMemcpyDeviceToHost));
  sw->have_counts = sw->count_on;
  sw->lanes = std::move(lanes);
  sw->n_cfgs = n;
  sw->kept = !sc;
  sw->bytes_back = bytes_back;
  return FVAD_OK;
}

// sc: null (the segments are kept), or each lane is scored by the shared core
// as k_sweep_score does it and keeps no segments
int run_host(fvad_sweep *sw, const fvad_vadm_config *cfgs, const std::vector<fvad::VadmConst> &K, Score *sc) {
  const fvad_sweep_config &c = sw->cfg;
  const size_t B = (size_t)c.n_streams, n = K.size(), nl = B * n;
  std::vector<Lane> lanes(nl);
  auto work = [&](size_t t, size_t nt) {
    for (size_t l = t; l < nl; l += nt) {
      const size_t s = l / n, m = l % n;
      const Windows &w = sw->win[s];
      fvad::host_vadm_lane(cfgs[m], c.sample_rate, c.fft_size, c.n_channels, c.n_bands, K[m].slot, w.n(),
                           w.band.data(), w.vad.data(), w.vr.data(), &lanes[l].snap, &lanes[l].segs);
      if (sc) {
        const std::vector<fvad_segment> &g = lanes[l].segs;
        if (g.size() > (size_t)c.seg_capacity)
          sc->status[l] = fvad::kEvalOverCapacity;
        else
          sc->status[l] = fvad::eval_lane(
              [&](size_t i, float *from, float *to) {
                *from = (float)g[i].sample_from / 48000.0f;
                *to = (float)g[i].sample_to / 48000.0f;
              },
              g.size(), sc->lab.data() + 2 * sc->off[s], (size_t)(sc->off[s + 1] - sc->off[s]),
              sc->stat[sc->n_stat == 1 ? 0 : m], &sc->single[l]);
        lanes[l].segs = {};
      } else if (lanes[l].segs.size() > (size_t)c.seg_capacity) {
        lanes[l].segs.resize((size_t)c.seg_capacity);
      }
    }
  };
  const size_t nt = std::max<size_t>(1, std::min<size_t>({(size_t)16, (size_t)std::thread::hardware_concurrency(), nl}));
  std::vector<std::thread> th;
  for (size_t t = 1; t < nt; t++) th.emplace_back(work, t, nt);
  work(0, nt);
  for (auto &x : th) x.join();
  sw->lanes = std::move(lanes);
  sw->n_cfgs = n;
  sw->have_counts = false;
  sw->kept = !sc;
  sw->bytes_back = 0;
  return FVAD_OK;
}

const Lane *lane_of(const fvad_sweep *sw, int stream, size_t cfg) {
  if (!sw || stream < 0 || stream >= sw->cfg.n_streams || cfg >= sw->n_cfgs) return nullptr;
  return &sw->lanes[(size_t)stream * sw->n_cfgs + cfg];
}
}  // namespace

extern "C" int fvad_sweep_create(const fvad_sweep_config *cfg, fvad_sweep **out) {
  if (!cfg || !out) return set_error(FVAD_EINVAL, "null argument");
  if (const int rc = check_config(*cfg)) return rc;
  fvad::stream_ptr stream;
  if (cfg->device != -1) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
      (void)hipGetLastError();
      return set_error(FVAD_EDEVICE, "no HIP device available (device = -1 makes a host-only sweep)");
    }
    if (cfg->device < 0 || cfg->device >= ndev) return set_error(FVAD_EDEVICE, "device ordinal out of range");
    HIP_TRY(hipSetDevice(cfg->device));
    if (const int rc = fvad::make_stream(stream, hipStreamDefault)) return rc;
  }
  fvad_sweep *sw = new fvad_sweep;
  sw->cfg = *cfg;
  sw->win.resize((size_t)cfg->n_streams);
  sw->stream = std::move(stream);
  *out = sw;
  return FVAD_OK;
}

extern "C" void fvad_sweep_destroy(fvad_sweep *sw) {
  if (!sw) return;
  if (sw->cfg.device != -1) (void)hipSetDevice(sw->cfg.device);
  delete sw;
}

extern "C" int fvad_sweep_set_windows(fvad_sweep *sw, int stream, size_t n_windows, const float *band,
                                      const float *vad, const float *vol_ratio) {
  if (!sw) return set_error(FVAD_EINVAL, "null sweep");
  if (stream < 0 || stream >= sw->cfg.n_streams) return set_error(FVAD_EINVAL, "stream index out of range");
  if (n_windows > 0 && (!band || !vol_ratio)) return set_error(FVAD_EINVAL, "null band or vol_ratio");
  if (n_windows > (size_t)0x7fffffff) return set_error(FVAD_EINVAL, "n_windows above 2^31 - 1");
  Windows &w = sw->win[(size_t)stream];
  const size_t per = (size_t)sw->cfg.n_channels * sw->cfg.n_bands;
  w.band.assign(band, band + n_windows * per);
  w.vr.assign(vol_ratio, vol_ratio + n_windows);
  if (vad && sw->cfg.use_denoiser)
    w.vad.assign(vad, vad + n_windows);
  else
    w.vad.assign(n_windows, 0.0f);  // fft_input.vad orelse 0 (VADMachine.zig:240-246)
  sw->dirty = true;
  return FVAD_OK;
}

extern "C" int fvad_sweep_append_outputs(fvad_sweep *sw, const fvad_outputs *out, int n_ticks,
                                         const int32_t *ticks_valid) {
  if (!sw || !out) return set_error(FVAD_EINVAL, "null argument");
  if (!out->win_flag || !out->win_ratio || !out->win_vad || !out->band)
    return set_error(FVAD_EINVAL, "win_flag, win_ratio, win_vad and band are required");
  if (n_ticks < 0) return set_error(FVAD_EINVAL, "n_ticks < 0");
  const fvad_sweep_config &c = sw->cfg;
  const size_t B = (size_t)c.n_streams, W = (size_t)fvad::windows_per_tick(c.fft_size),
               per = (size_t)c.n_channels * c.n_bands;
  // validate everything first: a bad value leaves the sweep as it was
  for (size_t s = 0; s < B; s++) {
    if (ticks_valid && (ticks_valid[s] < 0 || ticks_valid[s] > n_ticks))
      return set_error(FVAD_EINVAL, "ticks_valid out of range");
    const int nt = ticks_valid ? ticks_valid[s] : n_ticks;
    size_t add = 0;
    for (int t = 0; t < nt; t++) {
      const int32_t f = out->win_flag[(size_t)t * B + s];
      if (f < 0 || (size_t)f > W) return set_error(FVAD_EINVAL, "win_flag out of range [0, windows per tick]");
      add += (size_t)f;
    }
    if (sw->win[s].n() + add > (size_t)0x7fffffff) return set_error(FVAD_EINVAL, "a stream above 2^31 - 1 windows");
  }
  for (size_t s = 0; s < B; s++) {
    Windows &w = sw->win[s];
    const int nt = ticks_valid ? ticks_valid[s] : n_ticks;
    for (int t = 0; t < nt; t++)
      for (int32_t k = 0, f = out->win_flag[(size_t)t * B + s]; k < f; k++) {
        const size_t o = ((size_t)t * B + s) * W + (size_t)k;
        w.band.insert(w.band.end(), out->band + o * per, out->band + (o + 1) * per);
        w.vad.push_back(c.use_denoiser ? out->win_vad[o] : 0.0f);
        w.vr.push_back(out->win_ratio[o]);
      }
  }
  sw->dirty = true;
  return FVAD_OK;
}

extern "C" int fvad_sweep_run_host(fvad_sweep *sw, const fvad_vadm_config *cfgs, size_t n_cfgs) {
  if (const int rc = check_run(sw, cfgs, n_cfgs)) return rc;
  std::vector<fvad::VadmConst> K;
  std::vector<fvad::VadmState> s0;
  if (const int rc = prepare(sw->cfg, cfgs, n_cfgs, &K, &s0)) return rc;
  return run_host(sw, cfgs, K, nullptr);
}

extern "C" int fvad_sweep_run(fvad_sweep *sw, const fvad_vadm_config *cfgs, size_t n_cfgs) {
  if (const int rc = check_run(sw, cfgs, n_cfgs)) return rc;
  std::vector<fvad::VadmConst> K;
  std::vector<fvad::VadmState> s0;
  if (const int rc = prepare(sw->cfg, cfgs, n_cfgs, &K, &s0)) return rc;
  if (sw->cfg.device == -1) return run_host(sw, cfgs, K, nullptr);
  return run_device(sw, K, s0, nullptr);
}

extern "C" int fvad_sweep_run_score(fvad_sweep *sw, const fvad_vadm_config *cfgs, size_t n_cfgs,
                                    const float *const *ref_from_to, const size_t *n_ref,
                                    const fvad_stat_config *stat_cfgs, size_t n_stat_cfgs,
                                    fvad_aggregate_stats *agg_out, fvad_single_stats *single_out) {
  // everything that can be refused is refused before anything runs
  if (const int rc = check_run(sw, cfgs, n_cfgs)) return rc;
  if (!ref_from_to || !n_ref || !stat_cfgs || !agg_out) return set_error(FVAD_EINVAL, "null argument");
  if (n_stat_cfgs != 1 && n_stat_cfgs != n_cfgs)
    return set_error(FVAD_EINVAL, "n_stat_cfgs must be 1 or n_cfgs (" + std::to_string(n_cfgs) + "), not " +
                                      std::to_string(n_stat_cfgs));
  const size_t B = (size_t)sw->cfg.n_streams, n = n_cfgs;
  for (size_t s = 0; s < B; s++)
    if (n_ref[s] > 0 && !ref_from_to[s]) return set_error(FVAD_EINVAL, "null reference list");
  std::vector<fvad::VadmConst> K;
  std::vector<fvad::VadmState> s0;
  if (const int rc = prepare(sw->cfg, cfgs, n_cfgs, &K, &s0)) return rc;
  Score sc;
  sc.stat = stat_cfgs;
  sc.n_stat = n_stat_cfgs;
  sc.off.resize(B + 1);
  using Label = std::pair<float, float>;
  std::vector<Label> one;
  for (size_t s = 0; s < B; s++) {  // fvad_eval_stats' sort_by_start, once per stream
    sc.off[s] = (long long)(sc.lab.size() / 2);
    one.clear();
    for (size_t j = 0; j < n_ref[s]; j++) one.emplace_back(ref_from_to[s][2 * j], ref_from_to[s][2 * j + 1]);
    std::stable_sort(one.begin(), one.end(), [](const Label &a, const Label &b) { return a.first < b.first; });
    for (const auto &r : one) {
      sc.lab.push_back(r.first);
      sc.lab.push_back(r.second);
    }
  }
  sc.off[B] = (long long)(sc.lab.size() / 2);
  sc.single.resize(B * n);
  sc.status.assign(B * n, fvad::kEvalScored);
  if (const int rc = sw->cfg.device == -1 ? run_host(sw, cfgs, K, &sc) : run_device(sw, K, s0, &sc)) return rc;
  // the run stands (counts, snapshots); a lane that could not be scored fails the call
  for (size_t s = 0; s < B; s++)
    for (size_t m = 0; m < n; m++) {
      const std::string where = "stream " + std::to_string(s) + ", config " + std::to_string(m) + ": ";
      if (sc.status[s * n + m] == fvad::kEvalOverCapacity)
        return set_error(FVAD_EINVAL, where + std::to_string(sw->lanes[s * n + m].snap.n_segments) +
                                          " segments exceed seg_capacity, the score would be of a truncated list");
      if (sc.status[s * n + m] != fvad::kEvalScored)
        return set_error(FVAD_EINVAL, where + "segment starts are not in non-decreasing order, the lane was not scored");
    }
  std::vector<fvad_single_stats> st(B);
  for (size_t m = 0; m < n; m++) {
    for (size_t s = 0; s < B; s++) {
      st[s] = sc.single[s * n + m];
      if (single_out) single_out[m * B + s] = st[s];
    }
    fvad_eval_aggregate(st.data(), B, &agg_out[m]);
  }
  return FVAD_OK;
}

extern "C" int fvad_sweep_last_run(const fvad_sweep *sw, size_t *n_cfgs, int *kept_segments, size_t *bytes_back) {
  if (!sw) return set_error(FVAD_EINVAL, "null sweep");
  if (n_cfgs) *n_cfgs = sw->n_cfgs;
  if (kept_segments) *kept_segments = sw->kept ? 1 : 0;
  if (bytes_back) *bytes_back = sw->bytes_back;
  return FVAD_OK;
}

extern "C" size_t fvad_sweep_segments(const fvad_sweep *sw, int stream, size_t cfg, fvad_segment *out, size_t cap) {
  const Lane *l = lane_of(sw, stream, cfg);
  if (!l) return 0;
  const size_t k = std::min(l->segs.size(), cap);
  if (out)
    for (size_t i = 0; i < k; i++) out[i] = l->segs[i];
  return (size_t)l->snap.n_segments;
}

extern "C" int fvad_sweep_counts(const fvad_sweep *sw, uint64_t *out, size_t cap) {
  if (!sw || !out) return set_error(FVAD_EINVAL, "null argument");
  if (cap < sw->lanes.size()) return set_error(FVAD_EINVAL, "cap below n_streams * n_cfgs");
  for (size_t i = 0; i < sw->lanes.size(); i++) out[i] = sw->lanes[i].snap.n_segments;
  return FVAD_OK;
}

extern "C" int fvad_sweep_snapshot(const fvad_sweep *sw, int stream, size_t cfg, fvad_vadm_snapshot *out) {
  const Lane *l = lane_of(sw, stream, cfg);
  if (!l || !out) return set_error(FVAD_EINVAL, "no such (stream, config) in the last run");
  *out = l->snap;
  return FVAD_OK;
}

extern "C" int fvad_sweep_score(const fvad_sweep *sw, const float *const *ref_from_to, const size_t *n_ref,
                                const fvad_stat_config *stat_cfg, fvad_aggregate_stats *agg_out,
                                fvad_single_stats *single_out) {
  if (!sw || !ref_from_to || !n_ref || !stat_cfg || !agg_out) return set_error(FVAD_EINVAL, "null argument");
  if (sw->n_cfgs == 0) return set_error(FVAD_EINVAL, "no run to score");
  if (!sw->kept)
    return set_error(FVAD_EINVAL, "the last run (fvad_sweep_run_score) kept no segments: nothing to score");
  const size_t B = (size_t)sw->cfg.n_streams, n = sw->n_cfgs;
  for (size_t s = 0; s < B; s++) {
    if (n_ref[s] > 0 && !ref_from_to[s]) return set_error(FVAD_EINVAL, "null reference list");
    for (size_t m = 0; m < n; m++)
      if (sw->lanes[s * n + m].snap.n_segments > (uint64_t)sw->cfg.seg_capacity)
        return set_error(FVAD_EINVAL, "stream " + std::to_string(s) + ", config " + std::to_string(m) + ": " +
                                          std::to_string(sw->lanes[s * n + m].snap.n_segments) +
                                          " segments exceed seg_capacity, the score would be of a truncated list");
  }
  std::vector<fvad_single_stats> st(B);
  std::vector<float> vs;
  for (size_t m = 0; m < n; m++) {
    for (size_t s = 0; s < B; s++) {
      vs.clear();
      for (const fvad_segment &g : sw->lanes[s * n + m].segs) {  // as the simulator converts them
        vs.push_back((float)g.sample_from / 48000.0f);
        vs.push_back((float)g.sample_to / 48000.0f);
      }
      if (const int rc = fvad_eval_stats(vs.data(), vs.size() / 2, ref_from_to[s], n_ref[s], stat_cfg, &st[s]))
        return rc;
      if (single_out) single_out[m * B + s] = st[s];
    }
    fvad_eval_aggregate(st.data(), B, &agg_out[m]);
  }
  return FVAD_OK;
}

extern "C" size_t fvad_sweep_bytes(const fvad_sweep_config *cfg, const fvad_vadm_config *cfgs, size_t n_cfgs) {
  if (!cfg || !cfgs || n_cfgs < 1 || check_config(*cfg)) return 0;
  std::vector<fvad::VadmConst> K;
  std::vector<fvad::VadmState> s0;
  if (prepare(*cfg, cfgs, n_cfgs, &K, &s0)) return 0;
  return chunk_bytes(*cfg, K, 0, n_cfgs);
}

extern "C" int fvad_sweep_set_debug(fvad_sweep *sw, int key, int value) {
  if (!sw) return set_error(FVAD_EINVAL, "null sweep");
  switch (key) {
    case FVAD_SWEEP_DEBUG_BOUND_SCALE:
      if (value < -1) return set_error(FVAD_EINVAL, "value >= -1 required");
      sw->bound_scale = value == -1 ? HUGE_VAL : (value == 0 ? 1.0 : (double)value);
      return FVAD_OK;
    case FVAD_SWEEP_DEBUG_DEFER_MAX:
      if (value < 0) return set_error(FVAD_EINVAL, "value >= 0 required");
      sw->defer_max = (unsigned)value;
      return FVAD_OK;
    case FVAD_SWEEP_DEBUG_CHUNK:
      if (value < 0) return set_error(FVAD_EINVAL, "value >= 0 required");
      sw->chunk = (size_t)value;
      return FVAD_OK;
    case FVAD_SWEEP_DEBUG_COUNT:
      sw->count_on = value != 0;
      return FVAD_OK;
    default:
      return set_error(FVAD_EINVAL, "unknown debug key");
  }
}

extern "C" int fvad_sweep_debug_counts(const fvad_sweep *sw, unsigned long long *out, int n) {
  if (!sw || !out || n < 1) return set_error(FVAD_EINVAL, "invalid argument");
  if (!sw->have_counts) return set_error(FVAD_EINVAL, "the last run did not count (FVAD_SWEEP_DEBUG_COUNT, a device run)");
  const int k = std::min(n, (int)fvad::kVadmCounts);
  for (int i = 0; i < k; i++) out[i] = sw->counts[i];
  return k;
}
