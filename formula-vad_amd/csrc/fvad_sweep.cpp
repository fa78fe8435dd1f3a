// Config sweep (include/fvad.h: fvad_sweep_*): the recorded windows, the
// validation, the device run in chunks (k_vadm_sweep, fvad_sweep.hip; with
// fvad_sweep_run_score each chunk's k_sweep_score behind it,
// fvad_sweep_score.hip), the host run (the host VADMachine, fvad_machine.cpp)
// and the scores (fvad_sweep_score: the host evaluator, fvad_eval.cpp;
// fvad_sweep_run_score: the shared core, fvad_eval_core.h).  Everything but
// fvad_sweep_run and fvad_sweep_run_score on a device sweep is host code.
//
// A spectral sweep (fvad_sweep_create_spectral) records magnitude spectra in
// the band sums' place: Windows::band then holds [window][channel][n_spec],
// a run lists its configs' distinct bands, and each chunk's band minima come
// from k_sweep_bandmin (the host path: fvad_bandsum_core.h) instead of
// k_sweep_min; the machines run unchanged with n_bands = the chunk's bands.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/fvad.h"
#include "fvad_bandsum_core.h"
#include "fvad_eval_core.h"
#include "fvad_hip_own.h"
#include "fvad_internal.h"
#include "fvad_machine.h"
#include "fvad_sweep.h"

using fvad::set_error;

#define HIP_TRY(expr)                                                                                          \
  do {                                                                                                         \
    hipError_t e_ = (expr);                                                                                    \
    if (e_ != hipSuccess) return set_error(FVAD_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

namespace {
constexpr size_t kSweepBudget = (size_t)4 << 30;  // device bytes of one chunk's machines

struct Windows {  // one stream's recorded sequence (band: a spectral sweep's magnitudes)
  std::vector<float> band, vad, vr;
  size_t n() const { return vr.size(); }
};
struct Lane {  // results of (stream, config)
  fvad_vadm_snapshot snap{};
  std::vector<fvad_segment> segs;  // the first min(total, seg_capacity)
};

// Device elements of T, grown on demand: never shrinks, holds 256 bytes at
// least, and is empty (cap 0) after a failed grow.  The copies and the clear
// count in elements; a count of 0 does nothing (the buffer may not exist).
template <typename T>
struct DevBuf {
  fvad::dev_ptr<T> p;
  size_t cap = 0;  // elements
  T *get() const { return p.get(); }
  int grow(size_t count) {
    if (count <= cap) return FVAD_OK;
    p.reset();
    cap = 0;
    const size_t n = std::max(count, (256 + sizeof(T) - 1) / sizeof(T));
    if (const int rc = fvad::make_dev(p, n)) return rc;
    cap = n;
    return FVAD_OK;
  }
  hipError_t put(const T *src, size_t count) const {
    return count ? hipMemcpy(p.get(), src, count * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
  }
  hipError_t put_async(const T *src, size_t count, hipStream_t s) const {
    return count ? hipMemcpyAsync(p.get(), src, count * sizeof(T), hipMemcpyHostToDevice, s) : hipSuccess;
  }
  hipError_t zero_async(size_t count, hipStream_t s) const { return hipMemsetAsync(p.get(), 0, count * sizeof(T), s); }
  // *back (the run's device-to-host bytes) grows by what was copied; U: T, or
  // the same record under its API name (VadmSeg as fvad_segment, fvad_machine.h)
  template <typename U>
  hipError_t fetch(U *dst, size_t count, size_t *back = nullptr) const {
    static_assert(sizeof(U) == sizeof(T), "fetch into records of the buffer's size");
    if (back) *back += count * sizeof(T);
    return hipMemcpy(dst, p.get(), count * sizeof(T), hipMemcpyDeviceToHost);
  }
};

struct Score {  // one fvad_sweep_run_score call: what the lanes are scored against, and their scores
  std::vector<float> lab;      // every stream's (from, to), each stream's stably sorted by start
  std::vector<long long> off;  // [n_streams + 1] first label of a stream
  const fvad_stat_config *stat = nullptr;
  size_t n_stat = 0;  // 1 or n_cfgs
  std::vector<fvad_single_stats> single;  // [stream][cfg]
  std::vector<unsigned> status;           // [stream][cfg] fvad::kEval*
};

// The machines of configs [c0, c1) over B streams as the device holds them.
// Making one places each config's long-term rows (K[m].lt_off).
struct Chunk {
  size_t c0, c1, B, seg_cap;
  size_t lt = 0, max_st = 0, max_r = 0;  // long-term floats; the longest short-term and ratio buffers
  Chunk(const fvad_sweep_config &c, std::vector<fvad::VadmConst> &K, size_t c0_, size_t c1_)
      : c0(c0_), c1(c1_), B((size_t)c.n_streams), seg_cap((size_t)c.seg_capacity) {
    for (size_t m = c0; m < c1; m++) {
      K[m].lt_off = (long long)lt;
      lt += (size_t)K[m].lt_pitch * B;
      max_st = std::max(max_st, (size_t)K[m].n_st);
      max_r = std::max(max_r, (size_t)K[m].n_r);
    }
  }
  size_t n_cfgs() const { return c1 - c0; }
  size_t lanes() const { return B * n_cfgs(); }
  size_t bytes() const {
    return (lt + (max_st + max_r) * lanes()) * sizeof(float) + lanes() * sizeof(fvad::VadmState) +
           lanes() * seg_cap * sizeof(fvad::VadmSeg) + n_cfgs() * sizeof(fvad::VadmConst);
  }
};

// A spectral run's bands: the distinct (lo, hi) of its configs in order of
// first appearance, and each config's index among them.
struct Bands {
  std::vector<int2> list;
  std::vector<int> of;  // [config]
  std::map<std::pair<int, int>, int> index;
};
// The distinct bands of the configs [c0, c0 + n) in order of first appearance
// (local), and for each band of the run its slot among them or -1 (slot_of)
struct ChunkBands {
  std::vector<int2> local;
  std::vector<int> slot_of;
  explicit ChunkBands(const Bands &b) : slot_of(b.list.size(), -1) {}
  void add(const Bands &b, size_t m) {
    int &sl = slot_of[(size_t)b.of[m]];
    if (sl < 0) {
      sl = (int)local.size();
      local.push_back(b.list[(size_t)b.of[m]]);
    }
  }
  bool has(const Bands &b, size_t m) const { return slot_of[(size_t)b.of[m]] >= 0; }
};
}  // namespace

struct fvad_sweep {
  fvad_sweep_config cfg{};
  // spectral sweep: the windows hold the magnitudes of the bins spec_lo..spec_hi
  bool spectral = false;
  int spec_lo = 0, spec_hi = 0;
  int n_spec() const { return spec_hi - spec_lo + 1; }
  // floats of a recorded window's row in Windows::band
  size_t per() const { return (size_t)cfg.n_channels * (spectral ? (size_t)n_spec() : (size_t)cfg.n_bands); }
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
  DevBuf<float> d_band, d_wmin, d_wvad, d_wvr, d_lt, d_sbuf, d_rbuf;
  DevBuf<long long> d_off;
  DevBuf<int> d_nwin;
  DevBuf<int2> d_bands;  // spectral: the chunk's distinct bands
  // k_sweep_bandmin's event time over the last device run's chunks (fvad_sweep_bandmin_ms)
  fvad::event_ptr ev_bandmin[2];
  double bandmin_ms = 0;
  DevBuf<fvad::VadmConst> d_K;
  DevBuf<fvad::VadmState> d_st;
  DevBuf<fvad::VadmSeg> d_seg;
  DevBuf<unsigned long long> d_count;
  // fvad_sweep_run_score
  DevBuf<float> d_lab;
  DevBuf<long long> d_lab_off;
  DevBuf<fvad_stat_config> d_stat;
  DevBuf<fvad_single_stats> d_single;
  DevBuf<unsigned> d_status;
  long long n_windows = 0;
};

namespace {
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
// (sw: null for fvad_sweep_bytes, a plain sweep's).  A spectral sweep accepts
// every band inside its range: *bands lists the distinct ones, and the slot
// (the band's index there) is set again for each chunk.
int prepare(const fvad_sweep_config &c, const fvad_sweep *sw, const fvad_vadm_config *cfgs, size_t n,
            std::vector<fvad::VadmConst> *K, std::vector<fvad::VadmState> *s0, Bands *bands) {
  K->resize(n);
  s0->resize(n);
  for (size_t m = 0; m < n; m++) {
    const fvad::VadmDerived d = fvad::vadm_derive(cfgs[m], c.sample_rate, c.fft_size);
    (*K)[m] = d.K;
    (*s0)[m] = d.s0;
    if (sw && sw->spectral) {
      if (d.lo < sw->spec_lo || d.hi > sw->spec_hi || d.hi < d.lo)
        return set_error(FVAD_EINVAL, "config " + std::to_string(m) + ": its speech band (bins " + std::to_string(d.lo) +
                                          ".." + std::to_string(d.hi) + ") lies outside the sweep's spectrum range (" +
                                          std::to_string(sw->spec_lo) + ".." + std::to_string(sw->spec_hi) + ")");
      const auto at = bands->index.emplace(std::make_pair(d.lo, d.hi), (int)bands->list.size());
      if (at.second) bands->list.push_back(make_int2(d.lo, d.hi));
      bands->of.push_back(at.first->second);
      (*K)[m].slot = at.first->second;
      continue;
    }
    (*K)[m].slot = fvad::band_slot(c.band_lo, c.band_hi, c.n_bands, d.lo, d.hi);
    if ((*K)[m].slot < 0)
      return set_error(FVAD_EINVAL, "config " + std::to_string(m) + ": its speech band (bins " + std::to_string(d.lo) +
                                        ".." + std::to_string(d.hi) + ") is none of the sweep's bands");
  }
  return FVAD_OK;
}

int check_run(const fvad_sweep *sw, const fvad_vadm_config *cfgs, size_t n_cfgs) {
  if (!sw || !cfgs || n_cfgs < 1) return set_error(FVAD_EINVAL, "invalid argument");
  if (n_cfgs > ((size_t)1 << 24)) return set_error(FVAD_EINVAL, "n_cfgs above 2^24");
  return FVAD_OK;
}

std::string over_capacity(size_t stream, size_t cfg, uint64_t n_segments) {
  return "stream " + std::to_string(stream) + ", config " + std::to_string(cfg) + ": " + std::to_string(n_segments) +
         " segments exceed seg_capacity, the score would be of a truncated list";
}

// Config by config: every stream's statistics (single_of(s, m, &st), an FVAD_*
// status) into single_out[m][s] where asked for, and their aggregate into agg_out[m]
template <typename F>
int aggregate_configs(size_t B, size_t n, F &&single_of, fvad_aggregate_stats *agg_out, fvad_single_stats *single_out) {
  std::vector<fvad_single_stats> st(B);
  for (size_t m = 0; m < n; m++) {
    for (size_t s = 0; s < B; s++) {
      if (const int rc = single_of(s, m, &st[s])) return rc;
      if (single_out) single_out[m * B + s] = st[s];
    }
    fvad_eval_aggregate(st.data(), B, &agg_out[m]);
  }
  return FVAD_OK;
}

int upload_windows(fvad_sweep *sw) {
  const fvad_sweep_config &c = sw->cfg;
  const size_t B = (size_t)c.n_streams, per = sw->per();
  std::vector<long long> off(B);
  std::vector<int> nwin(B);
  size_t total = 0;
  for (size_t s = 0; s < B; s++) {
    off[s] = (long long)total;
    nwin[s] = (int)sw->win[s].n();
    total += sw->win[s].n();
  }
  // (a spectral sweep's rows go up stream by stream: no second host copy of the spectra)
  std::vector<float> band(sw->spectral ? 0 : total * per), vad(total), vr(total);
  for (size_t s = 0; s < B; s++) {
    const Windows &w = sw->win[s];
    if (!sw->spectral) std::copy(w.band.begin(), w.band.end(), band.begin() + (size_t)off[s] * per);
    std::copy(w.vad.begin(), w.vad.end(), vad.begin() + off[s]);
    std::copy(w.vr.begin(), w.vr.end(), vr.begin() + off[s]);
  }
  int rc;
  if ((rc = sw->d_band.grow(total * per)) || (rc = sw->d_wvad.grow(total)) || (rc = sw->d_wvr.grow(total)) ||
      (rc = sw->d_off.grow(B)) || (rc = sw->d_nwin.grow(B)))
    return rc;
  if (!sw->spectral && (rc = sw->d_wmin.grow(total * c.n_bands))) return rc;  // (spectral: per chunk, run_device)
  if (sw->spectral) {
    for (size_t s = 0; s < B; s++)
      if (!sw->win[s].band.empty())
        HIP_TRY(hipMemcpy(sw->d_band.get() + (size_t)off[s] * per, sw->win[s].band.data(),
                          sw->win[s].band.size() * sizeof(float), hipMemcpyHostToDevice));
  } else {
    HIP_TRY(sw->d_band.put(band.data(), band.size()));
  }
  HIP_TRY(sw->d_wvad.put(vad.data(), total));
  HIP_TRY(sw->d_wvr.put(vr.data(), total));
  HIP_TRY(sw->d_off.put(off.data(), B));
  HIP_TRY(sw->d_nwin.put(nwin.data(), B));
  sw->n_windows = (long long)total;
  if (!sw->spectral) {
    fvad::SweepArgs a{};
    a.n_channels = c.n_channels;
    a.n_bands = c.n_bands;
    a.n_windows = sw->n_windows;
    a.band = sw->d_band.get();
    a.wmin = sw->d_wmin.get();
    HIP_TRY(fvad::launch_sweep_min(a, sw->stream.get()));
    HIP_TRY(hipStreamSynchronize(sw->stream.get()));
  }
  sw->dirty = false;
  return FVAD_OK;
}

// sc: null (the segments come back), or the lanes are scored on the device and
// their statistics and status words come back instead
// bands: a spectral run's (empty otherwise)
int run_device(fvad_sweep *sw, std::vector<fvad::VadmConst> &K, const std::vector<fvad::VadmState> &s0,
               const Bands &bands, Score *sc) {
  const fvad_sweep_config &c = sw->cfg;
  const size_t B = (size_t)c.n_streams, n = K.size();
  const hipStream_t stream = sw->stream.get();
  HIP_TRY(hipSetDevice(c.device));
  if (sw->dirty)
    if (const int rc = upload_windows(sw)) return rc;
  int rc;
  if (sw->count_on) {
    if ((rc = sw->d_count.grow(fvad::kVadmCounts))) return rc;
    HIP_TRY(sw->d_count.zero_async(fvad::kVadmCounts, stream));
  }
  if (sc) {  // the labels and the stat configs, once per call
    if ((rc = sw->d_lab.grow(sc->lab.size())) || (rc = sw->d_lab_off.grow(sc->off.size())) ||
        (rc = sw->d_stat.grow(sc->n_stat)))
      return rc;
    HIP_TRY(sw->d_lab.put_async(sc->lab.data(), sc->lab.size(), stream));
    HIP_TRY(sw->d_lab_off.put_async(sc->off.data(), sc->off.size(), stream));
    HIP_TRY(sw->d_stat.put_async(sc->stat, sc->n_stat, stream));
  }
  if (sw->spectral)
    for (fvad::event_ptr &ev : sw->ev_bandmin)
      if (!ev && (rc = fvad::make_event(ev, true))) return rc;
  double bandmin_ms = 0;
  std::vector<Lane> lanes(B * n);
  std::vector<fvad::VadmState> st;
  std::vector<fvad_segment> seg;  // (a VadmSeg is an fvad_segment: fvad_machine.h)
  std::vector<fvad_single_stats> single;
  std::vector<unsigned> status;
  size_t bytes_back = 0;
  for (size_t c0 = 0; c0 < n;) {
    // the chunk: configs [c0, c1), by the test hook or as many as the budget holds (one at least)
    // (spectral: the chunk's band minima, windows x its distinct bands, count too)
    size_t c1 = c0 + 1;
    ChunkBands cb(bands);
    const size_t wmin_per_band = (size_t)sw->n_windows * sizeof(float);
    if (sw->spectral) cb.add(bands, c0);
    if (sw->chunk) {
      c1 = std::min(n, c0 + sw->chunk);
      if (sw->spectral)
        for (size_t m = c0 + 1; m < c1; m++) cb.add(bands, m);
    } else {
      while (c1 < n) {
        const size_t D1 = sw->spectral ? cb.local.size() + (cb.has(bands, c1) ? 0 : 1) : 0;
        if (Chunk(c, K, c0, c1 + 1).bytes() + D1 * wmin_per_band > kSweepBudget) break;
        if (sw->spectral) cb.add(bands, c1);
        c1++;
      }
    }
    const Chunk ch(c, K, c0, c1);
    const size_t nc = ch.n_cfgs(), nl = ch.lanes();
    const int D = sw->spectral ? (int)cb.local.size() : c.n_bands;
    if (sw->spectral) {
      for (size_t m = c0; m < c1; m++) K[m].slot = cb.slot_of[(size_t)bands.of[m]];
      if ((rc = sw->d_bands.grow((size_t)D)) || (rc = sw->d_wmin.grow((size_t)sw->n_windows * D))) return rc;
      HIP_TRY(sw->d_bands.put_async(cb.local.data(), (size_t)D, stream));
      fvad::BandMinArgs b{};
      b.n_channels = c.n_channels;
      b.n_spec = sw->n_spec();
      b.spec_lo = sw->spec_lo;
      b.n_bands = D;
      b.n_windows = sw->n_windows;
      b.spec = sw->d_band.get();
      b.bands = sw->d_bands.get();
      b.wmin = sw->d_wmin.get();
      HIP_TRY(hipEventRecord(sw->ev_bandmin[0].get(), stream));
      HIP_TRY(fvad::launch_sweep_bandmin(b, stream));
      HIP_TRY(hipEventRecord(sw->ev_bandmin[1].get(), stream));
    }
    if ((rc = sw->d_K.grow(nc)) || (rc = sw->d_st.grow(nl)) || (rc = sw->d_lt.grow(ch.lt)) ||
        (rc = sw->d_sbuf.grow(ch.max_st * nl)) || (rc = sw->d_rbuf.grow(ch.max_r * nl)) ||
        (rc = sw->d_seg.grow(nl * ch.seg_cap)))
      return rc;
    if (sc && ((rc = sw->d_single.grow(nl)) || (rc = sw->d_status.grow(nl)))) return rc;
    st.resize(nl);
    for (size_t s = 0; s < B; s++)
      for (size_t m = 0; m < nc; m++) st[s * nc + m] = s0[c0 + m];
    HIP_TRY(sw->d_K.put_async(K.data() + c0, nc, stream));
    HIP_TRY(sw->d_st.put_async(st.data(), nl, stream));
    // entries never pushed are never read (lt_nw, the counts); zeroed all the same
    HIP_TRY(sw->d_lt.zero_async(ch.lt, stream));
    HIP_TRY(sw->d_sbuf.zero_async(ch.max_st * nl, stream));
    HIP_TRY(sw->d_rbuf.zero_async(ch.max_r * nl, stream));
    fvad::SweepArgs a{};
    a.n_streams = c.n_streams;
    a.n_cfgs = (int)nc;
    a.n_channels = c.n_channels;
    a.n_bands = D;
    a.seg_cap = c.seg_capacity;
    a.K = sw->d_K.get();
    a.st = sw->d_st.get();
    a.lt = sw->d_lt.get();
    a.sbuf = sw->d_sbuf.get();
    a.rbuf = sw->d_rbuf.get();
    a.seg = sw->d_seg.get();
    a.win_off = sw->d_off.get();
    a.n_win = sw->d_nwin.get();
    a.band = sw->d_band.get();
    a.wmin = sw->d_wmin.get();
    a.wvad = sw->d_wvad.get();
    a.wvr = sw->d_wvr.get();
    a.n_windows = sw->n_windows;
    a.fft = (unsigned long long)c.fft_size;
    a.bound_scale = sw->bound_scale;
    a.defer_max = sw->defer_max;
    a.count = sw->count_on ? sw->d_count.get() : nullptr;
    HIP_TRY(fvad::launch_vadm_sweep(a, stream));
    if (sc) {
      fvad::ScoreArgs b{};
      b.n_streams = c.n_streams;
      b.n_cfgs = (int)nc;
      b.seg_cap = c.seg_capacity;
      b.st = a.st;
      b.seg = a.seg;
      b.lab = sw->d_lab.get();
      b.lab_off = sw->d_lab_off.get();
      b.stat_stride = sc->n_stat == 1 ? 0 : 1;
      b.stat = sw->d_stat.get() + c0 * (size_t)b.stat_stride;
      b.single = sw->d_single.get();
      b.status = sw->d_status.get();
      HIP_TRY(fvad::launch_sweep_score(b, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    if (sw->spectral) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, sw->ev_bandmin[0].get(), sw->ev_bandmin[1].get()));
      bandmin_ms += ms;
    }
    HIP_TRY(sw->d_st.fetch(st.data(), nl, &bytes_back));
    if (sc) {
      single.resize(nl);
      status.resize(nl);
      HIP_TRY(sw->d_single.fetch(single.data(), nl, &bytes_back));
      HIP_TRY(sw->d_status.fetch(status.data(), nl, &bytes_back));
    } else {
      seg.resize(nl * ch.seg_cap);
      HIP_TRY(sw->d_seg.fetch(seg.data(), seg.size(), &bytes_back));
    }
    for (size_t s = 0; s < B; s++)
      for (size_t m = 0; m < nc; m++) {
        const size_t from = s * nc + m, to = s * n + c0 + m;
        fvad::vadm_snapshot_of(st[from], &lanes[to].snap);
        if (sc) {
          sc->status[to] = status[from];
          sc->single[to] = single[from];
        } else {
          const fvad_segment *g = seg.data() + from * ch.seg_cap;
          lanes[to].segs.assign(g, g + std::min<size_t>(st[from].n_segs, ch.seg_cap));
        }
      }
    c0 = c1;
  }
  if (sw->count_on) HIP_TRY(sw->d_count.fetch(sw->counts, fvad::kVadmCounts));
  sw->have_counts = sw->count_on;
  sw->lanes = std::move(lanes);
  sw->n_cfgs = n;
  sw->kept = !sc;
  sw->bytes_back = bytes_back;
  sw->bandmin_ms = bandmin_ms;
  return FVAD_OK;
}

// sc: null (the segments are kept), or each lane is scored by the shared core
// as k_sweep_score does it and keeps no segments
// A spectral sweep (bands: the run's) works by (stream, band): the band's sums
// over the stream's windows once (fvad_bandsum_core.h: k_sweep_bandmin's
// chains), then every config of that band over them.
int run_host(fvad_sweep *sw, const fvad_vadm_config *cfgs, const std::vector<fvad::VadmConst> &K, const Bands &bands,
             Score *sc) {
  const fvad_sweep_config &c = sw->cfg;
  const size_t B = (size_t)c.n_streams, n = K.size(), nl = B * n;
  std::vector<Lane> lanes(nl);
  // one lane over `band` [window][channel][n_bands], reading slot `slot`
  auto lane = [&](size_t l, const float *band, int n_bands, int slot) {
    const size_t s = l / n, m = l % n;
    const Windows &w = sw->win[s];
    fvad::host_vadm_lane(cfgs[m], c.sample_rate, c.fft_size, c.n_channels, n_bands, slot, w.n(), band, w.vad.data(),
                         w.vr.data(), &lanes[l].snap, &lanes[l].segs);
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
  };
  std::vector<std::vector<size_t>> cfgs_of(bands.list.size());  // spectral: the configs of each band
  for (size_t m = 0; m < bands.of.size(); m++) cfgs_of[(size_t)bands.of[m]].push_back(m);
  const size_t units = sw->spectral ? B * bands.list.size() : nl;
  auto work = [&](size_t t, size_t nt) {
    std::vector<float> sums;
    for (size_t u = t; u < units; u += nt) {
      if (!sw->spectral) {
        lane(u, sw->win[u / n].band.data(), c.n_bands, K[u % n].slot);
        continue;
      }
      const size_t s = u / bands.list.size(), g = u % bands.list.size(), C = (size_t)c.n_channels, per = sw->per();
      const Windows &w = sw->win[s];
      sums.resize(w.n() * C);
      for (size_t i = 0; i < w.n() * C; i++)
        sums[i] = fvad::band_chain(w.band.data() + (i / C) * per + (i % C) * (size_t)sw->n_spec(), sw->spec_lo,
                                   bands.list[g].x, bands.list[g].y);
      for (const size_t m : cfgs_of[g]) lane(s * n + m, sums.data(), 1, 0);
    }
  };
  const size_t nt =
      std::max<size_t>(1, std::min<size_t>({(size_t)16, (size_t)std::thread::hardware_concurrency(), units}));
  std::vector<std::thread> th;
  for (size_t t = 1; t < nt; t++) th.emplace_back(work, t, nt);
  work(0, nt);
  for (auto &x : th) x.join();
  sw->lanes = std::move(lanes);
  sw->n_cfgs = n;
  sw->have_counts = false;
  sw->kept = !sc;
  sw->bytes_back = 0;
  sw->bandmin_ms = 0;
  return FVAD_OK;
}

// fvad_sweep_run, _run_host and _run_score: the configs over the recorded
// windows, on the host for a device = -1 sweep or when forced
int run(fvad_sweep *sw, const fvad_vadm_config *cfgs, size_t n_cfgs, bool force_host, Score *sc) {
  if (const int rc = check_run(sw, cfgs, n_cfgs)) return rc;
  std::vector<fvad::VadmConst> K;
  std::vector<fvad::VadmState> s0;
  Bands bands;
  if (const int rc = prepare(sw->cfg, sw, cfgs, n_cfgs, &K, &s0, &bands)) return rc;
  if (force_host || sw->cfg.device == -1) return run_host(sw, cfgs, K, bands, sc);
  return run_device(sw, K, s0, bands, sc);
}

const Lane *lane_of(const fvad_sweep *sw, int stream, size_t cfg) {
  if (!sw || stream < 0 || stream >= sw->cfg.n_streams || cfg >= sw->n_cfgs) return nullptr;
  return &sw->lanes[(size_t)stream * sw->n_cfgs + cfg];
}
}  // namespace

namespace {
int create(const fvad_sweep_config *cfg, fvad_sweep **out) {
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
}  // namespace

extern "C" int fvad_sweep_create(const fvad_sweep_config *cfg, fvad_sweep **out) {
  if (!cfg || !out) return set_error(FVAD_EINVAL, "null argument");
  return create(cfg, out);
}

extern "C" int fvad_sweep_create_spectral(const fvad_sweep_config *cfg, int spec_lo, int spec_hi, fvad_sweep **out) {
  if (!cfg || !out) return set_error(FVAD_EINVAL, "null argument");
  fvad_sweep_config c = *cfg;  // n_bands and the bands are ignored: one band, the range, for check_config
  c.n_bands = 1;
  c.band_lo[0] = spec_lo;
  c.band_hi[0] = spec_hi;
  if (c.fft_size >= 2 && (spec_lo < 0 || spec_hi < spec_lo || spec_hi > c.fft_size / 2))
    return set_error(FVAD_EINVAL, "invalid spectrum range: 0 <= spec_lo <= spec_hi <= fft_size / 2 required");
  if (const int rc = create(&c, out)) return rc;
  (*out)->spectral = true;
  (*out)->spec_lo = spec_lo;
  (*out)->spec_hi = spec_hi;
  return FVAD_OK;
}

extern "C" void fvad_sweep_destroy(fvad_sweep *sw) {
  if (!sw) return;
  if (sw->cfg.device != -1) (void)hipSetDevice(sw->cfg.device);
  delete sw;
}

namespace {
// the setters' kinds: band sums go to a plain sweep, spectra to a spectral one
int check_kind(const fvad_sweep *sw, bool spectral) {
  if (sw->spectral == spectral) return FVAD_OK;
  return set_error(FVAD_EINVAL, spectral ? "not a spectral sweep (fvad_sweep_create_spectral): it records band sums"
                                         : "a spectral sweep records spectra (fvad_sweep_set_spectra, _append_spectra)");
}

// fvad_sweep_set_windows / _set_spectra: band holds sw->per() floats per window
int set_rows(fvad_sweep *sw, int stream, size_t n_windows, const float *band, const float *vad,
             const float *vol_ratio) {
  if (stream < 0 || stream >= sw->cfg.n_streams) return set_error(FVAD_EINVAL, "stream index out of range");
  if (n_windows > 0 && (!band || !vol_ratio))
    return set_error(FVAD_EINVAL, sw->spectral ? "null spectrum or vol_ratio" : "null band or vol_ratio");
  if (n_windows > (size_t)0x7fffffff) return set_error(FVAD_EINVAL, "n_windows above 2^31 - 1");
  Windows &w = sw->win[(size_t)stream];
  const size_t per = sw->per();
  w.band.assign(band, band + n_windows * per);
  w.vr.assign(vol_ratio, vol_ratio + n_windows);
  if (vad && sw->cfg.use_denoiser)
    w.vad.assign(vad, vad + n_windows);
  else
    w.vad.assign(n_windows, 0.0f);  // fft_input.vad orelse 0 (VADMachine.zig:240-246)
  sw->dirty = true;
  return FVAD_OK;
}

// fvad_sweep_append_outputs / _append_spectra: rows [tick][stream][slot] of sw->per() floats
int append_rows(fvad_sweep *sw, const fvad_outputs *out, const float *rows, int n_ticks, const int32_t *ticks_valid) {
  if (n_ticks < 0) return set_error(FVAD_EINVAL, "n_ticks < 0");
  const fvad_sweep_config &c = sw->cfg;
  const size_t B = (size_t)c.n_streams, W = (size_t)fvad::windows_per_tick(c.fft_size), per = sw->per();
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
        w.band.insert(w.band.end(), rows + o * per, rows + (o + 1) * per);
        w.vad.push_back(c.use_denoiser ? out->win_vad[o] : 0.0f);
        w.vr.push_back(out->win_ratio[o]);
      }
  }
  sw->dirty = true;
  return FVAD_OK;
}
}  // namespace

extern "C" int fvad_sweep_set_windows(fvad_sweep *sw, int stream, size_t n_windows, const float *band,
                                      const float *vad, const float *vol_ratio) {
  if (!sw) return set_error(FVAD_EINVAL, "null sweep");
  if (const int rc = check_kind(sw, false)) return rc;
  return set_rows(sw, stream, n_windows, band, vad, vol_ratio);
}

extern "C" int fvad_sweep_set_spectra(fvad_sweep *sw, int stream, size_t n_windows, const float *spectrum,
                                      const float *vad, const float *vol_ratio) {
  if (!sw) return set_error(FVAD_EINVAL, "null sweep");
  if (const int rc = check_kind(sw, true)) return rc;
  return set_rows(sw, stream, n_windows, spectrum, vad, vol_ratio);
}

extern "C" int fvad_sweep_append_outputs(fvad_sweep *sw, const fvad_outputs *out, int n_ticks,
                                         const int32_t *ticks_valid) {
  if (!sw || !out) return set_error(FVAD_EINVAL, "null argument");
  if (const int rc = check_kind(sw, false)) return rc;
  if (!out->win_flag || !out->win_ratio || !out->win_vad || !out->band)
    return set_error(FVAD_EINVAL, "win_flag, win_ratio, win_vad and band are required");
  return append_rows(sw, out, out->band, n_ticks, ticks_valid);
}

extern "C" int fvad_sweep_append_spectra(fvad_sweep *sw, const fvad_outputs *out, const float *spectrum, int n_ticks,
                                         const int32_t *ticks_valid) {
  if (!sw || !out) return set_error(FVAD_EINVAL, "null argument");
  if (const int rc = check_kind(sw, true)) return rc;
  if (!out->win_flag || !out->win_ratio || !out->win_vad || !spectrum)
    return set_error(FVAD_EINVAL, "win_flag, win_ratio, win_vad and spectrum are required");
  return append_rows(sw, out, spectrum, n_ticks, ticks_valid);
}

extern "C" int fvad_sweep_run_host(fvad_sweep *sw, const fvad_vadm_config *cfgs, size_t n_cfgs) {
  return run(sw, cfgs, n_cfgs, true, nullptr);
}

extern "C" int fvad_sweep_run(fvad_sweep *sw, const fvad_vadm_config *cfgs, size_t n_cfgs) {
  return run(sw, cfgs, n_cfgs, false, nullptr);
}

extern "C" int fvad_sweep_run_score(fvad_sweep *sw, const fvad_vadm_config *cfgs, size_t n_cfgs,
                                    const float *const *ref_from_to, const size_t *n_ref,
                                    const fvad_stat_config *stat_cfgs, size_t n_stat_cfgs,
                                    fvad_aggregate_stats *agg_out, fvad_single_stats *single_out) {
  // everything that can be refused is refused before anything runs, the
  // run's own arguments first (run checks them again)
  if (const int rc = check_run(sw, cfgs, n_cfgs)) return rc;
  if (!ref_from_to || !n_ref || !stat_cfgs || !agg_out) return set_error(FVAD_EINVAL, "null argument");
  if (n_stat_cfgs != 1 && n_stat_cfgs != n_cfgs)
    return set_error(FVAD_EINVAL, "n_stat_cfgs must be 1 or n_cfgs (" + std::to_string(n_cfgs) + "), not " +
                                      std::to_string(n_stat_cfgs));
  const size_t B = (size_t)sw->cfg.n_streams, n = n_cfgs;
  for (size_t s = 0; s < B; s++)
    if (n_ref[s] > 0 && !ref_from_to[s]) return set_error(FVAD_EINVAL, "null reference list");
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
  if (const int rc = run(sw, cfgs, n_cfgs, false, &sc)) return rc;
  // the run stands (counts, snapshots); a lane that could not be scored fails the call
  for (size_t s = 0; s < B; s++)
    for (size_t m = 0; m < n; m++) {
      if (sc.status[s * n + m] == fvad::kEvalOverCapacity)
        return set_error(FVAD_EINVAL, over_capacity(s, m, sw->lanes[s * n + m].snap.n_segments));
      if (sc.status[s * n + m] != fvad::kEvalScored)
        return set_error(FVAD_EINVAL, "stream " + std::to_string(s) + ", config " + std::to_string(m) +
                                          ": segment starts are not in non-decreasing order, the lane was not scored");
    }
  return aggregate_configs(
      B, n,
      [&](size_t s, size_t m, fvad_single_stats *st) {
        *st = sc.single[s * n + m];
        return FVAD_OK;
      },
      agg_out, single_out);
}

extern "C" int fvad_sweep_last_run(const fvad_sweep *sw, size_t *n_cfgs, int *kept_segments, size_t *bytes_back) {
  if (!sw) return set_error(FVAD_EINVAL, "null sweep");
  if (n_cfgs) *n_cfgs = sw->n_cfgs;
  if (kept_segments) *kept_segments = sw->kept ? 1 : 0;
  if (bytes_back) *bytes_back = sw->bytes_back;
  return FVAD_OK;
}

extern "C" int fvad_sweep_bandmin_ms(const fvad_sweep *sw, double *ms) {
  if (!sw || !ms) return set_error(FVAD_EINVAL, "null argument");
  if (!sw->spectral) return set_error(FVAD_EINVAL, "not a spectral sweep");
  *ms = sw->bandmin_ms;
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
        return set_error(FVAD_EINVAL, over_capacity(s, m, sw->lanes[s * n + m].snap.n_segments));
  }
  std::vector<float> vs;
  return aggregate_configs(
      B, n,
      [&](size_t s, size_t m, fvad_single_stats *st) {
        vs.clear();
        for (const fvad_segment &g : sw->lanes[s * n + m].segs) {  // as the simulator converts them
          vs.push_back((float)g.sample_from / 48000.0f);
          vs.push_back((float)g.sample_to / 48000.0f);
        }
        return fvad_eval_stats(vs.data(), vs.size() / 2, ref_from_to[s], n_ref[s], stat_cfg, st);
      },
      agg_out, single_out);
}

extern "C" size_t fvad_sweep_bytes(const fvad_sweep_config *cfg, const fvad_vadm_config *cfgs, size_t n_cfgs) {
  if (!cfg || !cfgs || n_cfgs < 1 || check_config(*cfg)) return 0;
  std::vector<fvad::VadmConst> K;
  std::vector<fvad::VadmState> s0;
  Bands none;
  if (prepare(*cfg, nullptr, cfgs, n_cfgs, &K, &s0, &none)) return 0;
  return Chunk(*cfg, K, 0, n_cfgs).bytes();
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
