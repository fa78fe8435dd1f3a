// The batched engine's per-stream lifecycle: reset, save and restore of listed
// streams (fvad_lifecycle.h), the stream blob's header and checks.
#include <algorithm>
#include <cstring>
#include <vector>

#include "fvad_engine_impl.h"

using namespace fvad::eng;

// ---------------------------------------------------------------------------
// Stream lifecycle: per-stream reset, save and restore (fvad_lifecycle.h)
// ---------------------------------------------------------------------------
static_assert(sizeof(fvad_stream_blob_header) == FVAD_STREAM_BLOB_HEADER_BYTES, "blob header layout");
static_assert(sizeof(fvad::XferArgs) <= 4096 && sizeof(fvad::VClearArgs) <= 4096, "kernel argument blocks");

namespace {

template <typename T>
uint64_t fnv_add(uint64_t h, const T &v) {
  return fnv1a(h, &v, sizeof(T));
}

// a save's or restore's compatibility fields (include/fvad.h)
uint64_t config_hash_of(const fvad_engine *e) {
  const fvad_engine_config &c = e->cfg;
  uint64_t h = kFnvBasis;
  for (int v : {c.mode, c.n_channels, c.fft_size, c.use_denoiser, c.sample_rate, c.n_bands}) h = fnv_add(h, v);
  for (int b = 0; b < c.n_bands; b++) {
    h = fnv_add(h, c.band_lo[b]);
    h = fnv_add(h, c.band_hi[b]);
  }
  h = fnv_add(h, (int)e->vadm.cfgs.size());
  for (const fvad_vadm_config &m : e->vadm.cfgs) {  // field by field: the struct has padding
    for (float v : {m.speech_min_freq, m.speech_max_freq, m.long_term_speech_avg_sec}) h = fnv_add(h, v);
    h = fnv_add(h, (int)(m.has_initial_long_term_avg != 0));
    h = fnv_add(h, m.has_initial_long_term_avg ? m.initial_long_term_avg : 0.0);
    for (float v : {m.short_term_speech_avg_sec, m.speech_threshold_factor, m.channel_vol_ratio_avg_sec,
                    m.channel_vol_ratio_threshold, m.min_consecutive_sec_to_open, m.max_speech_gap_sec,
                    m.min_vad_duration_sec})
      h = fnv_add(h, v);
  }
  // a resampling engine's rate; an engine of 48 kHz input hashes what it always did
  // (per-stream rates: the marker, not input_rate_max -- a record carries its stream's rate)
  if (e->rs) h = fnv_add(h, e->rs->plan.on() ? (int)FVAD_INPUT_RATE_PER_STREAM : e->rs->d.rate);
  // likewise the rate of the denoised PCM, when it is not the 48 kHz signal
  // (per-stream denoised rates: the marker, not denoised_rate_max)
  if (e->ro) h = fnv_add(h, e->ro->plan.on() ? (int)FVAD_DENOISED_RATE_PER_STREAM : e->ro->d.rate);
  return h;
}

fvad::BlobLayout layout_of(const fvad_engine *e, int seg_cap) {
  return fvad::blob_layout(e->cfg.n_channels, e->cfg.fft_size, e->cfg.use_denoiser, e->vadm.args, seg_cap,
                           e->rs ? resample_tail_words(e, fvad::rs::Dir::kIn) : 0,
                           e->ro ? resample_tail_words(e, fvad::rs::Dir::kOut) : 0, e->rs && e->rs->plan.on(),
                           e->ro && e->ro->plan.on());
}

fvad_stream_blob_header header_of(const fvad_engine *e, int count) {
  fvad_stream_blob_header h{};
  const int cap = e->vadm.on() ? e->vadm.args.seg_cap : 0;
  h.magic = FVAD_STREAM_BLOB_MAGIC;
  h.version = FVAD_STREAM_BLOB_VERSION;
  h.header_bytes = FVAD_STREAM_BLOB_HEADER_BYTES;
  h.count = (uint32_t)count;
  h.stream_bytes = (uint64_t)layout_of(e, cap).words * 4;
  h.mode = (uint32_t)e->cfg.mode;
  h.n_channels = (uint32_t)e->cfg.n_channels;
  h.fft_size = (uint32_t)e->cfg.fft_size;
  h.use_denoiser = (uint32_t)(e->cfg.use_denoiser != 0);
  h.n_bands = (uint32_t)e->cfg.n_bands;
  h.n_machines = (uint32_t)e->vadm.args.n;
  h.seg_capacity = (uint32_t)cap;
  h.state_words = fvad::st::kWords;
  h.config_hash = config_hash_of(e);
  h.model_hash = e->model_hash;
  h.sample_rate = (uint32_t)e->cfg.sample_rate;
  h.reserved[0] = !e->rs ? 0u : e->rs->plan.on() ? 0xFFFFFFFFu : (uint32_t)e->rs->d.rate;
  h.reserved[1] = !e->ro ? 0u : e->ro->plan.on() ? 0xFFFFFFFFu : (uint32_t)e->ro->d.rate;
  return h;
}

int parse_blob_header(const void *blob, size_t len, fvad_stream_blob_header *out) {
  if (!blob || !out) return fail(FVAD_EINVAL, "null argument");
  if (len < sizeof(fvad_stream_blob_header)) return fail(FVAD_EFORMAT, "stream blob shorter than its header");
  fvad_stream_blob_header h;
  std::memcpy(&h, blob, sizeof(h));
  if (h.magic != FVAD_STREAM_BLOB_MAGIC) return fail(FVAD_EFORMAT, "not a stream blob (magic)");
  if (h.version != FVAD_STREAM_BLOB_VERSION) return fail(FVAD_EFORMAT, "unsupported stream blob version");
  if (h.header_bytes != FVAD_STREAM_BLOB_HEADER_BYTES) return fail(FVAD_EFORMAT, "stream blob header size");
  const size_t body = len - h.header_bytes;
  if (h.stream_bytes == 0 || h.stream_bytes % 16 != 0 || (h.count > 0 && h.stream_bytes > body / h.count))
    return fail(FVAD_EFORMAT, "stream blob records overrun its length");
  *out = h;
  return FVAD_OK;
}

// device staging of `bytes` (grown on demand, kept)
int ensure_blob(fvad_engine *e, size_t bytes) {
  if (bytes <= e->blob_cap) return FVAD_OK;
  e->d_blob.reset();
  e->blob_cap = 0;
  if (const int rc = fvad::make_dev(e->d_blob, (bytes + 3) / 4)) return rc;
  e->blob_cap = bytes;
  return FVAD_OK;
}

fvad::XferArgs xfer_args(const fvad_engine *e, const fvad::BlobLayout &lay) {
  fvad::XferArgs a{};
  a.state = e->d_state.get();
  a.ring = e->d_ring.get();
  a.ring_len = e->ring_len;
  a.n_streams = e->cfg.n_streams;
  a.vadm = e->vadm.args;
  a.lay = lay;
  a.blob = e->d_blob.get();
  a.rs_tails = e->rs ? e->rs->tails.get() : nullptr;
  a.ro_tails = e->ro ? e->ro->tails.get() : nullptr;
  return a;
}

// a restored record's counters and write indices: what the kernels index with
int check_record(const fvad_engine *e, const fvad::BlobLayout &lay, const float *rec) {
  namespace st = fvad::st;
  if (e->cfg.use_denoiser) {
    const int *ist = reinterpret_cast<const int *>(rec);
    if (ist[st::kFramesDone] < 0 || ist[st::kFramesDone] > 0x7fffffff - e->cfg.max_ticks)
      return fail(FVAD_EFORMAT, "stream record: tick counter out of range");
    if (ist[st::kMemId] < 0 || ist[st::kMemId] >= fvad::kCeps)
      return fail(FVAD_EFORMAT, "stream record: cepstral memory index out of range");
  }
  for (int m = 0; m < e->vadm.args.n; m++) {
    const fvad::VadmConst &K = e->vadm.args.c[m];
    fvad::VadmState S;
    std::memcpy(&S, rec + lay.o_mach[m], sizeof(S));
    const unsigned nl = (unsigned)K.n_lt, ns = (unsigned)K.n_st, nr = (unsigned)K.n_r;
    if (S.lt_widx >= nl || S.st_widx >= ns || S.r_widx >= nr || S.lt_count > nl || S.st_count > ns || S.r_count > nr ||
        S.lt_nw > nl || S.lt_neg < 0 || S.lt_neg > K.n_lt || S.state < 0 || S.state > 3)
      return fail(FVAD_EFORMAT, "stream record: machine state out of range");
  }
  return FVAD_OK;
}

// Per-stream rates: a record carries its stream's rate in word o_word (three
// zero words behind it).  Nothing to do for a plan that is not on.
void save_rates(const RatePlan &p, const int32_t *streams, int n, char *body, size_t stream_bytes, long long o_word) {
  for (int i = 0; p.on() && i < n; i++) {
    const uint32_t w[4] = {p.save_rate(streams[i]), 0u, 0u, 0u};
    std::memcpy(body + (size_t)i * stream_bytes + 4 * (size_t)o_word, w, sizeof(w));
  }
}

// the rates of the records about to be restored, each checked
int restored_rates(const RatePlan &p, const int32_t *index, int n, const char *body, size_t stream_bytes,
                   long long o_word, std::vector<int> &rates, const char *off_list, const char *above_max) {
  for (int i = 0; p.on() && i < n; i++) {
    uint32_t rate;
    std::memcpy(&rate, body + (size_t)(index ? index[i] : i) * stream_bytes + 4 * (size_t)o_word, sizeof(rate));
    int r;
    if (const int bad = p.check_restored_rate(rate, &r)) return fail(FVAD_EFORMAT, bad == 1 ? off_list : above_max);
    rates.push_back((int)rate);
  }
  return FVAD_OK;
}

// blobs of engines with per-stream configs are a later change: a v1 record's
// layout and config_hash assume one config per machine (include/fvad.h)
int refuse_per_stream(const fvad_engine *e, const char *what) {
  if (!e->vadm.ps) return FVAD_OK;
  return fail(FVAD_EINVAL, std::string(what) + " is not available on an engine attached with fvad_engine_attach_vadm_ex");
}

}  // namespace

// n distinct indices in [0, n_streams)
int fvad::eng::check_stream_list(const fvad_engine *e, const int32_t *streams, int n) {
  if (n < 0 || (n > 0 && !streams)) return fail(FVAD_EINVAL, "invalid stream list");
  if (n > e->cfg.n_streams) return fail(FVAD_EINVAL, "more listed streams than the engine has (duplicates)");
  std::vector<char> seen((size_t)e->cfg.n_streams, 0);
  for (int i = 0; i < n; i++) {
    if (streams[i] < 0 || streams[i] >= e->cfg.n_streams) return fail(FVAD_EINVAL, "stream index out of range");
    if (seen[streams[i]]) return fail(FVAD_EINVAL, "duplicate stream index");
    seen[streams[i]] = 1;
  }
  return FVAD_OK;
}

// Three launches at most, each in order on the stream whose kernels own what
// it clears: st::kPitch / st::kHp are k_prep3's, on the
// prep stream; every other state word and the ring belong to the engine
// stream's kernels; the machine data to the side stream, behind the pending
// push's machine pass.  No event is added and nothing waits on the host.
extern "C" int fvad_engine_reset_streams(fvad_engine *e, const int32_t *streams, int n) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  if (const int rc = check_stream_list(e, streams, n)) return rc;
  if (n == 0) return FVAD_OK;
  if (e->vadm.on() && e->vadm.lt_full)
    return fail(FVAD_EINVAL, "fvad_engine_reset_streams is not available under FVAD_DEBUG_VADM_LT_FULL");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const bool split = e->cfg.mode != FVAD_MODE_FUSED && e->cfg.use_denoiser;
  // the previous push's machine pass sees the old state: queued first
  if (e->vadm.on() && e->vadm.pend)
    if (const int rc = vadm_flush(e, false)) return rc;
  int rc;
  // test hook FVAD_DEBUG_RESET_TIMES: this call's three timers (made on first use)
  // (a begin drops the sample its slot held kRtSlots calls ago, if still unread)
  const bool rt = e->dbg_reset_times;
  const int r0 = 3 * e->rt_next;
  if (rt) {
    e->rt_next = (e->rt_next + 1) % fvad_engine::kRtSlots;
    if ((rc = e->rt.create(r0, 3))) return rc;
  }
  fvad::ClearArgs ca{};
  ca.state = e->d_state.get();
  ca.ring = e->d_ring.get();
  ca.ring_len = e->ring_len;
  ca.n_channels = e->cfg.n_channels;
  fvad::VClearArgs va{};
  if (e->vadm.on()) {
    va.vadm = e->vadm.args;
    va.n_streams = e->cfg.n_streams;
    for (int m = 0; m < e->vadm.args.n; m++) va.init[m] = e->vadm.init[(size_t)m * e->cfg.n_streams];
  }
  if (rt && ((rc = e->rt.begin(r0, e->stream.get())) || (split && (rc = e->rt.begin(r0 + 1, e->pstream))) ||
             (e->vadm.on() && (rc = e->rt.begin(r0 + 2, e->side)))))
    return rc;
  for (int i0 = 0; i0 < n; i0 += fvad::kListMax) {
    ca.ids.n = std::min(fvad::kListMax, n - i0);
    std::memcpy(ca.ids.id, streams + i0, sizeof(int) * (size_t)ca.ids.n);
    ca.mode = split ? fvad::kClearMain : fvad::kClearAll;
    HIP_TRY(fvad::launch_stream_clear(ca, e->stream.get()));
    if (split) {
      ca.mode = fvad::kClearPrep;
      HIP_TRY(fvad::launch_stream_clear(ca, e->pstream));
    }
    if (e->vadm.on()) {
      va.ids = ca.ids;
      HIP_TRY(fvad::launch_stream_vclear(va, e->side));
    }
    if ((rc = resample_reset_streams(e, ca.ids))) return rc;  // the resamplers' tails
  }
  // clip capture: the streams' positions restart behind the appends already
  // queued, their pending clips go behind the passes already queued
  if (e->cap && (rc = capture_set_streams(e, streams, nullptr, n))) return rc;
  if (rt && ((rc = e->rt.end(r0, e->stream.get(), 0)) || (split && (rc = e->rt.end(r0 + 1, e->pstream, 1))) ||
             (e->vadm.on() && (rc = e->rt.end(r0 + 2, e->side, 2)))))
    return rc;
  return FVAD_OK;
}

extern "C" int fvad_engine_reset_times(fvad_engine *e, double *ms_avg, int *n_runs) {
  if (!e || !ms_avg) return fail(FVAD_EINVAL, "null argument");
  if (const int rc = fvad_engine_sync(e)) return rc;
  if (const int rc = e->rt.collect()) return rc;
  for (int k = 0; k < 3; k++) e->rt.read(k, &ms_avg[k], n_runs ? &n_runs[k] : nullptr);
  e->rt.clear();  // (a read starts the next measurement)
  return FVAD_OK;
}

extern "C" size_t fvad_engine_save_size(const fvad_engine *e, int n) {
  if (!e || n < 0) return 0;
  return sizeof(fvad_stream_blob_header) + (size_t)n * (size_t)header_of(e, n).stream_bytes;
}

extern "C" int fvad_stream_blob_info(const void *blob, size_t len, fvad_stream_blob_header *out) {
  return parse_blob_header(blob, len, out);
}

// gather the listed streams into one device staging buffer, one copy to the host
extern "C" int fvad_engine_save_streams(fvad_engine *e, const int32_t *streams, int n, void *blob, size_t cap) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  if (const int rc = refuse_per_stream(e, "fvad_engine_save_streams")) return rc;
  if (const int rc = check_stream_list(e, streams, n)) return rc;
  if (n == 0) return FVAD_OK;
  if (!blob || cap < fvad_engine_save_size(e, n)) return fail(FVAD_EINVAL, "blob buffer smaller than fvad_engine_save_size");
  const fvad_stream_blob_header h = header_of(e, n);
  int rc = fvad_engine_sync(e);  // every queued push, the pending machine pass as final
  if (rc) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t body = (size_t)n * (size_t)h.stream_bytes;
  if ((rc = ensure_blob(e, body))) return rc;
  fvad::XferArgs a = xfer_args(e, layout_of(e, (int)h.seg_capacity));
  for (int i0 = 0; i0 < n; i0 += fvad::kListMax) {
    a.slots.n = a.recs.n = std::min(fvad::kListMax, n - i0);
    for (int i = 0; i < a.slots.n; i++) {
      a.slots.id[i] = streams[i0 + i];
      a.recs.id[i] = i0 + i;
    }
    HIP_TRY(fvad::launch_stream_gather(a, e->stream.get()));
  }
  HIP_TRY(hipMemcpyAsync(static_cast<char *>(blob) + sizeof(h), e->d_blob.get(), body, hipMemcpyDeviceToHost, e->stream.get()));
  HIP_TRY(hipStreamSynchronize(e->stream.get()));
  // per-stream rates: each record's rate and denoised rate (the gather leaves these words alone)
  if ((e->rs && e->rs->plan.on()) || (e->ro && e->ro->plan.on())) {
    const fvad::BlobLayout lay = layout_of(e, (int)h.seg_capacity);
    char *recs = static_cast<char *>(blob) + sizeof(h);
    if (e->rs) save_rates(e->rs->plan, streams, n, recs, (size_t)h.stream_bytes, lay.o_rate);
    if (e->ro) save_rates(e->ro->plan, streams, n, recs, (size_t)h.stream_bytes, lay.o_orate);
  }
  std::memcpy(blob, &h, sizeof(h));
  return FVAD_OK;
}

// everything checked on the host, then one copy to the device and the scatter
extern "C" int fvad_engine_restore_streams(fvad_engine *e, const int32_t *streams, int n, const void *blob, size_t len,
                                           const int32_t *index) {
  if (!e) return fail(FVAD_EINVAL, "null engine");
  int rc = refuse_per_stream(e, "fvad_engine_restore_streams");
  if (rc) return rc;
  if ((rc = check_stream_list(e, streams, n))) return rc;
  if (n == 0) return FVAD_OK;
  fvad_stream_blob_header h;
  if ((rc = parse_blob_header(blob, len, &h))) return rc;
  const fvad_stream_blob_header mine = header_of(e, 0);
  if (h.mode != mine.mode || h.n_channels != mine.n_channels || h.fft_size != mine.fft_size ||
      h.use_denoiser != mine.use_denoiser || h.n_bands != mine.n_bands || h.n_machines != mine.n_machines ||
      h.state_words != mine.state_words || h.sample_rate != mine.sample_rate)
    return fail(FVAD_EFORMAT, "stream blob from an engine with another mode, channels, fft_size, bands or machines");
  if (h.reserved[0] != mine.reserved[0]) return fail(FVAD_EFORMAT, "stream blob from an engine with another input_rate");
  if (h.reserved[1] != mine.reserved[1]) return fail(FVAD_EFORMAT, "stream blob from an engine with another denoised_rate");
  if (h.config_hash != mine.config_hash) return fail(FVAD_EFORMAT, "stream blob from another engine configuration");
  if (h.model_hash != mine.model_hash) return fail(FVAD_EFORMAT, "stream blob from another model");
  if ((h.n_machines > 0) != (h.seg_capacity > 0) || h.seg_capacity > 0x7fffffffu / 32)
    return fail(FVAD_EFORMAT, "stream blob segment capacity");
  const fvad::BlobLayout lay = layout_of(e, (int)h.seg_capacity);
  if ((uint64_t)lay.words * 4 != h.stream_bytes) return fail(FVAD_EFORMAT, "stream blob record size");
  for (int i = 0; i < n; i++) {
    const long long r = index ? index[i] : i;
    if (r < 0 || r >= (long long)h.count) return fail(FVAD_EINVAL, "record index past the blob's count");
  }
  const char *body = static_cast<const char *>(blob) + h.header_bytes;
  for (int i = 0; i < n; i++) {
    const size_t r = (size_t)(index ? index[i] : i);
    std::vector<float> head((size_t)lay.words);  // (aligned copy of the record: the blob may sit anywhere)
    std::memcpy(head.data(), body + r * (size_t)h.stream_bytes, (size_t)h.stream_bytes);
    if ((rc = check_record(e, lay, head.data()))) return rc;
  }
  // per-stream rates: the records' rates, checked before a device byte is written
  std::vector<int> rec_rates, rec_orates;
  if (e->rs && (rc = restored_rates(e->rs->plan, index, n, body, (size_t)h.stream_bytes, lay.o_rate, rec_rates,
                                    "stream record: not a listed rate",
                                    "stream record: its rate exceeds this engine's input_rate_max")))
    return rc;
  if (e->ro && (rc = restored_rates(e->ro->plan, index, n, body, (size_t)h.stream_bytes, lay.o_orate, rec_orates,
                                    "stream record: not a listed denoised rate",
                                    "stream record: its denoised rate exceeds this engine's denoised_rate_max")))
    return rc;
  if ((rc = fvad_engine_sync(e))) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t bytes = (size_t)h.count * (size_t)h.stream_bytes;
  if ((rc = ensure_blob(e, bytes))) return rc;
  HIP_TRY(hipMemcpyAsync(e->d_blob.get(), body, bytes, hipMemcpyHostToDevice, e->stream.get()));
  fvad::XferArgs a = xfer_args(e, lay);
  for (int i0 = 0; i0 < n; i0 += fvad::kListMax) {
    a.slots.n = a.recs.n = std::min(fvad::kListMax, n - i0);
    for (int i = 0; i < a.slots.n; i++) {
      a.slots.id[i] = streams[i0 + i];
      a.recs.id[i] = index ? index[i0 + i] : i0 + i;
    }
    HIP_TRY(fvad::launch_stream_scatter(a, e->stream.get()));
  }
  HIP_TRY(hipStreamSynchronize(e->stream.get()));
  // the slots take their records' rates and denoised rates: the layouts of the next push follow
  if (!rec_rates.empty()) e->rs->plan.apply(streams, n, rec_rates.data());
  if (!rec_orates.empty()) e->ro->plan.apply(streams, n, rec_orates.data());
  if (e->cap) {
    // the slots continue at their records' sample counts with nothing held
    // (a blob carries no audio and no pending clip)
    std::vector<uint64_t> at((size_t)n);
    for (int i = 0; i < n; i++) {
      int ticks;
      std::memcpy(&ticks, body + (size_t)(index ? index[i] : i) * (size_t)h.stream_bytes + 4 * fvad::st::kFramesDone,
                  sizeof(ticks));
      at[i] = (uint64_t)ticks * fvad::kFrame;
    }
    if ((rc = capture_set_streams(e, streams, at.data(), n))) return rc;
    HIP_TRY(hipStreamSynchronize(capture_appender(e)));
    HIP_TRY(hipStreamSynchronize(e->side));
  }
  return FVAD_OK;
}
