/*
 * fvad.h — C ABI of the MI355X-native Formula-VAD hot path (libfvad.so).
 *
 * Plain C types only (pointers, sizes, ints, floats): a Zig host can
 * @cImport this header exactly as the reference @cImports rnnoise.h and
 * kiss_fftr.h today (src/Denoiser.zig:12-14, src/FFT.zig:5-9).
 *
 * Three layers:
 *   1. compatibility shims with the signatures and semantics the reference
 *      binds today (rnnoise_*, kiss_fftr*) — batch-of-1 calls into the HIP
 *      kernels;
 *   2. the batched engine (fvad_engine_*): thousands of concurrent 48 kHz
 *      streams per GPU, one tick = 480 samples per channel per stream;
 *   3. the host mirror of the reference pipeline / evaluator API
 *      (fvad_pipeline_*, fvad_vadm_*, fvad_eval_*), C++ above this ABI.
 *
 * Every entry point returns an int status (FVAD_OK = 0, negative = error)
 * unless noted; fvad_last_error() gives the message of the last failure on the
 * calling thread.  Ownership: the library owns device buffers and handles; the
 * caller owns every host array it passes.
 */
#ifndef FVAD_H
#define FVAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FVAD_OK 0
#define FVAD_EINVAL (-1)   /* invalid argument / size (Denoiser.zig:48-54, FFT.zig:29-31,71-81) */
#define FVAD_EDEVICE (-2)  /* HIP runtime / device error, or no device */
#define FVAD_ENOMEM (-3)   /* host or device allocation failed */
#define FVAD_EIO (-4)      /* file could not be opened */
#define FVAD_EFORMAT (-5)  /* malformed model / plan / label file */
#define FVAD_ERATE (-6)    /* sample rate != 48000 (VAD.zig:101-104) */

const char *fvad_last_error(void);
const char *fvad_version(void);

/* ------------------------------------------------------------------ */
/* 1a. rnnoise compatibility (replaces lib/rnnoise as bound by          */
/*     src/Denoiser.zig:12-14,23,36,60,69)                              */
/* ------------------------------------------------------------------ */
typedef struct fvad_model fvad_model;
typedef struct DenoiseState DenoiseState;
typedef struct fvad_model RNNModel;

/* rnnoise_create(RNNModel *model) — Denoiser.zig:23.  model == NULL selects
 * the process-wide default model (fvad_set_default_model, else the synthetic
 * model with seed 0, since rnn_data.c is not available).  Returns NULL on
 * failure (as upstream; Denoiser.zig:46 checks for it). */
DenoiseState *rnnoise_create(RNNModel *model);
/* rnnoise_destroy — Denoiser.zig:36 */
void rnnoise_destroy(DenoiseState *st);
/* rnnoise_process_frame — Denoiser.zig:60.  in/out: 480 floats in s16 scale;
 * returns the VAD probability.  Runs the HIP frame kernel (batch of 1). */
float rnnoise_process_frame(DenoiseState *st, float *out, const float *in);
/* rnnoise_get_frame_size — Denoiser.zig:69 (returns 480) */
int rnnoise_get_frame_size(void);
void fvad_set_default_model(const fvad_model *model);

/* ------------------------------------------------------------------ */
/* 1b. kissfft compatibility (replaces lib/kissfft as bound by           */
/*     src/FFT.zig:5-9,90,179-208)                                       */
/* ------------------------------------------------------------------ */
typedef struct { float r; float i; } kiss_fft_cpx;
typedef struct kiss_fftr_state *kiss_fftr_cfg;
/* kiss_fftr_alloc — FFT.zig:183,199.  Same lenmem protocol: with mem == NULL
 * or *lenmem too small it returns NULL and writes the required size into
 * *lenmem; otherwise the config lives in the caller's memory.  Forward only;
 * nfft must be even (kissfft's mixed radix: factors 4, 2, 3, 5 and generic
 * primes, as kf_factor picks them; the reference uses 2048). */
kiss_fftr_cfg kiss_fftr_alloc(int nfft, int inverse_fft, void *mem, size_t *lenmem);
/* kiss_fftr — FFT.zig:90.  timedata: nfft floats; freqdata: nfft/2+1 bins. */
void kiss_fftr(kiss_fftr_cfg cfg, const float *timedata, kiss_fft_cpx *freqdata);

/* ------------------------------------------------------------------ */
/* Models (rnn_data.c / rnn_reader.c replacement)                       */
/* ------------------------------------------------------------------ */
int fvad_model_synthetic(uint64_t seed, fvad_model **out);
int fvad_model_load_text(const char *path, fvad_model **out);
void fvad_model_free(fvad_model *m);
/* all int8 arrays in text-file order; returns the count (blob may be NULL) */
size_t fvad_model_blob(const fvad_model *m, int8_t *blob);

/* ------------------------------------------------------------------ */
/* 2. Batched engine — the hot path                                     */
/*    One engine = one GPU = a partition of streams.  A tick is 480      */
/*    samples of every channel of every stream (VAD.zig:214-251 frame    */
/*    loop, Denoiser per channel on one shared state VAD.zig:274-296,    */
/*    480 -> fft_size re-blocking VAD.zig:298-348, FFT B + band sum      */
/*    PipelineFFT.zig:88-112).                                            */
/* ------------------------------------------------------------------ */
typedef struct fvad_engine fvad_engine;

#define FVAD_MAX_CHANNELS 8
#define FVAD_MAX_BANDS 4

typedef struct {
  int n_streams;        /* streams in this engine's partition */
  int n_channels;       /* channels per stream (2 = onboard stereo) */
  int device;           /* HIP device ordinal */
  int sample_rate;      /* must be 48000 */
  int fft_size;         /* VAD.Config.fft_size: even, 2..4194304 (FFT.zig:29-31; fused mode: 480..2048,
                         * radices 2..5).  Below 480 one tick completes several windows (VAD.zig:307-347):
                         * see fvad_engine_windows_per_tick */
  int max_ticks;        /* largest n_ticks per push */
  int n_bands;          /* band sums to report per window, 1..4 */
  int band_lo[FVAD_MAX_BANDS]; /* inclusive FFT-B bin ranges (FFT.freqToBin) */
  int band_hi[FVAD_MAX_BANDS];
  int want_denoised;    /* keep denoised PCM (VAD.zig temp_denoiser_segment); 2: keep it on the device only, for a
                         * capture of it (fvad_engine_enable_capture_ex): computed as with 1, never copied to the
                         * host -- no pinned slot buffer, and fvad_outputs.denoised is FVAD_EINVAL */
  int mode;             /* FVAD_MODE_STAGED (default), FVAD_MODE_FUSED, FVAD_MODE_FP16, FVAD_MODE_FP16_FUSED or
                         * FVAD_MODE_F32_FAST */
  int use_denoiser;     /* VAD.Config.use_denoiser (default 1).  0: fft_size frames of raw input go
                         * straight to FFT B (VAD.zig:206-212,239-249); per-tick vad / ratio are -1,
                         * the window ratio is preAnalyzeSegment's over the frame, window vad -1 */
  int want_spectrum;    /* 1: FFT B also writes every completed window's magnitudes of the bins
                         * spec_lo..spec_hi (section 2c below; default 0: nothing of it exists) */
  int spec_lo, spec_hi; /* inclusive FFT-B bin range, 0 <= spec_lo <= spec_hi <= fft_size / 2 (default 0, 1024);
                         * read only with want_spectrum */
  /* ABI note: want_spectrum, spec_lo and spec_hi stand in front of input_rate, which stays the struct's
   * last field; a binding that declares the struct itself must insert them here */
  /* ABI note (r5): the trailing `unsigned cu_mask[8]` of earlier builds was removed; a binding
   * compiled against them must drop it (fvad_engine_config_default fills every field) */
  int denoised_rate_max; /* read only with denoised_rate = FVAD_DENOISED_RATE_PER_STREAM (section 2d-ps below):
                         * the highest rate a stream's denoised PCM may take, 8000, 16000, 24000, 32000,
                         * 44100, 48000 or 96000; it bounds the device's output rows and the pinned slots.
                         * Default 0; any other value with another denoised_rate is FVAD_ERATE */
  /* ABI note: denoised_rate_max stands in front of input_rate_max, denoised_rate and input_rate, which
   * stay the struct's last three fields; a binding that declares the struct itself must insert it here */
  int input_rate_max;   /* read only with input_rate = FVAD_INPUT_RATE_PER_STREAM (section 2b-ps below): the
                         * highest rate a stream of the engine may take, 8000, 16000, 24000, 32000, 44100,
                         * 48000 or 96000; it bounds the raw staging buffers and the pinned slots.  Default
                         * 0; any other value with another input_rate is FVAD_ERATE */
  /* ABI note: input_rate_max stands in front of denoised_rate and input_rate, which stay the struct's
   * last two fields; a binding that declares the struct itself must insert it here */
  int denoised_rate;    /* the rate of the denoised PCM the engine returns: 0 or 48000 (default 0) for the
                         * 48 kHz signal, or 8000, 16000, 24000, 32000, 44100, 96000 for an engine that
                         * brings every push's denoised rows to that rate on the device (section 2d below);
                         * FVAD_ERATE otherwise.  A listed rate needs want_denoised = 1 and use_denoiser = 1
                         * (FVAD_EINVAL), or FVAD_DENOISED_RATE_PER_STREAM for an engine whose streams each
                         * get their denoised PCM at a rate of their own (section 2d-ps; want_denoised = 1 and
                         * use_denoiser = 1, FVAD_EINVAL otherwise).  Independent of input_rate */
  /* ABI note: denoised_rate stands in front of input_rate, which stays the struct's last field; a
   * binding that declares the struct itself must insert it here */
  int input_rate;      /* the rate of the pushed samples: 0 or 48000 (default 0) for 48 kHz input, or 8000,
                         * 16000, 24000, 32000, 44100, 96000 for an engine that resamples every push to
                         * 48 kHz on the device (section 2b below), or FVAD_INPUT_RATE_PER_STREAM for an
                         * engine whose streams each have a rate of their own (section 2b-ps);
                         * FVAD_ERATE otherwise.  sample_rate, the pipeline's rate, stays 48000 */
} fvad_engine_config;

/* fvad_engine_config.input_rate: every stream has its own input rate (section 2b-ps) */
#define FVAD_INPUT_RATE_PER_STREAM (-1)
/* fvad_engine_config.denoised_rate: every stream has its own denoised rate (section 2d-ps) */
#define FVAD_DENOISED_RATE_PER_STREAM (-1)

/* staged: time-parallel frame kernels + a thin per-stream recurrence kernel;
 * fused: one workgroup runs every frame of a stream (lower memory); staged
 * and fused give identical results (bit-exact with the CPU reference).
 * fp16: BASELINE configs[4] -- the staged pipeline with the GRU stack on the
 * matrix cores (int8 weights as f16, f16 inputs, f32 accumulation): within
 * the stated tolerance (vad |d| <= 2e-2), not bit-exact.
 * fp16_fused: configs[4]'s fused FFT -> feature -> GRU kernel -- fp16 with
 * the pitch-spectrum FFT and its features computed inside the GRU kernel
 * (k_fused16 replaces k_pspecw + k_gru16); results identical to fp16's.
 * f32_fast: the staged pipeline in f32 with every term of the GRU / dense
 * sums a fused multiply-add (k_rnn3f replaces k_rnn3); everything before the
 * GRU stack -- spectra, features, pitch, volume ratios -- stays bit-exact, as
 * do FFT B and the window bookkeeping.  Within the fp32 tolerance (vad |d| <= 1e-4, denoised rel-RMS
 * <= 1e-5, band sums rel <= 1e-5, identical segments), not bit-exact.  With
 * use_denoiser = 0 it is the staged path. */
#define FVAD_MODE_STAGED 0
#define FVAD_MODE_FUSED 1
#define FVAD_MODE_FP16 2
#define FVAD_MODE_FP16_FUSED 3
#define FVAD_MODE_F32_FAST 4
#define FVAD_MAX_TIMES 16

void fvad_engine_config_default(fvad_engine_config *cfg, int n_streams, int n_channels);

int fvad_engine_create(const fvad_engine_config *cfg, const fvad_model *model, fvad_engine **out);
void fvad_engine_destroy(fvad_engine *e);
/* reset every stream to a freshly created rnnoise / VAD state */
int fvad_engine_reset(fvad_engine *e);

/* Stream lifecycle: reset, save and restore single streams of a live engine
 * (a serving host's streams start, stop and move at different times).
 * `streams` lists n distinct indices in [0, n_streams); n == 0 is a no-op
 * (FVAD_OK).  A duplicate or out-of-range index is FVAD_EINVAL and nothing is
 * touched.
 *
 * fvad_engine_reset_streams: the listed streams become exactly what
 * fvad_engine_reset makes them -- rnnoise state, high-pass memory, pitch
 * history, the tick / sample counters (sample indices restart at 0), the
 * window volume accumulator, the re-block ring rows and, per attached machine,
 * its initial state, empty rolling averages and an empty segment list; every
 * other stream is untouched.  Every engine mode.  It takes effect between the
 * pushes submitted before the call and those submitted after it: earlier
 * pushes still in flight (submit without collect, run_resident without sync)
 * keep their outputs, their device VADMachine pass included.  It never waits
 * for the device: a few small kernels go onto the engine's own streams, each
 * behind the work that owns what it clears, so a host may call it between
 * every pair of pushes.  The position in a resident input cycle
 * (fvad_engine_load_synthetic_ex) belongs to the engine, not to a stream, and
 * stays.  While the test hook FVAD_DEBUG_VADM_LT_FULL is set on an engine
 * with machines it returns FVAD_EINVAL (that hook's initial state is a
 * whole-engine timing fixture).
 *
 * fvad_engine_save_streams / fvad_engine_restore_streams move streams between
 * engines as a blob: a checkpoint, or a migration to another slot, engine or
 * GPU.  Both are sync points like fvad_engine_segments (they wait for every
 * queued push and run the pending machine pass as final) and may block.  A
 * blob restores into an engine that may differ in n_streams, max_ticks,
 * device, seg_capacity and slot, and must agree in mode, n_channels, fft_size,
 * use_denoiser, sample_rate, the band table, the machine configs (count and
 * every field) and the model.  Record index[i] of the blob (i when index is
 * NULL) goes to slot streams[i]; the stream then continues as if it had never
 * moved.  A target with a smaller seg_capacity keeps the first seg_capacity
 * segments and the true total, as the list does on overflow.
 *
 * A restore validates everything on the host before it writes a device byte:
 * the header against len, every compatibility field and both hashes, the
 * counters and write indices of the records it will use (FVAD_EFORMAT), and
 * the stream list and index (FVAD_EINVAL).  After an error the engine is
 * exactly as it was.  save returns FVAD_EINVAL when cap <
 * fvad_engine_save_size(e, n).
 *
 * Blob layout (little endian): a fvad_stream_blob_header of header_bytes
 * (128), then count records of stream_bytes each.  A record, in 32-bit words,
 * every section padded to 4 words:
 *   the stream's state record (state_words words);
 *   per channel, P = (fft_size + 2) & ~3 words: the pending part of the
 *     current FFT window in sample order -- samples % fft_size of them (the
 *     state record holds the counter), zeros after.  Not the ring itself: the
 *     ring is indexed by absolute sample mod its length, which depends on
 *     max_ticks;
 *   per machine: its state (40 words), the long-term average's entries
 *     (padded to 4), the short-term's, the volume ratio's, and seg_capacity
 *     segments of 6 words (min(total, seg_capacity) stored, zeros after). */
#define FVAD_STREAM_BLOB_MAGIC 0x42535646u /* "FVSB" */
#define FVAD_STREAM_BLOB_VERSION 1
#define FVAD_STREAM_BLOB_HEADER_BYTES 128
typedef struct {
  uint32_t magic;         /*   0 FVAD_STREAM_BLOB_MAGIC */
  uint32_t version;       /*   4 FVAD_STREAM_BLOB_VERSION */
  uint32_t header_bytes;  /*   8 FVAD_STREAM_BLOB_HEADER_BYTES */
  uint32_t count;         /*  12 stream records that follow */
  uint64_t stream_bytes;  /*  16 bytes per record */
  uint32_t mode;          /*  24 the saving engine's config ... */
  uint32_t n_channels;    /*  28 */
  uint32_t fft_size;      /*  32 */
  uint32_t use_denoiser;  /*  36 */
  uint32_t n_bands;       /*  40 */
  uint32_t n_machines;    /*  44 attached device VADMachines */
  uint32_t seg_capacity;  /*  48 of the saving engine (0 without machines) */
  uint32_t state_words;   /*  52 32-bit words of a stream's state record */
  uint64_t config_hash;   /*  56 FNV-1a 64 of mode, n_channels, fft_size, use_denoiser, sample_rate,
                           *     n_bands, the band ranges, n_machines and every machine config field */
  uint64_t model_hash;    /*  64 FNV-1a 64 of fvad_model_blob's bytes */
  uint32_t sample_rate;   /*  72 */
  uint32_t reserved[13];  /*  76 [0]: the saving engine's input_rate when it resamples (its records then end
                           *     with the resampler's tails, per channel (taps_per_phase + 2) & ~3 words, and
                           *     config_hash covers the rate), 0 otherwise; a blob restores only into an
                           *     engine of the same input_rate; 0xFFFFFFFF: a per-stream engine, section
                           *     2b-ps).  [1]: the saving engine's denoised_rate when it
                           *     is a listed rate (its records then end with the output resampler's tails, behind
                           *     the input tails if there are any, per channel (K + 2) & ~3 words, K section 2d's
                           *     taps_per_phase, and config_hash covers the rate), 0 otherwise; a blob restores
                           *     only into an engine of the same denoised_rate; 0xFFFFFFFF: an engine of
                           *     per-stream denoised rates, section 2d-ps.  [2..12]: zero */
} fvad_stream_blob_header;
int fvad_engine_reset_streams(fvad_engine *e, const int32_t *streams, int n);
/* bytes a save of n streams needs (0 for a NULL engine or n < 0) */
size_t fvad_engine_save_size(const fvad_engine *e, int n);
int fvad_engine_save_streams(fvad_engine *e, const int32_t *streams, int n, void *blob, size_t cap);
int fvad_engine_restore_streams(fvad_engine *e, const int32_t *streams, int n, const void *blob, size_t len,
                                const int32_t *index);
/* Parses and validates a blob's header on the host alone (no GPU): magic,
 * version, header_bytes, and header_bytes + count * stream_bytes <= len;
 * FVAD_EFORMAT otherwise.  *out receives the header. */
int fvad_stream_blob_info(const void *blob, size_t len, fvad_stream_blob_header *out);

/* Per-tick outputs, host arrays owned by the caller, indexed [tick][stream]...
 * Any pointer may be NULL to skip that output.  The window outputs have W =
 * fvad_engine_windows_per_tick(e) slots per (tick, stream): W = 1 for fft_size
 * >= 480 (the layout is then [ticks][streams]...), more below 480, where one
 * 480-sample frame fills several FFT buffers (VAD.zig:307-347); slot w < the
 * tick's win_flag holds the tick's w-th completed window, in sample order. */
typedef struct {
  float *vad;          /* [ticks][streams]  min over channels of rnnoise vad (VAD.zig:284-293) */
  float *ratio;        /* [ticks][streams]  preAnalyzeSegment volume ratio (VAD.zig:253-272) */
  int32_t *win_flag;   /* [ticks][streams]  FFT-B windows completed in this tick (0..W; 0 or 1 when W = 1) */
  float *win_ratio;    /* [ticks][streams][W]  share-weighted window volume ratio (VAD.zig:319-325) */
  float *win_vad;      /* [ticks][streams][W]  window vad = last frame's vad (VAD.zig:330) */
  float *band;         /* [ticks][streams][W][channels][n_bands] band sums (PipelineFFT.zig:99-112); 0 in
                        * slots without a window */
  float *denoised;     /* [ticks][streams][channels][480] normalised denoised PCM (want_denoised); with
                        * denoised_rate [ticks][streams][channels][fvad_engine_denoised_frame(e)] (section 2d);
                        * with per-stream denoised rates packed [ticks][streams][channels][rate(stream) / 100],
                        * n_ticks * offsets[n_streams] floats (section 2d-ps) */
} fvad_outputs;

/* W, the window slots per (tick, stream) of fvad_outputs: 1 for fft_size >=
 * 480, else floor((fft_size - 1 + 480) / fft_size) -- the most windows one
 * tick can complete */
int fvad_engine_windows_per_tick(const fvad_engine *e);

/* pcm: host [ticks][streams][channels][480] normalised f32.  ticks_valid
 * (nullable): stream s only consumes its first ticks_valid[s] ticks (ragged
 * end of file; the rest of its slots are ignored).  Synchronous. */
int fvad_engine_push(fvad_engine *e, const float *pcm, int n_ticks, const int32_t *ticks_valid,
                     fvad_outputs *out);
/* The same with last_tick_samples (nullable): stream s's last valid tick holds
 * only last_tick_samples[s] (1..480) real samples, the rest of its slot is
 * ignored.  Only use_denoiser = 0 engines accept a partial tick: that path
 * reads fft_size frames (VAD.zig:206-220) and counts samples, so a window
 * completes as soon as its last sample is in, whatever the push sizes; with
 * the denoiser a frame needs all 480 samples (FVAD_EINVAL otherwise). */
int fvad_engine_push_ex(fvad_engine *e, const float *pcm, int n_ticks, const int32_t *ticks_valid,
                        const int32_t *last_tick_samples, fvad_outputs *out);

/* Streaming ingest (the simulator's read loop, SimulationInstance.zig:194-203,
 * reads the next chunk while the pipeline works on the last one).  Up to
 * FVAD_MAX_IN_FLIGHT pushes may be in flight: submit copies the input into a
 * pinned slot (or takes it in place when pcm is the pointer
 * fvad_engine_input_slot returned), queues the H2D copy on its own stream --
 * overlapping the earlier pushes' kernels; it waits only until the device
 * input buffer it fills has been read by the k_prep3 of the push two before --
 * then the kernels and the output copies into pinned memory, and returns
 * without waiting.  collect returns the outputs of the oldest submitted push
 * (blocking until they are on the host; out may be NULL, *n_ticks its tick
 * count).  submit fails with FVAD_EINVAL while FVAD_MAX_IN_FLIGHT pushes are
 * uncollected. */
#define FVAD_MAX_IN_FLIGHT 3
/* the pinned [max_ticks][streams][channels][480] slot the next submit reads;
 * blocks until that slot's previous copy to the device finished; NULL on error */
float *fvad_engine_input_slot(fvad_engine *e);
int fvad_engine_submit(fvad_engine *e, const float *pcm, int n_ticks, const int32_t *ticks_valid);
int fvad_engine_submit_ex(fvad_engine *e, const float *pcm, int n_ticks, const int32_t *ticks_valid,
                          const int32_t *last_tick_samples);
int fvad_engine_collect(fvad_engine *e, fvad_outputs *out, int *n_ticks);
/* 16-bit PCM ingest (onboard WAV audio is 16-bit): the same push as
 * fvad_engine_submit_ex on the samples k / 32768.0f (libsndfile's short ->
 * float normalisation, as the reference's sf_read_float gives
 * AudioPipeline.pushSamples, src/AudioPipeline.zig:86-120; exact in f32), so
 * the outputs are bit-identical to a float submit of those samples.  Half the
 * host-to-device bytes; the conversion runs on the device: staged engines
 * with the denoiser read the 16-bit samples in k_prep3 itself, the others
 * convert on the copy stream (k_pcm16).  The slot and the submit/collect
 * rules are fvad_engine_input_slot's and fvad_engine_submit's. */
int16_t *fvad_engine_input_slot_i16(fvad_engine *e);
int fvad_engine_submit_i16(fvad_engine *e, const int16_t *pcm, int n_ticks, const int32_t *ticks_valid,
                           const int32_t *last_tick_samples);

/* Device-resident variants for benchmarking / zero-copy producers. */
/* allocate a device input of n_ticks and fill it with the synthetic generator */
int fvad_engine_load_synthetic(fvad_engine *e, int n_ticks, uint32_t stream_id_base);
/* n_pushes distinct pushes of n_ticks resident in HBM: stream s's first
 * n_pushes * n_ticks ticks of fvad_synth_stream(stream_id_base + s) (generated
 * at that length); run_resident cycles through them, starting at push 0 */
int fvad_engine_load_synthetic_ex(fvad_engine *e, int n_ticks, int n_pushes, uint32_t stream_id_base);
/* the resident push the next run_resident reads */
int fvad_engine_resident_seek(fvad_engine *e, int push);
/* run one push over the resident device input (the next one of the cycle),
 * async on the engine stream */
int fvad_engine_run_resident(fvad_engine *e, int n_ticks);
int fvad_engine_sync(fvad_engine *e);
/* average per-launch kernel durations (ms) of the timed resident runs,
 * measured with HIP events on the engine's stream.  ms_avg holds
 * FVAD_MAX_TIMES doubles: [0] whole push (GPU time from its first to its last
 * kernel; staged kernels may overlap), [1 + i] kernel i (names below).  With
 * device VADMachines the last two names are k_vadm_hbm (a push's machine run
 * beside the next push) and k_vadm_par (the push whose machine ran at a sync
 * point, nothing queued behind it), each averaged over its own runs. */
int fvad_engine_kernel_times(fvad_engine *e, double *ms_avg, int *n_runs);
/* name of kernel i of this engine's mode, NULL past the last one */
const char *fvad_engine_kernel_name(const fvad_engine *e, int i);
int fvad_engine_clear_times(fvad_engine *e);
/* copy outputs of the last resident run to host */
int fvad_engine_fetch(fvad_engine *e, int n_ticks, fvad_outputs *out);

/* ------------------------------------------------------------------ */
/* 2b. Input resampling (fvad_engine_config.input_rate)                 */
/* ------------------------------------------------------------------ */
/* An engine created with input_rate R in {8000, 16000, 24000, 32000, 44100,
 * 96000} takes its pushes at R and resamples them to 48 kHz on the device
 * (k_resample, the first kernel of the push) in front of the unchanged
 * pipeline.  A tick stays 10 ms: frame_in = R / 100 samples per channel in,
 * 480 out.  Every input shape of section 2 becomes
 * [ticks][streams][channels][frame_in] -- fvad_engine_push[_ex],
 * fvad_engine_submit[_ex], fvad_engine_submit_i16 and both input slots;
 * the outputs keep their shapes (denoised is the 48 kHz signal, unless
 * denoised_rate, section 2d, asks for another rate).
 *
 * The resampler, to the bit: g = gcd(48000, R), L = 48000 / g, M = R / g,
 * K = 48 max(1, ceil(M / L)) taps per phase; the prototype of N = L K taps at
 * the rate Fp = L R is a Kaiser-windowed sinc, designed in f64: A = 80,
 * beta = 0.1102 (A - 8.7), df = (A - 8) / (2.285 (N - 1)) Fp / (2 pi),
 * f_stop = min(R, 48000) / 2, fc = f_stop - df / 2,
 * proto[j] = sinc(2 fc / Fp (j - (N - 1) / 2)) I0(beta sqrt(1 - (2 j / (N - 1) - 1)^2)) / I0(beta),
 * scaled to sum L; taps[p][k] = (float)proto[k L + p].  Output r (0..479) of
 * tick t: i = floor(r M / L), p = r M mod L, acc = 0.0f, then for k = 0 .. K - 1
 * acc = acc + taps[p][k] * x[t frame_in + i - k], product and sum each rounded
 * to f32, nothing fused.  x before a stream's first sample is 0; across pushes
 * it continues from the stream's last K - 1 input samples (kept on the device;
 * reset, saved and restored with the stream).  16-bit input k is
 * (float)k / 32768 first.  Only a stream's ticks_valid ticks are consumed.
 *
 * Every sample index the engine reports -- segments, events, clips -- counts
 * 48 kHz samples of the resampled signal.  The position in the source is
 * index * R / 48000 - delay * R / 48000 source samples, delay =
 * (N - 1) / (2 M) in 48 kHz samples (fvad_resample_info).
 *
 * Not available on a resampling engine (FVAD_EINVAL, the engine unchanged): a
 * partial last tick (last_tick_samples other than frame_in),
 * fvad_engine_load_synthetic[_ex] and fvad_engine_run_resident (the generator
 * is 48 kHz).  The rnnoise compat path, fvad_pipeline_*, fvad_multi_*, the
 * simulator and fvad_sweep_* stay 48 kHz only (FVAD_ERATE). */
typedef struct {
  int input_rate;
  int L, M;            /* 48000 / g and input_rate / g */
  int taps_per_phase;  /* K */
  int frame_in;        /* input samples per tick and channel */
  double delay;        /* the filter's group delay in 48 kHz samples, (L K - 1) / (2 M) */
} fvad_resample_desc;
/* host only (no GPU).  FVAD_ERATE for a rate off the list (0 and 48000 too) */
int fvad_resample_info(int input_rate, fvad_resample_desc *out);
/* the [L][K] tap table; copies min(count, cap) floats (out may be NULL) and
 * returns the count, 0 for a rate off the list */
size_t fvad_resample_taps(int input_rate, float *out, size_t cap);
/* One channel on the host, the arithmetic above (the kernel's mirror): in is
 * n_ticks * frame_in samples, out n_ticks * 480.  tail: the K - 1 samples
 * before in[0], read and replaced by the last K - 1 of this call's input
 * (carry it to continue a stream); NULL: zeros, nothing kept. */
int fvad_resample_host(int input_rate, const float *in, size_t n_ticks, float *tail, float *out);
/* input samples per tick and channel: frame_in, 480 on a plain engine (FVAD_EINVAL on a
 * per-stream engine, section 2b-ps) */
int fvad_engine_input_frame(const fvad_engine *e);
/* The 48 kHz device input of the last push, [ticks][streams][channels][480]:
 * what k_resample wrote (zeros in the ticks past a stream's ticks_valid).  A
 * sync point.  Resampling engines only (FVAD_EINVAL otherwise). */
int fvad_engine_fetch_input(fvad_engine *e, int n_ticks, float *pcm48);
/* average event time (ms) of a push's resample launches (k_resample and the
 * tail update behind it) and the pushes measured; a sync point */
int fvad_engine_resample_times(fvad_engine *e, double *ms_avg, int *n_runs);

/* ------------------------------------------------------------------ */
/* 2b-ps. Per-stream input rates (input_rate = FVAD_INPUT_RATE_PER_STREAM) */
/* ------------------------------------------------------------------ */
/* An engine created with input_rate = FVAD_INPUT_RATE_PER_STREAM and
 * input_rate_max = Rmax carries streams of different input rates at once.  A
 * stream's rate is one of 8000, 16000, 24000, 32000, 44100, 48000, 96000 and
 * at most Rmax; every stream starts at Rmax.  Each stream is resampled to
 * 48 kHz exactly as a section-2b engine of its rate resamples it (the same
 * taps, arithmetic and K - 1 samples of history).  A 48000 stream is not
 * resampled: float samples pass by their bits, 16-bit samples k as
 * (float)k * (1.0f / 32768.0f), and it has no history.  The input side only:
 * clips are the engine's, as before, and the denoised PCM's rate is a setting
 * of its own, per engine (section 2d) or per stream (section 2d-ps).
 *
 * Layout.  A push is packed [tick][stream][channel][rate(stream) / 100]:
 * offsets[s] is stream s's first sample inside a tick, offsets[n_streams] a
 * tick's length in samples (fvad_input_layout; fvad_engine_input_layout is the
 * same over the engine's current rates).  fvad_engine_push[_ex],
 * fvad_engine_submit[_ex], fvad_engine_submit_i16 and both input slots carry
 * n_ticks * offsets[n_streams] samples in that layout; a pinned slot holds
 * max_ticks * n_streams * n_channels * Rmax / 100 samples.
 * fvad_engine_input_frame is FVAD_EINVAL: no single frame length exists.
 *
 * fvad_engine_set_stream_rates gives the n listed streams the listed rates.
 * Indices must be distinct and in range (FVAD_EINVAL), every rate a listed one
 * or 48000 and at most Rmax (FVAD_ERATE); on either error nothing is touched.
 * n == 0 is a no-op.  It never waits for the device and takes effect between
 * the pushes submitted before it and those submitted after it: pushes still in
 * flight (submitted, not collected) keep the rates, the layout and the
 * history they were submitted with.  Each listed stream's resampler history
 * becomes zeros -- also when its rate did not change; nothing else of the
 * stream and nothing of any other stream is touched (a host that wants a
 * fresh stream also calls fvad_engine_reset_streams).  On any other engine it
 * is FVAD_EINVAL.  fvad_engine_stream_rates returns the rates the next
 * submitted push will use.
 *
 * As on a section-2b engine: last_tick_samples must be whole ticks, each
 * stream's value its own rate / 100 (FVAD_EINVAL otherwise); ticks_valid,
 * fvad_engine_fetch_input (48 kHz rows, [tick][stream][channel][480]) and
 * fvad_engine_resample_times (all of a push's resample launches together)
 * work unchanged, and every reported sample index counts 48 kHz samples.
 * Resident input is refused as there: fvad_engine_load_synthetic[_ex] and
 * fvad_engine_run_resident are FVAD_EINVAL.  fvad_engine_reset and
 * fvad_engine_reset_streams zero the history; the streams keep their rates.
 *
 * Stream blobs.  A per-stream engine's header carries reserved[0] =
 * 0xFFFFFFFF; its records end with n_channels rows of 96 words (the
 * stream's K - 1 history samples, zeros after) and 4 words behind them (the
 * stream's rate, then zeros).  Such blobs move only between per-stream
 * engines (FVAD_EFORMAT otherwise, as between engines of different
 * input_rate); config_hash covers the marker, not input_rate_max.  A restore
 * gives the target slot its record's rate, so the layout of the next push
 * changes; a record whose rate exceeds the target's input_rate_max is
 * FVAD_EFORMAT, found before anything is written. */
/* host only (no GPU): offsets[n_streams + 1] of the packed layout above.
 * FVAD_ERATE for a rate that is neither listed nor 48000 */
int fvad_input_layout(const int *rates, int n_streams, int n_channels, int64_t *offsets /* n_streams + 1 */);
int fvad_engine_input_layout(const fvad_engine *e, int64_t *offsets /* n_streams + 1 */);
int fvad_engine_set_stream_rates(fvad_engine *e, const int *streams, int n, const int *rates);
int fvad_engine_stream_rates(const fvad_engine *e, int *rates /* n_streams */);

/* ------------------------------------------------------------------ */
/* 2c. Window spectra (fvad_engine_config.want_spectrum)                */
/* ------------------------------------------------------------------ */
/* An engine created with want_spectrum keeps, beside the band sums, the
 * magnitude spectrum of every completed window: n_spec = spec_hi - spec_lo + 1
 * f32 per channel, bin k = sqrtf(re * re + im * im) * norm of kiss_fftr's
 * output over the Hann-windowed fft_size samples -- the reference's
 * Spectrogram.compute at hop_size == fft_size (Spectrogram.zig:30-94), and the
 * very values FFT B sums into the bands: a band sum is
 * acc = 0.0f; for k = lo .. hi: acc += spectrum[k], in f32, to the bit.
 * Every staged-family mode, with or without the denoiser or input_rate;
 * FVAD_MODE_FUSED with want_spectrum is FVAD_EINVAL, as is a bad range.  The
 * tap has no per-stream state and changes no other output; an engine without
 * it allocates and launches what it always did.
 *
 * The device holds the spectra of one push, [ticks][streams][W][channels]
 * [n_spec] (fvad_outputs.band's layout with n_spec for n_bands, W =
 * fvad_engine_windows_per_tick): slot w < win_flag of a valid tick is the
 * tick's w-th completed window, every other slot reads 0.  The next launched
 * push overwrites them: fvad_outputs, the pinned output slots and the output
 * log carry no spectra.
 *
 * fvad_engine_spectrum_bins: n_spec and (nullable) the range; 0 when the tap
 * is off.  fvad_engine_fetch_spectrum: a sync point; the first n_ticks ticks
 * of the last launched push's spectra -- of fvad_engine_push[_ex], of
 * fvad_engine_run_resident, or of the only outstanding submit once collected.
 * FVAD_EINVAL while a submitted push is uncollected, without the tap, and for
 * n_ticks < 1 or above that push's ticks. */
int fvad_engine_spectrum_bins(const fvad_engine *e, int *lo, int *hi);
int fvad_engine_fetch_spectrum(fvad_engine *e, int n_ticks, float *out);

/* ------------------------------------------------------------------ */
/* 2d. Output rate of the denoised PCM (fvad_engine_config.denoised_rate) */
/* ------------------------------------------------------------------ */
/* An engine created with denoised_rate R in {8000, 16000, 24000, 32000, 44100,
 * 96000} (want_denoised = 1, use_denoiser = 1, any mode, any input_rate)
 * returns its denoised PCM at R: k_resample_out, queued behind the push's last
 * writer of the 48 kHz denoised rows, brings them to R on the device, and
 * every place that delivers denoised PCM -- fvad_engine_push[_ex],
 * fvad_engine_submit* / fvad_engine_collect, fvad_engine_fetch -- delivers
 * [ticks][streams][channels][frame_out], frame_out = R / 100 samples per tick
 * and channel (fvad_engine_denoised_frame).  Every other output is what an
 * engine without the field gives, and segments, events and clips keep counting
 * (and holding) the 48 kHz signal.  Ticks past a stream's ticks_valid are
 * zeros.
 *
 * The downsampler, to the bit: g = gcd(48000, R), L = R / g, M = 48000 / g,
 * K = 48 max(1, ceil(M / L)) taps per phase; the prototype of N = L K taps at
 * the rate Fp = 48000 L is section 2b's Kaiser-windowed sinc with 48000 as the
 * source rate, designed in f64: A = 80, beta = 0.1102 (A - 8.7),
 * df = (A - 8) / (2.285 (N - 1)) Fp / (2 pi), f_stop = min(R, 48000) / 2,
 * fc = f_stop - df / 2,
 * proto[j] = sinc(2 fc / Fp (j - (N - 1) / 2)) I0(beta sqrt(1 - (2 j / (N - 1) - 1)^2)) / I0(beta),
 * scaled to sum L; taps[p][k] = (float)proto[k L + p].  A tick stays 10 ms:
 * 480 L / M = frame_out, so every tick starts at phase 0.  Output r
 * (0 .. frame_out - 1) of tick t: i = floor(r M / L), p = r M mod L,
 * acc = 0.0f, then for k = 0 .. K - 1 acc = acc + taps[p][k] * y[480 t + i - k],
 * product and sum each rounded to f32, nothing fused or re-associated.  y is
 * the stream's 48 kHz denoised signal: 0 before the stream's first sample;
 * across pushes it continues from the row's last K - 1 denoised samples (kept
 * on the device; reset, saved and restored with the stream; K - 1 <= 480, so
 * they lie inside one tick).  Only a stream's ticks_valid ticks are consumed.
 *
 *   R      L    M    K   frame_out  delay in 48 kHz samples, (L K - 1) / (2 L)
 *   8000   1    6    288    80      143.5
 *   16000  1    3    144   160       71.5
 *   24000  1    2     96   240       47.5
 *   32000  2    3     96   320       47.75
 *   44100  147  160   96   441       14111 / 294
 *   96000  2    1     48   960       23.75
 *
 * The rnnoise compat path, fvad_pipeline_*, fvad_multi_* and the simulator
 * stay 48 kHz. */
typedef struct {
  int rate;
  int L, M;            /* rate / g and 48000 / g */
  int taps_per_phase;  /* K */
  int frame_out;       /* output samples per tick and channel */
  double delay;        /* the filter's group delay in 48 kHz samples, (L K - 1) / (2 L) */
} fvad_resample_out_desc;
/* host only (no GPU).  FVAD_ERATE for a rate off the list (0 and 48000 too) */
int fvad_resample_out_info(int rate, fvad_resample_out_desc *out);
/* the [L][K] tap table; copies min(count, cap) floats (out may be NULL) and
 * returns the count, 0 for a rate off the list */
size_t fvad_resample_out_taps(int rate, float *out, size_t cap);
/* One channel on the host, the arithmetic above (the kernel's mirror): in48 is
 * n_ticks * 480 samples, out n_ticks * frame_out.  tail: the K - 1 samples
 * before in48[0], read and replaced by the last K - 1 of this call's input
 * (carry it to continue a stream); NULL: zeros, nothing kept. */
int fvad_resample_out_host(int rate, const float *in48, size_t n_ticks, float *tail, float *out);
/* denoised samples per tick and channel: frame_out, 480 on a plain engine */
int fvad_engine_denoised_frame(const fvad_engine *e);
/* average event time (ms) of a push's two output-resample launches
 * (k_resample_out and the tail update behind it) and the pushes measured; a
 * sync point.  denoised_rate engines only (FVAD_EINVAL otherwise). */
int fvad_engine_resample_out_times(fvad_engine *e, double *ms_avg, int *n_runs);

/* ------------------------------------------------------------------ */
/* 2d-ps. Per-stream denoised rates (denoised_rate = FVAD_DENOISED_RATE_PER_STREAM) */
/* ------------------------------------------------------------------ */
/* An engine created with denoised_rate = FVAD_DENOISED_RATE_PER_STREAM and
 * denoised_rate_max = Rmax (want_denoised = 1 and use_denoiser = 1, FVAD_EINVAL
 * otherwise -- want_denoised = 2 too; any mode; any input_rate, also
 * FVAD_INPUT_RATE_PER_STREAM: the two sets of rates are independent) returns
 * every stream's denoised PCM at that stream's own rate.  A stream's rate is
 * one of 8000, 16000, 24000, 32000, 44100, 48000, 96000 and at most Rmax;
 * every stream starts at Rmax.  A stream at a listed rate R is downsampled
 * exactly as section 2d specifies for R (the same taps, arithmetic and K - 1
 * samples of history); a 48000 stream's rows are the 48 kHz denoised rows bit
 * for bit.  Ticks past a stream's ticks_valid are zeros.  Every other output,
 * segment, event and clip is what a plain engine gives.
 *
 * Layout.  The denoised PCM is packed [tick][stream][channel][rate(stream) /
 * 100]: offsets[s] is stream s's first sample inside a tick, offsets[n_streams]
 * a tick's length in samples (fvad_denoised_layout, fvad_input_layout's
 * arithmetic; fvad_engine_denoised_layout is the same over the engine's current
 * rates: the layout the next submitted push will be delivered in).
 * fvad_engine_push[_ex], fvad_engine_submit* / fvad_engine_collect,
 * fvad_engine_fetch and the pinned output slots deliver n_ticks *
 * offsets[n_streams] floats in that layout, which is what fvad_outputs.denoised
 * must hold; the pinned slots and the device's output rows hold max_ticks *
 * n_streams * n_channels * Rmax / 100.  A collected push is delivered in the
 * layout the engine had when it was submitted: a host that changes rates with
 * pushes in flight takes fvad_engine_denoised_layout at every submit and keeps
 * it with the push.  fvad_engine_denoised_frame is FVAD_EINVAL: no single frame
 * length exists.
 *
 * fvad_engine_set_stream_denoised_rates gives the n listed streams the listed
 * rates.  Indices must be distinct and in range (FVAD_EINVAL), every rate a
 * listed one or 48000 and at most Rmax (FVAD_ERATE); on either error nothing
 * is touched.  n == 0 is a no-op.  It never waits for the device and takes
 * effect between the pushes submitted before it and those submitted after it.
 * On any other engine it is FVAD_EINVAL.  fvad_engine_stream_denoised_rates
 * returns the rates the next submitted push will use.
 *
 * History.  Unlike the input side's, a row's history does not depend on its
 * rate: it is the row's last 287 48 kHz denoised samples (K - 1 at 8 kHz, the
 * longest), of which a stream at rate R reads the last K(R) - 1.  A change of
 * rate therefore clears nothing and has no onset transient: the stream's first
 * tick at the new rate R' is fvad_resample_out_host(R', ..., tail = the
 * K(R') - 1 denoised samples before it).  48000 streams keep their history
 * too, so they may take a listed rate later.  fvad_engine_reset and
 * fvad_engine_reset_streams zero the history; the streams keep their rates.
 *
 * Stream blobs.  Such an engine's header carries reserved[1] = 0xFFFFFFFF; its
 * records end -- behind the input tails and the input rate word, if the engine
 * has them -- with n_channels rows of 288 words (the 287 history samples, then
 * one zero word) and 4 words behind them (the stream's denoised rate, then
 * zeros).  Such blobs move only between engines of per-stream denoised rates
 * (FVAD_EFORMAT otherwise, as between engines of different denoised_rate);
 * config_hash covers the marker, not denoised_rate_max.  A restore gives the
 * target slot its record's rate, so the layout of the next push changes; a
 * record whose rate exceeds the target's denoised_rate_max is FVAD_EFORMAT,
 * found before anything is written.
 *
 * fvad_engine_resample_out_times works and reports all of a push's
 * output-resample launches together.  A capture of the denoised rows
 * (fvad_engine_enable_capture_ex with FVAD_CLIP_SOURCE_DENOISED) is FVAD_EINVAL
 * on such an engine: clips at a stream's own rate do not exist.  A capture of
 * the input, events and machines work unchanged. */
/* host only (no GPU): offsets[n_streams + 1] of the packed layout above.
 * FVAD_ERATE for a rate that is neither listed nor 48000 */
int fvad_denoised_layout(const int *rates, int n_streams, int n_channels, int64_t *offsets /* n_streams + 1 */);
int fvad_engine_denoised_layout(const fvad_engine *e, int64_t *offsets /* n_streams + 1 */);
int fvad_engine_set_stream_denoised_rates(fvad_engine *e, const int *streams, int n, const int *rates);
int fvad_engine_stream_denoised_rates(const fvad_engine *e, int *rates /* n_streams */);

/* ------------------------------------------------------------------ */
/* 3. Host mirror of the reference API (C++ above this ABI)             */
/* ------------------------------------------------------------------ */
/* VADMachine.Config (VADMachine.zig:18-39) */
typedef struct {
  float speech_min_freq, speech_max_freq;
  float long_term_speech_avg_sec;
  int has_initial_long_term_avg;
  double initial_long_term_avg;
  float short_term_speech_avg_sec;
  float speech_threshold_factor;
  float channel_vol_ratio_avg_sec;
  float channel_vol_ratio_threshold;
  float min_consecutive_sec_to_open;
  float max_speech_gap_sec;
  float min_vad_duration_sec;
} fvad_vadm_config;
void fvad_vadm_config_default(fvad_vadm_config *c);

/* VAD.VADSpeechSegment (VAD.zig:25-30) */
typedef struct {
  uint64_t sample_from, sample_to;
  float debug_rnn_vad, debug_avg_speech_vol_ratio;
} fvad_segment;

/* VADMachine (VADMachine.zig:65-310) on its own: feed it one FFT-B window at a
 * time (absolute sample index of the window start, the per-channel band sums
 * of its speech band, the window's vad and volume ratio). */
typedef struct fvad_vadm fvad_vadm;
int fvad_vadm_create(const fvad_vadm_config *cfg, int sample_rate, int fft_size, int n_channels, fvad_vadm **out);
void fvad_vadm_destroy(fvad_vadm *v);
/* speech band as FFT-B bins (FFT.freqToBin of speech_min/max_freq) */
void fvad_vadm_bins(const fvad_vadm *v, int *lo, int *hi);
int fvad_vadm_run(fvad_vadm *v, uint64_t index, const float *band_per_channel, float vad, float vol_ratio);
size_t fvad_vadm_segments(const fvad_vadm *v, fvad_segment *out, size_t cap);
/* speech state (0 closed, 1 opening, 2 open, 3 closing) and the current speech
 * start / end sample indices, as fvad_engine_vadm_state reports them (each
 * output nullable) */
int fvad_vadm_state(const fvad_vadm *v, int *speech_state, uint64_t *speech_start, uint64_t *speech_end);

/* Device VADMachines (VADMachine.zig:126-230 run on the GPU, one lane per
 * stream, after FFT B of every push).  Staged engines only.
 * Each config's speech band (FFT.freqToBin of speech_min/max_freq) must be one
 * of the engine's bands.  Up to FVAD_MAX_BANDS machines; segments accumulate
 * on the device, seg_capacity per (stream, machine); a reset clears them.
 * A push's machines are enqueued when the next push is launched (beside it, on
 * a side stream) or at the next sync point (fvad_engine_sync, _segments,
 * _vadm_state, _vadm_snapshot, _kernel_times), so after submit / collect the
 * last collected push's windows are not in the machine state yet; every
 * reader above flushes them first.  A reset or destroy drops them. */
int fvad_engine_attach_vadm(fvad_engine *e, const fvad_vadm_config *cfgs, int n, int seg_capacity);

/* Per-stream configs: a machine config per (machine, stream) that can be
 * changed between pushes without touching any other stream -- where a config
 * sweep's winner per stream (fvad_sweep_run_score's single_out) goes.
 *
 * RollingAverage lengths a config needs at (sample_rate, fft_size): out[0] long-term,
 * out[1] short-term, out[2] volume ratio.  Host only. */
int fvad_vadm_lengths(const fvad_vadm_config *cfg, int sample_rate, int fft_size, int out[3]);
/* fvad_engine_attach_vadm with a config per (machine, stream) that can be changed later.
 * cfgs[n]: the config every stream starts with on machine m.  room[n_room] (nullable, n_room 0):
 * configs that are never run and only size the rolling buffers -- each of a machine's three
 * lengths is the maximum over cfgs[m] and every room config.  All or nothing, like
 * fvad_engine_attach_vadm.  Such an engine runs k_vadm_hbm_ps / k_vadm_par_ps, which read a
 * stream's constants from a device table (fvad_engine_kernel_name reports them in k_vadm_hbm's
 * and k_vadm_par's places), also while every stream still runs cfgs[m]; results are those of
 * fvad_engine_attach_vadm for the same configs.  Everything else -- readers, the event feed,
 * clip capture, fvad_engine_share_streams, the test hooks -- works as on a plain engine, except:
 * fvad_engine_save_streams and fvad_engine_restore_streams return FVAD_EINVAL (the v1 blob's
 * record layout and config_hash assume one config per machine; a v2 record that carries its
 * configs is a later change). */
int fvad_engine_attach_vadm_ex(fvad_engine *e, const fvad_vadm_config *cfgs, int n, int seg_capacity,
                               const fvad_vadm_config *room, int n_room);
/* Machine `machine` of the n listed streams becomes a freshly constructed machine of cfgs[i].
 * Takes effect between the pushes submitted before the call and those submitted after it, as
 * fvad_engine_reset_streams does (a pending machine pass of the previous push is queued first
 * and sees the old config), and never waits for the device: the rows reach it in the argument
 * blocks of k_vadm_retarget launches on the side stream, 47 rows a launch, so no buffer of the
 * caller's has to outlive the call.  The new machine's state is fvad_vadm_create's for cfgs[i]
 * with its three rolling buffers empty, but its window count is kept (window sample indices
 * continue where the stream is); a deferred long-term fold the old machine owed is dropped
 * with it.  Segments already emitted stay in fvad_engine_segments' list, and n_segments and
 * the feed's seq continue.  A speech in progress (opening, open or closing) is abandoned: it
 * produces no segment and no SEGMENT event, so a SPEECH_OPEN event already delivered for it
 * stays unmatched.  Pending clips of clip capture are untouched.
 * Checked before any device work (FVAD_EINVAL, the engine exactly as it was): the engine was
 * attached with fvad_engine_attach_vadm_ex; the streams are distinct and in range and
 * machine < n; each config's speech band is one of the engine's bands (the band slot is per
 * stream); each of its three lengths fits the attached room (the message names the stream,
 * the length and the room); FVAD_DEBUG_VADM_LT_FULL is not set.  n == 0: FVAD_OK.
 * fvad_engine_reset_streams and fvad_engine_reset give each stream a fresh machine of its
 * current config: the configs survive a reset. */
int fvad_engine_set_stream_vadm(fvad_engine *e, const int32_t *streams, int n, int machine,
                                const fvad_vadm_config *cfgs);
/* The config (stream, machine) runs now (host mirror, no sync). */
int fvad_engine_stream_vadm_config(const fvad_engine *e, int stream, int machine, fvad_vadm_config *out);

/* total segments of (stream, machine) so far; copies min(total, capacity, cap) */
size_t fvad_engine_segments(fvad_engine *e, int stream, int machine, fvad_segment *out, size_t cap);
/* the same from segment index `first` on (returns the total count) */
size_t fvad_engine_segments_range(fvad_engine *e, int stream, int machine, size_t first, fvad_segment *out,
                                  size_t cap);
/* speech state of an attached machine (VADMachine.zig:11-16: 0 closed, 1 opening,
 * 2 open, 3 closing) and its current speech start / end sample indices */
int fvad_engine_vadm_state(fvad_engine *e, int stream, int machine, int *speech_state, uint64_t *speech_start,
                           uint64_t *speech_end);
/* The whole state of an attached machine in the reference's terms
 * (VADMachine.zig:65-125 fields; RollingAverage.zig:5-14 for long_term [0],
 * short_term [1] and the channel volume ratio [2]), after every queued push:
 * what a checker compares with a CPU VADMachine fed the same windows. */
typedef struct {
  int speech_state;                 /* 0 closed, 1 opening, 2 open, 3 closing */
  uint64_t speech_start, speech_end;  /* speech_start_index, speech_end_index */
  uint64_t windows;                 /* windows the machine has run */
  double avg[3];                    /* RollingAverage.last_avg (0 before the first avg) */
  uint64_t write_idx[3];            /* RollingAverage.write_idx */
  uint64_t written[3];              /* RollingAverage.written_count */
  float speech_rnn_vad, speech_vol_ratio;  /* the current speech's tracked sums */
  uint64_t speech_rnn_vad_count, speech_vol_ratio_count;
  uint64_t n_segments;              /* segments emitted so far (also past seg_capacity) */
} fvad_vadm_snapshot;
int fvad_engine_vadm_snapshot(fvad_engine *e, int stream, int machine, fvad_vadm_snapshot *out);
/* RollingAverage.data of (stream, machine), which = 0 long-term, 1 short-term,
 * 2 volume ratio, as doubles: copies min(len, cap) entries, returns len (< 0:
 * error code) */
long fvad_engine_vadm_rolling(fvad_engine *e, int stream, int machine, int which, double *out, size_t cap);

/* Speech event feed: what the device VADMachines decided, push by push,
 * without a sync point.  Every reader above waits for the queued pushes and
 * serves one (stream, machine); the feed is one list for the whole engine that
 * a poll reads without waiting, it is lossless past seg_capacity, and it also
 * reports speech starting. */
#define FVAD_EVENT_SPEECH_OPEN 1 /* Opening -> Open (VADMachine.zig run) */
#define FVAD_EVENT_SEGMENT 2     /* onSpeechEnd emitted a segment (len >= min_vad_duration_sec) */
typedef struct {
  uint32_t kind;
  int32_t stream, machine;
  uint32_t seq;  /* segments this (stream, machine) had emitted before this event; for SEGMENT its index
                    in fvad_engine_segments' list (also past seg_capacity) */
  uint64_t push; /* ordinal of the producing push since create / fvad_engine_reset (the first is 0) */
  uint64_t sample_from, sample_to; /* SEGMENT: the fvad_segment's; OPEN: speech_start_index, and the start
                                      index of the window in which the machine opened */
  float debug_rnn_vad, debug_avg_speech_vol_ratio; /* SEGMENT: the fvad_segment's; OPEN: 0 */
} fvad_event; /* 48 bytes, little endian, no padding */
/* Start the feed (after fvad_engine_attach_vadm, once, with no push submitted
 * and not yet collected: FVAD_EINVAL otherwise); events start with the next
 * submitted push.  ring_capacity: events the engine holds between polls, 0 =
 * the default (65536).  FVAD_ENOMEM leaves the engine unchanged.  An engine
 * that never calls it launches and allocates nothing for the feed. */
int fvad_engine_enable_events(fvad_engine *e, size_t ring_capacity);
/* Up to cap events of the machine passes that have finished on the device, in
 * order: ascending push, then stream, then machine, then as the machine
 * produced them -- the same list for the same pushes whatever the schedule.
 * Never waits for queued pushes or for a machine pass (a push's pass is
 * enqueued with the next push or at a sync point, see above); after
 * fvad_engine_sync, polls deliver every event of every push submitted so far.
 * *n: events written; *lost (nullable): events dropped so far because the
 * ring was full -- a pass writes what fits behind the unpolled events, in
 * order, and counts the rest; polling makes room for later passes.
 * fvad_engine_reset discards unpolled events and zeroes push and lost;
 * fvad_engine_reset_streams leaves queued events in place and restarts the
 * listed streams' seq at 0; fvad_engine_restore_streams continues seq from the
 * blob's segment count (a stream restored Open emits no second OPEN). */
int fvad_engine_poll_events(fvad_engine *e, fvad_event *out, size_t cap, size_t *n, uint64_t *lost);
/* How far the feed has got, without waiting: *pushes_done = p means every event
 * of the pushes with ordinal < p has been polled or is ready to be (what a
 * host merging several engines' feeds per push needs). */
int fvad_engine_event_progress(fvad_engine *e, uint64_t *pushes_done);
/* k_vadm_events' own time: the average (ms) over the timed passes since the
 * last fvad_engine_clear_times, and how many (synchronises the engine) */
int fvad_engine_event_times(fvad_engine *e, double *ms_avg, int *n_runs);

/* Clip capture: the Recorder (AudioPipeline.zig:134-195, Recorder.zig:52-146)
 * for the batched engine.  The engine keeps the last history_sec of every
 * stream's input on the device and, for each SEGMENT event of one machine,
 * hands over the raw input of [sample_from, sample_to) -- the floats of a
 * float push, k / 32768.0f of the 16-bit ingest -- on the channel
 * fvad_recording_channel chooses over exactly the delivered samples.  A clip
 * completes in the machine pass of the first push at whose end its stream
 * holds sample_to samples (sample_to = speech_end + 2 s: usually a later push
 * than the segment's); until then it waits in the stream's queue of 4, and a
 * clip that finds the queue full is lost (counted).  Clips are delivered in
 * order of completing push, then stream, then seq -- the same list for the
 * same pushes whatever the schedule. */
#define FVAD_CLIP_HEAD_SHORT 1 /* samples before first_sample were no longer held */
#define FVAD_CLIP_TAIL_SHORT 2 /* cut by fvad_engine_capture_flush before sample_to was pushed */
#define FVAD_CLIP_NO_AUDIO 4   /* the pool had no room (or nothing was held): n_samples = 0, channel = -1, counted in lost */
typedef struct {
  int32_t stream;
  uint32_t seq; /* the SEGMENT event's seq */
  int32_t channel;
  uint32_t flags;
  uint64_t push;                    /* ordinal of the push whose machine pass completed the clip */
  uint64_t sample_from, sample_to;  /* the segment's */
  uint64_t first_sample, n_samples; /* what is delivered: [first_sample, first_sample + n_samples) */
  uint64_t reserved;                /* 0 for an INPUT / F32 capture; else rate | format << 32 | source << 40 (below) */
} fvad_clip; /* 64 bytes, little endian, no padding */
/* Start capturing machine `machine`'s segments (the reference records the main
 * machine, 0).  After fvad_engine_attach_vadm and fvad_engine_enable_events,
 * once, with no push submitted and not yet collected, on a staged-family
 * engine (FVAD_MODE_STAGED, FP16, FP16_FUSED, F32_FAST) with use_denoiser = 1:
 * FVAD_EINVAL otherwise.  A sync point.  history_sec >= 4 bounds how far back
 * a clip may start: at the end of a push that leaves a stream at sample n the
 * engine holds [max(base, n - floor(48000 * history_sec)), n) of it, base the
 * stream's first sample of this life (0, or the position of its last reset or
 * restore); earlier samples are cut from a clip (FVAD_CLIP_HEAD_SHORT).
 * pool_samples: the samples of finished clips held between polls, 0 = 64 Mi.
 * FVAD_ENOMEM leaves the engine unchanged.  An engine that never calls it
 * allocates and launches nothing for capture. */
int fvad_engine_enable_capture(fvad_engine *e, int machine, double history_sec, size_t pool_samples);
/* The oldest finished clip, without waiting for the device: 1 and the clip in
 * *info and pcm[0, n_samples), or 0 when none is ready.  cap_samples <
 * n_samples: *info is filled, the clip stays queued, FVAD_EINVAL.  A delivered
 * clip frees its pool space for later passes.  A pass places its clips in
 * order behind the unread ones: a full pool loses the newest clips' audio
 * (the descriptor still arrives, FVAD_CLIP_NO_AUDIO), a full descriptor ring
 * the descriptor too; *lost (nullable) counts both, and the clips a full
 * pending queue turned away, so far.  After fvad_engine_sync, polls deliver
 * every clip completed by every push submitted so far.  fvad_engine_reset
 * discards pending and unpolled clips and zeroes the counts;
 * fvad_engine_reset_streams drops the listed streams' pending clips and
 * restarts their positions at 0 (queued clips stay; no host wait);
 * fvad_engine_restore_streams sets the listed streams' position to the blob's
 * sample count: a blob carries no audio history and no pending clip. */
int fvad_engine_poll_clip(fvad_engine *e, fvad_clip *info, float *pcm, size_t cap_samples, uint64_t *lost);
/* A sync point: the pending clips of the n listed streams (NULL: of all) are
 * completed now, each cut at its stream's current sample count
 * (FVAD_CLIP_TAIL_SHORT), delivered in stream order, then seq, with the last
 * push's ordinal.  For a stream's end, before fvad_engine_reset_streams. */
int fvad_engine_capture_flush(fvad_engine *e, const int32_t *streams, int n);
/* Average times (ms) over the timed pushes since the last
 * fvad_engine_clear_times: ms_avg[0] k_hist_append, ms_avg[1] the capture pass
 * (its four kernels); *n_runs (nullable): the timed passes.  Synchronises. */
int fvad_engine_capture_times(fvad_engine *e, double *ms_avg, int *n_runs);

/* Denoised clips, at the output rate, as f32 or 16-bit PCM.
 * fvad_engine_enable_capture_ex is fvad_engine_enable_capture with a source
 * and a format; the old call equals it with {machine, history_sec,
 * pool_samples, INPUT, F32}, and everything said above holds for both.
 *
 * source DENOISED records the engine's denoised rows instead of its input: the
 * denoised signal of a stream is the concatenation of its valid ticks' rows,
 * the very values push / collect / fetch deliver, at the clip rate R =
 * fvad_engine_clip_rate: the engine's denoised_rate, 48000 without one (INPUT:
 * always 48000).  It needs want_denoised != 0 (FVAD_EINVAL otherwise); with
 * want_denoised = 2 the rows never leave the device and only the clips cross
 * to the host.  A bad source or format is FVAD_EINVAL; a failed call leaves
 * the engine unchanged.
 *
 * Units.  sample_from and sample_to stay the segment's 48 kHz values;
 * first_sample and n_samples count samples of the clip rate, sample r of a
 * stream being row r / (R / 100), column r % (R / 100).  With R = 48000 L / M
 * in lowest terms, the segment covers the r with sample_from <= r M / L <
 * sample_to, [ceil(sample_from L / M), ceil(sample_to L / M)), which
 * fvad_clip_range computes.  A stream at 48 kHz sample n is at n L / M
 * clip-rate samples (exact: n is a multiple of 480), so a clip completes in
 * the same push as an INPUT clip, and the engine holds [max(base L / M, n L /
 * M - floor(R * history_sec)), n L / M) of it.  The flags keep their meaning.
 * The output resampler's causal delay, (L K - 1) / (2 L) 48 kHz samples
 * ("Output rate of the denoised PCM"), is NOT compensated:
 * the clip holds the resampler's outputs of those indices, which lag the
 * 48 kHz signal by that much; the segment's 2 s tail covers it.
 * channel: fvad_recording_channel over exactly the delivered f32 samples of
 * the source, before any conversion.
 *
 * format S16 delivers q = clamp(rint(x * 32768.0f), -32768, 32767), ties to
 * even, NaN -> 0 (fvad_pcm_f32_to_s16, bit for bit), converted on the device
 * as the clip is copied: read it with fvad_engine_poll_clip_s16; an F32
 * capture is read with fvad_engine_poll_clip, and the other call is
 * FVAD_EINVAL.  pool_samples counts samples in either format (an S16 pool
 * takes half the pinned bytes). */
#define FVAD_CLIP_SOURCE_INPUT 0    /* what fvad_engine_enable_capture records */
#define FVAD_CLIP_SOURCE_DENOISED 1 /* the engine's denoised rows, at fvad_engine_clip_rate */
#define FVAD_CLIP_F32 0
#define FVAD_CLIP_S16 1
typedef struct {
  int machine;
  double history_sec;
  size_t pool_samples; /* as fvad_engine_enable_capture's */
  int source, format;
} fvad_capture_config;
void fvad_capture_config_default(fvad_capture_config *c); /* machine 0, 10 s, 0, INPUT, F32 */
int fvad_engine_enable_capture_ex(fvad_engine *e, const fvad_capture_config *c);
int fvad_engine_poll_clip_s16(fvad_engine *e, fvad_clip *info, int16_t *pcm, size_t cap_samples, uint64_t *lost);
/* 48000 for INPUT; the denoised rate for DENOISED; 0 without capture */
int fvad_engine_clip_rate(const fvad_engine *e);
/* Host mirrors, no GPU: the S16 conversion, and the clip-rate samples
 * [*first, *end) a 48 kHz range [from48, to48) covers at `rate` (the identity
 * at 48000; FVAD_ERATE off the list of rates, FVAD_EINVAL for to48 < from48;
 * from48, to48 < 2^56). */
void fvad_pcm_f32_to_s16(const float *x, int16_t *q, size_t n);
int fvad_clip_range(int rate, uint64_t from48, uint64_t to48, uint64_t *first, uint64_t *end);

/* Several engines on one GPU (e.g. a GPU's streams split into sub-partitions
 * that push concurrently): e runs its k_prep3 (FVAD_SHARE_PREP) and / or its
 * device VADMachine kernels (FVAD_SHARE_SIDE, both engines with machines
 * attached) on other's streams from now on, so the engines' side work queues
 * in order instead of taking a hardware queue each (a process gets
 * GPU_MAX_HW_QUEUES of them, 4 by default, shared round-robin once they run
 * out: a main stream sharing one with another engine's k_prep3 waits for it).
 * Synchronises both engines; results are unchanged (dependencies are events).
 * Only k_prep3 moves: an engine alone on its prep stream also runs k_fftAw
 * there (beside its previous push's tail), one whose prep stream is shared
 * runs k_fftAw on its own engine stream, so the main pipelines stay
 * uncoupled.  The last engine using a stream destroys it. */
#define FVAD_SHARE_PREP 1
#define FVAD_SHARE_SIDE 2
int fvad_engine_share_streams(fvad_engine *e, fvad_engine *other, int which);

/* Test hooks: knobs and a recorder the parity tests use; no product path sets
 * them.  fvad_engine_set_debug keys:
 *   FVAD_DEBUG_VADM_PAR_SERIAL_EVERY  value k > 0: k_vadm_par hands every
 *     stream s with s % k == 0 to its in-kernel serial walk (the fallback for a
 *     machine outside the window-parallel case); 0: never (default)
 *   FVAD_DEBUG_VADM_ALWAYS_PAR  value 1: every push's VADMachine runs as
 *     k_vadm_par, not only the one flushed at a sync point
 *   FVAD_DEBUG_VADM_LT_FULL  value 1: the machines restart (as by a reset)
 *     with every long-term entry counted as pushed, holding (float)init: the
 *     long-term walk of a stream past its first long_term_speech_avg_sec, for
 *     timing (tools/vadm_steady.py); the values then differ from the reference
 *   FVAD_DEBUG_VADM_DEFER_MAX  value k > 0: between sync points k_vadm_hbm
 *     folds a machine's long-term average once k long pushes are owed (1: at
 *     the end of every push); 0: the default bound (4096).  Results are the
 *     same for every k: a sync point resolves every owed fold
 *   FVAD_DEBUG_VADM_BOUND_SCALE  value k > 0: the lazy long-term walk's error
 *     bound E (fvad_exact.h lt_bound) times k; -1: infinite, so every test the
 *     estimate would decide takes the exact fold instead; 0: back to 1.
 *     Results are the same for every k >= 1
 *   FVAD_DEBUG_VADM_COUNT  value 1: count the long-term tests by how they were
 *     decided (fvad_engine_debug_counts), from zero; 0: stop counting
 *   FVAD_DEBUG_VADM_NEGATE_AT  value k >= 0: window k of every stream enters
 *     every machine with its band minimum negated (a value the pipeline never
 *     produces: the path that folds exactly until that entry has left the
 *     long-term buffer); -1: off (default) */
#define FVAD_DEBUG_VADM_PAR_SERIAL_EVERY 1
#define FVAD_DEBUG_VADM_ALWAYS_PAR 2
#define FVAD_DEBUG_VADM_LT_FULL 3
#define FVAD_DEBUG_VADM_DEFER_MAX 4
#define FVAD_DEBUG_VADM_BOUND_SCALE 5
#define FVAD_DEBUG_VADM_COUNT 6
#define FVAD_DEBUG_VADM_NEGATE_AT 7
/*   FVAD_DEBUG_RESET_TIMES  value 1: fvad_engine_reset_streams brackets each of
 *     its launches with a timing event pair (fvad_engine_reset_times) */
#define FVAD_DEBUG_RESET_TIMES 8
/*   FVAD_DEBUG_EVENTS_CHUNK  value k > 0: k_vadm_events packs k lanes per
 *     iteration (k below its workgroup size: the carry across chunks at a
 *     small engine); 0: the default.  Results are the same for every k */
#define FVAD_DEBUG_EVENTS_CHUNK 9
int fvad_engine_set_debug(fvad_engine *e, int key, int value);
/* FVAD_DEBUG_RESET_TIMES' samples: average event time (ms) of a
 * fvad_engine_reset_streams call's launches on [0] the engine stream, [1] the
 * prep stream, [2] the side stream, and how many each averages (the last 64
 * calls at most); synchronises the engine and clears the samples */
int fvad_engine_reset_times(fvad_engine *e, double *ms_avg, int *n_runs);
/* FVAD_DEBUG_VADM_COUNT's counters, out[0..min(n, 4)): long-term tests decided
 * from an exact average, tests the bound settled from the estimate, tests it
 * left open (an exact fold), folds at the end of a push.  Returns the count
 * written (synchronises the engine). */
int fvad_engine_debug_counts(fvad_engine *e, unsigned long long *out, int n);
/* Output log: the per-tick outputs (fvad_outputs without denoised) of the next
 * n_pushes pushes are copied into device memory on the engine stream as each
 * push's kernels end -- no host synchronisation, so a run of asynchronous
 * pushes (run_resident, submit) keeps its schedule; read them back after the
 * pushes with fvad_engine_output_log_read (push = 0 .. n_pushes - 1 in launch
 * order).  n_pushes = 0 frees the log.  Staged / fp16 engines with the denoiser. */
int fvad_engine_output_log(fvad_engine *e, int n_pushes);
int fvad_engine_output_log_read(fvad_engine *e, int push, fvad_outputs *out, int *n_ticks);

/* VAD.Config (VAD.zig:17-23) */
typedef struct {
  int fft_size;                                     /* even, 2..4194304 (FFT.zig:28-31) */
  int use_denoiser;                                 /* 0: fft_size frames of raw input to FFT B */
  fvad_vadm_config vad_machine_config;              /* main machine */
  const fvad_vadm_config *alt_vad_machine_configs;  /* alternative machines (training), nullable */
  int n_alt;                                        /* <= FVAD_MAX_BANDS - 1 */
} fvad_vad_config;
void fvad_vad_config_default(fvad_vad_config *c);

/* AudioPipeline (AudioPipeline.zig:20-26,39-120) for one stream, backed by a
 * 1-stream engine.  n_alt alternative VADMachine configs (VAD.zig:20-23). */
typedef struct fvad_pipeline fvad_pipeline;
int fvad_pipeline_create(int sample_rate, int n_channels, const fvad_model *model, int device,
                         const fvad_vadm_config *main_cfg, const fvad_vadm_config *alt_cfgs, int n_alt,
                         fvad_pipeline **out);
/* the same with a whole VAD.Config (fft_size, use_denoiser, machines) */
int fvad_pipeline_create_ex(int sample_rate, int n_channels, const fvad_model *model, int device,
                            const fvad_vad_config *vad_config, fvad_pipeline **out);
void fvad_pipeline_destroy(fvad_pipeline *p);
/* pushSamples: planar channel pointers, n samples each; *first_index receives
 * the absolute index of the first pushed sample (AudioPipeline.zig:86-120) */
int fvad_pipeline_push(fvad_pipeline *p, const float *const *channel_pcm, size_t n, uint64_t *first_index);
/* vad_segments of the main (alt < 0) or an alternative machine */
size_t fvad_pipeline_segments(const fvad_pipeline *p, int alt, fvad_segment *out, size_t cap);

/* Recorder (Recorder.zig:95-110 findBestChannel): the channel with the lowest
 * rmsVolume (audio_utils.zig:14-24) over n samples; the first one on ties. */
int fvad_recording_channel(const float *const *channel_pcm, int n_channels, size_t n);
/* on_recording (AudioPipeline.zig:15-18, :134-195, Recorder.zig:52-146): called
 * from fvad_pipeline_push once per completed main-machine segment with the raw
 * pushed input of [sample_from, sample_to) on its lowest-RMS channel
 * (AudioBuffer: one channel, global_start_frame_number = start_sample).
 * fn = NULL detaches; only segments completed after attaching are recorded. */
typedef void (*fvad_recording_fn)(void *ctx, const float *pcm, size_t n, uint64_t start_sample, int channel);
int fvad_pipeline_set_recorder(fvad_pipeline *p, fvad_recording_fn fn, void *ctx);

/* Multi-stream simulator core (simulator.zig:217-228 runs one thread per
 * instance): streams grouped by channel count, each group partitioned
 * contiguously over the devices, one engine + host thread per part, lock-step
 * pushes of ticks_per_push ticks.  pcm[s] points to planar [channels][len[s]]
 * audio of stream s (fvad_multi_run), or a reader pulls it push by push
 * (fvad_multi_run_stream: the simulator's streaming read loop,
 * SimulationInstance.zig:171-203). */
typedef struct fvad_multi fvad_multi;
int fvad_multi_create(int n_streams, int n_channels, const fvad_model *model, const int *devices,
                      int n_devices, const fvad_vadm_config *cfg, int ticks_per_push, fvad_multi **out);
/* per-stream channel counts and a whole VAD.Config */
int fvad_multi_create_ex(int n_streams, const int *n_channels, const fvad_model *model, const int *devices,
                         int n_devices, const fvad_vad_config *vad_config, int ticks_per_push, fvad_multi **out);
void fvad_multi_destroy(fvad_multi *m);
int fvad_multi_run(fvad_multi *m, const float *const *pcm, const size_t *len);
/* reader: write up to max_frames frames of stream `stream` planar into
 * channel_dst[c][0..), return the count (0 = end of stream).  Called from the
 * part threads; a stream is always read by the same thread, in order. */
typedef size_t (*fvad_read_fn)(void *ctx, int stream, float *const *channel_dst, size_t max_frames);
int fvad_multi_run_stream(fvad_multi *m, fvad_read_fn read, void *ctx);
/* segments of the main machine (machine 0) or alternative machine i (machine i + 1) */
size_t fvad_multi_segments_alt(const fvad_multi *m, int stream, int machine, fvad_segment *out, size_t cap);
size_t fvad_multi_segments(const fvad_multi *m, int stream, fvad_segment *out, size_t cap);

/* Evaluator / statistics (Evaluator.zig:90-156, statistics.zig:85-284) */
typedef struct {
  float ignore_shorter_than_sec, extrude_start, extrude_end, fill_gaps;
} fvad_stat_config;
typedef struct {
  float total_positives_sec, true_positives_sec, false_positives_sec, false_negatives_sec;
  float true_positive_rate, false_negative_rate, false_discovery_rate, precision;
  float fm_index, f_score, f_score_beta;
} fvad_single_stats;
typedef struct { float overall, min, max, avg; } fvad_agg_stat;
typedef struct {
  float total_positives_sec, true_positives_sec, false_positives_sec, false_negatives_sec;
  fvad_agg_stat true_positive_rate, false_negative_rate, false_discovery_rate, precision;
  float fm_index, f_score, f_score_beta;
} fvad_aggregate_stats;
/* segments as (from_sec, to_sec) pairs */
int fvad_eval_stats(const float *vad_from_to, size_t n_vad, const float *ref_from_to, size_t n_ref,
                    const fvad_stat_config *cfg, fvad_single_stats *out);
void fvad_eval_aggregate(const fvad_single_stats *stats, size_t n, fvad_aggregate_stats *out);
/* formats.parseAudacitySegments (formats.zig:7-36): returns count or <0 */
long fvad_parse_audacity(const char *txt, size_t len, float *from_to, size_t cap);

/* Config sweep: many VADMachine configs over recorded window sequences (the
 * tuning loop of VAD.zig:375-380's alt_vad_machine_configs).  A VADMachine
 * sees nothing of the audio but a completed window's band sums, vad and volume
 * ratio, so a sweep records each stream's windows once -- from any engine's
 * pushes, or set directly -- and runs any number of configs over them: one
 * GPU lane per (stream, config) (k_vadm_sweep, the engine's device machine
 * over the whole sequence), each from a freshly constructed machine, bit for
 * bit the host VADMachine's segments and state.  Independent of any engine. */
typedef struct {
  int n_streams;
  int n_channels;              /* 1..FVAD_MAX_CHANNELS */
  int sample_rate;             /* 48000 (FVAD_ERATE otherwise) */
  int fft_size;                /* even, 2..4194304: a window is fft_size samples */
  int n_bands;                 /* 1..FVAD_MAX_BANDS bands per recorded window, as the engine's */
  int band_lo[FVAD_MAX_BANDS];
  int band_hi[FVAD_MAX_BANDS];
  int use_denoiser;            /* 0: every window's vad enters the machines as 0 (VADMachine.zig:240-246) */
  int seg_capacity;            /* >= 1: segments kept per (stream, config) */
  int device;                  /* HIP device, or -1: a host-only sweep (needs no GPU; run = run_host) */
} fvad_sweep_config;
typedef struct fvad_sweep fvad_sweep;
int fvad_sweep_create(const fvad_sweep_config *cfg, fvad_sweep **out);
void fvad_sweep_destroy(fvad_sweep *sw);
/* A stream's whole window sequence, in order: band [n_windows][n_channels]
 * [n_bands] (one window slot of fvad_outputs.band each), vad [n_windows]
 * (nullable: 0), vol_ratio [n_windows].  Replaces what the stream held; a
 * stream never set has 0 windows.  Window w enters every machine with sample
 * index w * fft_size. */
int fvad_sweep_set_windows(fvad_sweep *sw, int stream, size_t n_windows, const float *band, const float *vad,
                           const float *vol_ratio);
/* Appends the completed windows of one push's outputs (win_flag, win_ratio,
 * win_vad, band: all required; the layout of an engine with the sweep's
 * streams, channels, bands and fft_size) to every stream: ticks in order, then
 * a tick's slots w < win_flag; stream s only its first ticks_valid[s] ticks
 * (nullable: all).  Host code: any engine mode's pushes can fill a sweep. */
int fvad_sweep_append_outputs(fvad_sweep *sw, const fvad_outputs *out, int n_ticks, const int32_t *ticks_valid);
/* Runs every config over every stream, each from a freshly constructed machine
 * (fvad_engine_attach_vadm's initial state), replacing the previous run's
 * results.  Each config's speech band (FFT.freqToBin of speech_min/max_freq at
 * fft_size) must be one of the sweep's bands: FVAD_EINVAL naming the config
 * otherwise, with nothing run.  On a device sweep the configs run on the GPU,
 * in chunks when their buffers exceed the budget (results do not depend on the
 * chunking); fvad_sweep_run_host runs the host VADMachine instead (always, on
 * a host-only sweep). */
int fvad_sweep_run(fvad_sweep *sw, const fvad_vadm_config *cfgs, size_t n_cfgs);
int fvad_sweep_run_host(fvad_sweep *sw, const fvad_vadm_config *cfgs, size_t n_cfgs);
/* total segments of (stream, config) in the last run; copies min(total, seg_capacity, cap) */
size_t fvad_sweep_segments(const fvad_sweep *sw, int stream, size_t cfg, fvad_segment *out, size_t cap);
/* every total, out[stream * n_cfgs + cfg] */
int fvad_sweep_counts(const fvad_sweep *sw, uint64_t *out, size_t cap);
/* the machine's final state (every owed long-term fold resolved: avg[0] is the reference's bits) */
int fvad_sweep_snapshot(const fvad_sweep *sw, int stream, size_t cfg, fvad_vadm_snapshot *out);
/* Scores of the last run: per config, fvad_eval_stats per stream on its
 * segments as (float)sample / 48000.0f seconds against ref_from_to[stream]
 * (n_ref[stream] (from, to) pairs), then fvad_eval_aggregate over the streams
 * into agg_out[cfg]; single_out (nullable) [cfg][stream].  A lane that
 * overflowed seg_capacity would be scored from a truncated list:
 * FVAD_EINVAL naming it. */
int fvad_sweep_score(const fvad_sweep *sw, const float *const *ref_from_to, const size_t *n_ref,
                     const fvad_stat_config *stat_cfg, fvad_aggregate_stats *agg_out, fvad_single_stats *single_out);
/* fvad_sweep_run followed by fvad_sweep_score, for a tuning loop that wants a
 * score per config and not the segments: on a device sweep each lane is scored
 * on the GPU where k_vadm_sweep left its segments (k_sweep_score, the
 * evaluator's order of operations: fvad_eval_stats' bits, NaN for NaN), and
 * the statistics come back instead of the segments; a host-only sweep scores
 * with the same code on the host.  agg_out [cfg], single_out (nullable)
 * [cfg][stream], as fvad_sweep_score's.  What differs:
 *  - n_stat_cfgs is 1 (stat_cfgs[0] for every config) or n_cfgs (config m is
 *    scored with stat_cfgs[m], e.g. ignore_shorter_than_sec =
 *    min_vad_duration_sec of that machine, as the simulator scores).
 *  - The segments are not kept: afterwards fvad_sweep_counts, _snapshot and
 *    _debug_counts describe this run, fvad_sweep_segments returns the lane's
 *    total and copies nothing, and fvad_sweep_score returns FVAD_EINVAL until
 *    the next fvad_sweep_run / _run_host.
 *  - Null arguments, a null label list with n_ref[s] > 0, n_stat_cfgs not in
 *    {1, n_cfgs} and a config whose speech band is none of the sweep's give
 *    FVAD_EINVAL before anything runs: the previous run's results stay.  A
 *    lane whose total exceeds seg_capacity shows only after the run:
 *    FVAD_EINVAL naming the first such (stream, config) in fvad_sweep_score's
 *    order, agg_out / single_out unspecified, counts and snapshots valid.
 * Measured (MI355X, 64 streams x 20 000 windows x 1 024 configs at
 * seg_capacity 136, tools/sweep_score_times.py, profiles/sweep_score_times.json,
 * wall clock around the calls, interleaved in one process): 94.8 ms against
 * 1 203.9 ms for fvad_sweep_run + fvad_sweep_score, 13.6 MB copied back
 * against 224.4 MB, the same aggregates by their bits. */
int fvad_sweep_run_score(fvad_sweep *sw, const fvad_vadm_config *cfgs, size_t n_cfgs,
                         const float *const *ref_from_to, const size_t *n_ref, const fvad_stat_config *stat_cfgs,
                         size_t n_stat_cfgs, fvad_aggregate_stats *agg_out, fvad_single_stats *single_out);
/* The last run (each pointer nullable): its configs (0 before any), whether
 * its segments were kept (fvad_sweep_run_score: 0), and the bytes it copied
 * back from the device (0 for a host run). */
int fvad_sweep_last_run(const fvad_sweep *sw, size_t *n_cfgs, int *kept_segments, size_t *bytes_back);
/* Device memory the machines of a run need when all configs run in one chunk
 * (buffers, states, segments, constants; the recorded windows come on top:
 * (n_channels * n_bands + n_bands + 2) floats each); 0 on invalid arguments. */
size_t fvad_sweep_bytes(const fvad_sweep_config *cfg, const fvad_vadm_config *cfgs, size_t n_cfgs);
/* Spectral sweeps: any speech band per config.  A band sum cannot be rebuilt
 * from other band sums (it is one f32 chain in bin order), so a spectral sweep
 * records each window's magnitudes of the bins spec_lo..spec_hi (section 2c:
 * what an engine with want_spectrum and the same range fetches) instead of
 * band sums.  cfg->n_bands and band_lo / band_hi are ignored; the range check
 * is the engine's (FVAD_EINVAL); device = -1 makes a host-only spectral sweep.
 *
 * fvad_sweep_set_spectra and fvad_sweep_append_spectra are fvad_sweep_set_windows
 * and fvad_sweep_append_outputs with spectrum [n_windows][n_channels][n_spec],
 * or fvad_engine_fetch_spectrum's layout beside the push's outputs (win_flag,
 * win_ratio, win_vad required), in band's place: the same window order and
 * ticks_valid rules.  The band-sum setters on a spectral sweep and the
 * spectral setters on a plain sweep are FVAD_EINVAL.
 *
 * fvad_sweep_run, _run_host and _run_score accept every config whose speech
 * band [lo, hi] lies inside [spec_lo, spec_hi] (FVAD_EINVAL naming the first
 * config otherwise, nothing run).  The distinct bands of a chunk of configs,
 * in order of first appearance, get a slot each; k_sweep_bandmin turns the
 * recorded spectra into the windows' band minima of those D bands -- per
 * channel acc = 0.0f; for k = lo .. hi: acc += spectrum[k], then the minimum
 * over channels from 999 with strict < -- and the machines run unchanged over
 * them.  The host path runs the same sums (fvad_bandsum_core.h).  A chunk's
 * minima (windows * D floats) count against the chunk budget;
 * fvad_sweep_bytes does not include them, nor the spectra
 * (n_channels * n_spec + 2 floats per window). */
int fvad_sweep_create_spectral(const fvad_sweep_config *cfg, int spec_lo, int spec_hi, fvad_sweep **out);
int fvad_sweep_set_spectra(fvad_sweep *sw, int stream, size_t n_windows, const float *spectrum, const float *vad,
                           const float *vol_ratio);
int fvad_sweep_append_spectra(fvad_sweep *sw, const fvad_outputs *out, const float *spectrum, int n_ticks,
                              const int32_t *ticks_valid);
/* k_sweep_bandmin's time in the last run of a spectral sweep, by HIP events round
 * its launches, summed over the chunks (0 after a host run); FVAD_EINVAL on a
 * plain sweep */
int fvad_sweep_bandmin_ms(const fvad_sweep *sw, double *ms);
/* Test hooks (results are identical for every setting), for the next runs:
 *   FVAD_SWEEP_DEBUG_BOUND_SCALE  the lazy long-term test's bound times value (-1: infinite, 0: default)
 *   FVAD_SWEEP_DEBUG_DEFER_MAX    settle an owed fold once value long pushes are owed (0: default)
 *   FVAD_SWEEP_DEBUG_CHUNK        configs per chunk (0: by the memory budget)
 *   FVAD_SWEEP_DEBUG_COUNT        value != 0: count how long-term tests were decided (device sweeps)
 * fvad_sweep_debug_counts: the last run's counters -- decided from an exact
 * average, settled from the estimate, left open by the bound (folded), folds at
 * a block's or the stream's end; returns how many were written (< 0: error). */
#define FVAD_SWEEP_DEBUG_BOUND_SCALE 1
#define FVAD_SWEEP_DEBUG_DEFER_MAX 2
#define FVAD_SWEEP_DEBUG_CHUNK 3
#define FVAD_SWEEP_DEBUG_COUNT 4
int fvad_sweep_set_debug(fvad_sweep *sw, int key, int value);
int fvad_sweep_debug_counts(const fvad_sweep *sw, unsigned long long *out, int n);

/* Synthetic 48 kHz onboard audio; returns label count */
long fvad_synth_stream(uint32_t stream_id, size_t n, int n_channels, float *out, float *labels,
                       size_t label_cap);

/* The same streams in the engine's push layout: ticks [tick0, tick0 + n_ticks)
 * of streams base .. base + n_streams - 1, each generated at total_ticks * 480
 * samples, into out[t][s][c][480].  The last whole block is cached in host
 * memory (fvad_synth_cache_clear frees it). */
int fvad_synth_ticks(uint32_t stream_id_base, int n_streams, int n_channels, int total_ticks, int tick0,
                     int n_ticks, float *out);
void fvad_synth_cache_clear(void);

/* simulator -i plan.json (simulator.zig:74-139) — returns process exit code */
int fvad_simulator_main(int argc, char **argv);

#ifdef __cplusplus
}
#endif
#endif
