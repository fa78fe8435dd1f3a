"""Python bindings (ctypes) for libfvad.so — the MI355X-native Formula-VAD hot path.

Mirrors the reference's API surface for this path:
  * Denoiser        (src/Denoiser.zig)        -> rnnoise_* C ABI on the GPU
  * KissFFTR        (src/FFT.zig kissfft use) -> kiss_fftr_* C ABI on the GPU
  * Engine          batched multi-stream hot path (fvad_engine_*)
  * AudioPipeline   (src/AudioPipeline.zig pushSamples + VAD + VADMachine)
  * Multi           multi-stream simulator core (simulator.zig runAll)
  * evaluate/aggregate/parse_audacity (src/Evaluator/*)
  * Sweep           many VADMachine configs over recorded windows (fvad_sweep_*;
                    VAD.zig:375-380's alt_vad_machine_configs as a tuning loop)

All compute goes through the HIP kernels in libfvad.so; there is no CPU
fallback — operations raise FvadError when the library or the GPU is missing.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("FVAD_LIB", os.path.join(PKG_ROOT, "lib", "libfvad.so"))

FVAD_OK = 0
F32P = C.POINTER(C.c_float)
I32P = C.POINTER(C.c_int32)
MAX_BANDS = 4
FRAME = 480


class FvadError(RuntimeError):
    """code: the FVAD_E* status of the failed call (None when there is none)."""
    code = None


class EngineConfig(C.Structure):
    _fields_ = [("n_streams", C.c_int), ("n_channels", C.c_int), ("device", C.c_int), ("sample_rate", C.c_int),
                ("fft_size", C.c_int), ("max_ticks", C.c_int), ("n_bands", C.c_int),
                ("band_lo", C.c_int * MAX_BANDS), ("band_hi", C.c_int * MAX_BANDS), ("want_denoised", C.c_int),
                ("mode", C.c_int), ("use_denoiser", C.c_int),
                ("want_spectrum", C.c_int), ("spec_lo", C.c_int), ("spec_hi", C.c_int),
                ("denoised_rate_max", C.c_int), ("input_rate_max", C.c_int), ("denoised_rate", C.c_int),
                ("input_rate", C.c_int)]


class ResampleDesc(C.Structure):
    """fvad_resample_desc (include/fvad.h)."""
    _fields_ = [("input_rate", C.c_int), ("L", C.c_int), ("M", C.c_int), ("taps_per_phase", C.c_int),
                ("frame_in", C.c_int), ("delay", C.c_double)]


class ResampleOutDesc(C.Structure):
    """fvad_resample_out_desc (include/fvad.h)."""
    _fields_ = [("rate", C.c_int), ("L", C.c_int), ("M", C.c_int), ("taps_per_phase", C.c_int),
                ("frame_out", C.c_int), ("delay", C.c_double)]


MODE_STAGED, MODE_FUSED, MODE_FP16, MODE_FP16_FUSED, MODE_F32_FAST = 0, 1, 2, 3, 4
MAX_TIMES = 16


class Outputs(C.Structure):
    _fields_ = [("vad", F32P), ("ratio", F32P), ("win_flag", I32P), ("win_ratio", F32P), ("win_vad", F32P),
                ("band", F32P), ("denoised", F32P)]


class VadmConfig(C.Structure):
    _fields_ = [("speech_min_freq", C.c_float), ("speech_max_freq", C.c_float),
                ("long_term_speech_avg_sec", C.c_float), ("has_initial_long_term_avg", C.c_int),
                ("initial_long_term_avg", C.c_double), ("short_term_speech_avg_sec", C.c_float),
                ("speech_threshold_factor", C.c_float), ("channel_vol_ratio_avg_sec", C.c_float),
                ("channel_vol_ratio_threshold", C.c_float), ("min_consecutive_sec_to_open", C.c_float),
                ("max_speech_gap_sec", C.c_float), ("min_vad_duration_sec", C.c_float)]

    @classmethod
    def default(cls):
        c = cls()
        lib().fvad_vadm_config_default(C.byref(c))
        return c


class VadConfig(C.Structure):
    """VAD.Config (VAD.zig:17-23)."""
    _fields_ = [("fft_size", C.c_int), ("use_denoiser", C.c_int), ("vad_machine_config", VadmConfig),
                ("alt_vad_machine_configs", C.c_void_p), ("n_alt", C.c_int)]

    @classmethod
    def make(cls, fft_size=2048, use_denoiser=True, main_cfg=None, alt_cfgs=()):
        c = cls()
        lib().fvad_vad_config_default(C.byref(c))
        c.fft_size = fft_size
        c.use_denoiser = int(use_denoiser)
        if main_cfg is not None:
            c.vad_machine_config = main_cfg
        arr = (VadmConfig * max(1, len(alt_cfgs)))(*alt_cfgs)
        c._alts = arr
        c.alt_vad_machine_configs = C.cast(arr, C.c_void_p) if alt_cfgs else None
        c.n_alt = len(alt_cfgs)
        return c


class VadmSnapshot(C.Structure):
    """fvad_vadm_snapshot (include/fvad.h): a device machine's whole state."""
    _fields_ = [("speech_state", C.c_int), ("speech_start", C.c_uint64), ("speech_end", C.c_uint64),
                ("windows", C.c_uint64), ("avg", C.c_double * 3), ("write_idx", C.c_uint64 * 3),
                ("written", C.c_uint64 * 3), ("speech_rnn_vad", C.c_float), ("speech_vol_ratio", C.c_float),
                ("speech_rnn_vad_count", C.c_uint64), ("speech_vol_ratio_count", C.c_uint64),
                ("n_segments", C.c_uint64)]

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n in ("avg", "write_idx", "written") else getattr(self, n))
                for n, _ in self._fields_}


DEBUG_VADM_PAR_SERIAL_EVERY, DEBUG_VADM_ALWAYS_PAR, DEBUG_VADM_LT_FULL, DEBUG_VADM_DEFER_MAX = 1, 2, 3, 4
DEBUG_VADM_BOUND_SCALE, DEBUG_VADM_COUNT, DEBUG_VADM_NEGATE_AT, DEBUG_RESET_TIMES = 5, 6, 7, 8
DEBUG_EVENTS_CHUNK = 9
EVENT_SPEECH_OPEN, EVENT_SEGMENT = 1, 2  # fvad_event.kind
CLIP_HEAD_SHORT, CLIP_TAIL_SHORT, CLIP_NO_AUDIO = 1, 2, 4  # fvad_clip.flags
SHARE_PREP, SHARE_SIDE = 1, 2  # fvad_engine_share_streams

# stream blobs (fvad_engine_save_streams): include/fvad.h documents the layout
STREAM_BLOB_MAGIC, STREAM_BLOB_VERSION, STREAM_BLOB_HEADER_BYTES = 0x42535646, 1, 128


class StreamBlobHeader(C.Structure):
    """fvad_stream_blob_header (include/fvad.h)."""
    _fields_ = [("magic", C.c_uint32), ("version", C.c_uint32), ("header_bytes", C.c_uint32), ("count", C.c_uint32),
                ("stream_bytes", C.c_uint64), ("mode", C.c_uint32), ("n_channels", C.c_uint32),
                ("fft_size", C.c_uint32), ("use_denoiser", C.c_uint32), ("n_bands", C.c_uint32),
                ("n_machines", C.c_uint32), ("seg_capacity", C.c_uint32), ("state_words", C.c_uint32),
                ("config_hash", C.c_uint64), ("model_hash", C.c_uint64), ("sample_rate", C.c_uint32),
                ("reserved", C.c_uint32 * 13)]


READ_FN = C.CFUNCTYPE(C.c_size_t, C.c_void_p, C.c_int, C.POINTER(F32P), C.c_size_t)


class Segment(C.Structure):
    _fields_ = [("sample_from", C.c_uint64), ("sample_to", C.c_uint64), ("debug_rnn_vad", C.c_float),
                ("debug_avg_speech_vol_ratio", C.c_float)]


class Event(C.Structure):
    """fvad_event (include/fvad.h): one entry of the speech event feed, 48 bytes."""
    _fields_ = [("kind", C.c_uint32), ("stream", C.c_int32), ("machine", C.c_int32), ("seq", C.c_uint32),
                ("push", C.c_uint64), ("sample_from", C.c_uint64), ("sample_to", C.c_uint64),
                ("debug_rnn_vad", C.c_float), ("debug_avg_speech_vol_ratio", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Clip(C.Structure):
    """fvad_clip (include/fvad.h): the descriptor of one captured clip, 64 bytes."""
    _fields_ = [("stream", C.c_int32), ("seq", C.c_uint32), ("channel", C.c_int32), ("flags", C.c_uint32),
                ("push", C.c_uint64), ("sample_from", C.c_uint64), ("sample_to", C.c_uint64),
                ("first_sample", C.c_uint64), ("n_samples", C.c_uint64), ("reserved", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


CLIP_SOURCE_INPUT, CLIP_SOURCE_DENOISED = 0, 1  # fvad_capture_config.source
CLIP_F32, CLIP_S16 = 0, 1                       # fvad_capture_config.format


class CaptureConfig(C.Structure):
    """fvad_capture_config (include/fvad.h)."""
    _fields_ = [("machine", C.c_int), ("history_sec", C.c_double), ("pool_samples", C.c_size_t),
                ("source", C.c_int), ("format", C.c_int)]

    @classmethod
    def default(cls):
        c = cls()
        lib().fvad_capture_config_default(C.byref(c))
        return c


class StatConfig(C.Structure):
    _fields_ = [("ignore_shorter_than_sec", C.c_float), ("extrude_start", C.c_float), ("extrude_end", C.c_float),
                ("fill_gaps", C.c_float)]


_STAT_FIELDS = ("total_positives_sec", "true_positives_sec", "false_positives_sec", "false_negatives_sec",
                "true_positive_rate", "false_negative_rate", "false_discovery_rate", "precision", "fm_index",
                "f_score", "f_score_beta")


class SingleStats(C.Structure):
    _fields_ = [(n, C.c_float) for n in _STAT_FIELDS]


class AggStat(C.Structure):
    _fields_ = [("overall", C.c_float), ("min", C.c_float), ("max", C.c_float), ("avg", C.c_float)]


class AggregateStats(C.Structure):
    _fields_ = [("total_positives_sec", C.c_float), ("true_positives_sec", C.c_float),
                ("false_positives_sec", C.c_float), ("false_negatives_sec", C.c_float),
                ("true_positive_rate", AggStat), ("false_negative_rate", AggStat),
                ("false_discovery_rate", AggStat), ("precision", AggStat), ("fm_index", C.c_float),
                ("f_score", C.c_float), ("f_score_beta", C.c_float)]


class SweepConfig(C.Structure):
    """fvad_sweep_config (include/fvad.h)."""
    _fields_ = [("n_streams", C.c_int), ("n_channels", C.c_int), ("sample_rate", C.c_int), ("fft_size", C.c_int),
                ("n_bands", C.c_int), ("band_lo", C.c_int * MAX_BANDS), ("band_hi", C.c_int * MAX_BANDS),
                ("use_denoiser", C.c_int), ("seg_capacity", C.c_int), ("device", C.c_int)]


SWEEP_DEBUG_BOUND_SCALE, SWEEP_DEBUG_DEFER_MAX, SWEEP_DEBUG_CHUNK, SWEEP_DEBUG_COUNT = 1, 2, 3, 4


class KissCpx(C.Structure):
    _fields_ = [("r", C.c_float), ("i", C.c_float)]


# Every symbol include/fvad.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("fvad_last_error", C.c_char_p, []),
    ("fvad_version", C.c_char_p, []),
    ("rnnoise_create", C.c_void_p, [C.c_void_p]),
    ("rnnoise_destroy", None, [C.c_void_p]),
    ("rnnoise_process_frame", C.c_float, [C.c_void_p, F32P, F32P]),
    ("rnnoise_get_frame_size", C.c_int, []),
    ("fvad_set_default_model", None, [C.c_void_p]),
    ("kiss_fftr_alloc", C.c_void_p, [C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_size_t)]),
    ("kiss_fftr", None, [C.c_void_p, F32P, C.c_void_p]),
    ("fvad_model_synthetic", C.c_int, [C.c_uint64, C.POINTER(C.c_void_p)]),
    ("fvad_model_load_text", C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    ("fvad_model_free", None, [C.c_void_p]),
    ("fvad_model_blob", C.c_size_t, [C.c_void_p, C.c_void_p]),
    ("fvad_engine_config_default", None, [C.c_void_p, C.c_int, C.c_int]),
    ("fvad_engine_create", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    ("fvad_engine_destroy", None, [C.c_void_p]),
    ("fvad_engine_reset", C.c_int, [C.c_void_p]),
    ("fvad_engine_reset_streams", C.c_int, [C.c_void_p, I32P, C.c_int]),
    ("fvad_engine_save_size", C.c_size_t, [C.c_void_p, C.c_int]),
    ("fvad_engine_save_streams", C.c_int, [C.c_void_p, I32P, C.c_int, C.c_void_p, C.c_size_t]),
    ("fvad_engine_restore_streams", C.c_int, [C.c_void_p, I32P, C.c_int, C.c_void_p, C.c_size_t, I32P]),
    ("fvad_stream_blob_info", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    ("fvad_engine_reset_times", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("fvad_engine_push", C.c_int, [C.c_void_p, F32P, C.c_int, I32P, C.c_void_p]),
    ("fvad_engine_push_ex", C.c_int, [C.c_void_p, F32P, C.c_int, I32P, I32P, C.c_void_p]),
    ("fvad_engine_submit_ex", C.c_int, [C.c_void_p, F32P, C.c_int, I32P, I32P]),
    ("fvad_engine_input_slot", C.c_void_p, [C.c_void_p]),
    ("fvad_engine_submit", C.c_int, [C.c_void_p, F32P, C.c_int, I32P]),
    ("fvad_engine_collect", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    ("fvad_engine_input_slot_i16", C.c_void_p, [C.c_void_p]),
    ("fvad_engine_submit_i16", C.c_int, [C.c_void_p, C.POINTER(C.c_int16), C.c_int, I32P, I32P]),
    ("fvad_engine_load_synthetic", C.c_int, [C.c_void_p, C.c_int, C.c_uint32]),
    ("fvad_engine_load_synthetic_ex", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint32]),
    ("fvad_engine_resident_seek", C.c_int, [C.c_void_p, C.c_int]),
    ("fvad_engine_run_resident", C.c_int, [C.c_void_p, C.c_int]),
    ("fvad_engine_sync", C.c_int, [C.c_void_p]),
    ("fvad_engine_kernel_times", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("fvad_engine_kernel_name", C.c_char_p, [C.c_void_p, C.c_int]),
    ("fvad_engine_windows_per_tick", C.c_int, [C.c_void_p]),
    ("fvad_engine_attach_vadm", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    ("fvad_vadm_lengths", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    ("fvad_engine_attach_vadm_ex", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    ("fvad_engine_set_stream_vadm", C.c_int, [C.c_void_p, I32P, C.c_int, C.c_int, C.c_void_p]),
    ("fvad_engine_stream_vadm_config", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    ("fvad_engine_segments", C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    ("fvad_engine_segments_range", C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t]),
    ("fvad_engine_vadm_state", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64)]),
    ("fvad_engine_vadm_snapshot", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    ("fvad_engine_vadm_rolling", C.c_long, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    ("fvad_engine_enable_events", C.c_int, [C.c_void_p, C.c_size_t]),
    ("fvad_engine_poll_events", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                          C.POINTER(C.c_uint64)]),
    ("fvad_engine_event_progress", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("fvad_engine_event_times", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("fvad_engine_enable_capture", C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_size_t]),
    ("fvad_engine_poll_clip", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]),
    ("fvad_engine_capture_flush", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("fvad_engine_capture_times", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("fvad_capture_config_default", None, [C.c_void_p]),
    ("fvad_engine_enable_capture_ex", C.c_int, [C.c_void_p, C.c_void_p]),
    ("fvad_engine_poll_clip_s16", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]),
    ("fvad_engine_clip_rate", C.c_int, [C.c_void_p]),
    ("fvad_pcm_f32_to_s16", None, [F32P, C.POINTER(C.c_int16), C.c_size_t]),
    ("fvad_clip_range", C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("fvad_engine_set_debug", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("fvad_engine_debug_counts", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("fvad_engine_share_streams", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("fvad_engine_output_log", C.c_int, [C.c_void_p, C.c_int]),
    ("fvad_engine_output_log_read", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    ("fvad_engine_clear_times", C.c_int, [C.c_void_p]),
    ("fvad_engine_fetch", C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    ("fvad_resample_info", C.c_int, [C.c_int, C.c_void_p]),
    ("fvad_resample_taps", C.c_size_t, [C.c_int, F32P, C.c_size_t]),
    ("fvad_resample_host", C.c_int, [C.c_int, F32P, C.c_size_t, F32P, F32P]),
    ("fvad_engine_input_frame", C.c_int, [C.c_void_p]),
    ("fvad_engine_fetch_input", C.c_int, [C.c_void_p, C.c_int, F32P]),
    ("fvad_input_layout", C.c_int, [I32P, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    ("fvad_engine_input_layout", C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("fvad_engine_set_stream_rates", C.c_int, [C.c_void_p, I32P, C.c_int, I32P]),
    ("fvad_engine_stream_rates", C.c_int, [C.c_void_p, I32P]),
    ("fvad_engine_resample_times", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("fvad_resample_out_info", C.c_int, [C.c_int, C.c_void_p]),
    ("fvad_resample_out_taps", C.c_size_t, [C.c_int, F32P, C.c_size_t]),
    ("fvad_resample_out_host", C.c_int, [C.c_int, F32P, C.c_size_t, F32P, F32P]),
    ("fvad_engine_denoised_frame", C.c_int, [C.c_void_p]),
    ("fvad_engine_resample_out_times", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("fvad_denoised_layout", C.c_int, [I32P, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    ("fvad_engine_denoised_layout", C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("fvad_engine_set_stream_denoised_rates", C.c_int, [C.c_void_p, I32P, C.c_int, I32P]),
    ("fvad_engine_stream_denoised_rates", C.c_int, [C.c_void_p, I32P]),
    ("fvad_engine_spectrum_bins", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("fvad_engine_fetch_spectrum", C.c_int, [C.c_void_p, C.c_int, F32P]),
    ("fvad_vadm_config_default", None, [C.c_void_p]),
    ("fvad_vadm_create", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("fvad_vadm_destroy", None, [C.c_void_p]),
    ("fvad_vadm_bins", None, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("fvad_vadm_run", C.c_int, [C.c_void_p, C.c_uint64, F32P, C.c_float, C.c_float]),
    ("fvad_vadm_segments", C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("fvad_vadm_state", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("fvad_pipeline_create", C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                       C.POINTER(C.c_void_p)]),
    ("fvad_pipeline_destroy", None, [C.c_void_p]),
    ("fvad_pipeline_push", C.c_int, [C.c_void_p, C.POINTER(F32P), C.c_size_t, C.POINTER(C.c_uint64)]),
    ("fvad_pipeline_segments", C.c_size_t, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    ("fvad_recording_channel", C.c_int, [C.POINTER(F32P), C.c_int, C.c_size_t]),
    ("fvad_pipeline_set_recorder", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("fvad_multi_create", C.c_int, [C.c_int, C.c_int, C.c_void_p, I32P, C.c_int, C.c_void_p, C.c_int,
                                    C.POINTER(C.c_void_p)]),
    ("fvad_multi_create_ex", C.c_int, [C.c_int, I32P, C.c_void_p, I32P, C.c_int, C.c_void_p, C.c_int,
                                       C.POINTER(C.c_void_p)]),
    ("fvad_multi_run_stream", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("fvad_multi_segments_alt", C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    ("fvad_vad_config_default", None, [C.c_void_p]),
    ("fvad_pipeline_create_ex", C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    ("fvad_multi_destroy", None, [C.c_void_p]),
    ("fvad_multi_run", C.c_int, [C.c_void_p, C.POINTER(F32P), C.POINTER(C.c_size_t)]),
    ("fvad_multi_segments", C.c_size_t, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    ("fvad_eval_stats", C.c_int, [F32P, C.c_size_t, F32P, C.c_size_t, C.c_void_p, C.c_void_p]),
    ("fvad_eval_aggregate", None, [C.c_void_p, C.c_size_t, C.c_void_p]),
    ("fvad_parse_audacity", C.c_long, [C.c_char_p, C.c_size_t, F32P, C.c_size_t]),
    ("fvad_sweep_create", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    ("fvad_sweep_destroy", None, [C.c_void_p]),
    ("fvad_sweep_set_windows", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, F32P, F32P, F32P]),
    ("fvad_sweep_append_outputs", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, I32P]),
    ("fvad_sweep_run", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("fvad_sweep_run_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("fvad_sweep_segments", C.c_size_t, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t]),
    ("fvad_sweep_counts", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("fvad_sweep_snapshot", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]),
    ("fvad_sweep_score", C.c_int, [C.c_void_p, C.POINTER(F32P), C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    ("fvad_sweep_run_score", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(F32P), C.POINTER(C.c_size_t),
                                       C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    ("fvad_sweep_last_run", C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int),
                                      C.POINTER(C.c_size_t)]),
    ("fvad_sweep_bytes", C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("fvad_sweep_create_spectral", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("fvad_sweep_set_spectra", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, F32P, F32P, F32P]),
    ("fvad_sweep_append_spectra", C.c_int, [C.c_void_p, C.c_void_p, F32P, C.c_int, I32P]),
    ("fvad_sweep_bandmin_ms", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("fvad_sweep_set_debug", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("fvad_sweep_debug_counts", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("fvad_synth_stream", C.c_long, [C.c_uint32, C.c_size_t, C.c_int, F32P, F32P, C.c_size_t]),
    ("fvad_synth_ticks", C.c_int, [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, F32P]),
    ("fvad_synth_cache_clear", None, []),
    ("fvad_simulator_main", C.c_int, [C.c_int, C.POINTER(C.c_char_p)]),
]

_lib = None


def lib():
    """Load libfvad.so (built in-tree by `make -C formula-vad_amd`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FvadError("libfvad.so not built: run `make -C formula-vad_amd` (%s)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error():
    return lib().fvad_last_error().decode()


def _check(rc, what):
    if rc != FVAD_OK:
        err = FvadError("%s failed (%d): %s" % (what, rc, last_error()))
        err.code = rc
        raise err


EINVAL, EFORMAT = -1, -5


def _ids(ids):
    a = np.ascontiguousarray(list(ids) if not isinstance(ids, np.ndarray) else ids, np.int64)
    if a.ndim != 1 or (a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31)):
        raise ValueError("stream indices: a flat list of 32-bit integers")
    return np.ascontiguousarray(a, np.int32)


def stream_blob_info(blob):
    """fvad_stream_blob_info: the validated header of a stream blob as a dict (host only)."""
    b = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if not isinstance(blob, np.ndarray) else blob, np.uint8)
    h = StreamBlobHeader()
    _check(lib().fvad_stream_blob_info(b.ctypes.data_as(C.c_void_p), b.size, C.byref(h)), "fvad_stream_blob_info")
    return {n: getattr(h, n) for n, _ in h._fields_ if n != "reserved"}


def fptr(a):
    return a.ctypes.data_as(F32P)


class Model:
    def __init__(self, seed=None, path=None):
        h = C.c_void_p()
        if path is not None:
            _check(lib().fvad_model_load_text(path.encode(), C.byref(h)), "fvad_model_load_text")
        else:
            _check(lib().fvad_model_synthetic(0 if seed is None else seed, C.byref(h)), "fvad_model_synthetic")
        self.h = h

    def blob(self):
        n = lib().fvad_model_blob(self.h, None)
        b = np.zeros(n, np.int8)
        lib().fvad_model_blob(self.h, b.ctypes.data_as(C.c_void_p))
        return b

    def __del__(self):
        try:
            lib().fvad_model_free(self.h)
        except Exception:
            pass


def synth_stream(stream_id, n_samples, n_channels=2, label_cap=4096):
    """Synthetic 48 kHz onboard audio (planar [ch][n]) and its speech labels (seconds)."""
    out = np.zeros((n_channels, n_samples), np.float32)
    lab = np.zeros(2 * label_cap, np.float32)
    n = lib().fvad_synth_stream(stream_id, n_samples, n_channels, fptr(out), fptr(lab), label_cap)
    return out, lab[: 2 * min(n, label_cap)].reshape(-1, 2).copy()


def synth_ticks(base, n_streams, n_channels, total_ticks, tick0=0, n_ticks=None, out=None):
    """fvad_synth_ticks: [n_ticks][n_streams][n_channels][480] of the streams
    base.. generated at total_ticks * 480 samples (nothing cached); into `out`
    (a C-contiguous float32 array of that shape, e.g. a pinned input slot) if given."""
    n_ticks = total_ticks - tick0 if n_ticks is None else n_ticks
    shape = (n_ticks, n_streams, n_channels, FRAME)
    if out is None:
        out = np.zeros(shape, np.float32)
    elif out.shape != shape or out.dtype != np.float32 or not out.flags.c_contiguous:
        raise ValueError("synth_ticks: out must be C-contiguous float32 %s" % (shape,))
    _check(lib().fvad_synth_ticks(base, n_streams, n_channels, total_ticks, tick0, n_ticks, fptr(out)),
           "fvad_synth_ticks")
    return out


def synth_cache_clear():
    lib().fvad_synth_cache_clear()


def resample_info(input_rate):
    """fvad_resample_info: the resampler of an input rate as a dict -- L, M,
    taps_per_phase, frame_in and the delay in 48 kHz samples (host only)."""
    d = ResampleDesc()
    _check(lib().fvad_resample_info(input_rate, C.byref(d)), "fvad_resample_info")
    return {n: getattr(d, n) for n, _ in d._fields_}


def resample_taps(input_rate):
    """fvad_resample_taps: the [L][taps_per_phase] float32 tap table (host only)."""
    d = resample_info(input_rate)
    out = np.zeros((d["L"], d["taps_per_phase"]), np.float32)
    n = lib().fvad_resample_taps(input_rate, fptr(out), out.size)
    assert n == out.size, (n, out.shape)
    return out


def resample_host(input_rate, x, tail=None):
    """fvad_resample_host: one channel's whole ticks x ([n_ticks * frame_in]
    float32) at 48 kHz ([n_ticks * 480]), the arithmetic of the engine's
    k_resample.  tail (float32 [taps_per_phase - 1], updated in place): the
    samples before x[0]; None: zeros, nothing kept."""
    d = resample_info(input_rate)
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    assert x.size % d["frame_in"] == 0, (x.size, d["frame_in"])
    n_ticks = x.size // d["frame_in"]
    if tail is not None:
        assert tail.dtype == np.float32 and tail.flags.c_contiguous and tail.size == d["taps_per_phase"] - 1
    out = np.zeros(n_ticks * FRAME, np.float32)
    _check(lib().fvad_resample_host(input_rate, fptr(x), n_ticks, fptr(tail) if tail is not None else None,
                                    fptr(out)), "fvad_resample_host")
    return out


INPUT_RATE_PER_STREAM = -1
ERATE = -6


def input_layout(rates, n_channels):
    """fvad_input_layout (host only): offsets[n_streams + 1] (int64) of a per-stream
    engine's packed push [tick][stream][channel][rate(stream) / 100] -- offsets[s] is
    stream s's first sample inside a tick, offsets[-1] a tick's length in samples."""
    r = _ids(rates)
    off = np.zeros(r.size + 1, np.int64)
    _check(lib().fvad_input_layout(r.ctypes.data_as(I32P), r.size, n_channels,
                                   off.ctypes.data_as(C.POINTER(C.c_int64))), "fvad_input_layout")
    return off


DENOISED_RATE_PER_STREAM = -1


def denoised_layout(rates, n_channels):
    """fvad_denoised_layout (host only): offsets[n_streams + 1] (int64) of the packed
    denoised PCM [tick][stream][channel][rate(stream) / 100] of an engine of per-stream
    denoised rates -- offsets[s] is stream s's first sample inside a tick, offsets[-1] a
    tick's length in samples."""
    r = _ids(rates)
    off = np.zeros(r.size + 1, np.int64)
    _check(lib().fvad_denoised_layout(r.ctypes.data_as(I32P), r.size, n_channels,
                                      off.ctypes.data_as(C.POINTER(C.c_int64))), "fvad_denoised_layout")
    return off


def resample_out_info(rate):
    """fvad_resample_out_info: the downsampler from 48 kHz to rate as a dict --
    L, M, taps_per_phase, frame_out and the delay in 48 kHz samples (host only)."""
    d = ResampleOutDesc()
    _check(lib().fvad_resample_out_info(rate, C.byref(d)), "fvad_resample_out_info")
    return {n: getattr(d, n) for n, _ in d._fields_}


def resample_out_taps(rate):
    """fvad_resample_out_taps: the [L][taps_per_phase] float32 tap table (host only)."""
    d = resample_out_info(rate)
    out = np.zeros((d["L"], d["taps_per_phase"]), np.float32)
    n = lib().fvad_resample_out_taps(rate, fptr(out), out.size)
    assert n == out.size, (n, out.shape)
    return out


def resample_out_host(rate, y, tail=None):
    """fvad_resample_out_host: one channel's whole 48 kHz ticks y ([n_ticks * 480]
    float32) at rate ([n_ticks * frame_out]), the arithmetic of the engine's
    k_resample_out.  tail (float32 [taps_per_phase - 1], updated in place): the
    samples before y[0]; None: zeros, nothing kept."""
    d = resample_out_info(rate)
    y = np.ascontiguousarray(y, np.float32).reshape(-1)
    assert y.size % FRAME == 0, y.size
    n_ticks = y.size // FRAME
    if tail is not None:
        assert tail.dtype == np.float32 and tail.flags.c_contiguous and tail.size == d["taps_per_phase"] - 1
    out = np.zeros(n_ticks * d["frame_out"], np.float32)
    _check(lib().fvad_resample_out_host(rate, fptr(y), n_ticks, fptr(tail) if tail is not None else None,
                                        fptr(out)), "fvad_resample_out_host")
    return out


def pcm_f32_to_s16(x):
    """fvad_pcm_f32_to_s16: clamp(rint(x * 32768), -32768, 32767), ties to even, NaN -> 0,
    as an int16 array of x's shape -- an s16 capture's conversion (host only)."""
    x = np.ascontiguousarray(x, np.float32)
    q = np.zeros(x.shape, np.int16)
    lib().fvad_pcm_f32_to_s16(fptr(x), q.ctypes.data_as(C.POINTER(C.c_int16)), x.size)
    return q


def clip_range(rate, from48, to48):
    """fvad_clip_range: the samples [first, end) of a signal at rate that the 48 kHz
    range [from48, to48) covers (host only)."""
    a, b = C.c_uint64(), C.c_uint64()
    _check(lib().fvad_clip_range(rate, from48, to48, C.byref(a), C.byref(b)), "fvad_clip_range")
    return a.value, b.value


class Engine:
    """Batched hot path for a partition of streams on one GPU."""

    def __init__(self, model, n_streams, n_channels=2, device=0, max_ticks=100, fft_size=2048, bands=((4, 64),),
                 want_denoised=False, mode="staged", use_denoiser=True, input_rate=48000, spectrum=None,
                 denoised_rate=48000, input_rate_max=0, denoised_rate_max=0):
        cfg = EngineConfig()
        lib().fvad_engine_config_default(C.byref(cfg), n_streams, n_channels)
        cfg.device = device
        cfg.max_ticks = max_ticks
        cfg.fft_size = fft_size
        cfg.n_bands = len(bands)
        for i, (lo, hi) in enumerate(bands):
            cfg.band_lo[i] = lo
            cfg.band_hi[i] = hi
        # "device": the denoised rows are computed and stay on the device, for a capture of
        # them (enable_capture(source="denoised")); nothing of them is copied to the host
        cfg.want_denoised = 2 if want_denoised == "device" else int(want_denoised)
        cfg.mode = {"staged": MODE_STAGED, "fused": MODE_FUSED, "fp16": MODE_FP16, "fp16_fused": MODE_FP16_FUSED,
                    "f32_fast": MODE_F32_FAST}[mode]
        cfg.use_denoiser = int(use_denoiser)
        # 8000 .. 96000: the pushes are at that rate, resampled to 48 kHz on the device
        # "per_stream": every stream has its own rate, at most input_rate_max (set_stream_rates)
        self.per_stream = input_rate in ("per_stream", INPUT_RATE_PER_STREAM)
        cfg.input_rate = INPUT_RATE_PER_STREAM if self.per_stream else 0 if input_rate in (0, 48000) else input_rate
        cfg.input_rate_max = input_rate_max
        # 8000 .. 96000: the denoised PCM comes back at that rate, downsampled on the device
        # (0 and 48000 both mean the 48 kHz signal: passed on as given)
        # "per_stream": every stream's denoised PCM at its own rate, at most denoised_rate_max
        # (set_stream_denoised_rates); out["denoised"] is then a list, one array per stream
        self.per_stream_out = denoised_rate in ("per_stream", DENOISED_RATE_PER_STREAM)
        cfg.denoised_rate = DENOISED_RATE_PER_STREAM if self.per_stream_out else denoised_rate
        cfg.denoised_rate_max = denoised_rate_max
        self._den_layouts, self._den_last = [], None  # the submitted pushes' layouts, oldest first; the last delivered
        # spectrum=(lo, hi): every completed window's magnitudes of the FFT-B bins lo..hi
        # are kept for fetch_spectrum, and push returns them as out["spectrum"]
        if spectrum is not None:
            cfg.want_spectrum, (cfg.spec_lo, cfg.spec_hi) = 1, spectrum
        self.cfg = cfg
        self.model = model
        h = C.c_void_p()
        _check(lib().fvad_engine_create(C.byref(cfg), model.h, C.byref(h)), "fvad_engine_create")
        self.h = h
        self.B, self.C, self.nb = n_streams, n_channels, len(bands)
        self.max_ticks = max_ticks
        # window slots per (tick, stream): 1 for fft_size >= 480, else several
        # (VAD.zig:307-347); with W > 1 the window outputs get a slot axis
        self.wpt = lib().fvad_engine_windows_per_tick(h)
        # input samples per tick and channel: input_rate / 100 (480 at 48 kHz)
        # (a per-stream engine has none: input_layout())
        self.frame_in = None if self.per_stream else lib().fvad_engine_input_frame(h)
        # denoised samples per tick and channel: denoised_rate / 100 (480 at 48 kHz)
        # (an engine of per-stream denoised rates has none: denoised_layout())
        self.frame_out = None if self.per_stream_out else lib().fvad_engine_denoised_frame(h)
        self.n_spec = lib().fvad_engine_spectrum_bins(h, None, None)  # 0: no tap

    def set_stream_rates(self, streams, rates):
        """fvad_engine_set_stream_rates: the listed streams take the listed rates between the
        pushes submitted before and after the call (their resampler history restarts from
        zeros); never waits for the device."""
        a, r = _ids(streams), _ids(rates)
        if a.size != r.size:
            raise ValueError("rates: one per listed stream")
        _check(lib().fvad_engine_set_stream_rates(self.h, a.ctypes.data_as(I32P), a.size, r.ctypes.data_as(I32P)),
               "fvad_engine_set_stream_rates")

    def stream_rates(self):
        """The rates the next submitted push will use (fvad_engine_stream_rates)."""
        r = np.zeros(self.B, np.int32)
        _check(lib().fvad_engine_stream_rates(self.h, r.ctypes.data_as(I32P)), "fvad_engine_stream_rates")
        return [int(v) for v in r]

    def input_layout(self):
        """fvad_engine_input_layout: input_layout() over the engine's current rates."""
        off = np.zeros(self.B + 1, np.int64)
        _check(lib().fvad_engine_input_layout(self.h, off.ctypes.data_as(C.POINTER(C.c_int64))),
               "fvad_engine_input_layout")
        return off

    def set_stream_denoised_rates(self, streams, rates):
        """fvad_engine_set_stream_denoised_rates: the listed streams' denoised PCM comes back at
        the listed rates from the next submitted push on (their history, 48 kHz samples, is
        kept: no onset transient); never waits for the device."""
        a, r = _ids(streams), _ids(rates)
        if a.size != r.size:
            raise ValueError("rates: one per listed stream")
        _check(lib().fvad_engine_set_stream_denoised_rates(self.h, a.ctypes.data_as(I32P), a.size,
                                                           r.ctypes.data_as(I32P)),
               "fvad_engine_set_stream_denoised_rates")

    def stream_denoised_rates(self):
        """The denoised rates the next submitted push will use (fvad_engine_stream_denoised_rates)."""
        r = np.zeros(self.B, np.int32)
        _check(lib().fvad_engine_stream_denoised_rates(self.h, r.ctypes.data_as(I32P)),
               "fvad_engine_stream_denoised_rates")
        return [int(v) for v in r]

    def denoised_layout(self):
        """fvad_engine_denoised_layout: denoised_layout() over the engine's current rates, the
        layout the next submitted push is delivered in."""
        off = np.zeros(self.B + 1, np.int64)
        _check(lib().fvad_engine_denoised_layout(self.h, off.ctypes.data_as(C.POINTER(C.c_int64))),
               "fvad_engine_denoised_layout")
        return off

    def unpack_denoised(self, flat, n_ticks, layout=None):
        """The packed denoised PCM of n_ticks ticks, [tick][stream][channel][rate / 100], as one
        [ticks][channels][rate / 100] array per stream.  layout: the offsets the push was
        submitted under (default: the current denoised_layout())."""
        off = self.denoised_layout() if layout is None else np.asarray(layout, np.int64)
        tick = int(off[-1])
        ticks = np.asarray(flat).reshape(-1)[: n_ticks * tick].reshape(n_ticks, tick)
        return [ticks[:, off[s]:off[s + 1]].reshape(n_ticks, self.C, int(off[s + 1] - off[s]) // self.C)
                for s in range(len(off) - 1)]

    def pack_input(self, rows):
        """rows: one [ticks][channels][rate / 100] array per stream, all float32 or all int16.
        Returns the packed push of the current layout, 1-D, [tick][stream][channel][rate / 100]."""
        off = self.input_layout()
        rows = [np.asarray(x) for x in rows]
        if len(rows) != self.B:
            raise ValueError("rows: one array per stream")
        dt = np.int16 if rows[0].dtype == np.int16 else np.float32
        T = rows[0].shape[0]
        out = np.zeros((T, int(off[-1])), dt)
        for s, x in enumerate(rows):
            n = int(off[s + 1] - off[s])
            if x.shape != (T, self.C, n // self.C) or (dt == np.int16) != (x.dtype == np.int16):
                raise ValueError("rows[%d]: shape %s, dtype %s; expected (%d, %d, %d) %s"
                                 % (s, x.shape, x.dtype, T, self.C, n // self.C, np.dtype(dt).name))
            out[:, off[s]:off[s + 1]] = x.reshape(T, n)
        return out.reshape(-1)

    def _slot_samples(self):
        return self.max_ticks * self.B * self.C * (self.cfg.input_rate_max // 100)

    def _packed(self, pcm, dtype):
        """A per-stream engine's push: the packed 1-D array, and its ticks."""
        pcm = np.ascontiguousarray(pcm, dtype).reshape(-1)
        tick = int(self.input_layout()[-1])
        if pcm.size == 0 or pcm.size % tick:
            raise ValueError("packed push: %d samples are no multiple of a tick's %d" % (pcm.size, tick))
        return pcm, pcm.size // tick

    def _alloc_out(self, n_ticks, denoised):
        T, B, Ch, nb, W = n_ticks, self.B, self.C, self.nb, self.wpt
        ws = (T, B) if W == 1 else (T, B, W)
        o = {"vad": np.zeros((T, B), np.float32), "ratio": np.zeros((T, B), np.float32),
             "win_flag": np.zeros((T, B), np.int32), "win_ratio": np.zeros(ws, np.float32),
             "win_vad": np.zeros(ws, np.float32), "band": np.zeros(ws + (Ch, nb), np.float32)}
        if denoised and self.per_stream_out:  # (packed: max_ticks-proof for any layout of the push)
            o["denoised"] = np.zeros(T * B * Ch * (self.cfg.denoised_rate_max // 100), np.float32)
        elif denoised:
            o["denoised"] = np.zeros((T, B, Ch, self.frame_out), np.float32)
        s = Outputs(fptr(o["vad"]), fptr(o["ratio"]), o["win_flag"].ctypes.data_as(I32P), fptr(o["win_ratio"]),
                    fptr(o["win_vad"]), fptr(o["band"]), fptr(o["denoised"]) if denoised else None)
        return o, s

    def push(self, pcm, ticks_valid=None, denoised=False, last_tick_samples=None):
        """pcm: [ticks][streams][channels][frame_in] normalised f32; last_tick_samples
        (no-denoiser engines): real samples in each stream's last valid tick."""
        if self.per_stream:
            pcm, T = self._packed(pcm, np.float32)
        else:
            pcm = np.ascontiguousarray(pcm, np.float32)
            T = pcm.shape[0]
            assert pcm.shape[1:] == (self.B, self.C, self.frame_in), pcm.shape
        o, s = self._alloc_out(T, denoised)
        lay = self.denoised_layout() if self.per_stream_out else None  # (the layout this push is delivered in)
        tv = None
        if ticks_valid is not None:
            tv = np.ascontiguousarray(ticks_valid, np.int32)
        lt = np.ascontiguousarray(last_tick_samples, np.int32) if last_tick_samples is not None else None
        _check(lib().fvad_engine_push_ex(self.h, fptr(pcm), T, tv.ctypes.data_as(I32P) if tv is not None else None,
                                         lt.ctypes.data_as(I32P) if lt is not None else None, C.byref(s)),
               "fvad_engine_push_ex")
        if self.per_stream_out:
            self._den_last = lay
            if denoised:
                o["denoised"] = self.unpack_denoised(o["denoised"], T, lay)
        if self.n_spec:
            o["spectrum"] = self.fetch_spectrum(T)
        return o

    def input_slot(self):
        """The engine's pinned input slot for the next submit, as a
        [max_ticks][streams][channels][frame_in] float32 view (fill it in place
        and pass it to submit: no host copy)."""
        p = lib().fvad_engine_input_slot(self.h)
        if not p:
            raise FvadError("fvad_engine_input_slot: %s" % last_error())
        if self.per_stream:  # (flat: max_ticks ticks of the highest rate)
            return np.ctypeslib.as_array(C.cast(p, F32P), shape=(self._slot_samples(),))
        n = self.max_ticks * self.B * self.C * self.frame_in
        arr = np.ctypeslib.as_array(C.cast(p, F32P), shape=(n,))
        return arr.reshape(self.max_ticks, self.B, self.C, self.frame_in)

    def submit(self, pcm, ticks_valid=None):
        """Asynchronous push (fvad_engine_submit): returns once queued."""
        if self.per_stream:
            pcm, T = self._packed(pcm, np.float32)
        else:
            pcm = np.ascontiguousarray(pcm, np.float32)
            assert pcm.shape[1:] == (self.B, self.C, self.frame_in), pcm.shape
            T = pcm.shape[0]
        tv = np.ascontiguousarray(ticks_valid, np.int32) if ticks_valid is not None else None
        self._sub_keep = tv
        _check(lib().fvad_engine_submit(self.h, fptr(pcm), T,
                                        tv.ctypes.data_as(I32P) if tv is not None else None), "fvad_engine_submit")
        if self.per_stream_out:
            self._den_layouts.append(self.denoised_layout())

    def input_slot_i16(self):
        """The pinned 16-bit input slot for the next submit_i16, as a
        [max_ticks][streams][channels][frame_in] int16 view."""
        p = lib().fvad_engine_input_slot_i16(self.h)
        if not p:
            raise FvadError("fvad_engine_input_slot_i16: %s" % last_error())
        if self.per_stream:
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int16)), shape=(self._slot_samples(),))
        n = self.max_ticks * self.B * self.C * self.frame_in
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int16)), shape=(n,))
        return arr.reshape(self.max_ticks, self.B, self.C, self.frame_in)

    def submit_i16(self, pcm, ticks_valid=None, last_tick_samples=None):
        """Asynchronous push of 16-bit samples k (fvad_engine_submit_i16): the
        same outputs as submit() of k / 32768.0f, half the PCIe bytes."""
        if self.per_stream:
            pcm, T = self._packed(pcm, np.int16)
        else:
            pcm = np.ascontiguousarray(pcm, np.int16)
            assert pcm.shape[1:] == (self.B, self.C, self.frame_in), pcm.shape
            T = pcm.shape[0]
        tv = np.ascontiguousarray(ticks_valid, np.int32) if ticks_valid is not None else None
        lt = np.ascontiguousarray(last_tick_samples, np.int32) if last_tick_samples is not None else None
        self._sub_keep = (tv, lt)
        _check(lib().fvad_engine_submit_i16(self.h, pcm.ctypes.data_as(C.POINTER(C.c_int16)), T,
                                            tv.ctypes.data_as(I32P) if tv is not None else None,
                                            lt.ctypes.data_as(I32P) if lt is not None else None),
               "fvad_engine_submit_i16")
        if self.per_stream_out:
            self._den_layouts.append(self.denoised_layout())

    def collect(self, denoised=False, want=True):
        """Outputs of the oldest submitted push (fvad_engine_collect)."""
        if not want:
            _check(lib().fvad_engine_collect(self.h, None, None), "fvad_engine_collect")
            if self.per_stream_out:
                self._den_last = self._den_layouts.pop(0)
            return None
        o, s = self._alloc_out(self.max_ticks, denoised)
        n = C.c_int()
        _check(lib().fvad_engine_collect(self.h, C.byref(s), C.byref(n)), "fvad_engine_collect")
        if self.per_stream_out:  # the layout this push was submitted under
            self._den_last = self._den_layouts.pop(0)
            den = o.pop("denoised", None)
            o = {k: v[: n.value] for k, v in o.items()}
            if den is not None:
                o["denoised"] = self.unpack_denoised(den, n.value, self._den_last)
            return o
        return {k: v[: n.value] for k, v in o.items()}

    def reset(self):
        _check(lib().fvad_engine_reset(self.h), "fvad_engine_reset")

    def reset_streams(self, ids):
        """The listed streams as fvad_engine_reset leaves them, between the pushes
        submitted before and after the call; never waits for the device."""
        a = _ids(ids)
        _check(lib().fvad_engine_reset_streams(self.h, a.ctypes.data_as(I32P), a.size), "fvad_engine_reset_streams")

    def save_streams(self, ids):
        """The listed streams' whole state as a blob (np.uint8; a sync point)."""
        a = _ids(ids)
        blob = np.zeros(lib().fvad_engine_save_size(self.h, a.size), np.uint8)
        _check(lib().fvad_engine_save_streams(self.h, a.ctypes.data_as(I32P), a.size,
                                              blob.ctypes.data_as(C.c_void_p), blob.size), "fvad_engine_save_streams")
        return blob

    def restore_streams(self, ids, blob, index=None):
        """Record index[i] of the blob (default i) into slot ids[i] (a sync point)."""
        a = _ids(ids)
        b = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if not isinstance(blob, np.ndarray) else blob, np.uint8)
        ix = _ids(index) if index is not None else None
        if ix is not None and ix.size != a.size:
            raise ValueError("index: one record per listed stream")
        _check(lib().fvad_engine_restore_streams(self.h, a.ctypes.data_as(I32P), a.size, b.ctypes.data_as(C.c_void_p),
                                                 b.size, ix.ctypes.data_as(I32P) if ix is not None else None),
               "fvad_engine_restore_streams")

    def reset_times(self):
        """DEBUG_RESET_TIMES' samples: ({stream: ms average}, {stream: runs})."""
        ms, n = (C.c_double * 3)(), (C.c_int * 3)()
        _check(lib().fvad_engine_reset_times(self.h, ms, n), "fvad_engine_reset_times")
        names = ("main", "prep", "side")
        return dict(zip(names, ms)), dict(zip(names, n))

    def load_synthetic(self, n_ticks, base=0, pushes=1):
        """pushes distinct resident pushes of n_ticks (run_resident cycles through them)."""
        _check(lib().fvad_engine_load_synthetic_ex(self.h, n_ticks, pushes, base), "fvad_engine_load_synthetic_ex")

    def resident_seek(self, push):
        _check(lib().fvad_engine_resident_seek(self.h, push), "fvad_engine_resident_seek")

    def run_resident(self, n_ticks):
        _check(lib().fvad_engine_run_resident(self.h, n_ticks), "fvad_engine_run_resident")

    def sync(self):
        _check(lib().fvad_engine_sync(self.h), "fvad_engine_sync")

    def kernel_times(self):
        """{"total_ms": push average, "kernels": {name: ms average}, "runs": n}"""
        ms = (C.c_double * MAX_TIMES)()
        n = C.c_int()
        _check(lib().fvad_engine_kernel_times(self.h, ms, C.byref(n)), "fvad_engine_kernel_times")
        names = []
        while len(names) < MAX_TIMES - 1:
            nm = lib().fvad_engine_kernel_name(self.h, len(names))
            if nm is None:
                break
            names.append(nm.decode())
        return {"total_ms": ms[0], "kernels": {nm: ms[1 + i] for i, nm in enumerate(names)}, "runs": n.value}

    def clear_times(self):
        _check(lib().fvad_engine_clear_times(self.h), "fvad_engine_clear_times")

    def attach_vadm(self, cfgs=None, seg_capacity=256, room=None):
        """Run VADMachines on the device after every push (default config if None).
        room not None (a list of VadmConfig, [] allowed): a config per (machine, stream)
        that set_stream_vadm can change later (fvad_engine_attach_vadm_ex); every stream
        starts on cfgs[m], and the rolling buffers are sized for cfgs and room together."""
        cfgs = list(cfgs) if cfgs else [VadmConfig.default()]
        arr = (VadmConfig * len(cfgs))(*cfgs)
        self._vadm_keep = arr
        if room is None:
            _check(lib().fvad_engine_attach_vadm(self.h, arr, len(cfgs), seg_capacity), "fvad_engine_attach_vadm")
            return
        room = list(room)
        rarr = (VadmConfig * max(1, len(room)))(*room)
        _check(lib().fvad_engine_attach_vadm_ex(self.h, arr, len(cfgs), seg_capacity, rarr if room else None,
                                                len(room)), "fvad_engine_attach_vadm_ex")

    def set_stream_vadm(self, ids, cfgs, machine=0):
        """Machine `machine` of stream ids[i] becomes a fresh machine of cfgs[i], between the
        pushes submitted before and after the call; never waits for the device
        (fvad_engine_set_stream_vadm; the engine was attached with room=...)."""
        a = _ids(ids)
        cfgs = list(cfgs)
        if len(cfgs) != a.size:
            raise ValueError("cfgs: one config per listed stream")
        arr = (VadmConfig * max(1, len(cfgs)))(*cfgs)
        _check(lib().fvad_engine_set_stream_vadm(self.h, a.ctypes.data_as(I32P), a.size, machine, arr),
               "fvad_engine_set_stream_vadm")

    def stream_vadm_config(self, stream, machine=0):
        """The VadmConfig (stream, machine) runs now (the host's mirror: no sync)."""
        c = VadmConfig()
        _check(lib().fvad_engine_stream_vadm_config(self.h, stream, machine, C.byref(c)),
               "fvad_engine_stream_vadm_config")
        return c

    def segments(self, stream, machine=0):
        n = lib().fvad_engine_segments(self.h, stream, machine, None, 0)
        buf = (Segment * max(1, n))()
        lib().fvad_engine_segments(self.h, stream, machine, buf, n)
        return [(s.sample_from, s.sample_to, s.debug_rnn_vad, s.debug_avg_speech_vol_ratio) for s in buf[:n]]

    def enable_events(self, capacity=0):
        """Start the speech event feed (fvad_engine_enable_events): after attach_vadm, with
        no submitted push uncollected; capacity events held between polls (0: the default)."""
        _check(lib().fvad_engine_enable_events(self.h, capacity), "fvad_engine_enable_events")

    def poll_events(self, max_events=4096):
        """(events of the machine passes the device has finished, as dicts in feed order;
        events lost to a full ring so far).  Never waits for the device."""
        buf = (Event * max(1, max_events))()
        n, lost = C.c_size_t(), C.c_uint64()
        _check(lib().fvad_engine_poll_events(self.h, buf, max_events, C.byref(n), C.byref(lost)),
               "fvad_engine_poll_events")
        return [buf[i].as_dict() for i in range(n.value)], lost.value

    def event_progress(self):
        """Pushes (ordinals below the result) whose events have all been polled or are ready."""
        n = C.c_uint64()
        _check(lib().fvad_engine_event_progress(self.h, C.byref(n)), "fvad_engine_event_progress")
        return n.value

    def event_times(self):
        """(k_vadm_events' average ms over the timed passes, how many) -- a sync point."""
        ms, n = C.c_double(), C.c_int()
        _check(lib().fvad_engine_event_times(self.h, C.byref(ms), C.byref(n)), "fvad_engine_event_times")
        return ms.value, n.value

    def enable_capture(self, machine=0, history_sec=10.0, pool_samples=0, source="input", fmt="f32"):
        """Record machine's segments on the device (fvad_engine_enable_capture[_ex]): after
        attach_vadm and enable_events; history_sec >= 4 of every stream's input is held,
        pool_samples of finished clips between polls (0: the default, 64 Mi).
        source="denoised": the engine's denoised rows at clip_rate() instead of its input
        (want_denoised=True or "device"); fmt="s16": the clips as 16-bit PCM."""
        if (source, fmt) == ("input", "f32"):
            _check(lib().fvad_engine_enable_capture(self.h, machine, history_sec, pool_samples),
                   "fvad_engine_enable_capture")
        else:
            c = CaptureConfig.default()
            c.machine, c.history_sec, c.pool_samples = machine, history_sec, pool_samples
            c.source = {"input": CLIP_SOURCE_INPUT, "denoised": CLIP_SOURCE_DENOISED}[source]
            c.format = {"f32": CLIP_F32, "s16": CLIP_S16}[fmt]
            _check(lib().fvad_engine_enable_capture_ex(self.h, C.byref(c)), "fvad_engine_enable_capture_ex")
        self._clip_s16 = fmt == "s16"

    def clip_rate(self):
        """Samples per second of the captured clips (fvad_engine_clip_rate): 48000 for the
        input, the engine's denoised rate for the denoised rows, 0 without capture."""
        return lib().fvad_engine_clip_rate(self.h)

    def poll_clips(self):
        """The finished clips, oldest first, as (descriptor dict, samples) -- float32, or
        int16 for an s16 capture; never waits for the device.  A non-zero `reserved` is
        decoded into the keys rate, format and source beside it.  The clips lost so far:
        capture_lost()."""
        out = []
        info, lost = Clip(), C.c_uint64()
        s16 = getattr(self, "_clip_s16", False)
        poll, name, dtype = (lib().fvad_engine_poll_clip_s16, "fvad_engine_poll_clip_s16", np.int16) if s16 else \
            (lib().fvad_engine_poll_clip, "fvad_engine_poll_clip", np.float32)
        buf = np.zeros(0, dtype)
        while True:
            rc = poll(self.h, C.byref(info), buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(lost))
            if rc == -1 and info.n_samples > buf.size:  # FVAD_EINVAL: the clip is still queued, its size known
                buf = np.zeros(int(info.n_samples), dtype)
                continue
            _check(min(rc, 0), name)
            self._clips_lost = lost.value
            if rc == 0:
                return out
            d = info.as_dict()
            if d["reserved"]:
                d.update(rate=d["reserved"] & 0xffffffff, format=d["reserved"] >> 32 & 0xff, source=d["reserved"] >> 40 & 0xff)
            out.append((d, buf[: info.n_samples].copy()))

    def capture_lost(self):
        """Clips that lost their audio or their descriptor so far, as of the last poll_clips()."""
        return getattr(self, "_clips_lost", 0)

    def capture_flush(self, ids=None):
        """Complete the listed streams' pending clips now (None: every stream's), cut at
        the stream's current sample count (fvad_engine_capture_flush; a sync point)."""
        if ids is None:
            _check(lib().fvad_engine_capture_flush(self.h, None, 0), "fvad_engine_capture_flush")
            return
        a = _ids(ids)
        _check(lib().fvad_engine_capture_flush(self.h, a.ctypes.data_as(C.c_void_p), a.size),
               "fvad_engine_capture_flush")

    def capture_times(self):
        """({"k_hist_append": ms, "capture_pass": ms} averages over the timed pushes, how
        many passes) -- a sync point."""
        ms, n = (C.c_double * 2)(), C.c_int()
        _check(lib().fvad_engine_capture_times(self.h, ms, C.byref(n)), "fvad_engine_capture_times")
        return {"k_hist_append": ms[0], "capture_pass": ms[1]}, n.value

    def vadm_snapshot(self, stream, machine=0):
        """The device machine's whole state (fvad_engine_vadm_snapshot) as a dict."""
        s = VadmSnapshot()
        _check(lib().fvad_engine_vadm_snapshot(self.h, stream, machine, C.byref(s)), "fvad_engine_vadm_snapshot")
        return s.as_dict()

    def vadm_rolling(self, stream, which, machine=0):
        """RollingAverage.data (which 0 long-term, 1 short-term, 2 volume ratio) as float64."""
        n = lib().fvad_engine_vadm_rolling(self.h, stream, machine, which, None, 0)
        if n < 0:
            raise FvadError("fvad_engine_vadm_rolling failed (%d): %s" % (n, last_error()))
        out = np.zeros(n, np.float64)
        lib().fvad_engine_vadm_rolling(self.h, stream, machine, which, out.ctypes.data_as(C.c_void_p), n)
        return out

    def share_streams(self, other, which=SHARE_PREP | SHARE_SIDE):
        """Run this engine's k_prep3 / VADMachine kernels on other's streams
        (fvad_engine_share_streams); either engine may be destroyed first:
        the last one using a stream destroys it."""
        _check(lib().fvad_engine_share_streams(self.h, other.h, which), "fvad_engine_share_streams")

    def set_debug(self, key, value):
        """Test hooks (fvad_engine_set_debug): DEBUG_VADM_PAR_SERIAL_EVERY, DEBUG_VADM_ALWAYS_PAR,
        DEBUG_VADM_LT_FULL, DEBUG_VADM_DEFER_MAX, DEBUG_VADM_BOUND_SCALE, DEBUG_VADM_COUNT, DEBUG_EVENTS_CHUNK."""
        _check(lib().fvad_engine_set_debug(self.h, key, value), "fvad_engine_set_debug")

    def debug_counts(self):
        """DEBUG_VADM_COUNT's counters (fvad_engine_debug_counts): long-term tests
        decided exactly / settled by the bound / left open by it (folded), and
        end-of-push folds."""
        out = np.zeros(4, np.uint64)
        n = lib().fvad_engine_debug_counts(self.h, out.ctypes.data_as(C.c_void_p), 4)
        _check(n if n < 0 else 0, "fvad_engine_debug_counts")
        return dict(zip(("exact", "settled", "open", "end_fold"), (int(v) for v in out[:n])))

    def output_log(self, n_pushes):
        """Record the per-tick outputs of the next n_pushes pushes on the device (no host sync)."""
        _check(lib().fvad_engine_output_log(self.h, n_pushes), "fvad_engine_output_log")

    def output_log_read(self, push):
        o, s = self._alloc_out(self.max_ticks, False)
        n = C.c_int()
        _check(lib().fvad_engine_output_log_read(self.h, push, C.byref(s), C.byref(n)), "fvad_engine_output_log_read")
        return {k: v[: n.value] for k, v in o.items()}

    def fetch_input(self, n_ticks):
        """fvad_engine_fetch_input: the 48 kHz device input of the last push of a
        resampling engine, [n_ticks][streams][channels][480] (a sync point)."""
        out = np.zeros((n_ticks, self.B, self.C, FRAME), np.float32)
        _check(lib().fvad_engine_fetch_input(self.h, n_ticks, fptr(out)), "fvad_engine_fetch_input")
        return out

    def fetch_spectrum(self, n_ticks):
        """fvad_engine_fetch_spectrum: the window spectra of the last launched push,
        [n_ticks][streams]([W])[channels][n_spec] like out["band"] (a sync point)."""
        ws = (n_ticks, self.B) if self.wpt == 1 else (n_ticks, self.B, self.wpt)
        out = np.zeros(ws + (self.C, max(1, self.n_spec)), np.float32)
        _check(lib().fvad_engine_fetch_spectrum(self.h, n_ticks, fptr(out)), "fvad_engine_fetch_spectrum")
        return out

    def resample_times(self):
        """(ms average of a push's resample launches, pushes measured); a sync point."""
        ms, n = C.c_double(), C.c_int()
        _check(lib().fvad_engine_resample_times(self.h, C.byref(ms), C.byref(n)), "fvad_engine_resample_times")
        return ms.value, n.value

    def resample_out_times(self):
        """(ms average of a push's two output-resample launches, pushes measured); a sync point."""
        ms, n = C.c_double(), C.c_int()
        _check(lib().fvad_engine_resample_out_times(self.h, C.byref(ms), C.byref(n)), "fvad_engine_resample_out_times")
        return ms.value, n.value

    def fetch(self, n_ticks, denoised=False):
        o, s = self._alloc_out(n_ticks, denoised)
        _check(lib().fvad_engine_fetch(self.h, n_ticks, C.byref(s)), "fvad_engine_fetch")
        if denoised and self.per_stream_out:  # (the layout of the push launched last)
            o["denoised"] = self.unpack_denoised(o["denoised"], n_ticks, self._den_last)
        return o

    def __del__(self):
        try:
            lib().fvad_engine_destroy(self.h)
        except Exception:
            pass



class EngineGroup:
    """One GPU's streams as `groups` engines of about n_streams / groups each,
    pushing concurrently: each engine its own main stream, k_prep3 and the
    VADMachines of all of them on engine 0's two side streams
    (fvad_engine_share_streams), so a group of two takes 4 streams where two
    separate engines would take 6 (the runtime shares its 4 hardware queues
    round the streams).  Results are each engine's own, bit-identical to one
    engine over all the streams (tests/test_gpu_groups.py).  Throughput
    (DESIGN.md section 8, r5): +2-3 % over one engine when it is the first
    group a process creates, down to -35 % when the runtime's queue placement
    puts a main stream beside the side work -- so bench.py runs one engine per
    GPU unless asked (--groups).  Engine g owns streams
    [first[g], first[g] + sizes[g])."""

    def __init__(self, model, n_streams, n_channels=2, groups=2, vadm=False, seg_capacity=256, vadm_room=None,
                 **kw):
        """vadm_room not None: per-stream configs (Engine.attach_vadm's room) on every engine."""
        if not 1 <= groups <= n_streams:
            raise ValueError("groups must be in [1, n_streams]")
        q, r = divmod(n_streams, groups)
        self.sizes = [q + (1 if g < r else 0) for g in range(groups)]
        self.first = [sum(self.sizes[:g]) for g in range(groups)]
        self.B, self.C = n_streams, n_channels
        self.engines = []
        for g, n in enumerate(self.sizes):
            # engine g's streams exist before engine g + 1's: the runtime hands
            # out hardware queues in creation order
            e = Engine(model, n, n_channels, **kw)
            if vadm:  # True: the default machine; or a list of VadmConfig
                e.attach_vadm(None if vadm is True else vadm, seg_capacity, room=vadm_room)
            if g and kw.get("mode", "staged") != "fused":  # the fused engine has no side streams
                e.share_streams(self.engines[0], SHARE_PREP | (SHARE_SIDE if vadm else 0))
            self.engines.append(e)

    def set_debug(self, key, value):
        for e in self.engines:
            e.set_debug(key, value)

    def load_synthetic(self, n_ticks, base=0, pushes=1):
        for e, f in zip(self.engines, self.first):
            e.load_synthetic(n_ticks, base=base + f, pushes=pushes)

    def run_resident(self, n_ticks):
        for e in self.engines:
            e.run_resident(n_ticks)

    def sync(self):
        for e in self.engines:
            e.sync()

    def clear_times(self):
        for e in self.engines:
            e.clear_times()

    def kernel_times(self):
        """Per kernel the mean over the engines of their launch averages (each
        launch covers one engine's streams, co-running with the others')."""
        ts = [e.kernel_times() for e in self.engines]
        names = ts[0]["kernels"].keys()
        return {"total_ms": sum(t["total_ms"] for t in ts) / len(ts),
                "kernels": {n: sum(t["kernels"].get(n, 0.0) for t in ts) / len(ts) for n in names},
                "runs": min(t["runs"] for t in ts)}

    def segments(self, stream, machine=0):
        g = max(i for i, f in enumerate(self.first) if f <= stream)
        return self.engines[g].segments(stream - self.first[g], machine)

    def enable_events(self, capacity=0):
        """Engine.enable_events on every engine of the group (capacity each)."""
        for e in self.engines:
            e.enable_events(capacity)
        self._ev_q = [[] for _ in self.engines]

    def poll_events(self, max_events=4096):
        """The engines' feeds as one, stream numbers in the group's numbering:
        ascending push, then stream (engine g's streams come before engine
        g + 1's), then each engine's own order.  A push's events are delivered
        once every engine's machine pass for it has finished
        (Engine.event_progress): (events, lost summed over the engines);
        max_events sizes each engine's polls, not the result."""
        lost = 0
        done = [e.event_progress() for e in self.engines]  # before the polls: all of these get drained
        for g, e in enumerate(self.engines):
            while True:
                ev, l = e.poll_events(max_events)
                for d in ev:
                    d["stream"] += self.first[g]
                self._ev_q[g].extend(ev)
                if len(ev) < max_events:
                    break
            lost += l
        upto = min(done)
        out = []
        for g in range(len(self.engines)):
            q = self._ev_q[g]
            k = 0
            while k < len(q) and q[k]["push"] < upto:
                k += 1
            out.extend(q[:k])
            del q[:k]
        out.sort(key=lambda d: d["push"])  # stable: engines are already in stream order
        return out, lost

    def reset_streams(self, global_ids):
        """Engine.reset_streams over the group's stream numbering."""
        ids = _ids(global_ids)
        if ids.size and (ids.min() < 0 or ids.max() >= self.B):
            raise ValueError("stream index out of range")
        if len(set(ids.tolist())) != ids.size:
            raise ValueError("duplicate stream index")
        for e, f, n in zip(self.engines, self.first, self.sizes):
            mine = ids[(ids >= f) & (ids < f + n)] - f
            if mine.size:
                e.reset_streams(mine)

    def set_stream_vadm(self, global_ids, cfgs, machine=0):
        """Engine.set_stream_vadm over the group's stream numbering."""
        ids = _ids(global_ids)
        cfgs = list(cfgs)
        if len(cfgs) != ids.size:
            raise ValueError("cfgs: one config per listed stream")
        if ids.size and (ids.min() < 0 or ids.max() >= self.B):
            raise ValueError("stream index out of range")
        if len(set(ids.tolist())) != ids.size:
            raise ValueError("duplicate stream index")
        for e, f, n in zip(self.engines, self.first, self.sizes):
            pick = np.flatnonzero((ids >= f) & (ids < f + n))
            if pick.size:
                e.set_stream_vadm(ids[pick] - f, [cfgs[i] for i in pick], machine)

class Denoiser:
    """src/Denoiser.zig over the rnnoise_* C ABI (GPU, batch of one)."""

    def __init__(self, model=None):
        self.model = model
        self.h = lib().rnnoise_create(model.h if model is not None else None)
        if not self.h:
            raise FvadError("rnnoise_create failed: %s" % last_error())

    @staticmethod
    def get_frame_size():
        return lib().rnnoise_get_frame_size()

    def process_s16(self, frame):
        frame = np.ascontiguousarray(frame, np.float32)
        if frame.shape != (FRAME,):
            raise ValueError("InvalidFrameSize")
        out = np.zeros(FRAME, np.float32)
        vad = lib().rnnoise_process_frame(self.h, fptr(out), fptr(frame))
        return out, vad

    def denoise(self, samples):
        """Denoiser.denoise: normalised [-1,1] in, normalised out, returns (out, vad)."""
        samples = np.asarray(samples, np.float32)
        if samples.shape != (FRAME,):
            raise ValueError("InvalidFrameSize")
        scaled = samples * np.float32(32767)
        out, vad = self.process_s16(scaled)
        return out * (np.float32(1.0) / np.float32(32767)), vad

    def __del__(self):
        try:
            lib().rnnoise_destroy(self.h)
        except Exception:
            pass


def kiss_fftr(x):
    """kiss_fftr over the GPU compat shim; returns complex64[n/2+1]."""
    x = np.ascontiguousarray(x, np.float32)
    n = len(x)
    lenmem = C.c_size_t(1)
    if lib().kiss_fftr_alloc(n, 0, None, C.byref(lenmem)) is not None:
        raise FvadError("size probe must fail")
    if lenmem.value == 0:
        raise ValueError("unsupported nfft %d" % n)
    mem = C.create_string_buffer(lenmem.value)
    cfg = lib().kiss_fftr_alloc(n, 0, mem, C.byref(lenmem))
    if not cfg:
        raise FvadError("kiss_fftr_alloc failed")
    out = np.zeros(2 * (n // 2 + 1), np.float32)
    lib().kiss_fftr(cfg, fptr(x), out.ctypes.data_as(C.c_void_p))
    return out[0::2] + 1j * out[1::2]


def vadm_lengths(cfg, sample_rate=48000, fft_size=2048):
    """(long-term, short-term, volume ratio) RollingAverage lengths cfg needs (fvad_vadm_lengths):
    what an Engine.attach_vadm room has to cover for set_stream_vadm to accept cfg."""
    out = (C.c_int * 3)()
    _check(lib().fvad_vadm_lengths(C.byref(cfg) if cfg is not None else None, sample_rate, fft_size, out),
           "fvad_vadm_lengths")
    return tuple(out)


class VADMachine:
    """src/AudioPipeline/VADMachine.zig (host decision logic)."""

    def __init__(self, cfg=None, n_channels=2, sample_rate=48000, fft_size=2048):
        c = cfg if cfg is not None else VadmConfig.default()
        self._cfg = c
        self.n_channels = n_channels
        h = C.c_void_p()
        _check(lib().fvad_vadm_create(C.byref(c), sample_rate, fft_size, n_channels, C.byref(h)), "fvad_vadm_create")
        self.h = h

    def bins(self):
        lo, hi = C.c_int(), C.c_int()
        lib().fvad_vadm_bins(self.h, C.byref(lo), C.byref(hi))
        return lo.value, hi.value

    def run(self, index, band_per_channel, vad, vol_ratio):
        b = np.ascontiguousarray(band_per_channel, np.float32)
        _check(lib().fvad_vadm_run(self.h, index, fptr(b), vad, vol_ratio), "fvad_vadm_run")

    def state(self):
        """(speech state 0 closed / 1 opening / 2 open / 3 closing, speech start, speech end)"""
        st, a, b = C.c_int(), C.c_uint64(), C.c_uint64()
        _check(lib().fvad_vadm_state(self.h, C.byref(st), C.byref(a), C.byref(b)), "fvad_vadm_state")
        return st.value, a.value, b.value

    def segments(self):
        n = lib().fvad_vadm_segments(self.h, None, 0)
        buf = (Segment * max(1, n))()
        lib().fvad_vadm_segments(self.h, buf, n)
        return [(s.sample_from, s.sample_to, s.debug_rnn_vad, s.debug_avg_speech_vol_ratio) for s in buf[:n]]

    def __del__(self):
        try:
            lib().fvad_vadm_destroy(self.h)
        except Exception:
            pass


# on_recording callback (fvad_recording_fn)
RECORDING_FN = C.CFUNCTYPE(None, C.c_void_p, F32P, C.c_size_t, C.c_uint64, C.c_int)


def recording_channel(channel_pcm):
    """Recorder.findBestChannel: index of the lowest-rmsVolume channel."""
    chans = [np.ascontiguousarray(c, np.float32) for c in channel_pcm]
    arr = (F32P * len(chans))(*[fptr(c) for c in chans])
    return lib().fvad_recording_channel(arr, len(chans), len(chans[0]))


class AudioPipeline:
    """src/AudioPipeline.zig for one stream (pushSamples -> VAD -> VADMachine)."""

    def __init__(self, model, n_channels=2, sample_rate=48000, device=0, main_cfg=None, alt_cfgs=(),
                 fft_size=2048, use_denoiser=True):
        self.model = model
        vc = VadConfig.make(fft_size, use_denoiser, main_cfg, tuple(alt_cfgs))
        self._keep = (vc,)
        self.n_alt = len(alt_cfgs)
        h = C.c_void_p()
        _check(lib().fvad_pipeline_create_ex(sample_rate, n_channels, model.h, device, C.byref(vc), C.byref(h)),
               "fvad_pipeline_create_ex")
        self.h = h

    def push_samples(self, channel_pcm):
        chans = [np.ascontiguousarray(c, np.float32) for c in channel_pcm]
        arr = (F32P * len(chans))(*[fptr(c) for c in chans])
        first = C.c_uint64()
        _check(lib().fvad_pipeline_push(self.h, arr, len(chans[0]), C.byref(first)), "fvad_pipeline_push")
        return first.value

    def record(self):
        """Attach the Recorder: completed main-machine segments are captured
        into self.recordings as (start_sample, channel, pcm) (on_recording)."""
        self.recordings = []

        def on_rec(ctx, pcm, n, start, channel):
            self.recordings.append((int(start), int(channel), np.ctypeslib.as_array(pcm, shape=(n,)).copy()))

        self._rec_cb = RECORDING_FN(on_rec)
        _check(lib().fvad_pipeline_set_recorder(self.h, C.cast(self._rec_cb, C.c_void_p), None),
               "fvad_pipeline_set_recorder")

    def segments(self, alt=-1):
        n = lib().fvad_pipeline_segments(self.h, alt, None, 0)
        buf = (Segment * max(1, n))()
        lib().fvad_pipeline_segments(self.h, alt, buf, n)
        return [(s.sample_from, s.sample_to, s.debug_rnn_vad, s.debug_avg_speech_vol_ratio) for s in buf[:n]]

    def __del__(self):
        try:
            lib().fvad_pipeline_destroy(self.h)
        except Exception:
            pass


class Multi:
    """Multi-stream simulator core: lock-step ticks, streams grouped by channel
    count and partitioned over devices (fvad_multi_create_ex)."""

    def __init__(self, model, n_streams, n_channels=2, devices=(0,), cfg=None, ticks_per_push=50, fft_size=2048,
                 use_denoiser=True, alt_cfgs=()):
        self.model = model
        self.n = n_streams
        d = np.ascontiguousarray(devices, np.int32)
        ch = np.ascontiguousarray([n_channels] * n_streams if np.isscalar(n_channels) else n_channels, np.int32)
        vc = VadConfig.make(fft_size, use_denoiser, cfg, tuple(alt_cfgs))
        self._keep = (d, ch, vc)
        h = C.c_void_p()
        _check(lib().fvad_multi_create_ex(n_streams, ch.ctypes.data_as(I32P), model.h, d.ctypes.data_as(I32P), len(d),
                                          C.byref(vc), ticks_per_push, C.byref(h)), "fvad_multi_create_ex")
        self.h = h

    def run_stream(self, streams, chunk=48000):
        """Pull each stream through fvad_multi_run_stream in reads of at most
        `chunk` frames (the simulator's streaming read loop)."""
        arrs = [np.ascontiguousarray(s, np.float32) for s in streams]
        pos = [0] * len(arrs)

        def read(ctx, s, dst, max_frames):
            a = arrs[s]
            k = min(max_frames, chunk, a.shape[1] - pos[s])
            for c in range(a.shape[0]):
                C.memmove(dst[c], a[c, pos[s]:].ctypes.data, k * 4)
            pos[s] += k
            return k

        cb = READ_FN(read)
        _check(lib().fvad_multi_run_stream(self.h, C.cast(cb, C.c_void_p), None), "fvad_multi_run_stream")

    def run(self, streams):
        """streams: list of planar float32 arrays [ch][len]."""
        arrs = [np.ascontiguousarray(s, np.float32) for s in streams]
        ptrs = (F32P * len(arrs))(*[fptr(a) for a in arrs])
        lens = (C.c_size_t * len(arrs))(*[a.shape[1] for a in arrs])
        _check(lib().fvad_multi_run(self.h, ptrs, lens), "fvad_multi_run")

    def segments(self, stream, machine=0):
        n = lib().fvad_multi_segments_alt(self.h, stream, machine, None, 0)
        buf = (Segment * max(1, n))()
        lib().fvad_multi_segments_alt(self.h, stream, machine, buf, n)
        return [(s.sample_from, s.sample_to, s.debug_rnn_vad, s.debug_avg_speech_vol_ratio) for s in buf[:n]]

    def __del__(self):
        try:
            lib().fvad_multi_destroy(self.h)
        except Exception:
            pass


def evaluate(vad_segs, ref_segs, ignore_shorter_than_sec=0.0, extrude_start=0.0, extrude_end=0.0, fill_gaps=0.0):
    v = np.ascontiguousarray(np.asarray(vad_segs, np.float32).reshape(-1, 2))
    r = np.ascontiguousarray(np.asarray(ref_segs, np.float32).reshape(-1, 2))
    cfg = StatConfig(ignore_shorter_than_sec, extrude_start, extrude_end, fill_gaps)
    out = SingleStats()
    _check(lib().fvad_eval_stats(fptr(v), len(v), fptr(r), len(r), C.byref(cfg), C.byref(out)), "fvad_eval_stats")
    return {n: getattr(out, n) for n in _STAT_FIELDS}


def aggregate(stats_list):
    arr = (SingleStats * max(1, len(stats_list)))()
    for i, s in enumerate(stats_list):
        for n in _STAT_FIELDS:
            setattr(arr[i], n, s[n])
    out = AggregateStats()
    lib().fvad_eval_aggregate(arr, len(stats_list), C.byref(out))
    return out


class Sweep:
    """Many VADMachine configs over recorded window sequences (fvad_sweep_*):
    one GPU lane per (stream, config), or the host VADMachine with device=-1."""

    def __init__(self, n_streams, n_channels=2, device=0, fft_size=2048, bands=((4, 64),), use_denoiser=True,
                 seg_capacity=256, sample_rate=48000, spectrum=None):
        """spectrum=(lo, hi): a spectral sweep (fvad_sweep_create_spectral) -- it records
        window spectra of the bins lo..hi (set_spectra, append_spectra) and runs configs
        of any speech band inside them; bands is then ignored."""
        cfg = SweepConfig()
        cfg.n_streams, cfg.n_channels, cfg.sample_rate, cfg.fft_size = n_streams, n_channels, sample_rate, fft_size
        cfg.n_bands = len(bands)
        for i, (lo, hi) in enumerate(bands[:MAX_BANDS]):
            cfg.band_lo[i] = lo
            cfg.band_hi[i] = hi
        cfg.use_denoiser, cfg.seg_capacity, cfg.device = int(use_denoiser), seg_capacity, device
        self.cfg = cfg
        self.h = None
        h = C.c_void_p()
        if spectrum is None:
            _check(lib().fvad_sweep_create(C.byref(cfg), C.byref(h)), "fvad_sweep_create")
        else:
            _check(lib().fvad_sweep_create_spectral(C.byref(cfg), spectrum[0], spectrum[1], C.byref(h)),
                   "fvad_sweep_create_spectral")
        self.h = h
        self.n_spec = 0 if spectrum is None else spectrum[1] - spectrum[0] + 1
        self.B, self.C, self.nb, self.n_cfgs = n_streams, n_channels, len(bands), 0
        self.kept_segments = True  # the last run kept its segments (run_score does not)

    @staticmethod
    def _cfgs(cfgs):
        cfgs = list(cfgs)
        return (VadmConfig * max(1, len(cfgs)))(*cfgs), len(cfgs)

    def set_windows(self, stream, band, vol_ratio, vad=None):
        """band [windows][channels][bands], vol_ratio [windows], vad [windows] or None (0)."""
        r = np.ascontiguousarray(vol_ratio, np.float32).reshape(-1)
        b = np.ascontiguousarray(band, np.float32).reshape(len(r), self.C, self.nb)
        v = np.ascontiguousarray(vad, np.float32).reshape(len(r)) if vad is not None else None
        _check(lib().fvad_sweep_set_windows(self.h, stream, len(r), fptr(b), fptr(v) if v is not None else None,
                                            fptr(r)), "fvad_sweep_set_windows")

    def append_outputs(self, out, ticks_valid=None):
        """The completed windows of one push (Engine.push's dict) appended to every stream."""
        T = out["win_flag"].shape[0]
        a = {k: np.ascontiguousarray(out[k], np.int32 if k == "win_flag" else np.float32)
             for k in ("win_flag", "win_ratio", "win_vad", "band")}
        s = Outputs(None, None, a["win_flag"].ctypes.data_as(I32P), fptr(a["win_ratio"]), fptr(a["win_vad"]),
                    fptr(a["band"]), None)
        tv = np.ascontiguousarray(ticks_valid, np.int32) if ticks_valid is not None else None
        _check(lib().fvad_sweep_append_outputs(self.h, C.byref(s), T, tv.ctypes.data_as(I32P) if tv is not None
                                               else None), "fvad_sweep_append_outputs")

    def set_spectra(self, stream, spectrum, vol_ratio, vad=None):
        """spectrum [windows][channels][n_spec], vol_ratio [windows], vad [windows] or None (0)."""
        r = np.ascontiguousarray(vol_ratio, np.float32).reshape(-1)
        b = np.ascontiguousarray(spectrum, np.float32)
        if self.n_spec:  # (a plain sweep: the library refuses the call)
            b = b.reshape(len(r), self.C, self.n_spec)
        v = np.ascontiguousarray(vad, np.float32).reshape(len(r)) if vad is not None else None
        _check(lib().fvad_sweep_set_spectra(self.h, stream, len(r), fptr(b), fptr(v) if v is not None else None,
                                            fptr(r)), "fvad_sweep_set_spectra")

    def append_spectra(self, out, spectrum=None, ticks_valid=None):
        """The completed windows of one push appended to every stream, with their spectra:
        out is Engine.push's dict, spectrum its out["spectrum"] unless given."""
        T = out["win_flag"].shape[0]
        a = {k: np.ascontiguousarray(out[k], np.int32 if k == "win_flag" else np.float32)
             for k in ("win_flag", "win_ratio", "win_vad")}
        sp = np.ascontiguousarray(out["spectrum"] if spectrum is None else spectrum, np.float32)
        s = Outputs(None, None, a["win_flag"].ctypes.data_as(I32P), fptr(a["win_ratio"]), fptr(a["win_vad"]), None, None)
        tv = np.ascontiguousarray(ticks_valid, np.int32) if ticks_valid is not None else None
        _check(lib().fvad_sweep_append_spectra(self.h, C.byref(s), fptr(sp), T, tv.ctypes.data_as(I32P)
                                               if tv is not None else None), "fvad_sweep_append_spectra")

    def bandmin_ms(self):
        """k_sweep_bandmin's event time in the last run of a spectral sweep, all chunks (ms)."""
        ms = C.c_double()
        _check(lib().fvad_sweep_bandmin_ms(self.h, C.byref(ms)), "fvad_sweep_bandmin_ms")
        return ms.value

    def run(self, cfgs):
        arr, n = self._cfgs(cfgs)
        _check(lib().fvad_sweep_run(self.h, arr, n), "fvad_sweep_run")
        self.n_cfgs, self.kept_segments = n, True

    def run_host(self, cfgs):
        arr, n = self._cfgs(cfgs)
        _check(lib().fvad_sweep_run_host(self.h, arr, n), "fvad_sweep_run_host")
        self.n_cfgs, self.kept_segments = n, True

    def segments(self, stream, cfg):
        """(total, the first min(total, seg_capacity) segments as tuples); after a
        run_score, which keeps no segments, (total, [])."""
        n = lib().fvad_sweep_segments(self.h, stream, cfg, None, 0)
        k = min(n, self.cfg.seg_capacity) if self.kept_segments else 0
        buf = (Segment * max(1, k))()
        lib().fvad_sweep_segments(self.h, stream, cfg, buf, k)
        return n, [(s.sample_from, s.sample_to, s.debug_rnn_vad, s.debug_avg_speech_vol_ratio) for s in buf[:k]]

    def counts(self):
        """Segment totals [stream][cfg]."""
        out = np.zeros((self.B, self.n_cfgs), np.uint64)
        _check(lib().fvad_sweep_counts(self.h, out.ctypes.data_as(C.c_void_p), out.size), "fvad_sweep_counts")
        return out

    def snapshot(self, stream, cfg):
        s = VadmSnapshot()
        _check(lib().fvad_sweep_snapshot(self.h, stream, cfg, C.byref(s)), "fvad_sweep_snapshot")
        return s.as_dict()

    def score(self, refs, ignore_shorter_than_sec=0.0, extrude_start=0.0, extrude_end=0.0, fill_gaps=0.0,
              single=False):
        """refs: per stream a list of (from_sec, to_sec).  Returns the AggregateStats
        per config (and with single=True the per-stream stats dicts [cfg][stream])."""
        arrs = [np.ascontiguousarray(np.asarray(r, np.float32).reshape(-1, 2)) for r in refs]
        assert len(arrs) == self.B, "one reference list per stream"
        ptrs = (F32P * self.B)(*[fptr(a) for a in arrs])
        lens = (C.c_size_t * self.B)(*[len(a) for a in arrs])
        sc = StatConfig(ignore_shorter_than_sec, extrude_start, extrude_end, fill_gaps)
        agg = (AggregateStats * max(1, self.n_cfgs))()
        one = (SingleStats * max(1, self.n_cfgs * self.B))() if single else None
        _check(lib().fvad_sweep_score(self.h, ptrs, lens, C.byref(sc), agg, one), "fvad_sweep_score")
        return self._scores(agg, one)

    def _scores(self, agg, one):
        if one is None:
            return list(agg[:self.n_cfgs])
        return list(agg[:self.n_cfgs]), [[{n: getattr(one[m * self.B + s], n) for n in _STAT_FIELDS}
                                          for s in range(self.B)] for m in range(self.n_cfgs)]

    def run_score(self, cfgs, refs, stat=None, single=False):
        """run(cfgs) and score(refs) in one call (fvad_sweep_run_score): the lanes are
        scored where they ran and the segments are not kept.  stat: a dict of
        StatConfig's four fields for every config, or a list of len(cfgs) such
        dicts (config m is scored with stat[m]); None: all zeros.  Returns what
        score returns."""
        arr, n = self._cfgs(cfgs)
        arrs = [np.ascontiguousarray(np.asarray(r, np.float32).reshape(-1, 2)) for r in refs]
        assert len(arrs) == self.B, "one reference list per stream"
        ptrs = (F32P * self.B)(*[fptr(a) for a in arrs])
        lens = (C.c_size_t * self.B)(*[len(a) for a in arrs])
        stats = [stat or {}] if stat is None or isinstance(stat, dict) else list(stat)
        sc = (StatConfig * max(1, len(stats)))(*[StatConfig(**d) for d in stats])
        agg = (AggregateStats * max(1, n))()
        one = (SingleStats * max(1, n * self.B))() if single else None
        try:
            _check(lib().fvad_sweep_run_score(self.h, arr, n, ptrs, lens, sc, len(stats), agg, one),
                   "fvad_sweep_run_score")
        finally:  # a call refused before it ran leaves the previous run; a lane over capacity leaves this one
            last = self.last_run()
            self.n_cfgs, self.kept_segments = last["n_cfgs"], last["kept_segments"]
        return self._scores(agg, one)

    @staticmethod
    def best_per_stream(single, field="f_score"):
        """One config index per stream from the per-stream stats score / run_score return
        with single=True (single[cfg][stream]): the argmax over configs of `field`, NaN
        counting as minus infinity, ties going to the lowest index (int64 array)."""
        v = np.array([[d[field] for d in row] for row in single], np.float64)
        if v.ndim != 2 or v.shape[0] < 1:
            raise ValueError("single: [cfg][stream] stats, at least one config")
        return np.argmax(np.where(np.isnan(v), -np.inf, v), axis=0)

    def last_run(self):
        """The last run: its configs, whether its segments were kept, the bytes copied back from the device."""
        n, kept, back = C.c_size_t(), C.c_int(), C.c_size_t()
        _check(lib().fvad_sweep_last_run(self.h, C.byref(n), C.byref(kept), C.byref(back)), "fvad_sweep_last_run")
        return {"n_cfgs": n.value, "kept_segments": bool(kept.value), "bytes_back": back.value}

    def bytes(self, cfgs):
        """Device bytes the machines of these configs need in one chunk (fvad_sweep_bytes)."""
        arr, n = self._cfgs(cfgs)
        return lib().fvad_sweep_bytes(C.byref(self.cfg), arr, n)

    def set_debug(self, key, value):
        """Test hooks: SWEEP_DEBUG_BOUND_SCALE, SWEEP_DEBUG_DEFER_MAX, SWEEP_DEBUG_CHUNK, SWEEP_DEBUG_COUNT."""
        _check(lib().fvad_sweep_set_debug(self.h, key, value), "fvad_sweep_set_debug")

    def debug_counts(self):
        out = np.zeros(4, np.uint64)
        n = lib().fvad_sweep_debug_counts(self.h, out.ctypes.data_as(C.c_void_p), 4)
        _check(n if n < 0 else 0, "fvad_sweep_debug_counts")
        return dict(zip(("exact", "settled", "open", "end_fold"), (int(v) for v in out[:n])))

    def __del__(self):
        try:
            if self.h:
                lib().fvad_sweep_destroy(self.h)
        except Exception:
            pass


def parse_audacity(txt):
    b = txt.encode() if isinstance(txt, str) else txt
    n = lib().fvad_parse_audacity(b, len(b), None, 0)
    if n < 0:
        raise ValueError("malformed Audacity label text")
    out = np.zeros(2 * max(1, n), np.float32)
    lib().fvad_parse_audacity(b, len(b), fptr(out), n)
    return out[: 2 * n].reshape(-1, 2)
