"""Shared by the window-spectrum tests (test_spectrum_cpu.py,
test_gpu_spectrum.py): the oracle-derived reference spectra, the test's own
sequential f32 band sums, and a generator of synthetic spectra for spectral
sweeps."""
import functools

import numpy as np

import sweep_util as su

FRAME = 480


def seq_sum(spec, lo, hi, spec_lo=0):
    """acc = 0.0f; for k = lo..hi: acc += spec[..., k], in np.float32 and in bin
    order (np.cumsum accumulates sequentially in its dtype; 0 + x is exact)."""
    x = np.ascontiguousarray(spec[..., lo - spec_lo:hi - spec_lo + 1], np.float32)
    return np.cumsum(x, axis=-1, dtype=np.float32)[..., -1]


def hz(fft_size, k):
    """A frequency FFT.freqToBin maps to bin k at 48 kHz (exact in f32 for the sizes used here)."""
    return k * 48000.0 / fft_size


def band_cfg(fvad, c, lo, hi, fft_size=su.FFT, **kw):
    return su.copy_cfg(fvad, c, speech_min_freq=hz(fft_size, lo), speech_max_freq=hz(fft_size, hi), **kw)


def window_spectra(oracle, sig, fft_size):
    """sig [channels][samples] -> [windows][channels][fft_size / 2 + 1]: the
    reference's FFT.fft(samples, hann, result) of each whole window (Spectrogram.compute
    at hop_size == fft_size), channel by channel."""
    C, n = sig.shape
    W = n // fft_size
    hann = oracle.hann_periodic(fft_size)
    out = np.zeros((W, C, fft_size // 2 + 1), np.float32)
    for w in range(W):
        for c in range(C):
            out[w, c] = oracle.fftzig(sig[c, w * fft_size:(w + 1) * fft_size], hann)
    return out


@functools.lru_cache(maxsize=None)
def denoised(stream_id, seconds_x10, n_channels=2):
    """(input [C][n], the oracle pipeline's denoised channels [C][n], its window trace at
    fft_size 2048) of synthetic stream stream_id, seconds_x10 / 10 seconds long.
    Computed once per stream and shared; callers do not modify the arrays."""
    import fvad
    import oracle
    n = 4800 * seconds_x10
    x = fvad.synth_stream(stream_id, n, n_channels)[0]
    p = oracle.Pipeline(n_channels, oracle.Model(seed=1), trace_windows=n // 2048 + 1, trace_denoised=n)
    p.push([x[c] for c in range(n_channels)])
    _, wins = p.trace()
    den = p.tden[:, :n].copy()
    for a in (x, den, wins):
        a.setflags(write=False)
    return x, den, wins


# ---- synthetic spectra for the host tests ----
SPEC = (2, 140)  # the recorded bins
# 13 distinct bands inside SPEC: one bin, the whole range, three sharing lo, three sharing hi, and
# bands that see the bursts (bins 10..40) fully, partly or not at all
BANDS = [(20, 20), SPEC, (4, 64), (4, 30), (4, 100), (13, 128), (50, 128), (100, 128), (10, 40), (41, 80), (80, 120),
         (2, 9), (130, 140)]


def gen_spectra(s, W):
    """Stream s's W windows: (spectrum [W][2][139], vad [W], vol_ratio [W]) with
    sweep_util's bursts.  Background: every bin 1.5e-5 (1 + 0.5 u); bursts: the
    bins 10..40 of channel 0 at 0.02 (1 + u), channel 1 at 0.8 of it -- a band
    over those bins rises a few hundred times, one beside them does not."""
    rng = np.random.default_rng(2000 + s)
    n_spec = SPEC[1] - SPEC[0] + 1
    sp = (1.5e-5 * (1.0 + 0.5 * rng.random((W, 2, n_spec)))).astype(np.float32)
    vad = np.full(W, 0.05, np.float32)
    vr = np.full(W, 0.2, np.float32)
    for w0, n in su.bursts(s, W):
        w1 = min(W, w0 + n)
        b = (0.02 * (1.0 + rng.random((w1 - w0, 31)))).astype(np.float32)
        sp[w0:w1, 0, 10 - SPEC[0]:41 - SPEC[0]] = b
        sp[w0:w1, 1, 10 - SPEC[0]:41 - SPEC[0]] = np.float32(0.8) * b
        vad[w0:w1] = 0.9
        vr[w0:w1] = 0.9
    return sp, vad, vr


def lanes_of(res, cols):
    """su.results restricted to the configs `cols`, renumbered 0.. (for su.assert_same)."""
    lanes, counts = res
    B = counts.shape[0]
    return ({(s, j): lanes[(s, m)] for s in range(B) for j, m in enumerate(cols)}, counts[:, list(cols)])
