"""Shared fixture of the config-sweep tests (test_sweep_cpu.py, test_gpu_sweep.py):
a deterministic window generator, the config grid, and the comparisons."""
import itertools

import numpy as np

BANDS = ((4, 64), (13, 128))  # 100..1500 Hz and 300..3000 Hz at fft_size 2048
FFT = 2048
N_STREAMS = 5


def stream_len(s):
    return 311 if s == 3 else 600  # stream 3 is ragged


def bursts(s, W):
    """(first window, length) of stream s's bursts."""
    return [(w0, 30 + 10 * (s % 4)) for w0 in range(20 + 7 * s, W, 150 + 13 * s)]


def gen(s, W, n_bands=2):
    """Stream s's W windows: (band [W][2][n_bands], vad [W], vol_ratio [W]).
    Background: band sums 1e-3 (1 + 0.5 u) per channel, ratio 0.2, vad 0.05.
    Bursts: channel 0 is 0.5 (1 + u), channel 1 0.8 of it, ratio 0.9, vad 0.9.
    Band 1 is band 0 times 0.7."""
    rng = np.random.default_rng(1000 + s)
    b0 = (1e-3 * (1.0 + 0.5 * rng.random((W, 2)))).astype(np.float32)
    ub = rng.random(W)
    vad = np.full(W, 0.05, np.float32)
    vr = np.full(W, 0.2, np.float32)
    for w0, n in bursts(s, W):
        w1 = min(W, w0 + n)
        c0 = (0.5 * (1.0 + ub[w0:w1])).astype(np.float32)
        b0[w0:w1, 0] = c0
        b0[w0:w1, 1] = np.float32(0.8) * c0
        vad[w0:w1] = 0.9
        vr[w0:w1] = 0.9
    band = np.stack([b0 * np.float32(0.7 ** k) for k in range(n_bands)], axis=2).astype(np.float32)
    return np.ascontiguousarray(band), vad, vr


def labels(s, W):
    """The bursts as (from_sec, to_sec) reference labels."""
    return [(w0 * FFT / 48000.0, min(W, w0 + n) * FFT / 48000.0) for w0, n in bursts(s, W)]


def grid(fvad, second_band_odd=True):
    """36 configs: long-term 1 / 10 / 180 s (23, 234, 4 218 entries at fft_size
    2048: many wraps, some, none), short-term 0.2 / 0.5 s, threshold factor 2 /
    18 / 2000, with and without the initial average; every odd config on the
    second band."""
    out = []
    for i, (lt, st, thr, init) in enumerate(itertools.product((1.0, 10.0, 180.0), (0.2, 0.5), (2.0, 18.0, 2000.0),
                                                              (1, 0))):
        c = fvad.VadmConfig.default()
        c.long_term_speech_avg_sec = lt
        c.short_term_speech_avg_sec = st
        c.speech_threshold_factor = thr
        c.has_initial_long_term_avg = init
        if second_band_odd and i % 2:
            c.speech_min_freq, c.speech_max_freq = 300.0, 3000.0
        out.append(c)
    return out


def copy_cfg(fvad, c, **kw):
    d = fvad.VadmConfig()
    for n, _ in c._fields_:
        setattr(d, n, getattr(c, n))
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def slot_of(c):
    return 1 if c.speech_min_freq == 300.0 else 0


def fill(sw, streams=range(N_STREAMS), W=None):
    data = []
    for i, s in enumerate(streams):
        band, vad, vr = gen(s, W if W is not None else stream_len(s))
        sw.set_windows(i, band, vr, vad)
        data.append((band, vad, vr))
    return data


def results(sw, n_cfgs):
    """Everything a run left: per lane (total, segments, snapshot), and the counts."""
    lanes = {(s, m): sw.segments(s, m) + (sw.snapshot(s, m),) for s in range(sw.B) for m in range(n_cfgs)}
    return lanes, sw.counts()


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64).tolist()


def assert_same(got, ref):
    """Lane by lane: totals, segments, every snapshot field, avg[0..2] by their bits."""
    (gl, gc), (rl, rc) = got, ref
    assert np.array_equal(gc, rc)
    assert gl.keys() == rl.keys()
    for k in rl:
        assert gl[k][0] == rl[k][0], (k, gl[k][0], rl[k][0])
        assert gl[k][1] == rl[k][1], (k, gl[k][1][:2], rl[k][1][:2])
        assert bits(gl[k][2]["avg"]) == bits(rl[k][2]["avg"]), (k, gl[k][2]["avg"], rl[k][2]["avg"])
        assert gl[k][2] == rl[k][2], (k, gl[k][2], rl[k][2])
