"""Per-stream VADMachine configs, the host-only parts: fvad_vadm_lengths (the
RollingAverage lengths a config needs, what an attach room has to cover) against
the oracle's buffers, and Sweep.best_per_stream (a sweep's winner per stream,
what fvad_engine_set_stream_vadm is fed) on a hand-made score table and on a
host-only sweep.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import sweep_util as su


def test_lengths_match_the_oracle(fvad_mod, oracle_mod):
    p = oracle_mod.Pipeline(2, oracle_mod.Model(seed=1))
    want = tuple(len(p.vadm_rolling(k)) for k in range(3))
    assert fvad_mod.vadm_lengths(fvad_mod.VadmConfig.default()) == want
    assert want[0] == 4218


def test_lengths_of_short_long_term_buffers(fvad_mod):
    c = fvad_mod.VadmConfig.default()
    c.long_term_speech_avg_sec = 10.0
    assert fvad_mod.vadm_lengths(c)[0] == 234
    c.long_term_speech_avg_sec = 2.0
    assert fvad_mod.vadm_lengths(c)[0] == 46
    # the lengths follow the window rate: sample_rate / fft_size windows per second
    c.long_term_speech_avg_sec, c.short_term_speech_avg_sec, c.channel_vol_ratio_avg_sec = 10.0, 0.5, 1.0
    assert fvad_mod.vadm_lengths(c, 48000, 1024) == (468, 23, 46)
    assert fvad_mod.vadm_lengths(c, 16000, 2048) == (78, 3, 7)


def test_lengths_refuse_bad_arguments(fvad_mod):
    L = fvad_mod.lib()
    c = fvad_mod.VadmConfig.default()
    out = (C.c_int * 3)()
    assert L.fvad_vadm_lengths(None, 48000, 2048, out) == fvad_mod.EINVAL
    assert L.fvad_vadm_lengths(C.byref(c), 48000, 2048, None) == fvad_mod.EINVAL
    assert L.fvad_vadm_lengths(C.byref(c), 0, 2048, out) == fvad_mod.EINVAL
    assert L.fvad_vadm_lengths(C.byref(c), 48000, 0, out) == fvad_mod.EINVAL
    assert L.fvad_vadm_lengths(C.byref(c), -48000, 2048, out) == fvad_mod.EINVAL
    assert L.fvad_vadm_lengths(C.byref(c), 48000, 2048, out) == 0 and tuple(out) == (4218, 4, 11)
    with pytest.raises(fvad_mod.FvadError):
        fvad_mod.vadm_lengths(None)


def test_best_per_stream_by_hand(fvad_mod):
    nan = float("nan")
    #            stream 0   1     2     3     4
    f = [[0.2, 0.5, nan, nan, 0.0],   # config 0
         [0.9, 0.5, 0.1, nan, -1.0],  # config 1
         [0.9, 0.4, nan, nan, nan],   # config 2
         [nan, 0.5, 0.3, nan, 0.0]]   # config 3
    single = [[{"f_score": v, "precision": 1.0 - v} for v in row] for row in f]
    best = fvad_mod.Sweep.best_per_stream(single)
    # stream 0: a tie of configs 1 and 2, the lower wins; 1: a three-way tie; 2: NaN never
    # beats a number; 3: all NaN, config 0; 4: a tie at 0.0 above a negative score and a NaN
    assert best.tolist() == [1, 0, 3, 0, 0]
    # another field: 1 - f, so the smallest f wins, NaN (1 - NaN) still last
    assert fvad_mod.Sweep.best_per_stream(single, field="precision").tolist() == [0, 2, 1, 0, 1]
    assert fvad_mod.Sweep.best_per_stream(single[:1]).tolist() == [0] * 5
    with pytest.raises(ValueError):
        fvad_mod.Sweep.best_per_stream([])


def test_best_per_stream_of_a_host_sweep(fvad_mod):
    """The pick equals a plain loop over what score(single=True) returned, and it is
    not one config for all streams (the streams differ in their bursts)."""
    sw = fvad_mod.Sweep(su.N_STREAMS, 2, device=-1, bands=su.BANDS)
    su.fill(sw)
    cfgs = su.grid(fvad_mod)[:12]
    sw.run(cfgs)
    refs = [su.labels(s, su.stream_len(s)) for s in range(su.N_STREAMS)]
    _, single = sw.score(refs, single=True)
    best = sw.best_per_stream(single)
    assert best.shape == (su.N_STREAMS,)
    for s in range(su.N_STREAMS):
        want, top = 0, -np.inf
        for m in range(len(cfgs)):
            v = single[m][s]["f_score"]
            v = -np.inf if np.isnan(v) else v
            if v > top:
                want, top = m, v
        assert best[s] == want, (s, best[s], want)
    tpr = sw.best_per_stream(single, field="true_positive_rate")
    assert all(0 <= m < len(cfgs) for m in tpr.tolist())
