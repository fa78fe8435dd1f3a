"""Spectral sweeps on the host (fvad.Sweep(spectrum=..., device=-1): no GPU):
a sweep that records window spectra runs configs of any speech band inside
them, each lane equal to a plain host sweep created with that band and fed the
test's own sequential np.float32 band sums; the reference's FFT.fft over
re-blocked denoised windows gives the trace's band sums that way, by bits; and
the argument errors leave the earlier run's results intact."""
import numpy as np
import pytest

import spectrum_util as sp
import sweep_util as su


def spectral_host(fvad, n_streams=su.N_STREAMS, spectrum=sp.SPEC, **kw):
    return fvad.Sweep(n_streams, 2, device=-1, spectrum=spectrum, **kw)


def grid_over_bands(fvad):
    """sweep_util's 36 configs, config i on band i % 13: every band at least twice."""
    return [sp.band_cfg(fvad, c, *sp.BANDS[i % len(sp.BANDS)])
            for i, c in enumerate(su.grid(fvad, second_band_odd=False))]


@pytest.fixture(scope="module")
def spectral_run(fvad_mod):
    sw = spectral_host(fvad_mod)
    data = []
    for s in range(su.N_STREAMS):
        spec, vad, vr = sp.gen_spectra(s, su.stream_len(s))
        sw.set_spectra(s, spec, vr, vad)
        data.append((spec, vad, vr))
    cfgs = grid_over_bands(fvad_mod)
    sw.run(cfgs)
    return sw, data, cfgs, su.results(sw, len(cfgs))


def test_spectral_host_sweep_matches_plain(fvad_mod, spectral_run):
    """36 configs over 13 distinct bands (one bin, the whole range, bands sharing
    lo, bands sharing hi, each band in two or three configs): every lane's total,
    segments and snapshot are those of a plain host sweep of that band over the
    sequential f32 sums."""
    sw, data, cfgs, res = spectral_run
    assert len(cfgs) == 36 and len(set(sp.BANDS)) >= 12
    for c, (lo, hi) in zip(cfgs, sp.BANDS * 3):
        assert fvad_mod.VADMachine(c).bins() == (lo, hi)
    total = 0
    for b, (lo, hi) in enumerate(sp.BANDS):
        cols = [m for m in range(len(cfgs)) if m % len(sp.BANDS) == b]
        plain = fvad_mod.Sweep(su.N_STREAMS, 2, device=-1, bands=((lo, hi),))
        for s, (spec, vad, vr) in enumerate(data):
            plain.set_windows(s, sp.seq_sum(spec, lo, hi, sp.SPEC[0])[:, :, None], vr, vad)
        plain.run([cfgs[m] for m in cols])
        ref = su.results(plain, len(cols))
        su.assert_same(sp.lanes_of(res, cols), ref)
        total += int(ref[1].sum())
    print("segments", total)
    assert total > 0
    # two configs that differ only in band ((10, 40) holds the bursts, (80, 120) none of them):
    # the plain sweeps alone tell them apart, and so does the spectral sweep
    g = su.grid(fvad_mod, second_band_odd=False)
    same_but_band = [sp.band_cfg(fvad_mod, g[0], 10, 40), sp.band_cfg(fvad_mod, g[0], 80, 120)]
    pa = fvad_mod.Sweep(1, 2, device=-1, bands=((10, 40),))
    pb = fvad_mod.Sweep(1, 2, device=-1, bands=((80, 120),))
    spec, vad, vr = data[0]
    pa.set_windows(0, sp.seq_sum(spec, 10, 40, sp.SPEC[0])[:, :, None], vr, vad)
    pb.set_windows(0, sp.seq_sum(spec, 80, 120, sp.SPEC[0])[:, :, None], vr, vad)
    pa.run(same_but_band[:1])
    pb.run(same_but_band[1:])
    assert pa.segments(0, 0)[1] != pb.segments(0, 0)[1] and pa.segments(0, 0)[0] > 0
    one = spectral_host(fvad_mod, n_streams=1)
    one.set_spectra(0, spec, vr, vad)
    one.run(same_but_band)
    assert one.segments(0, 0) == pa.segments(0, 0) and one.segments(0, 1) == pb.segments(0, 0)
    assert one.segments(0, 0)[1] != one.segments(0, 1)[1]


def test_run_host_and_run_score_on_a_spectral_host_sweep(fvad_mod, spectral_run):
    """run_host is run, and run_score is run followed by score, as on a plain sweep."""
    sw, _, cfgs, res = spectral_run
    refs = [su.labels(s, su.stream_len(s)) for s in range(su.N_STREAMS)]
    sw.run(cfgs)
    agg = sw.score(refs)
    sw.run_host(cfgs)
    su.assert_same(su.results(sw, len(cfgs)), res)
    got = sw.run_score(cfgs, refs)
    assert np.array_equal(sw.counts(), res[1])
    for a, b in zip(got, agg):
        assert bytes(a) == bytes(b)


def test_oracle_fft_gives_the_traced_band_sums(fvad_mod, oracle_mod):
    """One oracle pipeline run with trace (2 channels, 3 s): the traced denoised
    channels re-blocked into 2048-sample windows, each through FFT.fft with the
    periodic Hann window; the sequential f32 sum over the main band (bins 4..64)
    is the trace's band, by bits."""
    _, den, wins = sp.denoised(19, 30)
    spec = sp.window_spectra(oracle_mod, den, 2048)
    assert len(wins) == spec.shape[0] == 3 * 48000 // 2048
    got = sp.seq_sum(spec, 4, 64)
    assert got.dtype == np.float32 and got.shape == (len(wins), 2)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(wins["band"][:, :2]).view(np.uint32))
    assert (got > 0).all()


def test_argument_errors_leave_the_last_run(fvad_mod, spectral_run):
    sw, data, cfgs, res = spectral_run
    sw.run(cfgs)
    # a band outside the recorded range: the message names the config
    bad = list(cfgs)
    bad[5] = sp.band_cfg(fvad_mod, cfgs[5], 4, 141)
    for call in (sw.run, sw.run_host, lambda c: sw.run_score(c, [[] for _ in range(su.N_STREAMS)])):
        with pytest.raises(fvad_mod.FvadError) as e:
            call(bad)
        assert e.value.code == fvad_mod.EINVAL and "config 5" in str(e.value), str(e.value)
    bad[5] = sp.band_cfg(fvad_mod, cfgs[5], 1, 64)
    with pytest.raises(fvad_mod.FvadError) as e:
        sw.run(bad)
    assert e.value.code == fvad_mod.EINVAL and "config 5" in str(e.value)
    # a setter on the wrong kind of sweep
    spec, vad, vr = data[0]
    with pytest.raises(fvad_mod.FvadError) as e:
        sw.set_windows(0, np.zeros((len(vr), 2, 1), np.float32), vr, vad)
    assert e.value.code == fvad_mod.EINVAL
    out = {"win_flag": np.ones((1, su.N_STREAMS), np.int32), "win_ratio": np.zeros((1, su.N_STREAMS), np.float32),
           "win_vad": np.zeros((1, su.N_STREAMS), np.float32), "band": np.zeros((1, su.N_STREAMS, 2, 1), np.float32)}
    with pytest.raises(fvad_mod.FvadError) as e:
        sw.append_outputs(out)
    assert e.value.code == fvad_mod.EINVAL
    plain = fvad_mod.Sweep(su.N_STREAMS, 2, device=-1, bands=su.BANDS)
    with pytest.raises(fvad_mod.FvadError) as e:
        plain.set_spectra(0, spec, vr, vad)
    assert e.value.code == fvad_mod.EINVAL
    with pytest.raises(fvad_mod.FvadError) as e:
        plain.append_spectra(out, spectrum=np.zeros((1, su.N_STREAMS, 2, 139), np.float32))
    assert e.value.code == fvad_mod.EINVAL
    # a bad range
    for lo, hi in ((-1, 10), (11, 10), (0, 1025)):
        with pytest.raises(fvad_mod.FvadError) as e:
            spectral_host(fvad_mod, spectrum=(lo, hi))
        assert e.value.code == fvad_mod.EINVAL, (lo, hi)
    spectral_host(fvad_mod, spectrum=(0, 1024))
    spectral_host(fvad_mod, spectrum=(7, 7))
    # every refused call left the run and the recorded windows as they were
    su.assert_same(su.results(sw, len(cfgs)), res)
    sw.run(cfgs)
    su.assert_same(su.results(sw, len(cfgs)), res)


def test_append_spectra_compaction(fvad_mod):
    """append_spectra follows append_outputs' window order and ticks_valid rules:
    hand-built pushes (fft_size 200, up to 3 windows per tick) appended to a
    spectral sweep give the final states of a sweep set directly with the
    expected sequences."""
    B, C, W, T, lo, hi = 3, 2, 3, 6, 1, 9
    n_spec = hi - lo + 1
    rng = np.random.default_rng(11)
    flags = np.array([[3, 0, 1], [0, 2, 3], [2, 3, 0], [1, 1, 2], [3, 0, 3], [2, 2, 1]], np.int32)
    valid = np.array([6, 4, 0], np.int32)
    out = {"win_flag": flags, "win_ratio": rng.random((T, B, W)).astype(np.float32),
           "win_vad": rng.random((T, B, W)).astype(np.float32),
           "spectrum": rng.random((T, B, W, C, n_spec)).astype(np.float32)}
    sw = fvad_mod.Sweep(B, C, device=-1, fft_size=200, spectrum=(lo, hi))
    sw.append_spectra(out, ticks_valid=valid)
    sw.append_spectra({k: v[:2] for k, v in out.items()})
    exp = [[] for _ in range(B)]
    for n, tv in ((T, valid), (2, [2] * B)):
        for s in range(B):
            for t in range(min(n, tv[s])):
                for w in range(flags[t, s]):
                    exp[s].append((out["spectrum"][t, s, w], out["win_vad"][t, s, w], out["win_ratio"][t, s, w]))
    assert [len(e) for e in exp] == [14, 8, 4]
    sw2 = fvad_mod.Sweep(B, C, device=-1, fft_size=200, spectrum=(lo, hi))
    for s in range(B):
        sw2.set_spectra(s, np.stack([e[0] for e in exp[s]]), [e[2] for e in exp[s]], [e[1] for e in exp[s]])
    base = fvad_mod.VadmConfig.default()
    cfgs = [sp.band_cfg(fvad_mod, base, a, b, fft_size=200, long_term_speech_avg_sec=(k + 0.5) / 240.0,
                        short_term_speech_avg_sec=1e-4, channel_vol_ratio_avg_sec=1e-4, speech_threshold_factor=1.0,
                        has_initial_long_term_avg=0, channel_vol_ratio_threshold=0.0, min_consecutive_sec_to_open=0.0,
                        max_speech_gap_sec=0.0, min_vad_duration_sec=0.0)
            for k, (a, b) in enumerate(((1, 9), (2, 5), (9, 9)), 1)]
    sw.run(cfgs)
    sw2.run(cfgs)
    su.assert_same(su.results(sw, 3), su.results(sw2, 3))
    for s in range(B):  # the one-entry short-term average is the last window's band minimum
        last = exp[s][-1][0]
        assert sw.snapshot(s, 0)["windows"] == len(exp[s])
        assert sw.snapshot(s, 2)["avg"][1] == float(min(last[0, 8], last[1, 8])), s
    with pytest.raises(fvad_mod.FvadError) as e:
        sw.append_spectra(out, ticks_valid=[7, 0, 0])
    assert e.value.code == fvad_mod.EINVAL
