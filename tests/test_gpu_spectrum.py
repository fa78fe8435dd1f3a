"""Window spectra out of the batched engine (fvad_engine_config.want_spectrum:
the tap twins of the FFT-B kernels) and spectral sweeps on the device
(k_sweep_bandmin in front of the unchanged k_vadm_sweep).

The tap against the reference: the oracle pipeline's denoised channels (or the
raw input without the denoiser) re-blocked into fft_size windows, each through
FFT.fft with the periodic Hann window -- by bits, in the right slots, zeros
everywhere else, and every other output equal to the same engine's without the
tap.  The spectral sweep against its own host path and against an engine's
attached machines."""
import numpy as np
import pytest

import spectrum_util as sp
import sweep_util as su

pytestmark = pytest.mark.gpu

FRAME = 480
KEYS = ("vad", "ratio", "win_flag", "win_ratio", "win_vad", "band")


@pytest.fixture(scope="module")
def model(fvad_mod):
    return fvad_mod.Model(seed=1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pushes(eng, streams, lens, sizes, frame=FRAME, last=None):
    """Push the streams ([C][samples] each, lens[s] ticks of them) in pushes of
    sizes[i] ticks with ragged ticks_valid.  Returns per push (out, valid)."""
    got, t0 = [], 0
    C = streams[0].shape[0]
    for nt in sizes:
        pcm = np.zeros((nt, eng.B, C, frame), np.float32)
        valid = np.zeros(eng.B, np.int32)
        for s, x in enumerate(streams):
            v = max(0, min(nt, lens[s] - t0))
            valid[s] = v
            if v:
                pcm[:v, s] = x[:, t0 * frame:(t0 + v) * frame].reshape(C, v, frame).transpose(1, 0, 2)
        kw = {}
        if last is not None:  # the real samples of a stream's last tick, in the push that holds it
            kw["last_tick_samples"] = np.array([last[s] if t0 < lens[s] <= t0 + nt else frame
                                                for s in range(eng.B)], np.int32)
        got.append((eng.push(pcm, ticks_valid=valid, **kw), valid))
        t0 += nt
    assert t0 >= max(lens)
    return got


def windows_of(got, key, s, W):
    """Stream s's completed windows' rows of out[key], in order."""
    rows = []
    for out, valid in got:
        a = out[key].reshape((out["win_flag"].shape[0], out["win_flag"].shape[1], W) + out[key].shape[2 + (W > 1):])
        for t in range(valid[s]):
            for w in range(out["win_flag"][t, s]):
                rows.append(a[t, s, w])
    return rows


def check_slots(got, W):
    """Every slot that holds no window reads 0 (slots >= win_flag, ticks past ticks_valid, idle streams)."""
    for out, valid in got:
        T, B = out["win_flag"].shape
        a = out["spectrum"].reshape((T, B, W) + out["spectrum"].shape[-2:])
        used = np.zeros((T, B, W), bool)
        for s in range(B):
            for t in range(valid[s]):
                used[t, s, :out["win_flag"][t, s]] = True
        assert not a[~used].any()


def check_tap(fvad, model, oracle, streams, refsig, lens, sizes, fft=2048, rng_=None, max_ticks=None, bands=None,
              last=None, **kw):
    """The engine with the tap over bins rng_ against the reference spectra of
    refsig (per stream [C][samples]: what FFT B sees), and against the same
    engine without the tap."""
    lo, hi = rng_ if rng_ is not None else (0, fft // 2)
    B, C = len(streams), streams[0].shape[0]
    bands = bands or ((fft // 512 + 1, fft // 32),)
    mk = dict(max_ticks=max_ticks or max(sizes), fft_size=fft, bands=bands, **kw)
    tap = fvad.Engine(model, B, C, spectrum=(lo, hi), **mk)
    plain = fvad.Engine(model, B, C, **mk)
    assert tap.n_spec == hi - lo + 1 and plain.n_spec == 0
    got = pushes(tap, streams, lens, sizes, last=last)
    ref = pushes(plain, streams, lens, sizes, last=last)
    for (o, v), (r, _) in zip(got, ref):
        assert "spectrum" not in r
        for k in KEYS:
            for s in range(B):
                assert np.array_equal(bits(o[k][:v[s], s]) if k != "win_flag" else o[k][:v[s], s],
                                      bits(r[k][:v[s], s]) if k != "win_flag" else r[k][:v[s], s]), (k, s)
    W = tap.wpt
    check_slots(got, W)
    n_win = 0
    for s in range(B):
        n = lens[s] * FRAME if last is None else (lens[s] - 1) * FRAME + int(last[s])
        want = sp.window_spectra(oracle, refsig[s][:, :n], fft)
        rows = windows_of(got, "spectrum", s, W)
        assert len(rows) == want.shape[0] == n // fft, (s, len(rows), want.shape)
        if rows:
            assert np.array_equal(bits(np.stack(rows)), bits(want[:, :, lo:hi + 1])), s
            # and the engine's own band sums are the sequential sums of these magnitudes
            bsum = np.stack(windows_of(got, "band", s, W))
            for b, (blo, bhi) in enumerate(bands):
                if lo <= blo and bhi <= hi:
                    assert np.array_equal(bits(bsum[:, :, b]), bits(sp.seq_sum(np.stack(rows), blo, bhi, lo))), (s, b)
        n_win += len(rows)
    assert n_win > 0
    return got


def den_streams(ids, C=2):
    """(inputs, denoised) of the synthetic streams ids, 3 s each."""
    x, d = zip(*[sp.denoised(i, 30, C)[:2] for i in ids])
    return list(x), list(d)


def test_tap_parity_staged(fvad_mod, model, oracle_mod):
    """3 streams x 2 channels x 3 s (2.5 s, 1.7 s), fft 2048 (k_olafb_spec): uneven
    pushes so windows straddle them, ragged ticks_valid; the whole spectrum, then
    bins 3..700 as the slice of it."""
    x, d = den_streams((0, 19, 42))
    lens, sizes = [300, 250, 170], [37, 64, 5, 64, 64, 11, 55]
    full = check_tap(fvad_mod, model, oracle_mod, x, d, lens, sizes, max_ticks=64)
    part = check_tap(fvad_mod, model, oracle_mod, x, d, lens, sizes, rng_=(3, 700), max_ticks=64)
    for (a, _), (b, _) in zip(full, part):
        assert np.array_equal(bits(a["spectrum"][..., 3:701]), bits(b["spectrum"]))


def test_tap_five_channels_k_fftbw(fvad_mod, model, oracle_mod):
    x, d = den_streams((7,), C=5)
    check_tap(fvad_mod, model, oracle_mod, x, d, [130], [50, 7, 50, 23], max_ticks=50)


@pytest.mark.parametrize("fft", [512, 1000])
def test_tap_k_fftb_lds(fvad_mod, model, oracle_mod, fft):
    x, d = den_streams((0, 19))
    check_tap(fvad_mod, model, oracle_mod, x, d, [120, 77], [33, 50, 37], fft=fft, rng_=(1, fft // 2), max_ticks=50)


def test_tap_fft_200_three_slots(fvad_mod, model, oracle_mod):
    """fft_size 200 without the denoiser: up to three windows per tick, W = 3 slots; FFT B sees the raw input."""
    x, _ = den_streams((0, 19))
    got = check_tap(fvad_mod, model, oracle_mod, x, x, [100, 61], [40, 33, 27], fft=200, bands=((1, 6),),
                    use_denoiser=False, max_ticks=40)
    assert got[0][0]["spectrum"].shape == (40, 2, 3, 2, 101)
    assert max(o["win_flag"].max() for o, _ in got) == 3


def test_tap_fft_32768_scratch(fvad_mod, model, oracle_mod):
    """One stream, fft_size 32768: k_fftb's device-scratch form."""
    x, d = den_streams((19,))
    check_tap(fvad_mod, model, oracle_mod, x, d, [140], [100, 40], fft=32768, rng_=(5, 9000), bands=((100, 300),),
              max_ticks=100)


def test_tap_no_denoiser_partial_last_tick(fvad_mod, model, oracle_mod):
    x, _ = den_streams((0, 19))
    check_tap(fvad_mod, model, oracle_mod, x, x, [90, 47], [50, 40], use_denoiser=False, max_ticks=50,
              last=np.array([480, 133], np.int32))


def test_tap_input_rate_16000(fvad_mod, model):
    """A 16 kHz engine with the tap against a 48 kHz engine with the tap fed the host mirror's output."""
    rng = np.random.default_rng(5)
    T, B, C = 60, 2, 2
    x16 = (0.3 * rng.standard_normal((B, C, T * 160))).astype(np.float32)
    x48 = [np.stack([fvad_mod.resample_host(16000, x16[s, c]) for c in range(C)]) for s in range(B)]
    a = fvad_mod.Engine(model, B, C, max_ticks=25, input_rate=16000, spectrum=(0, 1024))
    b = fvad_mod.Engine(model, B, C, max_ticks=25, spectrum=(0, 1024))
    lens, sizes = [60, 51], [25, 10, 25]
    ga = pushes(a, list(x16), lens, sizes, frame=160)
    gb = pushes(b, x48, lens, sizes)
    for (oa, _), (ob, _) in zip(ga, gb):
        assert np.array_equal(bits(oa["spectrum"]), bits(ob["spectrum"]))
    for s in range(B):
        wa, wb = windows_of(ga, "spectrum", s, 1), windows_of(gb, "spectrum", s, 1)
        assert len(wa) == len(wb) == lens[s] * 480 // 2048 and np.array_equal(bits(np.stack(wa)), bits(np.stack(wb)))
        assert np.stack(wa).min() > 0
    check_slots(ga, 1)


@pytest.mark.parametrize("mode", ["f32_fast", "fp16"])
def test_tolerance_modes_sum_their_own_spectrum(fvad_mod, model, mode):
    """f32_fast and fp16 are not bit-exact with the reference, but their band sums
    are still the sequential f32 sums of their own spectra."""
    x, _ = den_streams((0, 19))
    bands = ((4, 64), (13, 128), (100, 250))
    eng = fvad_mod.Engine(model, 2, 2, max_ticks=64, bands=bands, mode=mode, spectrum=(0, 1024))
    got = pushes(eng, x, [200, 131], [64, 64, 64, 8])
    n = 0
    for s in range(2):
        spec = np.stack(windows_of(got, "spectrum", s, 1))
        band = np.stack(windows_of(got, "band", s, 1))
        for b, (lo, hi) in enumerate(bands):
            assert np.array_equal(bits(band[:, :, b]), bits(sp.seq_sum(spec, lo, hi))), (s, b)
        n += len(spec)
    assert n == 200 * 480 // 2048 + 131 * 480 // 2048
    check_slots(got, 1)


def test_refusals_and_fetch_rules(fvad_mod, model):
    with pytest.raises(fvad_mod.FvadError) as e:
        fvad_mod.Engine(model, 1, 2, max_ticks=8, mode="fused", spectrum=(0, 1024))
    assert e.value.code == fvad_mod.EINVAL
    for bad in ((-1, 5), (9, 8), (0, 1025)):
        with pytest.raises(fvad_mod.FvadError) as e:
            fvad_mod.Engine(model, 1, 2, max_ticks=8, spectrum=bad)
        assert e.value.code == fvad_mod.EINVAL, bad
    plain = fvad_mod.Engine(model, 1, 2, max_ticks=8)
    x, _ = den_streams((19,))
    pcm = x[0][:, :100 * FRAME].reshape(2, 100, FRAME).transpose(1, 0, 2)[:, None]
    plain.push(pcm[:8])
    with pytest.raises(fvad_mod.FvadError) as e:
        plain.fetch_spectrum(8)
    assert e.value.code == fvad_mod.EINVAL
    # submit / collect: refused while uncollected; afterwards the push route's bits
    sync = fvad_mod.Engine(model, 1, 2, max_ticks=50, spectrum=(2, 140))
    eng = fvad_mod.Engine(model, 1, 2, max_ticks=50, spectrum=(2, 140))
    for k in range(2):
        want = sync.push(pcm[50 * k:50 * k + 50])
        eng.submit(pcm[50 * k:50 * k + 50])
        with pytest.raises(fvad_mod.FvadError) as e:
            eng.fetch_spectrum(50)
        assert e.value.code == fvad_mod.EINVAL
        out = eng.collect()
        assert np.array_equal(out["win_flag"], want["win_flag"]) and want["win_flag"].sum() > 0
        assert np.array_equal(bits(eng.fetch_spectrum(50)), bits(want["spectrum"]))
        assert np.array_equal(bits(eng.fetch_spectrum(20)), bits(want["spectrum"][:20]))
    eng.push(pcm[:7])
    with pytest.raises(fvad_mod.FvadError) as e:
        eng.fetch_spectrum(8)
    assert e.value.code == fvad_mod.EINVAL
    with pytest.raises(fvad_mod.FvadError) as e:
        eng.fetch_spectrum(0)
    assert e.value.code == fvad_mod.EINVAL
    assert eng.fetch_spectrum(7).shape == (7, 1, 2, 139)
    # run_resident followed by a sync
    eng.load_synthetic(20, base=3)
    eng.run_resident(20)
    eng.sync()
    res = eng.fetch(20)
    spec = eng.fetch_spectrum(20)
    flags = res["win_flag"].astype(bool)
    assert not spec[~flags].any()
    if flags.any():
        assert np.array_equal(bits(res["band"][flags][..., 0]), bits(sp.seq_sum(spec[flags], 4, 64, 2)))


# ---- spectral sweeps on the device ----
SWEEP_SPEC = (2, 140)
SWEEP_BANDS = [(4, 64), (13, 128), (10, 40), SWEEP_SPEC] + \
              [(2 + 3 * k, 30 + 5 * k) for k in range(10)] + [(60 + k, 60 + k) for k in range(5)] + \
              [(90, 100 + 8 * k) for k in range(5)]


def both(sw, cfgs):
    sw.run_host(cfgs)
    ref = su.results(sw, len(cfgs))
    sw.run(cfgs)
    return su.results(sw, len(cfgs)), ref


def test_spectral_sweep_filled_from_an_engine(fvad_mod, model):
    """The streams and push size of test_gpu_sweep.test_sweep_filled_from_an_engine
    (one stream never gets a tick), every push appended with its spectra: 96
    configs over 24 distinct bands on the device equal run_host; the lanes of
    four bands equal the engine's own attached machines; run_score equals run
    followed by score; chunks of 1 and 5 configs change nothing."""
    assert len(set(SWEEP_BANDS)) == 24
    base = fvad_mod.VadmConfig.default()
    variants = ({}, {"speech_threshold_factor": 12.0}, {"short_term_speech_avg_sec": 0.5}, {"max_speech_gap_sec": 1.0})
    cfgs = [sp.band_cfg(fvad_mod, base, lo, hi, **kw) for kw in variants for lo, hi in SWEEP_BANDS]
    assert len(cfgs) == 96
    ids, secs = [0, 4, 19, 42, 7], [70.0, 55.5, 40.0, 66.0, 12.0]
    streams = [fvad_mod.synth_stream(i, int(48000 * s), 2)[0] for i, s in zip(ids, secs)]
    B = len(streams) + 1
    eng = fvad_mod.Engine(model, B, 2, max_ticks=64, bands=SWEEP_BANDS[:4], spectrum=SWEEP_SPEC)
    eng.attach_vadm(cfgs[:4])
    sw = fvad_mod.Sweep(B, 2, spectrum=SWEEP_SPEC)
    lens = [x.shape[1] // FRAME for x in streams]
    for t0 in range(0, max(lens), 64):
        nt = min(64, max(lens) - t0)
        pcm = np.zeros((nt, B, 2, FRAME), np.float32)
        valid = np.zeros(B, np.int32)
        for s, x in enumerate(streams):
            v = max(0, min(nt, lens[s] - t0))
            valid[s] = v
            if v:
                pcm[:v, s] = x[:, t0 * FRAME:(t0 + v) * FRAME].reshape(2, v, FRAME).transpose(1, 0, 2)
        sw.append_spectra(eng.push(pcm, ticks_valid=valid), ticks_valid=valid)
    got, ref = both(sw, cfgs)
    su.assert_same(got, ref)
    total = 0
    for s in range(len(streams)):
        for mi in range(4):
            n, segs = sw.segments(s, mi)
            assert segs == eng.segments(s, mi) and n == len(segs), (s, mi)
            total += n
    assert total > 0
    assert len({tuple(got[0][(0, m)][1]) for m in range(24)}) > 1  # the band matters
    assert all(sw.segments(B - 1, m) == (0, []) and sw.snapshot(B - 1, m)["windows"] == 0 for m in range(96))
    for chunk in (1, 5):
        sw.set_debug(fvad_mod.SWEEP_DEBUG_CHUNK, chunk)
        sw.run(cfgs)
        su.assert_same(su.results(sw, len(cfgs)), ref)
    sw.set_debug(fvad_mod.SWEEP_DEBUG_CHUNK, 0)
    labels = [fvad_mod.synth_stream(i, int(48000 * s), 2)[1] for i, s in zip(ids, secs)] + [[]]
    sw.run(cfgs)
    agg, one = sw.score(labels, single=True)
    for chunk in (0, 5):
        sw.set_debug(fvad_mod.SWEEP_DEBUG_CHUNK, chunk)
        agg2, one2 = sw.run_score(cfgs, labels, single=True)
        assert np.array_equal(sw.counts(), ref[1])
        assert [bytes(a) for a in agg2] == [bytes(a) for a in agg]
        assert repr(one2) == repr(one)


def rand_sweep(fvad, B, C, spectrum, fft, lens, seed):
    """A device spectral sweep over random spectra with sweep_util's burst pattern in vad / ratio."""
    rng = np.random.default_rng(seed)
    sw = fvad.Sweep(B, C, fft_size=fft, spectrum=spectrum)
    n_spec = spectrum[1] - spectrum[0] + 1
    for s, W in enumerate(lens):
        if W == 0:
            continue
        spec = (1e-4 * (1.0 + rng.random((W, C, n_spec)))).astype(np.float32)
        vad = np.full(W, 0.05, np.float32)
        vr = np.full(W, 0.2, np.float32)
        for w0 in range(5 + 3 * s, W, 40):
            w1 = min(W, w0 + 14)
            spec[w0:w1] *= np.float32(300.0) * (1.0 + rng.random((w1 - w0, C, n_spec))).astype(np.float32)
            vad[w0:w1] = 0.9
            vr[w0:w1] = 0.9
        sw.set_spectra(s, spec, vr, vad)
    return sw


def quick_cfg(fvad, lo, hi, fft, **kw):
    c = fvad.VadmConfig.default()
    d = dict(long_term_speech_avg_sec=30 * fft / 48000.0, short_term_speech_avg_sec=2.5 * fft / 48000.0,
             min_consecutive_sec_to_open=0.0, min_vad_duration_sec=0.0, max_speech_gap_sec=2.5 * fft / 48000.0,
             speech_threshold_factor=5.0, has_initial_long_term_avg=0)
    d.update(kw)
    return sp.band_cfg(fvad, c, lo, hi, fft_size=fft, **d)


@pytest.mark.parametrize("case", ["n_spec_1", "one_band", "bands_300_c8", "unstaged"])
def test_small_and_awkward_shapes(fvad_mod, case):
    """n_spec = 1; D = 1; 300 distinct bands (more than one pass of the 256
    threads) on 8 channels x 1 025 bins (the whole LDS stage); a window above
    the stage (8 channels x 2 049 bins, read from HBM); a stream with 0
    windows in each."""
    if case == "n_spec_1":
        sw = rand_sweep(fvad_mod, 3, 2, (7, 7), 2048, [90, 0, 61], 1)
        cfgs = [quick_cfg(fvad_mod, 7, 7, 2048), quick_cfg(fvad_mod, 7, 7, 2048, speech_threshold_factor=2.0)]
    elif case == "one_band":
        sw = rand_sweep(fvad_mod, 3, 2, (0, 200), 2048, [0, 90, 61], 2)
        cfgs = [quick_cfg(fvad_mod, 3, 150, 2048, speech_threshold_factor=f) for f in (2.0, 5.0, 50.0)]
    elif case == "bands_300_c8":
        sw = rand_sweep(fvad_mod, 2, 8, (0, 1024), 2048, [70, 0], 3)
        cfgs = [quick_cfg(fvad_mod, k, 1024 - 2 * k, 2048) for k in range(299)] + [quick_cfg(fvad_mod, 0, 0, 2048)]
        assert len({(round(c.speech_min_freq), round(c.speech_max_freq)) for c in cfgs}) == 300
    else:
        sw = rand_sweep(fvad_mod, 2, 8, (0, 2048), 4096, [70, 0], 4)
        cfgs = [quick_cfg(fvad_mod, lo, hi, 4096) for lo, hi in ((0, 2048), (2048, 2048), (5, 1500), (1024, 1031))]
    got, ref = both(sw, cfgs)
    su.assert_same(got, ref)
    assert ref[1].sum() > 0
    sw.set_debug(fvad_mod.SWEEP_DEBUG_CHUNK, 7)
    sw.run(cfgs)
    su.assert_same(su.results(sw, len(cfgs)), ref)
