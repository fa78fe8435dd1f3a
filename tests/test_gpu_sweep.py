"""Config sweep on the device (k_vadm_sweep: one lane per (stream, config), the
engine's device VADMachine over a stream's whole recorded window sequence)
against the host VADMachine (fvad_sweep_run_host) on the same sweep, and
against the engine's own attached machines on windows taken from its pushes.
Lane by lane: segment totals, segments with their debug averages, and every
field of the final state, the three averages by their bits."""
import numpy as np
import pytest

import sweep_util as su

pytestmark = pytest.mark.gpu


def both(sw, cfgs):
    """(device results, host results) of one sweep."""
    sw.run_host(cfgs)
    ref = su.results(sw, len(cfgs))
    sw.run(cfgs)
    return su.results(sw, len(cfgs)), ref


@pytest.fixture(scope="module")
def gen_sweep(fvad_mod):
    """The generator's 5 streams (one ragged) with the 36-config grid, half of
    it on the second band, and the host's results."""
    sw = fvad_mod.Sweep(su.N_STREAMS, 2, bands=su.BANDS)
    su.fill(sw)
    cfgs = su.grid(fvad_mod)
    sw.run_host(cfgs)
    return sw, cfgs, su.results(sw, len(cfgs))


def test_device_sweep_matches_host(fvad_mod, gen_sweep):
    """A partial wave of configs (36 of 64 lanes), ragged streams, long-term
    buffers that wrap many times / a few times / never, the non-lazy filling
    phase followed by the lazy walk."""
    sw, cfgs, ref = gen_sweep
    sw.run(cfgs)
    got = su.results(sw, len(cfgs))
    su.assert_same(got, ref)
    assert (ref[1] >= 2).sum() * 4 >= ref[1].size and (ref[1] == 0).sum() * 4 >= ref[1].size


def test_more_configs_than_a_wave(fvad_mod):
    """70 configs: two waves of configs per stream, the second partial; once
    more three configs per chunk (24 chunks)."""
    sw = fvad_mod.Sweep(2, 2, bands=su.BANDS)
    su.fill(sw, streams=[0, 1], W=300)
    g = su.grid(fvad_mod)
    cfgs = g + [su.copy_cfg(fvad_mod, c, min_vad_duration_sec=0.3) for c in g[:34]]
    assert len(cfgs) == 70
    got, ref = both(sw, cfgs)
    su.assert_same(got, ref)
    assert ref[1].sum() > 0
    sw.set_debug(fvad_mod.SWEEP_DEBUG_CHUNK, 3)
    sw.run(cfgs)
    su.assert_same(su.results(sw, len(cfgs)), ref)


@pytest.mark.parametrize("bound,defer", [(0, 0), (-1, 0), (0, 1), (0, 7), (-1, 5)])
def test_debug_hooks_change_nothing(fvad_mod, gen_sweep, bound, defer):
    """The lazy walk's bound made infinite (every test the estimate would
    settle folds exactly instead), owed folds settled after 1 / 7 / 5 long
    pushes: the results are the host's in every case, and the counters show
    that the branch ran."""
    _, cfgs, ref = gen_sweep
    sw = fvad_mod.Sweep(su.N_STREAMS, 2, bands=su.BANDS)
    su.fill(sw)
    sw.set_debug(fvad_mod.SWEEP_DEBUG_BOUND_SCALE, bound)
    sw.set_debug(fvad_mod.SWEEP_DEBUG_DEFER_MAX, defer)
    sw.set_debug(fvad_mod.SWEEP_DEBUG_COUNT, 1)
    sw.run(cfgs)
    cnt = sw.debug_counts()
    print(bound, defer, cnt)
    su.assert_same(su.results(sw, len(cfgs)), ref)
    if bound == -1:
        assert cnt["open"] > 0 and cnt["settled"] == 0, cnt
    elif defer == 0:
        assert cnt["settled"] > 0, cnt


def test_non_lazy_arms(fvad_mod):
    """A negative band value in one channel of window 60 (no bound holds while
    it sits in a long-term buffer: lt_neg's exact folds, then back to the lazy
    walk once it has left a 23- or 234-entry buffer) and a config with
    threshold factor -1 (never lazy)."""
    sw = fvad_mod.Sweep(1, 2, bands=su.BANDS)
    band, vad, vr = su.gen(2, 600)
    band[60, 1, :] = -band[60, 1, :]
    sw.set_windows(0, band, vr, vad)
    cfgs = su.grid(fvad_mod) + [su.copy_cfg(fvad_mod, fvad_mod.VadmConfig.default(), speech_threshold_factor=-1.0,
                                            long_term_speech_avg_sec=10.0)]
    got, ref = both(sw, cfgs)
    su.assert_same(got, ref)
    assert ref[1].sum() > 0


def test_segment_overflow(fvad_mod, gen_sweep):
    """seg_capacity 2: lanes with 3 or 4 segments report the true total and hold the first two."""
    _, cfgs, ref = gen_sweep
    sw = fvad_mod.Sweep(su.N_STREAMS, 2, bands=su.BANDS, seg_capacity=2)
    su.fill(sw)
    sw.run(cfgs)
    assert np.array_equal(sw.counts(), ref[1])
    over = 0
    for (s, m), (total, segs, snap) in ref[0].items():
        t, g = sw.segments(s, m)
        assert t == total and g == segs[:2] and sw.snapshot(s, m) == snap, (s, m)
        over += total > 2
    assert over > 0
    with pytest.raises(fvad_mod.FvadError):
        sw.score([su.labels(s, su.stream_len(s)) for s in range(su.N_STREAMS)])


def engine_pushes(fvad_mod, eng, streams, sw, max_ticks):
    """Ragged pushes of max_ticks ticks, each appended to the sweep."""
    B, C = len(streams), streams[0].shape[0]
    lens = [x.shape[1] // 480 for x in streams]
    for t0 in range(0, max(lens), max_ticks):
        nt = min(max_ticks, max(lens) - t0)
        pcm = np.zeros((nt, eng.B, C, 480), np.float32)
        valid = np.zeros(eng.B, np.int32)
        for s, x in enumerate(streams):
            v = max(0, min(nt, lens[s] - t0))
            valid[s] = v
            if v:
                pcm[:v, s] = x[:, t0 * 480:(t0 + v) * 480].reshape(C, v, 480).transpose(1, 0, 2)
        sw.append_outputs(eng.push(pcm, ticks_valid=valid), ticks_valid=valid)


def test_sweep_filled_from_an_engine(fvad_mod):
    """The five synthetic streams and both configs of
    test_gpu_vadm.test_device_vadm_matches_host, plus a sixth stream that never
    gets a tick (0 windows): every push appended to the sweep, which then runs
    those two configs and six grid neighbours.  Configs 0 and 1 give the
    engine's own attached machines' segments; and a one-config run works."""
    m = fvad_mod.Model(seed=1)
    alt = fvad_mod.VadmConfig.default()
    alt.speech_min_freq, alt.speech_max_freq = 300.0, 3000.0
    alt.min_vad_duration_sec = 0.3
    alt.long_term_speech_avg_sec = 10.0
    main = fvad_mod.VadmConfig.default()
    ids, secs = [0, 4, 19, 42, 7], [70.0, 55.5, 40.0, 66.0, 12.0]
    streams = [fvad_mod.synth_stream(i, int(48000 * s), 2)[0] for i, s in zip(ids, secs)]
    eng = fvad_mod.Engine(m, len(streams) + 1, 2, max_ticks=64, bands=su.BANDS)
    eng.attach_vadm([main, alt])
    sw = fvad_mod.Sweep(len(streams) + 1, 2, bands=su.BANDS)
    engine_pushes(fvad_mod, eng, streams, sw, 64)
    cfgs = [main, alt] + [su.copy_cfg(fvad_mod, c, **{k: v}) for c in (main, alt)
                          for k, v in (("speech_threshold_factor", 12.0), ("short_term_speech_avg_sec", 0.5),
                                       ("max_speech_gap_sec", 1.0))]
    assert len(cfgs) == 8
    got, ref = both(sw, cfgs)
    su.assert_same(got, ref)
    total = 0
    for s in range(len(streams)):
        for mi in range(2):
            n, segs = sw.segments(s, mi)
            assert segs == eng.segments(s, mi) and n == len(segs), (s, mi)
            total += n
    assert total > 0
    empty = len(streams)
    assert all(sw.segments(empty, mi) == (0, []) and sw.snapshot(empty, mi)["windows"] == 0 for mi in range(8))
    sw.run([alt])
    assert [sw.segments(s, 0) for s in range(len(streams) + 1)] == [got[0][(s, 1)][:2] for s in range(len(streams) + 1)]


def test_sweep_fft_size_200(fvad_mod):
    """fft_size 200 without the denoiser: up to three windows per tick in the
    outputs' slots; the sweep's segments are the attached machine's."""
    m = fvad_mod.Model(seed=1)
    cfg = fvad_mod.VadmConfig.default()
    cfg.long_term_speech_avg_sec = 1.0
    cfg.min_vad_duration_sec = 0.1
    cfg.max_speech_gap_sec = 0.3
    cfg.speech_threshold_factor = 3.0
    hz = 48000.0 / 200
    cfg.speech_min_freq, cfg.speech_max_freq = 1 * hz, 6 * hz
    streams = [fvad_mod.synth_stream(i, 48000 * 3, 2)[0] for i in (0, 19)]
    eng = fvad_mod.Engine(m, 2, 2, max_ticks=50, fft_size=200, bands=((1, 6),), use_denoiser=False)
    assert eng.wpt == 3
    eng.attach_vadm([cfg])
    sw = fvad_mod.Sweep(2, 2, fft_size=200, bands=((1, 6),), use_denoiser=False)
    engine_pushes(fvad_mod, eng, streams, sw, 50)
    cfgs = [cfg, su.copy_cfg(fvad_mod, cfg, speech_threshold_factor=6.0)]
    got, ref = both(sw, cfgs)
    su.assert_same(got, ref)
    for s in range(2):
        n, segs = sw.segments(s, 0)
        assert sw.snapshot(s, 0)["windows"] == 48000 * 3 // 200
        assert segs == eng.segments(s, 0) and n == len(segs), s
        assert sw.snapshot(s, 0) == eng.vadm_snapshot(s, 0), s
