"""Config sweep (fvad.Sweep) on the host: a device = -1 sweep needs no GPU and
runs the host VADMachine.  Its results against fvad.VADMachine fed window by
window, the compaction of a push's outputs into window sequences, the scores
against fvad.evaluate / fvad.aggregate, the validation, and k_vadm_sweep's
register budget from the compiler's remarks."""
import os

import numpy as np
import pytest

import sweep_util as su


def host_sweep(fvad, **kw):
    kw.setdefault("bands", su.BANDS)
    return fvad.Sweep(kw.pop("n_streams", su.N_STREAMS), 2, device=-1, **kw)


@pytest.fixture(scope="module")
def host_run(fvad_mod):
    sw = host_sweep(fvad_mod)
    data = su.fill(sw)
    cfgs = su.grid(fvad_mod)
    sw.run(cfgs)
    return sw, data, cfgs


def test_host_sweep_matches_vadmachine(fvad_mod, host_run):
    """Every lane of the generator's 5 streams x 36 configs equals a
    fvad.VADMachine fed the same windows one by one: segments with their debug
    averages, the segment total, and state().  Not vacuous: at least a quarter
    of the lanes have two or more segments and at least a quarter have none."""
    sw, data, cfgs = host_run
    counts = sw.counts()
    n2 = n0 = 0
    for s, (band, vad, vr) in enumerate(data):
        for m, c in enumerate(cfgs):
            vm = fvad_mod.VADMachine(c, n_channels=2)
            for w in range(len(vr)):
                vm.run(w * su.FFT, band[w, :, su.slot_of(c)], float(vad[w]), float(vr[w]))
            ref = vm.segments()
            total, segs = sw.segments(s, m)
            assert total == len(ref) == counts[s, m] and segs == ref, (s, m, segs[:2], ref[:2])
            snap = sw.snapshot(s, m)
            assert (snap["speech_state"], snap["speech_start"], snap["speech_end"]) == vm.state(), (s, m)
            assert snap["windows"] == len(vr) and snap["n_segments"] == len(ref)
            n2 += len(ref) >= 2
            n0 += len(ref) == 0
    lanes = len(data) * len(cfgs)
    print("lanes", lanes, "with >= 2 segments", n2, "with none", n0, "max", counts.max())
    assert 4 * n2 >= lanes and 4 * n0 >= lanes, (n2, n0, lanes)


def test_run_host_is_run_on_a_host_sweep(fvad_mod, host_run):
    sw, _, cfgs = host_run
    ref = su.results(sw, len(cfgs))
    sw.run_host(cfgs)
    su.assert_same(su.results(sw, len(cfgs)), ref)


@pytest.mark.parametrize("fft_size,W", [(2048, 1), (200, 3)])
def test_append_outputs_compaction(fvad_mod, fft_size, W):
    """Hand-built push outputs: ragged ticks_valid, ticks with win_flag 0..W.
    Each stream's sequence is its valid ticks' slots w < win_flag, in order;
    what lies in invalid ticks or in slots >= win_flag never enters."""
    B, C, nb, T = 3, 2, 2, 6
    rng = np.random.default_rng(7)
    flags = np.array([[1, 0, 1], [0, 1, 1], [1, 1, 0], [1, 0, 1], [0, 0, 1], [1, 1, 1]], np.int32)
    if W == 3:
        flags = np.array([[3, 0, 1], [0, 2, 3], [2, 3, 0], [1, 1, 2], [3, 0, 3], [2, 2, 1]], np.int32)
    valid = np.array([6, 4, 0], np.int32)
    ws = (T, B) if W == 1 else (T, B, W)
    out = {"win_flag": flags, "win_ratio": rng.random(ws).astype(np.float32),
           "win_vad": rng.random(ws).astype(np.float32), "band": rng.random(ws + (C, nb)).astype(np.float32)}
    cfg = fvad_mod.VadmConfig.default()
    hz = 48000.0 / fft_size
    cfg.speech_min_freq, cfg.speech_max_freq = 2 * hz, 20 * hz
    cfg.short_term_speech_avg_sec = cfg.channel_vol_ratio_avg_sec = 1e-4  # one entry: the averages are the last window's
    sw = fvad_mod.Sweep(B, C, device=-1, fft_size=fft_size, bands=((1, 9), (2, 20)))
    second = {k: v[:2] for k, v in out.items()}
    sw.append_outputs(out, ticks_valid=valid)
    sw.append_outputs(second)  # a second push, every tick valid
    exp = [[] for _ in range(B)]
    for o, tv in ((out, valid), (second, [2] * B)):
        r, v, b = (o[k].reshape((-1, B, W) + o[k].shape[len(ws):]) for k in ("win_ratio", "win_vad", "band"))
        for s in range(B):
            for t in range(tv[s]):
                for w in range(o["win_flag"][t, s]):
                    exp[s].append((b[t, s, w], v[t, s, w], r[t, s, w]))
    sw.run([cfg])
    for s in range(B):
        snap = sw.snapshot(s, 0)
        assert snap["windows"] == len(exp[s]), (s, snap["windows"], len(exp[s]))
        # the last window's values, seen through the one-entry averages (min over channels of band 1, ratio)
        band, _, ratio = exp[s][-1]
        assert snap["avg"][1] == float(min(band[0, 1], band[1, 1])) and snap["avg"][2] == float(ratio), s
    assert [len(e) for e in exp] == ([5, 3, 2] if W == 1 else [14, 8, 4])
    # the whole order: a sweep set directly with the expected sequences gives the same final states
    sw2 = fvad_mod.Sweep(B, C, device=-1, fft_size=fft_size, bands=((1, 9), (2, 20)))
    for s in range(B):
        sw2.set_windows(s, np.stack([e[0] for e in exp[s]]), [e[2] for e in exp[s]], [e[1] for e in exp[s]])
    # machines that react to every window: a window is speech iff its value exceeds the mean of the last k
    # values pushed, segments open and close at once, so the segment ends and the push counts trace the order
    cfgs = [cfg] + [su.copy_cfg(fvad_mod, cfg, long_term_speech_avg_sec=(k + 0.5) / hz, speech_threshold_factor=1.0,
                                has_initial_long_term_avg=0, channel_vol_ratio_threshold=0.0,
                                min_consecutive_sec_to_open=0.0, max_speech_gap_sec=0.0, min_vad_duration_sec=0.0)
                    for k in (1, 2, 3)]
    sw.run(cfgs)
    sw2.run(cfgs)
    su.assert_same(su.results(sw, 4), su.results(sw2, 4))
    # and they do tell one order from another: the same windows with the first two swapped
    e = exp[0][:2][::-1] + exp[0][2:]
    sw2.set_windows(0, np.stack([x[0] for x in e]), [x[2] for x in e], [x[1] for x in e])
    sw2.run(cfgs)
    assert any(sw2.snapshot(0, m) != sw.snapshot(0, m) for m in (1, 2, 3))
    with pytest.raises(fvad_mod.FvadError) as e:
        sw.append_outputs(out, ticks_valid=[7, 0, 0])
    assert e.value.code == fvad_mod.EINVAL


def test_score_matches_evaluator(fvad_mod, host_run):
    """score() against fvad.evaluate per stream and fvad.aggregate per config on
    the same segments (as seconds: (float)sample / 48000.0f) and labels."""
    sw, data, cfgs = host_run
    refs = [su.labels(s, len(d[2])) for s, d in enumerate(data)]
    kw = dict(ignore_shorter_than_sec=0.5, extrude_start=0.5, extrude_end=1.0, fill_gaps=0.5)
    agg, single = sw.score(refs, single=True, **kw)
    assert len(agg) == len(cfgs)
    nonzero = 0
    for m in range(len(cfgs)):
        stats = []
        for s in range(sw.B):
            segs = [(np.float32(a) / np.float32(48000.0), np.float32(b) / np.float32(48000.0))
                    for a, b, _, _ in sw.segments(s, m)[1]]
            stats.append(fvad_mod.evaluate(segs, refs[s], **kw))
            assert np.array_equal(np.array([single[m][s][n] for n in fvad_mod._STAT_FIELDS], np.float32),
                                  np.array([stats[-1][n] for n in fvad_mod._STAT_FIELDS], np.float32),
                                  equal_nan=True), (m, s)
        ref = fvad_mod.aggregate(stats)
        assert np.array_equal(np.frombuffer(bytes(agg[m]), np.float32), np.frombuffer(bytes(ref), np.float32),
                              equal_nan=True), m
        nonzero += agg[m].true_positives_sec > 0
    assert nonzero > 0


def test_score_refuses_a_truncated_lane(fvad_mod, host_run):
    _, data, cfgs = host_run
    sw = host_sweep(fvad_mod, seg_capacity=1)
    su.fill(sw)
    sw.run(cfgs)
    assert sw.counts().max() > 1
    with pytest.raises(fvad_mod.FvadError) as e:
        sw.score([su.labels(s, len(d[2])) for s, d in enumerate(data)])
    assert e.value.code == fvad_mod.EINVAL and "stream" in str(e.value) and "config" in str(e.value)


def test_validation(fvad_mod):
    sw = host_sweep(fvad_mod)
    su.fill(sw)
    bad = fvad_mod.VadmConfig.default()
    bad.speech_min_freq = 500.0  # bins 21..64: none of the sweep's bands
    cfgs = su.grid(fvad_mod)[:3] + [bad]
    with pytest.raises(fvad_mod.FvadError) as e:
        sw.run(cfgs)
    assert e.value.code == fvad_mod.EINVAL and "config 3" in str(e.value)
    assert sw.n_cfgs == 0  # nothing ran
    with pytest.raises(fvad_mod.FvadError) as e:
        fvad_mod.Sweep(2, 2, device=-1, fft_size=2047)
    assert e.value.code == fvad_mod.EINVAL
    with pytest.raises(fvad_mod.FvadError) as e:
        fvad_mod.Sweep(2, 2, device=-1, sample_rate=44100)
    assert e.value.code == -6  # FVAD_ERATE
    for kw in (dict(seg_capacity=0), dict(bands=()), dict(n_streams=0)):
        with pytest.raises(fvad_mod.FvadError) as e:
            host_sweep(fvad_mod, **kw)
        assert e.value.code == fvad_mod.EINVAL
    band, vad, vr = su.gen(0, 10)
    for s in (-1, su.N_STREAMS):
        with pytest.raises(fvad_mod.FvadError) as e:
            sw.set_windows(s, band, vr, vad)
        assert e.value.code == fvad_mod.EINVAL
    g = su.grid(fvad_mod)
    b1, b2, b36 = sw.bytes(g[:1]), sw.bytes(g[:2]), sw.bytes(g)
    assert 0 < b1 < b2 < b36
    assert sw.bytes(cfgs) == 0  # the bad band


def test_vad_is_zero_without_the_denoiser(fvad_mod):
    """use_denoiser = 0: every window's vad enters the machines as 0, so a
    segment's debug_rnn_vad is 0 where the same windows give 0.9 with it."""
    cfgs = su.grid(fvad_mod)
    out = []
    for den in (True, False):
        sw = host_sweep(fvad_mod, n_streams=1, use_denoiser=den)
        su.fill(sw, streams=[0])
        sw.run(cfgs)
        out.append([g for m in range(len(cfgs)) for g in sw.segments(0, m)[1]])
    assert len(out[0]) > 0 and len(out[0]) == len(out[1])
    assert all(a[:2] == b[:2] and a[3] == b[3] and a[2] > 0.5 and b[2] == 0.0 for a, b in zip(*out))


def test_sweep_kernel_resources():
    """k_vadm_sweep's budget as DESIGN.md section 7 states it: no scratch, no
    LDS beyond 160 KB, 3 waves per SIMD."""
    import test_kernel_resources as tkr
    if not os.path.exists(tkr.HIPCC):
        pytest.skip("hipcc not available")
    r = tkr.resources("fvad_sweep.hip")
    print(r)
    for k in ("k_vadm_sweep", "k_sweep_min"):
        assert k in r, sorted(r)
        assert r[k]["VGPRs_spill"] == 0 and r[k]["LDS"] <= 160 * 1024, (k, r[k])
    assert r["k_vadm_sweep"]["Occupancy"] >= 3, r["k_vadm_sweep"]
