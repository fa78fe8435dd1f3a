"""Shared by the run_score tests (test_sweep_score_cpu.py, test_gpu_sweep_score.py):
the expected scores -- fvad.evaluate per lane on a run's segments and
fvad.aggregate per config, the oracle -- the comparison by bits, the
adversarial label set and the many-segment workload."""
import numpy as np

import sweep_util as su

KW = dict(ignore_shorter_than_sec=0.5, extrude_start=0.5, extrude_end=1.0, fill_gaps=0.5)
F48 = np.float32(48000.0)


def secs(segs):
    """A lane's segments as the library converts them: (float)sample / 48000.0f."""
    return [(np.float32(a) / F48, np.float32(b) / F48) for a, b, _, _ in segs]


def lane_segments(sw, n_cfgs):
    """After run / run_host: {(stream, cfg): segments in seconds}."""
    out = {}
    for s in range(sw.B):
        for m in range(n_cfgs):
            total, segs = sw.segments(s, m)
            assert total == len(segs), (s, m, total)
            out[s, m] = secs(segs)
    return out


def expected(fvad, lanes, B, n_cfgs, refs, stat):
    """(aggregates [cfg], singles [cfg][stream]) by the host evaluator; stat: one
    dict, or one per config."""
    agg, single = [], []
    for m in range(n_cfgs):
        kw = stat if isinstance(stat, dict) else stat[m]
        single.append([fvad.evaluate(lanes[s, m], refs[s], **kw) for s in range(B)])
        agg.append(fvad.aggregate(single[-1]))
    return agg, single


def same_bits(got, exp):
    """float32 arrays: equal bits wherever exp is not NaN, NaN where it is."""
    g, e = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    nan = np.isnan(e)
    return bool(g.shape == e.shape and np.isnan(g[nan]).all() and
                np.array_equal(g[~nan].view(np.uint32), e[~nan].view(np.uint32)))


def assert_bits(got, exp, where):
    assert same_bits(got, exp), (where, got, exp)


def stat_vec(fvad, d):
    return np.array([d[n] for n in fvad._STAT_FIELDS], np.float32)


def agg_vec(a):
    return np.frombuffer(bytes(a), np.float32)


def assert_scores(fvad, got, exp):
    (ga, gs), (ea, es) = got, exp
    assert len(ga) == len(ea) and len(gs) == len(es)
    for m in range(len(ea)):
        for s in range(len(es[m])):
            assert_bits(stat_vec(fvad, gs[m][s]), stat_vec(fvad, es[m][s]), ("single", m, s))
        assert_bits(agg_vec(ga[m]), agg_vec(ea[m]), ("aggregate", m))


def plain_labels(data):
    return [su.labels(s, len(d[2])) for s, d in enumerate(data)]


def adversarial_labels(lanes, n_cfgs):
    """Per stream of sweep_util's five, in an order that is not sorted: every
    burst split into three labels with gaps of 0.2 s and 0.6 s (fill_gaps 0.5
    fills the first only), a label nested in the first, a second label with the
    first one's start, a zero-length label, a 0.1 s label away from the bursts
    (shorter than ignore_shorter_than_sec), and a label that ends exactly at
    the start, in f32 seconds, of the stream's first segment that starts after
    0.5 s (overlap 0: no opponent).  The last stream has no labels."""
    refs = []
    for s in range(su.N_STREAMS - 1):
        lab = []
        for k, (b0, b1) in enumerate(su.labels(s, su.stream_len(s))):
            x = (b1 - b0 - 0.8) / 3.0
            assert x > 0.05
            lab += [(b0, b0 + x), (b0 + x + 0.2, b0 + 2 * x + 0.2), (b0 + 2 * x + 0.8, b1)]
            if k == 0:
                lab += [(b0 + 0.25 * x, b0 + 0.5 * x), (b0, b0 + 0.5 * x), (b0 + 0.75 * x, b0 + 0.75 * x)]
        lab.append((0.05, 0.15))
        edge = [seg[0] for m in range(n_cfgs) for seg in lanes[s, m] if seg[0] > 0.5]
        if edge:  # not every stream has such a segment; test_adversarial_labels_are_not_vacuous asks for one
            lab.append((float(edge[0]) - 0.3, float(edge[0])))
        refs.append(lab[::2] + lab[1::2][::-1])
        starts = [a for a, _ in refs[-1]]
        assert starts != sorted(starts)
    refs.append([])
    return refs


def reactive_sweep(fvad, device, seg_capacity=64, n_streams=2, W=400):
    """test_append_outputs_compaction's reactive machines over random windows:
    threshold factor 1, no opening time, no gap, no minimum duration, a
    long-term buffer of one to three entries -- a window is speech iff its
    ratio is above 0 and it exceeds the mean of the last k values of windows
    that were not.  Returns (sweep, configs, labels)."""
    hz = 48000.0 / su.FFT
    base = fvad.VadmConfig.default()
    base.speech_min_freq, base.speech_max_freq = 2 * hz, 20 * hz
    base.short_term_speech_avg_sec = base.channel_vol_ratio_avg_sec = 1e-4
    cfgs = [su.copy_cfg(fvad, base, long_term_speech_avg_sec=(k + 0.5) / hz, speech_threshold_factor=1.0,
                        has_initial_long_term_avg=0, channel_vol_ratio_threshold=0.0,
                        min_consecutive_sec_to_open=0.0, max_speech_gap_sec=0.0, min_vad_duration_sec=0.0)
            for k in (1, 2, 3)]
    sw = fvad.Sweep(n_streams, 2, device=device, bands=((1, 9), (2, 20)), seg_capacity=seg_capacity)
    rng = np.random.default_rng(11)
    for s in range(n_streams):
        # the long-term buffer takes a window's value only while the condition is not met, so a machine closes
        # again only where the ratio test fails: runs of 2..4 windows with ratio 0 between runs of 2..6 with a
        # random one (two windows in a row open a segment, two close it)
        vr = np.concatenate([np.concatenate([rng.random(rng.integers(2, 7)) + 0.01, np.zeros(rng.integers(2, 5))])
                             for _ in range(W)])[:W].astype(np.float32)
        sw.set_windows(s, rng.random((W, 2, 2)).astype(np.float32), vr, rng.random(W).astype(np.float32))
    end = W * su.FFT / 48000.0
    refs = [[(1.0, 3.0), (2.5, 4.0), (6.0, 6.2), (0.4 * end, 0.7 * end), (end - 1.0, end + 1.0)][: 5 - s] + [(7.1, 7.1)]
            for s in range(n_streams)]
    return sw, cfgs, refs
