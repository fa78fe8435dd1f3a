"""Sweep.run_score on the device (k_sweep_score behind each chunk's
k_vadm_sweep) against the same sweep's run_host scored on the host with
fvad.evaluate and fvad.aggregate: every statistic of every lane and every
aggregate by its bits (NaN for NaN)."""
import numpy as np
import pytest

import sweep_score_util as ssu
import sweep_util as su

pytestmark = pytest.mark.gpu


def host_expected(fvad, sw, cfgs, refs, stat):
    """run_host on this sweep, scored by the host evaluator; with its counts and snapshots."""
    sw.run_host(cfgs)
    lanes = ssu.lane_segments(sw, len(cfgs))
    snaps = {k: sw.snapshot(*k) for k in lanes}
    return ssu.expected(fvad, lanes, sw.B, len(cfgs), refs, stat), lanes, sw.counts(), snaps


@pytest.fixture(scope="module")
def gen_sweep(fvad_mod):
    """sweep_util's 5 streams (one ragged) x 36 configs (a partial wave) x 600
    windows, the host's lanes and both label sets."""
    sw = fvad_mod.Sweep(su.N_STREAMS, 2, bands=su.BANDS)
    data = su.fill(sw)
    cfgs = su.grid(fvad_mod)
    sw.run_host(cfgs)
    lanes = ssu.lane_segments(sw, len(cfgs))
    labels = {"plain": ssu.plain_labels(data), "adversarial": ssu.adversarial_labels(lanes, len(cfgs))}
    return sw, cfgs, lanes, labels, sw.counts(), {k: sw.snapshot(*k) for k in lanes}


@pytest.mark.parametrize("which", ["plain", "adversarial"])
def test_grid_matches_host(fvad_mod, gen_sweep, which):
    sw, cfgs, lanes, labels, counts, snaps = gen_sweep
    exp = ssu.expected(fvad_mod, lanes, sw.B, len(cfgs), labels[which], ssu.KW)
    got = sw.run_score(cfgs, labels[which], stat=ssu.KW, single=True)
    ssu.assert_scores(fvad_mod, got, exp)
    assert any(a.true_positives_sec > 0 for a in exp[0])


def test_counts_and_snapshots_are_the_runs(fvad_mod, gen_sweep):
    """After run_score: counts and snapshots equal run's (the host's, which
    test_gpu_sweep shows run equals), no segments, and the copy back is the
    states, statistics and status words."""
    sw, cfgs, lanes, labels, counts, snaps = gen_sweep
    sw.run(cfgs)
    run = su.results(sw, len(cfgs))
    back_run = sw.last_run()["bytes_back"]
    sw.run_score(cfgs, labels["plain"], stat=ssu.KW)
    assert np.array_equal(sw.counts(), run[1]) and np.array_equal(run[1], counts)
    for k, (total, segs, snap) in run[0].items():
        assert sw.segments(*k) == (total, []) and sw.snapshot(*k) == snap == snaps[k], k
    last = sw.last_run()
    n = su.N_STREAMS * len(cfgs)
    assert last["n_cfgs"] == len(cfgs) and not last["kept_segments"]
    assert back_run - last["bytes_back"] == n * (24 * sw.cfg.seg_capacity - 44 - 4)
    with pytest.raises(fvad_mod.FvadError) as e:
        sw.score(labels["plain"])
    assert e.value.code == fvad_mod.EINVAL


def test_debug_counts_describe_the_run_score(fvad_mod, gen_sweep):
    """FVAD_SWEEP_DEBUG_COUNT: the counters after run_score are those of a run
    of the same configs (the machines' walk is the same kernel launch)."""
    _, cfgs, _, labels, _, _ = gen_sweep
    sw = fvad_mod.Sweep(su.N_STREAMS, 2, bands=su.BANDS)
    su.fill(sw)
    sw.set_debug(fvad_mod.SWEEP_DEBUG_COUNT, 1)
    sw.run(cfgs)
    cnt = sw.debug_counts()
    assert sum(cnt.values()) > 0, cnt
    sw.run(cfgs[:1])  # other counters in between
    assert sw.debug_counts() != cnt
    sw.run_score(cfgs, labels["plain"], stat=ssu.KW)
    assert sw.debug_counts() == cnt


def test_more_configs_than_a_wave_and_chunks(fvad_mod):
    """70 configs on 2 streams x 300 windows: two waves, the second partial;
    again three configs per chunk (24 chunks): the same bits."""
    sw = fvad_mod.Sweep(2, 2, bands=su.BANDS)
    data = su.fill(sw, streams=[0, 1], W=300)
    g = su.grid(fvad_mod)
    cfgs = g + [su.copy_cfg(fvad_mod, c, min_vad_duration_sec=0.3) for c in g[:34]]
    assert len(cfgs) == 70
    refs = [su.labels(s, 300) for s in (0, 1)]
    stats = [dict(ssu.KW, ignore_shorter_than_sec=0.02 * m) for m in range(70)]  # the chunk's offset into them
    exp, _, counts, _ = host_expected(fvad_mod, sw, cfgs, refs, stats)
    assert counts.sum() > 0
    got = sw.run_score(cfgs, refs, stat=stats, single=True)
    ssu.assert_scores(fvad_mod, got, exp)
    sw.set_debug(fvad_mod.SWEEP_DEBUG_CHUNK, 3)
    chunked = sw.run_score(cfgs, refs, stat=stats, single=True)
    ssu.assert_scores(fvad_mod, chunked, exp)
    assert np.array_equal(sw.counts(), counts)


@pytest.mark.parametrize("seg_capacity", [64, 41])
def test_many_short_overlapping_segments(fvad_mod, seg_capacity):
    """The reactive machines: 27 to 41 segments per lane whose padding
    overlaps, at seg_capacity 64 and at 41, where the busiest lane's row is
    exactly full (the kernel has one form: it reads the rows in place)."""
    sw, cfgs, refs = ssu.reactive_sweep(fvad_mod, device=0, seg_capacity=seg_capacity)
    exp, _, counts, _ = host_expected(fvad_mod, sw, cfgs, refs, ssu.KW)
    assert counts.min() >= 20 and counts.max() == 41, counts
    ssu.assert_scores(fvad_mod, sw.run_score(cfgs, refs, stat=ssu.KW, single=True), exp)
    assert np.array_equal(sw.counts(), counts)


def test_per_config_stat_configs(fvad_mod, gen_sweep):
    sw, cfgs, lanes, labels, _, _ = gen_sweep
    refs = labels["adversarial"]
    stats = [dict(ssu.KW, ignore_shorter_than_sec=0.05 * m) for m in range(len(cfgs))]
    exp = ssu.expected(fvad_mod, lanes, sw.B, len(cfgs), refs, stats)
    ssu.assert_scores(fvad_mod, sw.run_score(cfgs, refs, stat=stats, single=True), exp)


def test_empty_streams(fvad_mod):
    """Stream 1 has labels and no windows, stream 2 neither."""
    cfgs = su.grid(fvad_mod)[:4]
    sw = fvad_mod.Sweep(3, 2, bands=su.BANDS)
    su.fill(sw, streams=[0])
    refs = [su.labels(0, su.stream_len(0)), [(1.0, 2.5), (0.2, 0.4)], []]
    exp, _, _, _ = host_expected(fvad_mod, sw, cfgs, refs, ssu.KW)
    agg, single = sw.run_score(cfgs, refs, stat=ssu.KW, single=True)
    ssu.assert_scores(fvad_mod, (agg, single), exp)
    assert single[0][1]["false_negatives_sec"] == 1.5 and np.isnan(single[0][2]["precision"])


def test_over_capacity(fvad_mod, gen_sweep):
    _, cfgs, _, labels, counts, snaps = gen_sweep
    sw = fvad_mod.Sweep(su.N_STREAMS, 2, bands=su.BANDS, seg_capacity=1)
    su.fill(sw)
    s, m = next((s, m) for s in range(su.N_STREAMS) for m in range(len(cfgs)) if counts[s, m] > 1)
    with pytest.raises(fvad_mod.FvadError) as e:
        sw.run_score(cfgs, labels["plain"], stat=ssu.KW)
    assert e.value.code == fvad_mod.EINVAL and "stream %d, config %d:" % (s, m) in str(e.value), str(e.value)
    assert np.array_equal(sw.counts(), counts)
    assert all(sw.snapshot(*k) == v for k, v in snaps.items())
