"""Sweep.run_score (fvad_sweep_run_score) on host-only sweeps: the shared
evaluator core (fvad_eval_core.h, its host instantiation) against the host
evaluator -- fvad.evaluate per lane on run's segments, fvad.aggregate per
config -- by the statistics' bits, the call's validation and what it leaves
behind, and k_sweep_score's resources from the compiler's remarks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sweep_score_util as ssu
import sweep_util as su


def host_sweep(fvad, **kw):
    kw.setdefault("bands", su.BANDS)
    return fvad.Sweep(kw.pop("n_streams", su.N_STREAMS), 2, device=-1, **kw)


@pytest.fixture(scope="module")
def host_lanes(fvad_mod):
    """sweep_util's 5 streams x 36 configs x 600 windows run on the host: the
    configs, every lane's segments in seconds, both label sets."""
    sw = host_sweep(fvad_mod)
    data = su.fill(sw)
    cfgs = su.grid(fvad_mod)
    sw.run(cfgs)
    lanes = ssu.lane_segments(sw, len(cfgs))
    return cfgs, lanes, {"plain": ssu.plain_labels(data), "adversarial": ssu.adversarial_labels(lanes, len(cfgs))}


def scored(fvad, cfgs, refs, stat, **kw):
    sw = host_sweep(fvad, **kw)
    su.fill(sw)
    return sw.run_score(cfgs, refs, stat=stat, single=True)


@pytest.mark.parametrize("which", ["plain", "adversarial"])
def test_run_score_matches_evaluator(fvad_mod, host_lanes, which):
    cfgs, lanes, labels = host_lanes
    exp = ssu.expected(fvad_mod, lanes, su.N_STREAMS, len(cfgs), labels[which], ssu.KW)
    ssu.assert_scores(fvad_mod, scored(fvad_mod, cfgs, labels[which], ssu.KW), exp)
    # without single=True: the aggregates alone
    sw = host_sweep(fvad_mod)
    su.fill(sw)
    agg = sw.run_score(cfgs, labels[which], stat=ssu.KW)
    for m in range(len(cfgs)):
        ssu.assert_bits(ssu.agg_vec(agg[m]), ssu.agg_vec(exp[0][m]), m)


def test_adversarial_labels_are_not_vacuous(fvad_mod, host_lanes):
    """On the expected values, so the oracle alone has to satisfy them: a lane
    with TP, FP and FN all positive, a lane whose score depends on fill_gaps, one
    whose score depends on extrude_end, a segment with two or more opponents."""
    cfgs, lanes, labels = host_lanes
    refs = labels["adversarial"]
    n = len(cfgs)
    _, base = ssu.expected(fvad_mod, lanes, su.N_STREAMS, n, refs, ssu.KW)
    assert any(d["true_positives_sec"] > 0 and d["false_positives_sec"] > 0 and d["false_negatives_sec"] > 0
               for row in base for d in row)
    def differing(x, y):  # lanes whose statistics differ by bits, NaN equal to NaN
        return sum(not ssu.same_bits(ssu.stat_vec(fvad_mod, a), ssu.stat_vec(fvad_mod, b))
                   for ra, rb in zip(x, y) for a, b in zip(ra, rb))

    _, again = ssu.expected(fvad_mod, lanes, su.N_STREAMS, n, refs, ssu.KW)
    assert any(np.isnan(ssu.stat_vec(fvad_mod, d)).any() for row in base for d in row)  # NaN lanes are in play
    assert differing(base, again) == 0  # the comparison itself: the same evaluation twice is equal
    for k in ("fill_gaps", "extrude_end"):
        _, other = ssu.expected(fvad_mod, lanes, su.N_STREAMS, n, refs, dict(ssu.KW, **{k: 0.0}))
        assert differing(base, other) > 0, k
    most = 0
    for (s, m), segs in lanes.items():
        r = np.asarray(refs[s], np.float32).reshape(-1, 2)
        for f, t in segs:
            most = max(most, int((np.minimum(t, r[:, 1]) - np.maximum(f, r[:, 0]) > 0).sum()))
    assert most >= 2, most
    # and the exact edge: a label ends where a segment starts, overlap 0
    assert any(np.float32(r[1]) == seg[0] for (s, m), segs in lanes.items() for seg in segs for r in refs[s])


@pytest.mark.parametrize("seg_capacity", [64, 41])
def test_many_short_overlapping_segments(fvad_mod, seg_capacity):
    """27 to 41 segments per lane; at seg_capacity 41 the busiest lane's row is exactly full."""
    sw, cfgs, refs = ssu.reactive_sweep(fvad_mod, device=-1, seg_capacity=seg_capacity)
    sw.run(cfgs)
    counts = sw.counts()
    lanes = ssu.lane_segments(sw, len(cfgs))
    assert counts.min() >= 20 and counts.max() == 41, counts
    pad = [a[1] > b[0] for segs in lanes.values() for a, b in zip(segs, segs[1:])]
    assert sum(pad) * 2 > len(pad)  # neighbours overlap through their padding
    exp = ssu.expected(fvad_mod, lanes, sw.B, len(cfgs), refs, ssu.KW)
    got = sw.run_score(cfgs, refs, stat=ssu.KW, single=True)
    ssu.assert_scores(fvad_mod, got, exp)
    assert np.array_equal(sw.counts(), counts)


def test_per_config_stat_configs(fvad_mod, host_lanes):
    cfgs, lanes, labels = host_lanes
    refs = labels["adversarial"]
    stats = [dict(ssu.KW, ignore_shorter_than_sec=0.05 * m) for m in range(len(cfgs))]
    exp = ssu.expected(fvad_mod, lanes, su.N_STREAMS, len(cfgs), refs, stats)
    ssu.assert_scores(fvad_mod, scored(fvad_mod, cfgs, refs, stats), exp)
    # they do differ: one stat config for all gives other scores somewhere
    one = ssu.expected(fvad_mod, lanes, su.N_STREAMS, len(cfgs), refs, stats[0])
    assert any(ssu.agg_vec(a).tobytes() != ssu.agg_vec(b).tobytes() for a, b in zip(exp[0], one[0]))
    sw = host_sweep(fvad_mod)
    su.fill(sw)
    sw.run(cfgs[:3])
    with pytest.raises(fvad_mod.FvadError) as e:
        sw.run_score(cfgs, refs, stat=stats[:-1])
    assert e.value.code == fvad_mod.EINVAL and sw.n_cfgs == 3
    assert sw.last_run()["kept_segments"] and ssu.secs(sw.segments(0, 0)[1]) == lanes[0, 0]


def test_validation_leaves_the_previous_run(fvad_mod, host_lanes):
    cfgs, lanes, labels = host_lanes
    sw = host_sweep(fvad_mod)
    su.fill(sw)
    sw.run(cfgs[:2])
    before = su.results(sw, 2)
    bad = fvad_mod.VadmConfig.default()
    bad.speech_min_freq = 500.0  # none of the sweep's bands
    with pytest.raises(fvad_mod.FvadError) as e:
        sw.run_score(cfgs[:3] + [bad], labels["plain"])
    assert e.value.code == fvad_mod.EINVAL and "config 3" in str(e.value)
    L = fvad_mod.lib()
    arr, n = sw._cfgs(cfgs)
    agg = (fvad_mod.AggregateStats * n)()
    sc = fvad_mod.StatConfig(0, 0, 0, 0)
    ptrs = (fvad_mod.F32P * sw.B)()  # all null
    lens = (C.c_size_t * sw.B)(*([0] * (sw.B - 1) + [2]))  # a null list with labels
    assert L.fvad_sweep_run_score(sw.h, arr, n, ptrs, lens, C.byref(sc), 1, agg, None) == fvad_mod.EINVAL
    zero = (C.c_size_t * sw.B)()
    for args in ((None, n, ptrs, zero, C.byref(sc), 1, agg), (arr, n, None, zero, C.byref(sc), 1, agg),
                 (arr, n, ptrs, None, C.byref(sc), 1, agg), (arr, n, ptrs, zero, None, 1, agg),
                 (arr, n, ptrs, zero, C.byref(sc), 1, None), (arr, n, ptrs, zero, C.byref(sc), 0, agg),
                 (arr, n, ptrs, zero, C.byref(sc), 2, agg)):
        assert L.fvad_sweep_run_score(sw.h, *args, None) == fvad_mod.EINVAL, args
    assert sw.last_run() == {"n_cfgs": 2, "kept_segments": True, "bytes_back": 0}
    su.assert_same(su.results(sw, 2), before)


def test_empty_streams(fvad_mod):
    """A stream with labels and no windows has false negatives only; a stream
    with neither has NaN rates, as the host evaluator gives them."""
    cfgs = su.grid(fvad_mod)[:4]
    sw = host_sweep(fvad_mod, n_streams=3)
    su.fill(sw, streams=[0])
    refs = [su.labels(0, su.stream_len(0)), [(1.0, 2.5), (0.2, 0.4)], []]
    agg, single = sw.run_score(cfgs, refs, stat=ssu.KW, single=True)
    lanes = {(s, m): [] for s in (1, 2) for m in range(4)}
    sw.run(cfgs)
    lanes.update({(0, m): ssu.secs(sw.segments(0, m)[1]) for m in range(4)})
    ssu.assert_scores(fvad_mod, (agg, single), ssu.expected(fvad_mod, lanes, 3, 4, refs, ssu.KW))
    for m in range(4):
        only_fn, nothing = single[m][1], single[m][2]
        assert only_fn["false_negatives_sec"] == 1.5 and only_fn["total_positives_sec"] == 1.5
        assert only_fn["true_positives_sec"] == 0 and only_fn["false_positives_sec"] == 0
        assert only_fn["false_negative_rate"] == 1.0
        assert all(np.isnan(nothing[k]) for k in ("true_positive_rate", "false_negative_rate", "precision"))


def test_over_capacity_and_segments_not_kept(fvad_mod, host_lanes):
    cfgs, lanes, labels = host_lanes
    refs = labels["plain"]
    plain = host_sweep(fvad_mod, seg_capacity=1)
    su.fill(plain)
    plain.run(cfgs)
    counts = plain.counts()
    assert counts.max() > 1
    s, m = next((s, m) for s in range(su.N_STREAMS) for m in range(len(cfgs)) if counts[s, m] > 1)
    sw = host_sweep(fvad_mod, seg_capacity=1)
    su.fill(sw)
    with pytest.raises(fvad_mod.FvadError) as e:
        sw.run_score(cfgs, refs)
    assert e.value.code == fvad_mod.EINVAL and "stream %d, config %d:" % (s, m) in str(e.value), str(e.value)
    assert sw.n_cfgs == len(cfgs) and np.array_equal(sw.counts(), counts)
    assert sw.snapshot(s, m) == plain.snapshot(s, m)
    # a run that fits: the segments are not kept, score has nothing to score; a later run restores both
    sw = host_sweep(fvad_mod)
    su.fill(sw)
    sw.run(cfgs)
    before, score_before = su.results(sw, len(cfgs)), sw.score(refs, **ssu.KW)
    sw.run_score(cfgs, refs, stat=ssu.KW)
    assert not sw.last_run()["kept_segments"]
    with pytest.raises(fvad_mod.FvadError):  # a host run counts nothing, run_score's like run's
        sw.debug_counts()
    assert np.array_equal(sw.counts(), before[1])
    for (s, m), (total, segs, snap) in before[0].items():
        assert sw.segments(s, m) == (total, []) and sw.snapshot(s, m) == snap, (s, m)
    with pytest.raises(fvad_mod.FvadError) as e:
        sw.score(refs, **ssu.KW)
    assert e.value.code == fvad_mod.EINVAL and "kept no segments" in str(e.value)
    sw.run(cfgs)
    su.assert_same(su.results(sw, len(cfgs)), before)
    assert [bytes(a) for a in sw.score(refs, **ssu.KW)] == [bytes(a) for a in score_before]


def test_eval_core_against_the_evaluator(fvad_mod, tmp_path):
    """tests/eval_core_harness.cpp: fvad_eval_core.h's eval_lane, compiled as
    plain C++ (the kernel includes the same header), gives fvad_eval_stats'
    eleven statistics bit for bit (NaN for NaN) on 200 000 random cases --
    machine-like padded, overlapping segment lists; labels unsorted,
    overlapping, zero-length, with equal starts, touching a segment's edge
    exactly; every combination of the four stat-config fields zero or not --
    and reports a segment list whose starts decrease as not sorted, wherever
    the pair stands, while equal starts pass."""
    lib_dir = os.path.dirname(fvad_mod.LIB_PATH)
    csrc = os.path.join(os.path.dirname(lib_dir), "csrc")
    exe = tmp_path / "eval_core"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++20", "-Wno-unknown-pragmas", "-I", csrc,
                           os.path.join(os.path.dirname(os.path.abspath(__file__)), "eval_core_harness.cpp"),
                           "-o", str(exe), "-L", lib_dir, "-lfvad", "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 / 200000 mismatches" in out.stdout and "sortedness: 0 wrong" in out.stdout


def test_sweep_score_kernel_resources():
    """k_sweep_score compiles for gfx950 without scratch spills and within
    160 KB of LDS (it uses none)."""
    import test_kernel_resources as tkr
    if not os.path.exists(tkr.HIPCC):
        pytest.skip("hipcc not available")
    r = tkr.resources("fvad_sweep_score.hip")
    print(r)
    assert "k_sweep_score" in r, sorted(r)
    assert r["k_sweep_score"]["VGPRs_spill"] == 0 and r["k_sweep_score"]["LDS"] <= 160 * 1024, r
