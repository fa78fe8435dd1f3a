"""Engine mode "f32_fast" (FVAD_MODE_F32_FAST): the staged pipeline with every
term of the GRU / dense sums a fused multiply-add (k_rnn3f in k_rnn3's place),
compared with the CPU oracle at the fp32 tolerance of SURVEY.md 8(c), not bit
for bit:

  per-frame vad          |d| <= 1e-4 (absolute)
  denoised PCM           rel-RMS <= 1e-5 per stream
  band sums (FFT B)      |d| / max|band| <= 1e-5 per stream
  frame / window counts, volume ratios, window ratios   bit-identical
  segments, Evaluator TP/FP/FN                          identical

Everything before the GRU stack (spectra, features, pitch analysis, volume
ratios), FFT B and the window bookkeeping run the exact kernels, so every
discrete decision before the GRU is the staged mode's.

Measured maxima on an MI355X (each test prints its own):

  test                 max |dvad|   denoised rel-RMS               band rel
  ragged               5.96e-08     1.17e-07                       2.20e-07
  channels 1 / 3 / 8   5.96e-08     1.03e-07 / 1.09e-07 / 1.10e-07 3.96e-07 / 1.92e-07 / 2.92e-07
  partial workgroup    5.96e-08     1.16e-07                       2.46e-07
  segments (8 x 60 s)  5.96e-08     (not kept)                     3.02e-07
  fft_size 1000        5.96e-08     (not kept)                     2.60e-07

Segment lists (3 or 4 per stream) and TP/FP/FN equal the oracle's on all eight streams.
"""
import concurrent.futures as cf

import numpy as np
import pytest

import parity_util as pu

pytestmark = pytest.mark.gpu

VAD_ABS = 1e-4
DEN_RELRMS = 1e-5
BAND_REL = 1e-5

FAST = ("k_rnn3f",)
EXACT = ("k_rnn3",)


@pytest.fixture(scope="module")
def models(fvad_mod, oracle_mod):
    return fvad_mod.Model(seed=1), oracle_mod.Model(seed=1)


def check_stream(ref, got, ch, tag, denoised=True):
    """The 8(c) fp32 bounds of one stream; returns (max |dvad|, denoised rel-RMS, band rel)."""
    fr = ref["frames"]
    assert len(fr) == len(got["vad"]), tag
    dv = float(np.abs(fr["vad"] - got["vad"]).max()) if len(fr) else 0.0
    assert np.array_equal(fr["ratio"], got["ratio"]), tag
    rel = 0.0
    if denoised:
        dr, dg = ref["denoised"], got["denoised"]
        rel = float(np.sqrt(np.mean((dr - dg) ** 2)) / max(1e-12, np.sqrt(np.mean(dr ** 2))))
    wi = ref["windows"]
    assert len(wi) == int(got["win_flag"].sum()), tag
    assert np.array_equal(wi["ratio"], got["win_ratio"]), tag
    b_ref, b_got = wi["band"][:, :ch], got["band"][:, :, 0]
    brel = float(np.abs(b_ref - b_got).max() / max(1e-12, np.abs(b_ref).max())) if len(wi) else 0.0
    print("  stream %s: |dvad| %.3g, denoised rel-RMS %.3g, band rel %.3g" % (tag, dv, rel, brel))
    assert dv <= VAD_ABS, (tag, dv)
    assert rel <= DEN_RELRMS, (tag, rel)
    assert brel <= BAND_REL, (tag, brel)
    return dv, rel, brel


def report(name, worst):
    print("f32_fast %s: max |dvad| %.3g, denoised rel-RMS %.3g, band rel %.3g" %
          ((name,) + tuple(max(w[k] for w in worst) for k in range(3))))


def oracle_parallel(oracle_mod, om, streams, denoised=True):
    oracle_mod.tables()
    with cf.ThreadPoolExecutor(max_workers=16) as ex:
        return list(ex.map(lambda x: pu.oracle_run(oracle_mod, om, [x], denoised=denoised)[0], streams))


def test_f32_fast_ragged_vs_oracle(fvad_mod, oracle_mod, models):
    """Ragged stereo streams (digital silence included: stream 19) in ragged
    pushes, the case the exact modes pass exactly."""
    m, om = models
    secs = [12.0, 9.99, 7.0, 2.5]
    ids = [0, 1, 19, 42]
    streams = [fvad_mod.synth_stream(i, int(48000 * s), 2)[0] for i, s in zip(ids, secs)]
    ref = oracle_parallel(oracle_mod, om, streams)
    eng = fvad_mod.Engine(m, len(streams), 2, max_ticks=37, want_denoised=True, mode="f32_fast")
    got = pu.engine_run(fvad_mod, eng, streams, 37)
    report("ragged", [check_stream(r, g, 2, i) for r, g, i in zip(ref, got, ids)])


@pytest.mark.parametrize("n_channels", [1, 3, 8])
def test_f32_fast_channels(fvad_mod, oracle_mod, models, n_channels):
    """1, 3 and 8 channels (the shared denoiser state runs a stream's channels in series)."""
    m, om = models
    secs = 3 if n_channels == 8 else 6
    streams = [fvad_mod.synth_stream(i, 48000 * secs, n_channels)[0] for i in (5, 6)]
    ref = oracle_parallel(oracle_mod, om, streams)
    eng = fvad_mod.Engine(m, 2, n_channels, max_ticks=50, want_denoised=True, mode="f32_fast")
    got = pu.engine_run(fvad_mod, eng, streams, 50)
    report("%d channels" % n_channels, [check_stream(r, g, n_channels, s) for r, g, s in zip(ref, got, (5, 6))])


def test_f32_fast_partial_workgroup(fvad_mod, oracle_mod, models):
    """11 streams: k_rnn3f owns 8 per workgroup, so one full workgroup plus 3; ragged lengths."""
    m, om = models
    ids = list(range(100, 111))
    secs = [3.0 + 0.07 * (i % 11) for i in range(len(ids))]
    streams = [fvad_mod.synth_stream(i, int(48000 * s), 2)[0] for i, s in zip(ids, secs)]
    ref = oracle_parallel(oracle_mod, om, streams)
    eng = fvad_mod.Engine(m, len(streams), 2, max_ticks=64, want_denoised=True, mode="f32_fast")
    got = pu.engine_run(fvad_mod, eng, streams, 64)
    report("partial workgroup", [check_stream(r, g, 2, i) for r, g, i in zip(ref, got, ids)])


def test_f32_fast_segments_and_evaluator(fvad_mod, oracle_mod, models):
    """Eight 60 s stereo streams (2 and 42 are the two a build with contraction
    everywhere moves far outside the bounds) with device VADMachines: segment
    lists and Evaluator TP/FP/FN (simulator.zig's settings) equal the oracle's,
    no exceptions; vad and bands within the bounds on the way."""
    m, om = models
    ids, secs, T = [0, 1, 2, 3, 4, 5, 19, 42], 60.0, 100
    pairs = [fvad_mod.synth_stream(i, int(48000 * secs), 2) for i in ids]
    streams, labels = [p[0] for p in pairs], [p[1] for p in pairs]
    ref = oracle_parallel(oracle_mod, om, streams, denoised=False)
    eng = fvad_mod.Engine(m, len(ids), 2, max_ticks=T, mode="f32_fast")
    eng.attach_vadm()
    got = pu.engine_run(fvad_mod, eng, streams, T, denoised=False)
    report("segments", [check_stream(r, g, 2, i, denoised=False) for r, g, i in zip(ref, got, ids)])
    to_sec = lambda segs: [(a / 48000.0, b / 48000.0) for a, b, _, _ in segs]
    cfg = dict(ignore_shorter_than_sec=0.7, extrude_start=5, extrude_end=10, fill_gaps=5)
    keys = ("true_positives_sec", "false_positives_sec", "false_negatives_sec")
    for s, i in enumerate(ids):
        a = [(x[0], x[1]) for x in eng.segments(s)]
        b = [(x[0], x[1]) for x in ref[s]["segments"]]
        assert a == b, (i, sorted(set(a) ^ set(b)))
        sg = fvad_mod.evaluate(to_sec(eng.segments(s)), labels[s], **cfg)
        so = oracle_mod.evaluate(to_sec(ref[s]["segments"]), labels[s], **cfg)
        assert [sg[k] for k in keys] == [so[k] for k in keys], (i, sg, so)
    print("f32_fast segments: %s segments per stream, all equal to the oracle's" %
          [len(r["segments"]) for r in ref])


def test_f32_fast_fft_size_1000_segments(fvad_mod, oracle_mod, models):
    """A non-default VAD.Config (fft_size 1000: the exact k_ola / k_winmeta /
    k_fftb tail, bands from FFT.freqToBin) with device VADMachines: vad and
    bands within the bounds, ratios exact, segment lists identical."""
    m, om = models
    fft_size = 1000
    step = np.float32(48000) / np.float32(fft_size)
    bins = tuple(int(np.floor(np.float32(f) / step + np.float32(0.5))) for f in (100.0, 1500.0))
    ids, secs = (0, 19), (20.0, 13.3)
    streams = [fvad_mod.synth_stream(i, int(48000 * s), 2)[0] for i, s in zip(ids, secs)]
    eng = fvad_mod.Engine(m, len(streams), 2, max_ticks=50, fft_size=fft_size, bands=(bins,), mode="f32_fast")
    eng.attach_vadm()
    got = pu.engine_run(fvad_mod, eng, streams, 50, denoised=False)
    worst = []
    for s, x in enumerate(streams):
        n = x.shape[1]
        p = oracle_mod.Pipeline(2, om, fft_size=fft_size, trace_frames=n // 480 + 1,
                                trace_windows=n // fft_size + 2)
        for k in range(0, n, 48000):
            p.push([x[0, k:k + 48000], x[1, k:k + 48000]])
        fr, wi = p.trace()
        assert len(wi) > 0
        worst.append(check_stream({"frames": fr, "windows": wi}, got[s], 2, ids[s], denoised=False))
        assert [(a, b) for a, b, _, _ in eng.segments(s)] == [(a, b) for a, b, _, _ in p.segments()]
    report("fft_size 1000", worst)


def test_f32_fast_kernel_names(fvad_mod, models):
    """kernel_times() of an f32_fast engine lists the fused multiply-add
    kernel and not its exact twin; a staged engine's list is unchanged."""
    m, _ = models
    fast = list(fvad_mod.Engine(m, 2, 2, max_ticks=10, mode="f32_fast").kernel_times()["kernels"])
    staged = list(fvad_mod.Engine(m, 2, 2, max_ticks=10).kernel_times()["kernels"])
    assert staged == ["k_prep3", "k_fftAw", "k_plpc", "k_pcorr", "k_select", "k_pspecw", "k_rnn3", "k_synthw",
                      "k_olafb"], staged
    assert fast == ["k_prep3", "k_fftAw", "k_plpc", "k_pcorr", "k_select", "k_pspecw", "k_rnn3f", "k_synthw",
                    "k_olafb"], fast
    for k in FAST:
        assert k in fast and k not in staged
    for k in EXACT:
        assert k in staged and k not in fast
    # fft_size 1000: the exact tail in the new mode
    tail = list(fvad_mod.Engine(m, 2, 2, max_ticks=10, fft_size=1000, bands=((2, 31),),
                                mode="f32_fast").kernel_times()["kernels"])
    assert tail[8:] == ["k_ola", "k_winmeta", "k_fftbw"], tail


def test_f32_fast_leaves_staged_exact(fvad_mod, oracle_mod, models):
    """A staged engine created before an f32_fast engine in the same process
    and run beside it is still bit-identical to the oracle."""
    m, om = models
    x = fvad_mod.synth_stream(0, 48000 * 3, 2)[0]
    ref = pu.oracle_run(oracle_mod, om, [x])[0]
    staged = fvad_mod.Engine(m, 1, 2, max_ticks=50, want_denoised=True)
    fast = fvad_mod.Engine(m, 1, 2, max_ticks=50, want_denoised=True, mode="f32_fast")
    outs = {"staged": [], "fast": []}
    for t0 in range(0, 300, 50):  # the two engines' pushes interleaved
        pcm = x[:, t0 * 480:(t0 + 50) * 480].reshape(2, 50, 480).transpose(1, 0, 2)[:, None]
        outs["staged"].append(staged.push(pcm, denoised=True))
        outs["fast"].append(fast.push(pcm, denoised=True))
    cat = lambda k, key: np.concatenate([o[key][:, 0] for o in outs[k]])
    flags = cat("staged", "win_flag").astype(bool)
    assert np.array_equal(ref["frames"]["vad"], cat("staged", "vad"))
    assert np.array_equal(ref["frames"]["ratio"], cat("staged", "ratio"))
    assert np.array_equal(ref["windows"]["band"][:, :2], cat("staged", "band")[flags][:, :, 0])
    assert np.array_equal(ref["denoised"], cat("staged", "denoised").transpose(1, 0, 2).reshape(2, -1))
    dv = float(np.abs(ref["frames"]["vad"] - cat("fast", "vad")).max())
    print("f32_fast beside staged: staged exact; f32_fast max |dvad| %.3g" % dv)
    assert dv <= VAD_ABS


def test_f32_fast_no_denoiser_is_staged(fvad_mod, models):
    """use_denoiser = 0: the mode is accepted and is the staged no-denoiser path, bit for bit."""
    m, _ = models
    streams = [fvad_mod.synth_stream(i, 48000 * 2, 2)[0] for i in (3, 4)]
    res = []
    for mode in ("staged", "f32_fast"):
        eng = fvad_mod.Engine(m, 2, 2, max_ticks=50, want_denoised=True, mode=mode, use_denoiser=False)
        res.append(pu.engine_run(fvad_mod, eng, streams, 50))
    for a, b in zip(*res):
        assert int(a["win_flag"].sum()) > 0
        for k in a:
            assert np.array_equal(a[k], b[k]), k
