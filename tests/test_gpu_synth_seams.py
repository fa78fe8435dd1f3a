"""The overlap-add seams of the ys rows (fvad_staged.h: ys_seam, ys_tail_kept).

k_synthw adds a frame's second half to the next frame's first half in
registers when its wave runs both, one after the other; the consumers
(k_olafb, k_ola and the synthesis-memory copies) add only at a seam: a stream's
first frame of a push (the state's synthesis memory) and the first slot of a
batch of 8 frames (the tail of the row before).  The shapes here put seams
wherever they can fall: batches that straddle streams and hold invalid slots,
streams with 0 or 1 tick in a push, the synthesis memory crossing pushes,
every channel count's tick/batch phase, both consumer kernels.  Every output
is compared for bit equality with the CPU oracle, which knows nothing of
pushes or batches.

fp16 / fp16_fused / f32_fast share these kernels; their own modules
(test_gpu_fp16.py, test_gpu_fused16.py, test_gpu_f32_fast.py) hold them to
their previous outputs.
"""
import numpy as np
import pytest

import parity_util as pu

pytestmark = pytest.mark.gpu

FRAME = 480


@pytest.fixture(scope="module")
def models(fvad_mod, oracle_mod):
    return fvad_mod.Model(seed=1), oracle_mod.Model(seed=1)


def _speech(fvad_mod, sid, ticks, ch):
    """ticks of synthetic stream sid from 1 s in (past its quiet start)."""
    x = fvad_mod.synth_stream(sid, 48000 + ticks * FRAME, ch)[0]
    return np.ascontiguousarray(x[:, 48000:])


def _oracle(oracle_mod, om, x, fft_size=2048):
    ch, n = x.shape
    frames = n // FRAME
    p = oracle_mod.Pipeline(ch, om, fft_size=fft_size, trace_frames=frames + 1, trace_windows=frames + 1,
                            trace_denoised=frames * FRAME)
    p.push([x[c] for c in range(ch)])
    fr, wi = p.trace()
    return {"frames": fr, "windows": wi, "denoised": p.tden[:, : frames * FRAME].copy()}


def _engine(eng, streams, schedule):
    """Push schedule[k][s] ticks of stream s in push k; per-stream outputs as parity_util.engine_run's."""
    B, ch = len(streams), streams[0].shape[0]
    T = max(max(row) for row in schedule)
    done = [0] * B
    per = [{k: [] for k in ("vad", "ratio", "win_flag", "win_ratio", "win_vad", "band", "denoised")} for _ in range(B)]
    for row in schedule:
        pcm = np.zeros((T, B, ch, FRAME), np.float32)
        for s, (x, v) in enumerate(zip(streams, row)):
            if v:
                seg = x[:, done[s] * FRAME:(done[s] + v) * FRAME].reshape(ch, v, FRAME)
                pcm[:v, s] = seg.transpose(1, 0, 2)
        o = eng.push(pcm, ticks_valid=np.asarray(row, np.int32), denoised=True)
        for s, v in enumerate(row):
            cnt = o["win_flag"][:v, s]
            r = per[s]
            r["vad"].append(o["vad"][:v, s])
            r["ratio"].append(o["ratio"][:v, s])
            r["win_flag"].append(cnt)
            for key in ("win_ratio", "win_vad", "band"):
                r[key].append(pu.tick_windows(o[key][:v, s], cnt, 1))
            r["denoised"].append(o["denoised"][:v, s])
            done[s] += v
    out = []
    for s, r in enumerate(per):
        assert done[s] * FRAME == streams[s].shape[1], s
        g = {k: np.concatenate(v) for k, v in r.items()}
        g["denoised"] = g["denoised"].transpose(1, 0, 2).reshape(ch, -1)
        out.append(g)
    return out


def _assert_equal(ref, got, ch):
    fr, wi = ref["frames"], ref["windows"]
    assert len(fr) == len(got["vad"])
    assert np.array_equal(ref["denoised"], got["denoised"]), pu.first_mismatch(ref["denoised"], got["denoised"])
    assert np.array_equal(fr["vad"], got["vad"]), pu.first_mismatch(fr["vad"], got["vad"])
    assert np.array_equal(fr["ratio"], got["ratio"]), pu.first_mismatch(fr["ratio"], got["ratio"])
    assert len(wi) == int(got["win_flag"].sum())
    assert np.array_equal(wi["ratio"], got["win_ratio"])
    assert np.array_equal(wi["vad"], got["win_vad"])
    assert np.array_equal(wi["band"][:, :ch], got["band"][:, :, 0])
    return len(wi)


def _check(fvad_mod, oracle_mod, models, streams, schedule, fft_size=2048, bands=((4, 64),)):
    m, om = models
    ch = streams[0].shape[0]
    max_ticks = max(max(row) for row in schedule)
    eng = fvad_mod.Engine(m, len(streams), ch, max_ticks=max_ticks, fft_size=fft_size, bands=bands,
                          want_denoised=True)
    assert getattr(eng, "wpt", 1) == 1
    got = _engine(eng, streams, schedule)
    n_win = 0
    for x, g in zip(streams, got):
        n_win += _assert_equal(_oracle(oracle_mod, om, x, fft_size), g, ch)
    assert n_win > 0  # the band sums were compared


def _streams(fvad_mod, schedule, ch, ids=(3, 21, 44)):
    totals = [sum(row[s] for row in schedule) for s in range(len(schedule[0]))]
    return [_speech(fvad_mod, sid, t, ch) for sid, t in zip(ids, totals)]


# three pushes of up to 5 ticks: every stream has a full, a short and a 0- or
# 1-tick push; with V = 5 C frame slots per stream, batches of 8 straddle the
# streams and hold the invalid slots of the short ones
SCHED5 = [[5, 0, 3], [1, 5, 4], [4, 1, 5]]
SCHED7 = [[7, 3, 1], [0, 7, 5], [2, 1, 7]]


def test_straddling_batches(fvad_mod, oracle_mod, models):
    """3 streams x 2 ch, max_ticks 5 (V = 10): batches straddle streams, f % 8
    seams fall mid-stream, and the synthesis memory crosses three ragged pushes."""
    _check(fvad_mod, oracle_mod, models, _streams(fvad_mod, SCHED5, 2), SCHED5)


@pytest.mark.parametrize("ch", [1, 3])
def test_other_channel_counts(fvad_mod, oracle_mod, models, ch):
    """max_ticks 7: V = 7 (mono: a batch holds more than a stream) and V = 21."""
    _check(fvad_mod, oracle_mod, models, _streams(fvad_mod, SCHED7, ch), SCHED7)


def test_every_frame_a_seam(fvad_mod, oracle_mod, models):
    """1 stream x 1 ch, one tick per push, 10 pushes: every frame has v == 0."""
    sched = [[1]] * 10
    _check(fvad_mod, oracle_mod, models, _streams(fvad_mod, sched, 1), sched)


@pytest.mark.parametrize("ch,fft_size,bins", [(2, 512, (1, 16)), (5, 2048, (4, 64))])
def test_k_ola_paths(fvad_mod, oracle_mod, models, ch, fft_size, bins):
    """fft_size 512, and 5 channels: k_ola + k_winmeta + k_fftb(w) instead of
    k_olafb, on the straddling shapes."""
    _check(fvad_mod, oracle_mod, models, _streams(fvad_mod, SCHED5, ch), SCHED5, fft_size, (bins,))


def test_silence(fvad_mod, oracle_mod, models):
    """A stream of digital silence beside a speech stream with a silent gap:
    silent frames pass X through, on the same carry and add path."""
    sched = [[5, 3], [2, 5], [5, 1], [4, 5]]
    a, b = _streams(fvad_mod, sched, 2)
    a[:] = 0
    b[:, 4 * FRAME:7 * FRAME] = 0
    _check(fvad_mod, oracle_mod, models, [a, b], sched)


def test_staged_equals_fused(fvad_mod, models):
    """16 stereo streams x 24 ticks, two resident pushes: staged and fused
    give the same outputs, denoised samples included."""
    m, _ = models
    outs = []
    for mode in ("staged", "fused"):
        eng = fvad_mod.Engine(m, 16, 2, max_ticks=24, want_denoised=True, mode=mode)
        eng.load_synthetic(24, 11)
        res = []
        for _ in range(2):
            eng.run_resident(24)
            eng.sync()
            res.append(eng.fetch(24, denoised=True))
        outs.append(res)
    for a, b in zip(*outs):
        for k in ("denoised", "vad", "ratio", "win_flag", "win_ratio", "win_vad"):
            assert np.array_equal(a[k], b[k]), (k, pu.first_mismatch(a[k], b[k]))
        wf = a["win_flag"].astype(bool)
        assert wf.sum() > 0 and np.array_equal(a["band"][wf], b["band"][wf])
