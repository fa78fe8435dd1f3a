"""Per-stream input rates in one engine (input_rate = FVAD_INPUT_RATE_PER_STREAM;
k_resample_ps, csrc/fvad_resample.hip).

The oracle is the host mirror fvad_resample_host run per stream at the stream's
own rate (tests/test_resample_cpu.py holds it to an f64 computation); a 48000
stream's mirror is its samples.  The 48 kHz device input of a per-stream engine
(fetch_input) equals the mirror over each row's valid ticks by the bits and is
zeros past them, and everything behind it equals a 48 kHz engine pushed the
mirror's rows.  The slots past a stream's ticks_valid hold noise."""
import numpy as np
import pytest

import parity_util as pu
from test_gpu_resample import KEYS, bits, outputs_equal, valid_equal

pytestmark = pytest.mark.gpu

FRAME = 480
ALL = (8000, 16000, 24000, 32000, 44100, 48000, 96000)
EINVAL, EFORMAT, ERATE = -1, -5, -6
# 7 streams, max_ticks 4: a stream that skips a push, tails taken from a single
# tick (push 1: streams 0 and 6), short pushes (1 and 3), every stream full (2)
TV7 = ([4, 2, 0, 3, 4, 1, 4], [1, 0, 3, 2, 0, 2, 1], [4, 4, 4, 4, 4, 4, 4], [2, 1, 1, 0, 2, 1, 2], [2, 4, 2, 1, 3, 1, 2])
NT7 = (4, 3, 4, 2, 4)


@pytest.fixture(scope="module")
def model(fvad_mod):
    return fvad_mod.Model(seed=1)


def desc(fvad, rate):
    """(frame_in, K - 1) of a stream's rate: 48000 has no filter"""
    if rate == 48000:
        return FRAME, 0
    d = fvad.resample_info(rate)
    return d["frame_in"], d["taps_per_phase"] - 1


def source(rate, C, ticks, seed):
    """[C][ticks * rate / 100] float32 whose values are exact 16-bit samples k / 32768, and the k"""
    rng = np.random.default_rng(7919 * seed + rate // 100)
    t = np.arange(ticks * (rate // 100), dtype=np.float64)
    x = 0.25 * rng.uniform(-1.0, 1.0, (C, t.size))
    for c in range(C):
        x[c] += 0.4 * np.sin(2.0 * np.pi * (310.0 + 97.0 * (seed % 11) + 41.0 * c) * t / rate)
    k = np.round(x * 32768.0).astype(np.int16)
    return k.astype(np.float32) * np.float32(1.0 / 32768.0), k


class Feed:
    """Streams of their own rates: cuts each source into its rows of a push by
    ticks_valid and keeps the mirror -- each row's tail and the 48 kHz push."""

    def __init__(self, fvad, rates, C, ticks, seed=0):
        self.fvad, self.C, self.B, self.ticks = fvad, C, len(rates), ticks
        self.rates, self.src, self.pos, self.tail = [None] * self.B, [None] * self.B, [0] * self.B, [None] * self.B
        self.noise = np.random.default_rng(5 + seed)
        for s, r in enumerate(rates):
            self.set_rate(s, r, 100 * seed + s)

    def set_rate(self, s, rate, seed):
        """stream s continues at `rate` with a new source and a zero tail"""
        self.rates[s] = rate
        self.src[s] = source(rate, self.C, self.ticks, seed)
        self.pos[s] = 0
        self.tail[s] = np.zeros((self.C, desc(self.fvad, rate)[1]), np.float32)

    def reset(self, streams):
        for s in streams:
            self.tail[s][:] = 0.0

    def push(self, nt, valid):
        """(rows f32, rows int16 -- one [nt][C][n_in] array per stream --, the mirror's 48 kHz push)"""
        rows, rows16 = [], []
        pcm48 = np.zeros((nt, self.B, self.C, FRAME), np.float32)
        for s, rate in enumerate(self.rates):
            n_in = rate // 100
            k = self.noise.integers(-20000, 20000, (nt, self.C, n_in)).astype(np.int16)
            v, a = int(valid[s]), self.pos[s] * n_in
            x16 = self.src[s][1][:, a:a + v * n_in]
            assert x16.shape[1] == v * n_in, "source too short"
            k[:v] = x16.reshape(self.C, v, n_in).transpose(1, 0, 2)
            if v:
                for c in range(self.C):
                    x = np.ascontiguousarray(self.src[s][0][c, a:a + v * n_in])
                    if rate == 48000:
                        pcm48[:v, s, c] = x.reshape(v, FRAME)
                    else:
                        tail = self.tail[s][c].copy()
                        pcm48[:v, s, c] = self.fvad.resample_host(rate, x, tail).reshape(v, FRAME)
                        self.tail[s][c] = tail
            self.pos[s] += v
            rows16.append(k)
            rows.append(k.astype(np.float32) * np.float32(1.0 / 32768.0))
        return rows, rows16, pcm48


def make(fvad, model, rates, C, max_ticks, rate_max=None, **kw):
    eng = fvad.Engine(model, len(rates), C, max_ticks=max_ticks, input_rate="per_stream",
                      input_rate_max=rate_max or max(rates), **kw)
    assert eng.stream_rates() == [rate_max or max(rates)] * len(rates)  # every stream starts at the max
    eng.set_stream_rates(range(len(rates)), rates)
    assert eng.stream_rates() == list(rates)
    assert np.array_equal(eng.input_layout(), fvad.input_layout(rates, C))
    return eng


def check_input(eng, nt, pcm48, tv, what):
    got = eng.fetch_input(nt)
    valid_equal(got, pcm48, tv, what)
    for s, v in enumerate(tv):
        assert not got[v:, s].any(), (what, "past ticks_valid", s)


# ---------------------------------------------------------------------------
# 1, 2. kernel = mirror
# ---------------------------------------------------------------------------
def run_kernel_vs_mirror(fvad, model, rates, C, tvs, nts, max_ticks, i16, seed=0):
    feed = Feed(fvad, rates, C, sum(nts) + 1, seed)
    eng = make(fvad, model, rates, C, max_ticks)
    for p, (tv, nt) in enumerate(zip(tvs, nts)):
        rows, rows16, pcm48 = feed.push(nt, tv)
        if i16:
            eng.submit_i16(eng.pack_input(rows16), ticks_valid=tv)
            eng.collect(want=False)
        else:
            eng.push(eng.pack_input(rows), ticks_valid=tv)
        check_input(eng, nt, pcm48, tv, (tuple(rates), "i16" if i16 else "f32", "push", p))


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
def test_kernel_equals_mirror_every_rate(fvad_mod, model, i16):
    run_kernel_vs_mirror(fvad_mod, model, ALL, 2, TV7, NT7, 4, i16)


SHAPES = {
    "1x1": ([44100], 1),
    # rates repeated and interleaved: no rate's list is contiguous, the offsets are uneven
    "9x8": ([8000, 44100, 8000, 48000, 16000, 44100, 96000, 8000, 48000], 8),
    "65x1": ([16000] * 64 + [96000], 1),
}


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_kernel_equals_mirror_other_shapes(fvad_mod, model, shape, i16):
    rates, C = SHAPES[shape]
    rng = np.random.default_rng(len(rates))
    tvs = [list(rng.integers(0, 5, len(rates))) for _ in range(2)] + [[4] * len(rates)]
    run_kernel_vs_mirror(fvad_mod, model, rates, C, tvs, (4, 4, 4), 4, i16, seed=1)


# ---------------------------------------------------------------------------
# 3. identical rates = the fixed-rate engine
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["staged", "f32_fast"])
def test_identical_rates_equal_fixed_rate_engine(fvad_mod, model, mode):
    rates, C = [16000] * 3, 2
    feed = Feed(fvad_mod, rates, C, 21, seed=2)
    eng = make(fvad_mod, model, rates, C, 4, want_denoised=True, mode=mode)
    ref = fvad_mod.Engine(model, 3, C, max_ticks=4, want_denoised=True, mode=mode, input_rate=16000)
    keys = KEYS + ("denoised",)
    for p, tv in enumerate(TV7):
        tv = tv[:3]
        rows, _, _ = feed.push(4, tv)
        packed = eng.pack_input(rows)
        o = eng.push(packed, ticks_valid=tv, denoised=True)
        r = ref.push(packed.reshape(4, 3, C, 160), ticks_valid=tv, denoised=True)  # (one layout when the rates agree)
        outputs_equal(o, r, tv, (mode, p), keys)
        assert np.array_equal(bits(eng.fetch_input(4)), bits(ref.fetch_input(4))), (mode, p)


# ---------------------------------------------------------------------------
# 4. end to end: outputs, machines, events and clips of a 48 kHz engine pushed the mirror's rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["submit", "push"])
def test_end_to_end(fvad_mod, model, how):
    import test_gpu_capture as tc
    rates, T = [16000, 48000, 8000], 100
    streams, _ = pu.make_streams(fvad_mod, [0, 1, 0], tc.SECS)
    n_push = int(tc.SECS * 100) // T
    feed = Feed(fvad_mod, rates, 2, 1)
    for s, r in enumerate(rates):  # every 48000 / r-th sample: a signal at r, as exact 16-bit samples
        k = np.round(np.ascontiguousarray(streams[s][:, ::48000 // r]) * 32768.0).clip(-32768, 32767).astype(np.int16)
        feed.src[s] = (k.astype(np.float32) * np.float32(1.0 / 32768.0), k)

    def engine(**kw):
        e = fvad_mod.Engine(model, 3, 2, max_ticks=T, bands=tc.BANDS, want_denoised=True, **kw)
        e.attach_vadm(tc.make_cfgs(fvad_mod))
        e.enable_events()
        e.enable_capture(0, tc.HIST, tc.POOL)
        return e

    eng, ref = engine(input_rate="per_stream", input_rate_max=48000), engine()
    eng.set_stream_rates([0, 2], [16000, 8000])
    keys = KEYS + ("denoised",)
    ev, clips, outs = ([], []), ([], []), ([], [])
    tv = [T] * 3

    def after(i, e, o):
        outs[i].append(o)
        ev[i].extend(e.poll_events()[0])
        clips[i].extend(e.poll_clips())

    pending = 0
    for p in range(n_push):
        rows, _, pcm48 = feed.push(T, tv)
        for i, (e, pcm) in enumerate(((eng, eng.pack_input(rows)), (ref, pcm48))):
            if how == "push":
                after(i, e, e.push(pcm, denoised=True))
            else:  # two pushes in flight
                e.submit(pcm)
                if p >= 1:
                    after(i, e, e.collect(denoised=True))
    if how == "submit":
        for i, e in enumerate((eng, ref)):
            after(i, e, e.collect(denoised=True))
    for i, e in enumerate((eng, ref)):
        e.sync()
        e.capture_flush()
        ev[i].extend(tc.drain_events(e))
        clips[i].extend(e.poll_clips())
        assert e.capture_lost() == 0
    assert len(outs[0]) == len(outs[1]) == n_push
    for p in range(n_push):
        outputs_equal(outs[0][p], outs[1][p], tv, (how, p), keys)
    assert ev[0] == ev[1]
    assert len(clips[0]) == len(clips[1])
    for (d0, a0), (d1, a1) in zip(*clips):
        assert d0 == d1
        assert np.array_equal(bits(a0), bits(a1))
    for s in range(3):
        for m in range(2):
            assert eng.segments(s, m) == ref.segments(s, m)
            assert eng.vadm_snapshot(s, m) == ref.vadm_snapshot(s, m)
    # the equality is not empty
    assert sum(len(ref.segments(s, 0)) for s in range(3)) >= 1
    assert any(d["n_samples"] > 0 for d, _ in clips[1])


# ---------------------------------------------------------------------------
# 5. a rate change between two pushes in flight
# ---------------------------------------------------------------------------
def test_rate_change_between_pushes_without_a_wait(fvad_mod, model):
    rates, C = [8000, 16000, 48000, 44100], 2
    feed = Feed(fvad_mod, rates, C, 13, seed=3)
    eng = make(fvad_mod, model, rates, C, 4, rate_max=48000)
    tv0, tvA, tvB = [4, 3, 4, 2], [4, 4, 2, 3], [3, 4, 4, 4]
    rows, _, pcm48 = feed.push(4, tv0)  # (tails that are not zeros)
    eng.push(eng.pack_input(rows), ticks_valid=tv0)
    check_input(eng, 4, pcm48, tv0, "before")
    rowsA, _, wantA = feed.push(4, tvA)
    eng.submit(eng.pack_input(rowsA), ticks_valid=tvA)
    eng.set_stream_rates([0, 2], [16000, 44100])
    feed.set_rate(0, 16000, 50)
    feed.set_rate(2, 44100, 51)
    # the new state right after the call, push A still in flight
    assert eng.stream_rates() == [16000, 16000, 44100, 44100]
    assert np.array_equal(eng.input_layout(), fvad_mod.input_layout([16000, 16000, 44100, 44100], C))
    rowsB, _, wantB = feed.push(4, tvB)
    eng.submit(eng.pack_input(rowsB), ticks_valid=tvB)
    # A was resampled at the old rates: its 48000 stream's rows are its samples, through the outputs' eyes
    ref = fvad_mod.Engine(model, 4, C, max_ticks=4)
    ref.push(pcm48, ticks_valid=tv0)
    ra, rb = ref.push(wantA, ticks_valid=tvA), ref.push(wantB, ticks_valid=tvB)
    outputs_equal(eng.collect(), ra, tvA, "A")
    # B: the listed streams from a zero tail at the new rate, the others with their tails unbroken
    # (stream 0's ratio and vad continue the 48 kHz pipeline's state: only the resampler restarted)
    outputs_equal(eng.collect(), rb, tvB, "B")
    check_input(eng, 4, wantB, tvB, "B's input")
    # the restart is visible: stream 3 (unlisted, 44100) differs from a zero-tail run of the same rows
    x = np.ascontiguousarray(rowsB[3][:tvB[3], 0].reshape(-1))
    assert not np.array_equal(fvad_mod.resample_host(44100, x).reshape(-1, FRAME)[0], wantB[0, 3, 0])


def test_same_rate_restarts_the_history(fvad_mod, model):
    rates, C = [16000, 8000], 1
    feed = Feed(fvad_mod, rates, C, 9, seed=4)
    eng = make(fvad_mod, model, rates, C, 4)
    rows, _, pcm48 = feed.push(4, [4, 4])
    eng.push(eng.pack_input(rows))
    eng.set_stream_rates([1], [8000])  # also when the rate did not change
    feed.reset([1])
    rows, _, pcm48 = feed.push(4, [4, 4])
    eng.push(eng.pack_input(rows))
    check_input(eng, 4, pcm48, [4, 4], "after set_stream_rates at the same rate")


# ---------------------------------------------------------------------------
# 6. reset and blobs
# ---------------------------------------------------------------------------
def test_reset_streams_and_reset_keep_the_rates(fvad_mod, model):
    rates, C = [8000, 44100, 48000, 96000], 2
    feed = Feed(fvad_mod, rates, C, 13, seed=5)
    eng = make(fvad_mod, model, rates, C, 4)
    layout = eng.input_layout()
    rows, _, pcm48 = feed.push(4, [4, 4, 4, 3])
    eng.push(eng.pack_input(rows), ticks_valid=[4, 4, 4, 3])
    eng.reset_streams([1, 3])
    feed.reset([1, 3])
    assert eng.stream_rates() == rates and np.array_equal(eng.input_layout(), layout)
    rows, _, pcm48 = feed.push(4, [4, 2, 4, 4])
    eng.push(eng.pack_input(rows), ticks_valid=[4, 2, 4, 4])
    check_input(eng, 4, pcm48, [4, 2, 4, 4], "after reset_streams")  # (stream 0's tail was kept: it equals the mirror's)
    eng.reset()
    feed.reset(range(4))
    assert eng.stream_rates() == rates
    rows, _, pcm48 = feed.push(4, [4, 4, 4, 4])
    eng.push(eng.pack_input(rows))
    check_input(eng, 4, pcm48, [4, 4, 4, 4], "after reset")


def test_save_restore_moves_rates_and_tails(fvad_mod, model):
    C, keys = 2, KEYS + ("denoised",)
    ratesA = [8000, 44100, 48000, 16000]
    feed = Feed(fvad_mod, ratesA, C, 13, seed=6)
    A = make(fvad_mod, model, ratesA, C, 4, rate_max=48000, want_denoised=True)
    for tv in ([4, 3, 4, 2], [2, 4, 1, 4]):
        rows, _, _ = feed.push(4, tv)
        A.push(A.pack_input(rows), ticks_valid=tv)
    blob = A.save_streams([0, 1, 2])
    info = fvad_mod.stream_blob_info(blob)
    assert info["count"] == 3
    assert int(np.frombuffer(blob.tobytes()[76:80], np.uint32)[0]) == 0xFFFFFFFF
    # the target: another n_streams, max_ticks and input_rate_max; other slots
    Bn = make(fvad_mod, model, [16000] * 6, C, 6, rate_max=96000, want_denoised=True)
    Bn.restore_streams([5, 0, 3], blob)
    ratesB = [44100, 16000, 16000, 48000, 16000, 8000]
    assert Bn.stream_rates() == ratesB
    assert np.array_equal(Bn.input_layout(), fvad_mod.input_layout(ratesB, C))
    tv = [4, 3, 4, 4]
    rows, _, pcm48 = feed.push(4, tv)
    oa = A.push(A.pack_input(rows), ticks_valid=tv, denoised=True)
    ia = A.fetch_input(4)
    quiet = [np.zeros((4, C, 160), np.float32)] * 6
    rowsB = list(quiet)
    rowsB[5], rowsB[0], rowsB[3] = rows[0], rows[1], rows[2]
    ob = Bn.push(Bn.pack_input(rowsB), ticks_valid=[tv[1], 0, 0, tv[2], 0, tv[0]], denoised=True)
    ib = Bn.fetch_input(4)
    for sa, sb in ((0, 5), (1, 0), (2, 3)):
        v = tv[sa]
        assert np.array_equal(bits(ia[:v, sa]), bits(pcm48[:v, sa])), sa
        assert np.array_equal(bits(ib[:v, sb]), bits(pcm48[:v, sa])), (sa, sb)
        for k in keys:
            assert np.array_equal(bits(oa[k][:v, sa]), bits(ob[k][:v, sb])), (k, sa)


def test_blob_refusals_leave_the_target_untouched(fvad_mod, model):
    C = 2
    big = make(fvad_mod, model, [96000, 8000], C, 4)
    feedb = Feed(fvad_mod, [96000, 8000], C, 9, seed=7)
    rows, _, _ = feedb.push(4, [4, 4])
    big.push(big.pack_input(rows))
    blob = big.save_streams([1, 0])  # record 1 is the 96000 stream
    fixed = fvad_mod.Engine(model, 2, C, max_ticks=4, input_rate=16000)
    plain = fvad_mod.Engine(model, 2, C, max_ticks=4)
    small = make(fvad_mod, model, [16000, 8000], C, 4, rate_max=16000)
    feeds = Feed(fvad_mod, [16000, 8000], C, 9, seed=8)
    rows, _, pcm48 = feeds.push(4, [4, 4])
    small.push(small.pack_input(rows))

    def refused(call):
        with pytest.raises(fvad_mod.FvadError) as ei:
            call()
        assert ei.value.code == EFORMAT, ei.value

    refused(lambda: small.restore_streams([0, 1], blob))          # record 1 above input_rate_max
    refused(lambda: small.restore_streams([1], blob, index=[1]))
    refused(lambda: fixed.restore_streams([0], blob))             # per-stream -> fixed rate
    refused(lambda: plain.restore_streams([0], blob))             # per-stream -> 48 kHz
    refused(lambda: small.restore_streams([0], fixed.save_streams([0])))  # fixed rate -> per-stream
    refused(lambda: small.restore_streams([0], plain.save_streams([0])))
    assert small.stream_rates() == [16000, 8000]
    rows, _, pcm48 = feeds.push(4, [4, 4])
    small.push(small.pack_input(rows))
    check_input(small, 4, pcm48, [4, 4], "after the refused restores")
    small.restore_streams([0], blob, index=[0])  # the 8000 record fits
    assert small.stream_rates() == [8000, 8000]


# ---------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------
def test_refusals(fvad_mod, model):
    rates, C = [8000, 16000, 16000], 2
    eng = make(fvad_mod, model, rates, C, 4, rate_max=32000)
    feed = Feed(fvad_mod, rates, C, 9, seed=9)

    def refused(code, call):
        with pytest.raises(fvad_mod.FvadError) as ei:
            call()
        assert ei.value.code == code, ei.value

    refused(ERATE, lambda: eng.set_stream_rates([0], [11025]))
    refused(ERATE, lambda: eng.set_stream_rates([0, 1], [8000, 44100]))  # above the max: nothing touched
    refused(ERATE, lambda: eng.set_stream_rates([0], [48000]))
    refused(EINVAL, lambda: eng.set_stream_rates([1, 1], [8000, 8000]))
    refused(EINVAL, lambda: eng.set_stream_rates([3], [8000]))
    refused(EINVAL, lambda: eng.set_stream_rates([-1], [8000]))
    eng.set_stream_rates([], [])  # a no-op
    assert eng.stream_rates() == rates
    assert fvad_mod.lib().fvad_engine_input_frame(eng.h) == EINVAL and eng.frame_in is None
    rows, _, pcm48 = feed.push(4, [4, 4, 4])
    packed = eng.pack_input(rows)
    refused(EINVAL, lambda: eng.push(packed, last_tick_samples=[80, 160, 80]))
    refused(EINVAL, lambda: eng.push(packed, last_tick_samples=[160, 160, 160]))
    refused(EINVAL, lambda: eng.load_synthetic(4))
    refused(EINVAL, lambda: eng.run_resident(4))
    eng.push(packed, last_tick_samples=[80, 160, 160])  # each stream's own frame: whole ticks
    check_input(eng, 4, pcm48, [4, 4, 4], "the push after the refusals")
    for kw in (dict(input_rate=16000), dict()):
        other = fvad_mod.Engine(model, 3, C, max_ticks=4, **kw)
        refused(EINVAL, lambda: other.set_stream_rates([0], [16000]))
        refused(EINVAL, lambda: other.stream_rates())
        refused(EINVAL, lambda: other.input_layout())
    for kw in (dict(input_rate=16000), dict(), dict(input_rate=48000)):  # input_rate_max without the marker
        refused(ERATE, lambda: fvad_mod.Engine(model, 3, C, max_ticks=4, input_rate_max=16000, **kw))
    refused(ERATE, lambda: fvad_mod.Engine(model, 3, C, max_ticks=4, input_rate="per_stream"))
    refused(ERATE, lambda: fvad_mod.Engine(model, 3, C, max_ticks=4, input_rate="per_stream", input_rate_max=22050))


# ---------------------------------------------------------------------------
# 8. nothing new where it is off
# ---------------------------------------------------------------------------
def test_other_engines_launch_what_they_did(fvad_mod, model):
    """The kernels of a push as kernel_times names them: a per-stream engine's
    resampling stands in front of the same pipeline, and the fixed-rate and the
    48 kHz engine report the staged pipeline's names and count, no more."""
    names = {}
    for key, kw in (("plain", dict()), ("fixed", dict(input_rate=16000)),
                    ("ps", dict(input_rate="per_stream", input_rate_max=16000))):
        e = fvad_mod.Engine(model, 2, 2, max_ticks=4, **kw)
        names[key] = list(e.kernel_times()["kernels"])
    assert names["plain"] and names["plain"] == names["fixed"] == names["ps"]
    assert not any("resample" in n for n in names["plain"])
