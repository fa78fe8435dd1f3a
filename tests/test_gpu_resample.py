"""Input resampling on the GPU (fvad_engine_config.input_rate; k_resample,
csrc/fvad_resample.hip).

The oracle for the kernel is the host mirror fvad_resample_host, which
tests/test_resample_cpu.py holds to an independent f64 computation: the 48 kHz
device input of a resampling engine (fetch_input) equals the mirror run over
each row's valid ticks by the bits, and everything behind it equals a 48 kHz
engine of the same mode pushed the mirror's output.

Unless said otherwise an engine has 3 streams, 2 channels, max_ticks 4 and
pushes with ticks_valid TV: a stream that skips a push, a tail taken from a
single tick.  The input is random plus a sine; the slots past a stream's
ticks_valid hold noise, which nothing may read."""
import numpy as np
import pytest

import parity_util as pu

pytestmark = pytest.mark.gpu

FRAME = 480
RATES = (8000, 16000, 24000, 32000, 44100, 96000)
TV = ([4, 2, 0], [1, 0, 3], [4, 4, 4], [3, 4, 1], [2, 2, 2])
KEYS = ("vad", "ratio", "win_flag", "win_ratio", "win_vad", "band")
EINVAL, EFORMAT = -1, -5


@pytest.fixture(scope="module")
def model(fvad_mod):
    return fvad_mod.Model(seed=1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def source(fvad, rate, B, C, ticks, seed=0):
    """[B][C][ticks * frame_in] float32 whose values are exact 16-bit samples
    k / 32768, and the k as int16: the float and the 16-bit ingest see one signal."""
    n_in = fvad.resample_info(rate)["frame_in"]
    rng = np.random.default_rng(1000 * seed + rate // 100)
    t = np.arange(ticks * n_in, dtype=np.float64)
    x = 0.25 * rng.uniform(-1.0, 1.0, (B, C, t.size))
    for s in range(B):
        for c in range(C):
            x[s, c] += 0.4 * np.sin(2.0 * np.pi * (310.0 + 97.0 * s + 41.0 * c) * t / rate)
    k = np.round(x * 32768.0).astype(np.int16)
    return k.astype(np.float32) * np.float32(1.0 / 32768.0), k


class Feed:
    """Cuts a source into pushes [nt][B][C][frame_in] by ticks_valid and keeps
    the mirror: each row's tail, and the 48 kHz push the mirror makes of it."""

    def __init__(self, fvad, rate, src, src16=None):
        self.fvad, self.rate, self.src, self.src16 = fvad, rate, src, src16
        d = fvad.resample_info(rate)
        self.n_in, self.hist = d["frame_in"], d["taps_per_phase"] - 1
        self.B, self.C = src.shape[:2]
        self.pos = [0] * self.B
        self.tail = np.zeros((self.B, self.C, self.hist), np.float32)
        self.noise = np.random.default_rng(5)

    def reset(self, streams):
        for s in streams:
            self.tail[s] = 0.0

    def push(self, nt, valid):
        """(raw float push, raw int16 push or None, the mirror's 48 kHz push)"""
        n_in, B, C = self.n_in, self.B, self.C
        k = self.noise.integers(-20000, 20000, (nt, B, C, n_in)).astype(np.int16)
        raw = k.astype(np.float32) * np.float32(1.0 / 32768.0)
        raw16 = k if self.src16 is not None else None
        pcm48 = np.zeros((nt, B, C, FRAME), np.float32)
        for s in range(B):
            v = int(valid[s])
            a = self.pos[s] * n_in
            for c in range(C):
                x = self.src[s, c, a:a + v * n_in]
                raw[:v, s, c] = x.reshape(v, n_in)
                if raw16 is not None:
                    raw16[:v, s, c] = self.src16[s, c, a:a + v * n_in].reshape(v, n_in)
                if v:
                    tail = self.tail[s, c].copy()
                    pcm48[:v, s, c] = self.fvad.resample_host(self.rate, x, tail).reshape(v, FRAME)
                    self.tail[s, c] = tail
            self.pos[s] += v
        return raw, raw16, pcm48


def valid_equal(a, b, valid, what):
    for s, v in enumerate(valid):
        assert np.array_equal(bits(a[:v, s]), bits(b[:v, s])), (what, s, pu.first_mismatch(a[:v, s], b[:v, s]))


def outputs_equal(o, ref, valid, what, keys=KEYS):
    for k in keys:
        valid_equal(o[k].view(np.uint32), ref[k].view(np.uint32), valid, (what, k))


# ---------------------------------------------------------------------------
# 1. kernel = mirror
# ---------------------------------------------------------------------------
def run_kernel_vs_mirror(fvad, model, rate, B, C, tvs, max_ticks, i16):
    src, src16 = source(fvad, rate, B, C, sum(max(tv) for tv in tvs) + 1)
    feed = Feed(fvad, rate, src, src16 if i16 else None)
    eng = fvad.Engine(model, B, C, max_ticks=max_ticks, input_rate=rate)
    assert eng.frame_in == feed.n_in
    for p, tv in enumerate(tvs):
        nt = max_ticks if p % 2 == 0 else max(max(tv), 1)  # whole and shorter pushes
        raw, raw16, pcm48 = feed.push(nt, tv)
        if i16:
            eng.submit_i16(raw16, ticks_valid=tv)
            eng.collect(want=False)
        else:
            eng.push(raw, ticks_valid=tv)
        got = eng.fetch_input(nt)
        valid_equal(got, pcm48, tv, (rate, "i16" if i16 else "f32", "push", p))
        # (the slots past ticks_valid are written as zeros)
        for s, v in enumerate(tv):
            assert not got[v:, s].any()


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("rate", RATES)
def test_kernel_equals_mirror(fvad_mod, model, rate, i16):
    run_kernel_vs_mirror(fvad_mod, model, rate, 3, 2, TV[:3], 4, i16)


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("rate", [16000, 44100])
@pytest.mark.parametrize("B,C", [(1, 1), (65, 8)])
def test_kernel_equals_mirror_other_shapes(fvad_mod, model, rate, B, C, i16):
    rng = np.random.default_rng(B)
    tvs = [list(rng.integers(0, 5, B)) for _ in range(2)] + [[4] * B]
    run_kernel_vs_mirror(fvad_mod, model, rate, B, C, tvs, 4, i16)


# ---------------------------------------------------------------------------
# 2. end to end: the outputs of a 48 kHz engine pushed the mirror's output
# ---------------------------------------------------------------------------
MODES = {"staged": dict(mode="staged"), "fused": dict(mode="fused"), "fp16": dict(mode="fp16"),
         "f32_fast": dict(mode="f32_fast"), "nodenoise2048": dict(use_denoiser=False, fft_size=2048),
         "nodenoise512": dict(use_denoiser=False, fft_size=512, bands=((1, 16),))}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_end_to_end(fvad_mod, model, mode):
    kw = MODES[mode]
    den = kw.get("use_denoiser", True)
    keys = KEYS + (("denoised",) if den else ())
    for rate in (16000, 44100, 96000):
        src, _ = source(fvad_mod, rate, 3, 2, 20, seed=1)
        feed = Feed(fvad_mod, rate, src)
        eng = fvad_mod.Engine(model, 3, 2, max_ticks=4, want_denoised=den, input_rate=rate, **kw)
        ref = fvad_mod.Engine(model, 3, 2, max_ticks=4, want_denoised=den, **kw)
        assert ref.frame_in == FRAME
        for p, tv in enumerate(TV):
            raw, _, pcm48 = feed.push(4, tv)
            o = eng.push(raw, ticks_valid=tv, denoised=den)
            r = ref.push(pcm48, ticks_valid=tv, denoised=den)
            outputs_equal(o, r, tv, (mode, rate, p), keys)


# ---------------------------------------------------------------------------
# 3. machines, events, clips
# ---------------------------------------------------------------------------
def test_machines_events_clips(fvad_mod, model):
    import test_gpu_capture as tc
    rate, B, T = 16000, 2, 50
    streams, _ = pu.make_streams(fvad_mod, [0, 1], tc.SECS)
    x48 = np.stack(streams)                           # [B][2][n]
    src = np.ascontiguousarray(x48[:, :, ::3])        # every third sample: a 16 kHz signal
    n_push = int(tc.SECS * 100) // T
    feed = Feed(fvad_mod, rate, src)

    def make(**kw):
        e = fvad_mod.Engine(model, B, 2, max_ticks=T, bands=tc.BANDS, **kw)
        e.attach_vadm(tc.make_cfgs(fvad_mod))
        e.enable_events()
        e.enable_capture(0, tc.HIST, tc.POOL)
        return e

    eng, ref = make(input_rate=rate), make()
    ev, clips = ([], []), ([], [])
    for p in range(n_push):
        raw, _, pcm48 = feed.push(T, [T] * B)
        for i, (e, pcm) in enumerate(((eng, raw), (ref, pcm48))):
            e.push(pcm)
            ev[i].extend(e.poll_events()[0])
            clips[i].extend(e.poll_clips())
    for i, e in enumerate((eng, ref)):
        e.sync()
        e.capture_flush()
        ev[i].extend(tc.drain_events(e))
        clips[i].extend(e.poll_clips())
        assert e.capture_lost() == 0
    assert ev[0] == ev[1]
    assert len(clips[0]) == len(clips[1])
    for (d0, a0), (d1, a1) in zip(*clips):
        assert d0 == d1
        assert np.array_equal(bits(a0), bits(a1))
    for s in range(B):
        for m in range(2):
            assert eng.segments(s, m) == ref.segments(s, m)
            assert eng.vadm_snapshot(s, m) == ref.vadm_snapshot(s, m)
        # the equality is not empty
        assert len(ref.segments(s, 0)) >= 1
        assert any(d["stream"] == s and d["n_samples"] > 0 for d, _ in clips[1])


# ---------------------------------------------------------------------------
# 4. streaming ingest
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
def test_streaming_equals_synchronous(fvad_mod, model, i16):
    rate = 44100
    src, src16 = source(fvad_mod, rate, 3, 2, 13, seed=2)
    feed = Feed(fvad_mod, rate, src, src16)
    pushes = [feed.push(4, tv) for tv in TV[:3]]
    sync = fvad_mod.Engine(model, 3, 2, max_ticks=4, want_denoised=True, input_rate=rate)
    want = [sync.push(raw, ticks_valid=tv, denoised=True) for (raw, _, _), tv in zip(pushes, TV)]
    eng = fvad_mod.Engine(model, 3, 2, max_ticks=4, want_denoised=True, input_rate=rate)
    for (raw, raw16, _), tv in zip(pushes, TV):
        slot = eng.input_slot_i16() if i16 else eng.input_slot()
        assert slot.shape == (4, 3, 2, eng.frame_in) and eng.frame_in == 441
        slot[:] = raw16 if i16 else raw
        (eng.submit_i16 if i16 else eng.submit)(slot, ticks_valid=tv)
    for p, tv in enumerate(TV[:3]):
        outputs_equal(eng.collect(denoised=True), want[p], tv, ("collect", p), KEYS + ("denoised",))
    valid_equal(eng.fetch_input(4), pushes[2][2], TV[2], "the last push's input")


# ---------------------------------------------------------------------------
# 5. reset
# ---------------------------------------------------------------------------
def test_reset_streams_and_reset(fvad_mod, model):
    rate = 16000
    src, _ = source(fvad_mod, rate, 3, 2, 20, seed=3)
    keys = KEYS + ("denoised",)

    def run(action, first=0):
        """pushes first.. of TV's schedule on a new engine, `action` after the first of them"""
        feed = Feed(fvad_mod, rate, src)
        for tv in TV[:first]:  # (a fresh engine starts where the others are after `first` pushes)
            for s in range(3):
                feed.pos[s] += tv[s]
        eng = fvad_mod.Engine(model, 3, 2, max_ticks=4, want_denoised=True, input_rate=rate)
        out = []
        for p, tv in enumerate(TV[first:], first):
            raw, _, _ = feed.push(4, tv)
            o = eng.push(raw, ticks_valid=tv, denoised=True)
            o["input"] = eng.fetch_input(4)
            out.append(o)
            if p == first and action:
                action(eng)
        return out

    plain = run(None)
    fresh = run(None, first=1)
    one = run(lambda e: e.reset_streams([1]))
    every = run(lambda e: e.reset())
    for p in range(1, len(TV)):
        tv = TV[p]
        for k in keys + ("input",):
            for s in range(3):
                v = tv[s]
                want_one = fresh[p - 1] if s == 1 else plain[p]
                assert np.array_equal(bits(one[p][k][:v, s]), bits(want_one[k][:v, s])), ("reset_streams", p, k, s)
                assert np.array_equal(bits(every[p][k][:v, s]), bits(fresh[p - 1][k][:v, s])), ("reset", p, k, s)
    # the reset changed something: stream 1's first resampled tick after it
    p = next(p for p in range(1, len(TV)) if TV[p][1] > 0)
    assert not np.array_equal(one[p]["input"][0, 1], plain[p]["input"][0, 1])


# ---------------------------------------------------------------------------
# 6. save / restore
# ---------------------------------------------------------------------------
def test_save_restore_moves_the_tails(fvad_mod, model):
    rate = 16000
    src, _ = source(fvad_mod, rate, 3, 2, 20, seed=4)
    feed = Feed(fvad_mod, rate, src)
    keys = KEYS + ("denoised",)
    A = fvad_mod.Engine(model, 3, 2, max_ticks=4, want_denoised=True, input_rate=rate)
    for tv in TV[:2]:
        A.push(feed.push(4, tv)[0], ticks_valid=tv)
    blob = A.save_streams([0, 2])
    info = fvad_mod.stream_blob_info(blob)
    plain = fvad_mod.Engine(model, 3, 2, max_ticks=4, want_denoised=True)
    pinfo = fvad_mod.stream_blob_info(plain.save_streams([0]))
    assert set(info) == set(pinfo) and info["count"] == 2 and info["sample_rate"] == 48000
    assert int(np.frombuffer(blob.tobytes()[76:80], np.uint32)[0]) == 16000
    assert not np.frombuffer(blob.tobytes()[80:128], np.uint32).any()
    # a plain engine's blob is what it was: no machines, so state | C pending window parts
    words = pinfo["state_words"] + 2 * ((2048 - 1 + 3) & ~3)
    assert pinfo["stream_bytes"] == 4 * words and plain.save_streams([0]).size == 128 + 4 * words
    assert lib_save_size(fvad_mod, plain, 3) == 128 + 3 * 4 * words
    assert not np.frombuffer(plain.save_streams([0]).tobytes()[76:128], np.uint32).any()
    assert info["stream_bytes"] == 4 * (words + 2 * 48) and info["config_hash"] != pinfo["config_hash"]
    # refused by engines of another input rate, which stay as they were
    other = fvad_mod.Engine(model, 3, 2, max_ticks=4, want_denoised=True, input_rate=8000)
    for e in (plain, other):
        with pytest.raises(fvad_mod.FvadError) as ei:
            e.restore_streams([0, 1], blob)
        assert ei.value.code == EFORMAT
    src8, _ = source(fvad_mod, 8000, 3, 2, 5, seed=5)
    feed8 = Feed(fvad_mod, 8000, src8)
    raw8, _, pcm48 = feed8.push(4, [4, 4, 4])
    other.push(raw8)
    valid_equal(other.fetch_input(4), pcm48, [4, 4, 4], "the 8 kHz engine after the refused restore")
    # into other slots of an engine of another size
    Bn = fvad_mod.Engine(model, 5, 2, max_ticks=6, want_denoised=True, input_rate=rate)
    Bn.restore_streams([3, 1], blob)
    tv = TV[2]
    raw, _, pcm48 = feed.push(4, tv)
    oa = A.push(raw, ticks_valid=tv, denoised=True)
    ia = A.fetch_input(4)
    rawb = np.zeros((4, 5, 2, Bn.frame_in), np.float32)
    rawb[:, 3], rawb[:, 1] = raw[:, 0], raw[:, 2]
    ob = Bn.push(rawb, ticks_valid=[0, tv[2], 0, tv[0], 0], denoised=True)
    ib = Bn.fetch_input(4)
    for sa, sb in ((0, 3), (2, 1)):
        v = tv[sa]
        assert np.array_equal(bits(ia[:v, sa]), bits(ib[:v, sb])) and np.array_equal(bits(ia[:v, sa]), bits(pcm48[:v, sa]))
        for k in keys:
            assert np.array_equal(bits(oa[k][:v, sa]), bits(ob[k][:v, sb])), (k, sa)


def lib_save_size(fvad, eng, n):
    return fvad.lib().fvad_engine_save_size(eng.h, n)


# ---------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------
def test_refusals(fvad_mod, model):
    rate = 32000
    src, _ = source(fvad_mod, rate, 3, 2, 9, seed=6)
    for kw in (dict(), dict(use_denoiser=False)):
        feed = Feed(fvad_mod, rate, src)
        eng = fvad_mod.Engine(model, 3, 2, max_ticks=4, input_rate=rate, **kw)
        raw, _, pcm48 = feed.push(4, [4, 4, 4])
        for call in (lambda: eng.push(raw, last_tick_samples=[320, 100, 320]),
                     lambda: eng.push(raw, last_tick_samples=[480, 480, 480]),
                     lambda: eng.load_synthetic(4),
                     lambda: eng.run_resident(4)):
            with pytest.raises(fvad_mod.FvadError) as ei:
                call()
            assert ei.value.code == EINVAL
        eng.push(raw, last_tick_samples=[320, 320, 320])  # whole ticks
        valid_equal(eng.fetch_input(4), pcm48, [4, 4, 4], "the push after the refusals")
    plain = fvad_mod.Engine(model, 3, 2, max_ticks=4)
    with pytest.raises(fvad_mod.FvadError) as ei:
        plain.fetch_input(4)
    assert ei.value.code == EINVAL
    assert plain.frame_in == FRAME
