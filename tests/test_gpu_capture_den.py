"""Denoised clips at the output rate, float or 16-bit
(fvad_engine_enable_capture_ex / poll_clip_s16 / clip_rate, want_denoised = 2;
csrc/fvad_capture.hip's k_den_append and k_cap_copy_short) on the GPU.

Workload W of tests/test_gpu_capture.py: 8 stereo streams, 14 s, seven pushes
of 200 ticks, its make_cfgs and its Sim.

The expected audio of a DENOISED capture is not taken from the capture code: a
twin engine of the same mode and denoised_rate, with want_denoised = 1 and
without capture, is pushed the same input, and its returned denoised rows are
concatenated per stream (rows the existing suites hold to the oracle and to
the resampler's mirror).  SimR is tg.Sim over that array in clip-rate units:
a segment's bounds go through ceil(x L / M) in Python integers, the history is
floor(R * history_sec), positions and bases are the 48 kHz ones times L / M.
Every descriptor field is compared exactly and every sample by the bits."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import parity_util as pu
import test_gpu_capture as tg

pytestmark = pytest.mark.gpu

B, CH, T, NP, PUSH, SECS = tg.B, tg.CH, tg.T, tg.NP, tg.PUSH, tg.SECS
HEAD, TAIL, NOAUDIO = tg.HEAD, tg.TAIL, tg.NOAUDIO
EINVAL = -1
INPUT, DENOISED, F32, S16 = 0, 1, 0, 1


def lm(rate):
    g = math.gcd(48000, rate)
    return rate // g, 48000 // g


def to_rate(x, rate):
    """fvad_clip_range restated: ceil(x L / M)."""
    l, m = lm(rate)
    return -(-x * l // m)


class SimR(tg.Sim):
    """tg.Sim in samples of the clip rate.  pass_ / flush / drop still take the
    streams' 48 kHz counts and bases (multiples of 480, so the due test is the
    same in either unit); audio(s) -> [CH][n] at the clip rate."""

    def __init__(self, oracle, n_streams, audio, rate, source, fmt, history=tg.HIST, pool_cap=None):
        super().__init__(oracle, n_streams, audio, history, pool_cap)
        self.rate, self.frame = rate, rate // 100
        self.hist = int(np.floor(rate * history))
        self.reserved = 0 if (source, fmt) == (INPUT, F32) else rate | fmt << 32 | source << 40
        self.extra = dict(rate=rate, format=fmt, source=source) if self.reserved else {}

    def _cut(self, e, p, n_now):
        s = e["stream"]
        assert n_now % 480 == 0 and self.base[s] % 480 == 0
        now, base = n_now // 480 * self.frame, self.base[s] // 480 * self.frame
        a, b = to_rate(e["sample_from"], self.rate), to_rate(e["sample_to"], self.rate)
        lo = max(base, now - min(now, self.hist))
        first, end = max(a, lo), min(b, now)
        flags = (HEAD if a < lo else 0) | (TAIL if b > now else 0)
        n = max(0, end - first)
        if n == 0:
            flags |= NOAUDIO
            first = min(first, now)
        return dict(stream=s, seq=e["seq"], channel=-1, flags=flags, push=p, sample_from=e["sample_from"],
                    sample_to=e["sample_to"], first_sample=first, n_samples=n, reserved=self.reserved, **self.extra)


def finish(fvad, out, fmt):
    """The sim's list with the samples as the capture delivers them."""
    return [(d, fvad.pcm_f32_to_s16(a) if fmt == S16 else a) for d, a in out]


def assert_clips(got, want, what=""):
    for i, (g, e) in enumerate(zip(got, want)):
        assert g[0] == e[0], (what, i, g[0], e[0])
        assert g[1].dtype == e[1].dtype and g[1].shape == e[1].shape, (what, i, g[0], g[1].dtype, g[1].shape)
        assert g[1].tobytes() == e[1].tobytes(), (what, i, g[0], "samples differ")
    assert len(got) == len(want), (what, len(got), len(want))


def with_audio(clips):
    return [c for c, _ in clips if c["n_samples"]]


def engine(w, rate=0, mode="staged", den=True, n_streams=B):
    e = w.fvad.Engine(w.model, n_streams, CH, max_ticks=T, bands=tg.BANDS, mode=mode, want_denoised=den,
                      denoised_rate=rate)
    e.attach_vadm(tg.make_cfgs(w.fvad))
    e.enable_events()
    return e


def enable_ex(fvad, eng, source, fmt, history=tg.HIST, pool=tg.POOL, machine=0):
    """fvad_engine_enable_capture_ex itself (Engine.enable_capture takes the old call for INPUT / F32)."""
    c = fvad.CaptureConfig.default()
    c.machine, c.history_sec, c.pool_samples, c.source, c.format = machine, history, pool, source, fmt
    rc = fvad.lib().fvad_engine_enable_capture_ex(eng.h, C.byref(c))
    if rc == 0:
        eng._clip_s16 = fmt == S16
    return rc


def rows_of(outs, valid=None):
    """The pushes' denoised outputs [T][B][CH][n] -> per stream [CH][samples], valid ticks only."""
    nb = outs[0]["denoised"].shape[1]
    per = []
    for s in range(nb):
        parts = []
        for p, o in enumerate(outs):
            v = T if valid is None else int(valid[p][s])
            parts.append(o["denoised"][:v, s].transpose(1, 0, 2).reshape(CH, -1))
        per.append(np.ascontiguousarray(np.concatenate(parts, axis=1)))
    return per


@pytest.fixture(scope="module")
def world(fvad_mod, oracle_mod):
    fvad = fvad_mod
    model = fvad.Model(seed=1)
    streams, _ = pu.make_streams(fvad, list(range(B)), SECS)
    x = np.stack(streams)  # [B][CH][n]
    pcm = tg.split_pushes(x)
    for a in pcm:
        a.setflags(write=False)
    w = types.SimpleNamespace(fvad=fvad, oracle=oracle_mod, model=model, x=x, pcm=pcm, twins={})
    return w


def twin(w, rate, mode="staged"):
    """The twin of W's even pushes: (denoised rows per stream, outputs per push, events), computed once."""
    key = (rate, mode)
    if key not in w.twins:
        t = engine(w, rate, mode)
        outs = [t.push(a, denoised=True) for a in w.pcm]
        t.sync()
        events = tg.drain_events(t)
        den = rows_of(outs)
        for a in den:
            a.setflags(write=False)
        assert den[0].shape == (CH, NP * T * t.frame_out)
        w.twins[key] = (den, outs, events)
    return w.twins[key]


def expected(w, segs, den, rate, source, fmt, history=tg.HIST):
    """W's list: seven passes, then a flush of every stream.  (clips, how many before the flush)"""
    sim = SimR(w.oracle, B, lambda s: den[s], rate or 48000, source, fmt, history)
    counts = tg.even_counts()
    for p in range(NP):
        sim.pass_(p, segs, counts[p])
    k = len(sim.out)
    sim.flush(None, NP - 1, counts[-1])
    return finish(w.fvad, sim.out, fmt), k


def run_w(eng, pcm, poll_each=True):
    """Push W, poll [after every push and] after the sync, flush, poll.  (clips, before the flush, outputs)"""
    got, outs = [], []
    for a in pcm:
        outs.append(eng.push(a))
        if poll_each:
            got += eng.poll_clips()
    eng.sync()
    got += eng.poll_clips()
    k = len(got)
    eng.capture_flush()
    got += eng.poll_clips()
    return got, k, outs


@pytest.mark.parametrize("rate,fmt", [(0, F32), (16000, S16), (44100, F32), (8000, S16), (96000, S16)])
def test_rates_and_formats(world, rate, fmt):
    """A DENOISED capture at every kind of rate: none (the 48 kHz rows of d_den),
    a third and a sixth (rows of 160 and 80), 44.1 kHz (rows of 441: no row but
    every fourth is 16-byte aligned) and 96 kHz (rows of 960), f32 and s16."""
    w, fvad = world, world.fvad
    den, outs, events = twin(w, rate)
    eng = engine(w, rate)
    assert eng.clip_rate() == 0
    eng.enable_capture(0, tg.HIST, tg.POOL, source="denoised", fmt="s16" if fmt == S16 else "f32")
    R = rate or 48000
    assert eng.clip_rate() == R and eng.frame_out == R // 100
    got, k, mine = run_w(eng, w.pcm)
    assert all(tg.same_outputs(a, b) for a, b in zip(mine, outs))
    ev = tg.drain_events(eng)
    assert ev == events
    want, kw = expected(w, tg.seg0(ev), den, rate, DENOISED, fmt)
    print("rate %d: %s" % (R, [(c["stream"], c["seq"], c["push"], c["flags"], c["channel"], c["first_sample"],
                                c["n_samples"]) for c, _ in want]))
    assert len(with_audio(want)) >= 8
    assert any(c["flags"] & TAIL for c, _ in want) and any(c["flags"] == 0 for c, _ in want)
    assert_clips(got, want, "rate %d" % R)
    assert k == kw and eng.capture_lost() == 0
    for c, a in got:
        assert (c["rate"], c["format"], c["source"]) == (R, fmt, DENOISED)
        assert a.dtype == (np.int16 if fmt == S16 else np.float32)
        if not c["flags"]:  # a whole clip is fvad_clip_range of its segment
            assert (c["first_sample"], c["first_sample"] + c["n_samples"]) == \
                fvad.clip_range(R, c["sample_from"], c["sample_to"])
    if fmt == S16:  # not silence: the conversion saw real audio
        assert max(int(np.abs(a.astype(np.int32)).max()) for _, a in got if a.size) > 100


@pytest.mark.parametrize("history", [4.0, 4.001])
def test_44100_ring_wraps(world, history):
    """44.1 kHz with a short history: the ring (history + a push of 200 x 441
    samples) is passed more than twice in 14 s, delivered clips cross its end,
    and old samples are cut (HEAD_SHORT).  At 4 s the ring is a whole number of
    rows (600); at 4.001 s it is not (264 644 = 600 x 441 + 44), so rows
    straddle its end as well."""
    w, fvad = world, world.fvad
    rate = 44100
    den, _, events = twin(w, rate)
    eng = engine(w, rate)
    eng.enable_capture(0, history, tg.POOL, source="denoised", fmt="f32")
    got, k, _ = run_w(eng, w.pcm)
    ev = tg.drain_events(eng)
    assert ev == events
    want, _ = expected(w, tg.seg0(ev), den, rate, DENOISED, F32, history)
    H = (int(np.floor(rate * history)) + T * 441 + 3) & ~3
    assert (H % 441 != 0) == (history != 4.0) and NP * T * 441 > 2 * H
    aud = with_audio(want)
    assert len(aud) >= 8
    # (no reset: a stream's sample r sits at ring index r % H)
    assert any(c["first_sample"] // H != (c["first_sample"] + c["n_samples"] - 1) // H for c in aud)
    assert any(c["flags"] & HEAD for c in aud)
    assert_clips(got, want, "history %g" % history)
    assert eng.capture_lost() == 0


def test_ragged_pushes(world):
    """ticks_valid differs per stream and includes 0 (16 kHz, s16): stream 3
    gets no tick in push 2, stream 5 gets 137 of 200 in push 1.  The rows past
    ticks_valid -- zeros out of k_resample_out -- leave no trace in any clip."""
    w, fvad = world, world.fvad
    rate = 16000
    valid = np.full((NP, B), T, np.int32)
    valid[2, 3], valid[1, 5] = 0, 137
    at = np.zeros(B, np.int64)
    pushes, counts = [], []
    for p in range(NP):
        a = np.zeros((T, B, CH, 480), np.float32)
        for s in range(B):
            v = valid[p, s]
            a[:v, s] = w.x[s, :, at[s] * 480:(at[s] + v) * 480].reshape(CH, v, 480).transpose(1, 0, 2)
            at[s] += v
        pushes.append(a)
        counts.append([int(t) * 480 for t in at])
    t = engine(w, rate)
    outs = [t.push(a, ticks_valid=valid[p], denoised=True) for p, a in enumerate(pushes)]
    den = rows_of(outs, valid)
    eng = engine(w, rate)
    eng.enable_capture(0, tg.HIST, tg.POOL, source="denoised", fmt="s16")
    for p, a in enumerate(pushes):
        eng.push(a, ticks_valid=valid[p])
    eng.sync()
    got = eng.poll_clips()
    eng.capture_flush()
    got += eng.poll_clips()
    segs = tg.seg0(tg.drain_events(eng))
    sim = SimR(w.oracle, B, lambda s: den[s], rate, DENOISED, S16)
    for p in range(NP):
        sim.pass_(p, segs, counts[p])
    sim.flush(None, NP - 1, counts[-1])
    want = finish(fvad, sim.out, S16)
    assert len(with_audio(want)) >= 8
    assert any(c["stream"] == 3 and c["n_samples"] for c, _ in want)
    assert any(c["stream"] == 5 and c["n_samples"] for c, _ in want)
    assert_clips(got, want)
    assert eng.capture_lost() == 0


def test_device_only_rows(world):
    """want_denoised = 2 at 16 kHz s16: the clip list of the want_denoised = 1
    engine, every other output the twin's; a denoised array is refused by push
    (before anything runs: the refused push leaves no trace), by collect and by
    fetch; submit / collect work."""
    w, fvad = world, world.fvad
    rate = 16000
    den, outs, events = twin(w, rate)
    one = engine(w, rate)
    one.enable_capture(0, tg.HIST, tg.POOL, source="denoised", fmt="s16")
    ref, kref, _ = run_w(one, w.pcm, poll_each=False)
    dev = engine(w, rate, den="device")
    assert dev.cfg.want_denoised == 2
    dev.enable_capture(0, tg.HIST, tg.POOL, source="denoised", fmt="s16")
    assert dev.clip_rate() == rate
    mine = []
    for p in range(NP):
        if p == 1:
            with pytest.raises(fvad.FvadError):
                dev.push(w.pcm[p], denoised=True)
        dev.submit(w.pcm[p])
        if p == 3:
            with pytest.raises(fvad.FvadError):
                dev.collect(denoised=True)  # (the push stays to be collected)
        mine.append(dev.collect())
        if p == 2:
            with pytest.raises(fvad.FvadError):
                dev.fetch(T, denoised=True)
            assert tg.same_outputs(dev.fetch(T), outs[p])
    dev.sync()
    got = dev.poll_clips()
    assert len(got) == kref
    dev.capture_flush()
    got += dev.poll_clips()
    assert all(tg.same_outputs(a, b) for a, b in zip(mine, outs)) and len(mine) == NP
    ev = tg.drain_events(dev)
    assert ev == events
    assert len(with_audio(ref)) >= 8
    assert_clips(got, ref, "device-only against want_denoised = 1")
    want, _ = expected(w, tg.seg0(ev), den, rate, DENOISED, S16)
    assert_clips(got, want, "device-only against the twin")
    assert dev.capture_lost() == 0


def test_input_source_through_ex(world):
    """INPUT through fvad_engine_enable_capture_ex.  f32: enable_capture's list
    on the same run, reserved 0.  s16 with the 16-bit ingest: the clip's shorts
    are the pushed shorts."""
    w, fvad = world, world.fvad
    lists = []
    for ex in (False, True):
        eng = engine(w, den=False)
        if ex:
            assert enable_ex(fvad, eng, INPUT, F32) == 0
        else:
            eng.enable_capture(0, tg.HIST, tg.POOL)
        assert eng.clip_rate() == 48000
        got, k, _ = run_w(eng, w.pcm)
        lists.append((got, k, tg.seg0(tg.drain_events(eng))))
    (a, ka, ea), (b, kb, eb) = lists
    assert ea == eb and ka == kb and len(with_audio(a)) >= 8
    assert_clips(b, a, "_ex against enable_capture")
    assert all(c["reserved"] == 0 and "rate" not in c and s.dtype == np.float32 for c, s in b)
    sim = tg.Sim(w.oracle, B, lambda s: w.x[s])
    for p in range(NP):
        sim.pass_(p, eb, tg.even_counts()[p])
    sim.flush(None, NP - 1, tg.even_counts()[-1])
    assert_clips(b, sim.out, "_ex against the model")
    # s16 out of the 16-bit ingest
    q = np.clip(np.rint(w.x * 32768.0), -32768, 32767).astype(np.int16)
    xf = (q.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    assert np.array_equal(fvad.pcm_f32_to_s16(xf), q)
    eng = engine(w, den=False)
    assert enable_ex(fvad, eng, INPUT, S16) == 0
    for a in tg.split_pushes(q):
        eng.submit_i16(a)
        eng.collect(want=False)
    eng.sync()
    got = eng.poll_clips()
    eng.capture_flush()
    got += eng.poll_clips()
    segs = tg.seg0(tg.drain_events(eng))
    sim = SimR(w.oracle, B, lambda s: xf[s], 48000, INPUT, S16)
    for p in range(NP):
        sim.pass_(p, segs, tg.even_counts()[p])
    sim.flush(None, NP - 1, tg.even_counts()[-1])
    want = finish(fvad, sim.out, S16)
    assert len(with_audio(want)) >= 8
    assert_clips(got, want, "INPUT s16")
    for c, s in got:
        assert (c["rate"], c["format"], c["source"]) == (48000, S16, INPUT)
        assert np.array_equal(s, q[c["stream"], c["channel"], c["first_sample"]:c["first_sample"] + c["n_samples"]])


def test_lifecycle_16k(world):
    """At 16 kHz s16: capture_flush of some streams mid-run (TAIL_SHORT, cut at
    the stream's position in clip-rate samples), reset_streams of one stream
    between pushes (its base and HEAD_SHORT), save / restore into another slot
    and the later clips of that stream.  The twin goes through the same
    resets and restores, so its rows are the expected audio."""
    w, fvad = world, world.fvad
    rate, f = 16000, 160
    _, _, events = twin(w, rate)
    segs_w = tg.seg0(events)
    counts = tg.even_counts()
    # a clip pending after push k with three pushes left (tg.test_lifecycle's choice)
    s0, k = next((e["stream"], e["push"]) for e in segs_w if e["sample_to"] > (e["push"] + 1) * PUSH and e["push"] <= NP - 4)
    # the slot then takes another stream from its start, one whose first clip completes within those
    donor = next(e["stream"] for e in segs_w if e["sample_to"] <= 3 * PUSH and e["stream"] != s0)
    flush_also = [s for s in range(B) if s != s0][:2]

    def pushes_of(p):
        if p <= k:
            return w.pcm[p]
        a = w.pcm[p].copy()
        a[:, s0] = w.pcm[p - k - 1][:, donor]
        return a

    def drive(eng, capture):
        outs, got = [], []
        for p in range(NP):
            outs.append(eng.push(pushes_of(p), denoised=not capture))
            if p == k:
                if capture:
                    eng.capture_flush([s0] + flush_also)
                eng.reset_streams([s0])
        eng.sync()
        if capture:
            got = eng.poll_clips()
            eng.capture_flush()
            got += eng.poll_clips()
        return outs, got

    t = engine(w, rate)
    outs, _ = drive(t, False)
    den = rows_of(outs)
    after = k + 1  # pushes before the reset
    eng = engine(w, rate)
    eng.enable_capture(0, tg.HIST, tg.POOL, source="denoised", fmt="s16")
    _, got = drive(eng, True)
    segs = tg.seg0(tg.drain_events(eng))
    mine = [list(c) for c in counts]
    for p in range(after, NP):
        mine[p][s0] = (p - k) * PUSH
    sim = SimR(w.oracle, B, lambda s: den[s], rate, DENOISED, S16)
    for p in range(NP):
        sim.pass_(p, segs, mine[p])
        if p == k:
            sim.flush([s0] + flush_also, k, mine[k])
            sim.drop(s0, 0)
            # slot s0's samples count from 0 again: its rows from push k + 1 on
            sim.audio = lambda s: den[s][:, after * T * f:] if s == s0 else den[s]
    sim.flush(None, NP - 1, mine[-1])
    want = finish(fvad, sim.out, S16)
    assert_clips(got, want, "flush, reset")
    cut = [c for c, _ in got if c["push"] == k and c["flags"] & TAIL and c["stream"] in [s0] + flush_also]
    assert cut and all(c["first_sample"] + c["n_samples"] == (k + 1) * T * f for c in cut if c["n_samples"])
    assert any(c["stream"] == s0 for c in cut)
    again = [c for c, _ in got if c["stream"] == s0 and c["push"] > k]
    assert again and all(c["first_sample"] + c["n_samples"] <= (NP - after) * T * f for c in again)
    assert len(with_audio(want)) >= 8

    # save after push 3, restore into slot 2 of a three-stream engine
    at = 4 * PUSH
    sv = next(e["stream"] for e in segs_w if e["push"] >= 4 and e["sample_from"] < at)
    A = engine(w, rate)
    A.enable_capture(0, tg.HIST, tg.POOL, source="denoised", fmt="s16")
    for p in range(4):
        A.push(w.pcm[p])
    blob = A.save_streams([sv])
    runs = []
    for capture in (False, True):
        Bn = engine(w, rate, n_streams=3)
        if capture:
            Bn.enable_capture(0, tg.HIST, tg.POOL, source="denoised", fmt="s16")
        Bn.restore_streams([2], blob)
        o = []
        for p in range(4, NP):
            a = np.zeros((T, 3, CH, 480), np.float32)
            a[:, 2] = w.pcm[p][:, sv]
            o.append(Bn.push(a, denoised=not capture))
        Bn.sync()
        runs.append((Bn, o))
    (_, o), (Bn, _) = runs
    rows = rows_of(o)[2]
    # indexed by the stream's own sample index: the restored slot starts at at L / M
    full = np.concatenate([np.zeros((CH, at // 480 * f), np.float32), rows], axis=1)
    got = Bn.poll_clips()
    Bn.capture_flush()
    got += Bn.poll_clips()
    segs = tg.seg0(tg.drain_events(Bn))
    sim = SimR(w.oracle, 3, lambda s: full, rate, DENOISED, S16)
    sim.drop(2, at)
    for q in range(NP - 4):
        sim.pass_(q, segs, [0, 0, at + (q + 1) * PUSH])
    sim.flush(None, NP - 5, [0, 0, at + (NP - 4) * PUSH])
    want = finish(fvad, sim.out, S16)
    assert_clips(got, want, "restored")
    assert with_audio(got) and all(c["first_sample"] >= at // 480 * f for c, _ in got)
    assert any(c["flags"] & HEAD and c["first_sample"] == at // 480 * f for c, _ in got)

    # fvad_engine_reset discards and zeroes
    eng = engine(w, rate)
    eng.enable_capture(0, tg.HIST, tg.POOL, source="denoised", fmt="s16")
    for p in range(NP):
        eng.push(w.pcm[p])
    eng.sync()
    eng.reset()
    assert eng.poll_clips() == [] and eng.capture_lost() == 0
    eng.capture_flush()
    assert eng.poll_clips() == []
    den0, _, _ = twin(w, rate)
    sim = SimR(w.oracle, B, lambda s: den0[s], rate, DENOISED, S16)
    for p in range(3):
        eng.push(w.pcm[p])
        sim.pass_(p, segs_w, counts[p])
    eng.sync()
    assert with_audio(sim.out)
    assert_clips(eng.poll_clips(), finish(fvad, sim.out, S16), "after fvad_engine_reset")


def test_pool_overflow_s16(world):
    """An s16 pool of 200 000 samples and no poll until the end: in each pass's
    list the clips with audio are a prefix, the rest arrive NO_AUDIO and are
    counted, no unread clip's shorts are overwritten; after polling, the flush
    has room again."""
    w, fvad = world, world.fvad
    rate, pool = 16000, 200000
    den, _, events = twin(w, rate)
    segs = tg.seg0(events)
    sim = SimR(w.oracle, B, lambda s: den[s], rate, DENOISED, S16, pool_cap=pool)
    counts = tg.even_counts()
    for p in range(NP):
        sim.pass_(p, segs, counts[p])
    k = len(sim.out)
    sim.read()
    sim.flush(None, NP - 1, counts[-1])
    want = finish(fvad, sim.out, S16)
    kept = [c for c, _ in want[:k] if c["n_samples"]]
    lost = [c for c, _ in want[:k] if c["flags"] & NOAUDIO]
    assert kept and lost and sum(c["n_samples"] for c in kept) <= pool
    assert any(c["n_samples"] for c, _ in want[k:])
    eng = engine(w, rate, den="device")
    eng.enable_capture(0, tg.HIST, pool, source="denoised", fmt="s16")
    for p in range(NP):
        eng.submit(w.pcm[p])
        eng.collect(want=False)
    eng.sync()
    got = eng.poll_clips()
    assert tg.seg0(tg.drain_events(eng)) == segs
    assert_clips(got, want[:k], "before the flush")
    for p in range(NP):  # the clips with audio are a prefix of each pass's list
        has = [bool(c["n_samples"]) for c, _ in got if c["push"] == p]
        assert has == sorted(has, reverse=True), (p, has)
    assert eng.capture_lost() == len(lost)
    eng.capture_flush()
    got += eng.poll_clips()
    assert_clips(got, want)
    assert eng.capture_lost() == sim.lost


def test_fp16_and_argument_checks(world):
    """fp16 at 16 kHz s16 against a twin in fp16; the calls' preconditions."""
    w, fvad = world, world.fvad
    L = fvad.lib()
    rate = 16000
    den, outs, events = twin(w, rate, "fp16")
    eng = engine(w, rate, "fp16", den="device")
    eng.enable_capture(0, tg.HIST, tg.POOL, source="denoised", fmt="s16")
    got, k, mine = run_w(eng, w.pcm)
    assert all(tg.same_outputs(a, b) for a, b in zip(mine, outs))
    ev = tg.drain_events(eng)
    assert ev == events
    want, _ = expected(w, tg.seg0(ev), den, rate, DENOISED, S16)
    assert len(with_audio(want)) >= 8
    assert_clips(got, want, "fp16")
    # poll_clip on an s16 capture, and the converse
    info, lost = fvad.Clip(), C.c_uint64()
    buf = np.zeros(16, np.float32)
    assert L.fvad_engine_poll_clip(eng.h, C.byref(info), buf.ctypes.data_as(C.c_void_p), 16, C.byref(lost)) == EINVAL
    f32 = engine(w, rate)
    f32.enable_capture(0, tg.HIST, tg.POOL, source="denoised", fmt="f32")
    assert L.fvad_engine_poll_clip_s16(f32.h, C.byref(info), buf.ctypes.data_as(C.c_void_p), 16, C.byref(lost)) == EINVAL
    assert L.fvad_engine_poll_clip(f32.h, C.byref(info), buf.ctypes.data_as(C.c_void_p), 16, C.byref(lost)) == 0
    assert enable_ex(fvad, f32, DENOISED, F32) == EINVAL  # twice
    # DENOISED without want_denoised; a bad source or format; the engine stays as it was
    plain = engine(w, den=False)
    assert enable_ex(fvad, plain, DENOISED, S16) == EINVAL and plain.clip_rate() == 0
    assert enable_ex(fvad, plain, 2, F32) == EINVAL and enable_ex(fvad, plain, -1, F32) == EINVAL
    assert enable_ex(fvad, plain, INPUT, 2) == EINVAL and enable_ex(fvad, plain, INPUT, -1) == EINVAL
    assert enable_ex(fvad, plain, INPUT, F32, history=3.99) == EINVAL
    assert enable_ex(fvad, plain, INPUT, F32, machine=2) == EINVAL
    assert L.fvad_engine_enable_capture_ex(plain.h, None) == EINVAL and plain.clip_rate() == 0
    assert L.fvad_engine_poll_clip(plain.h, C.byref(info), None, 0, None) == EINVAL  # still not enabled
    assert enable_ex(fvad, plain, INPUT, S16) == 0 and plain.clip_rate() == 48000
    # the other preconditions are enable_capture's
    fused = fvad.Engine(w.model, 2, CH, max_ticks=T, mode="fused", want_denoised=True)
    assert enable_ex(fvad, fused, DENOISED, S16) == EINVAL
    nod = fvad.Engine(w.model, 2, CH, max_ticks=T, bands=tg.BANDS, use_denoiser=False)
    nod.attach_vadm(tg.make_cfgs(fvad))
    nod.enable_events()
    assert enable_ex(fvad, nod, INPUT, S16) == EINVAL
    bare = fvad.Engine(w.model, 2, CH, max_ticks=T, bands=tg.BANDS, want_denoised=True)
    bare.attach_vadm(tg.make_cfgs(fvad))
    assert enable_ex(fvad, bare, DENOISED, S16) == EINVAL  # before enable_events
    ms, runs = eng.capture_times()
    assert set(ms) == {"k_hist_append", "capture_pass"} and runs >= 0


def test_schedules_give_the_same_list(world):
    """submit three deep with polls only at the end gives the list of push with a
    poll per push (16 kHz s16, device-only rows)."""
    w, fvad = world, world.fvad
    rate = 16000
    den, _, events = twin(w, rate)
    a = engine(w, rate, den="device")
    a.enable_capture(0, tg.HIST, tg.POOL, source="denoised", fmt="s16")
    ref, kref, _ = run_w(a, w.pcm, poll_each=True)
    b = engine(w, rate, den="device")
    b.enable_capture(0, tg.HIST, tg.POOL, source="denoised", fmt="s16")
    for p in range(NP):
        b.submit(w.pcm[p])
        if p >= 2:
            b.collect(want=False)
    b.collect(want=False)
    b.collect(want=False)
    b.sync()
    got = b.poll_clips()
    assert len(got) == kref
    b.capture_flush()
    got += b.poll_clips()
    assert len(with_audio(ref)) >= 8
    assert_clips(got, ref, "in flight against synchronous")
    want, _ = expected(w, tg.seg0(events), den, rate, DENOISED, S16)
    assert_clips(got, want, "against the twin")
    assert tg.drain_events(b) == events and b.capture_lost() == 0
