"""Per-stream denoised rates in one engine (denoised_rate =
FVAD_DENOISED_RATE_PER_STREAM; k_resample_out_ps, csrc/fvad_resample_out.hip).

The oracle is a twin engine that returns the 48 kHz denoised rows -- the
feature does not change them -- pushed the same input, and the host mirror
fvad_resample_out_host (tests/test_resample_out_cpu.py holds it to an f64
computation) run per stream and channel at the stream's rate over its valid
ticks.  The mirror's tail is cut from a history of the row's last 287 48 kHz
samples, as the device keeps it: a stream at K taps reads the last K - 1.  A
48000 stream's oracle is the rows themselves.  Everything is compared by the
bits; every packed slot past a stream's ticks_valid is zero."""
import ctypes as C

import numpy as np
import pytest

import parity_util as pu
from test_gpu_resample import KEYS, bits, outputs_equal
from test_gpu_stream_rates import NT7, TV7, Feed, source

pytestmark = pytest.mark.gpu

FRAME = 480
HIST = 287  # rs::kMaxTailOut: K - 1 at 8 kHz
ALL = (8000, 16000, 24000, 32000, 44100, 48000, 96000)
EINVAL, EFORMAT, ERATE = -1, -5, -6


@pytest.fixture(scope="module")
def model(fvad_mod):
    return fvad_mod.Model(seed=1)


class Input48:
    """48 kHz streams cut into pushes by ticks_valid; the slots past them hold noise"""

    def __init__(self, B, C, ticks, seed=0):
        self.B, self.C = B, C
        self.src = [source(48000, C, ticks, 100 * seed + s)[0] for s in range(B)]
        self.pos = [0] * B
        self.noise = np.random.default_rng(11 + seed)

    def push(self, nt, valid):
        pcm = (self.noise.integers(-20000, 20000, (nt, self.B, self.C, FRAME)).astype(np.float32)
               * np.float32(1.0 / 32768.0))
        for s in range(self.B):
            v, a = int(valid[s]), self.pos[s] * FRAME
            x = self.src[s][:, a:a + v * FRAME]
            assert x.shape[1] == v * FRAME, "source too short"
            pcm[:v, s] = x.reshape(self.C, v, FRAME).transpose(1, 0, 2)
            self.pos[s] += v
        return pcm


class Mirror:
    """The oracle over the twin's 48 kHz denoised rows: each row's history (its
    last 287 48 kHz samples, whatever its rate) and the streams' rates."""

    def __init__(self, fvad, rates, C):
        self.fvad, self.C, self.rates = fvad, C, list(rates)
        self.hist = np.zeros((len(rates), C, HIST), np.float32)

    def reset(self, streams):
        for s in streams:
            self.hist[s] = 0.0

    def push(self, den48, valid):
        """den48 [nt][B][C][480] -> one [nt][C][rate / 100] array per stream, zeros past valid"""
        nt, out = den48.shape[0], []
        for s, rate in enumerate(self.rates):
            v, o = int(valid[s]), np.zeros((nt, self.C, rate // 100), np.float32)
            for c in range(self.C):
                y = np.ascontiguousarray(den48[:v, s, c]).reshape(-1)
                if v and rate == 48000:
                    o[:v, c] = y.reshape(v, FRAME)
                elif v:
                    k1 = self.fvad.resample_out_info(rate)["taps_per_phase"] - 1
                    tail = self.hist[s, c, HIST - k1:].copy()
                    o[:v, c] = self.fvad.resample_out_host(rate, y, tail).reshape(v, rate // 100)
                if v:
                    self.hist[s, c] = np.concatenate([self.hist[s, c], y])[-HIST:]
            out.append(o)
        return out


def make(fvad, model, rates, C, max_ticks, rate_max=None, **kw):
    rate_max = rate_max or max(rates)
    eng = fvad.Engine(model, len(rates), C, max_ticks=max_ticks, want_denoised=True, denoised_rate="per_stream",
                      denoised_rate_max=rate_max, **kw)
    assert eng.stream_denoised_rates() == [rate_max] * len(rates)  # every stream starts at the max
    assert eng.frame_out is None
    eng.set_stream_denoised_rates(range(len(rates)), rates)
    assert eng.stream_denoised_rates() == list(rates)
    assert np.array_equal(eng.denoised_layout(), fvad.denoised_layout(rates, C))
    return eng


def twin(fvad, model, B, C, max_ticks, **kw):
    return fvad.Engine(model, B, C, max_ticks=max_ticks, want_denoised=True, **kw)


def den_equal(got, want, valid, what):
    assert isinstance(got, list) and len(got) == len(want), what
    for s, v in enumerate(valid):
        assert got[s].shape == want[s].shape, (what, s, got[s].shape, want[s].shape)
        assert np.array_equal(bits(got[s][:v]), bits(want[s][:v])), (what, s, pu.first_mismatch(got[s][:v], want[s][:v]))
        assert not got[s][v:].any(), (what, "past ticks_valid", s)


# ---------------------------------------------------------------------------
# 1, 2. kernel = mirror
# ---------------------------------------------------------------------------
def run_kernel_vs_mirror(fvad, model, rates, C, tvs, nts, max_ticks, how, seed=0):
    B = len(rates)
    inp, mir = Input48(B, C, sum(nts) + 1, seed), Mirror(fvad, rates, C)
    eng, ref = make(fvad, model, rates, C, max_ticks), twin(fvad, model, B, C, max_ticks)
    for p, (tv, nt) in enumerate(zip(tvs, nts)):
        pcm = inp.push(nt, tv)
        r = ref.push(pcm, ticks_valid=tv, denoised=True)
        if how == "push":
            o = eng.push(pcm, ticks_valid=tv, denoised=True)
        else:
            eng.submit(pcm, ticks_valid=tv)
            o = eng.collect(denoised=True)
        outputs_equal(o, r, tv, (how, p))
        den_equal(o["denoised"], mir.push(r["denoised"], tv), tv, (tuple(rates), how, "push", p))


@pytest.mark.parametrize("how", ["push", "submit"])
def test_kernel_equals_mirror_every_rate(fvad_mod, model, how):
    run_kernel_vs_mirror(fvad_mod, model, ALL, 2, TV7, NT7, 4, how)


SHAPES = {
    "1x1": ([44100], 1),
    # rates repeated and interleaved: no rate's list is contiguous, the offsets are uneven
    "9x8": ([8000, 44100, 8000, 48000, 16000, 44100, 96000, 8000, 48000], 8),
    "65x1": ([16000] * 64 + [96000], 1),
    # 12 units at 8 kHz (tick x stream: no multiple of the workgroup's 8) and exactly one group at 32 kHz
    "5x1": ([8000, 8000, 48000, 8000, 32000], 1),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_kernel_equals_mirror_other_shapes(fvad_mod, model, shape):
    rates, C = SHAPES[shape]
    rng = np.random.default_rng(len(rates))
    tvs = [list(rng.integers(0, 5, len(rates))) for _ in range(3)] + [[4] * len(rates)]
    run_kernel_vs_mirror(fvad_mod, model, rates, C, tvs, (4, 4, 4, 4), 4, "push", seed=1)


# ---------------------------------------------------------------------------
# 3. identical rates = the fixed-rate engine
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["staged", "fused", "fp16", "f32_fast"])
def test_identical_rates_equal_fixed_rate_engine(fvad_mod, model, mode):
    rates, Ch, T = [16000] * 3, 2, 4
    inp = Input48(3, Ch, 21, seed=2)
    eng = make(fvad_mod, model, rates, Ch, T, mode=mode)
    ref = fvad_mod.Engine(model, 3, Ch, max_ticks=T, want_denoised=True, mode=mode, denoised_rate=16000)
    for p, tv in enumerate(TV7):
        tv = tv[:3]
        pcm = inp.push(T, tv)
        o = eng.push(pcm, ticks_valid=tv, denoised=True)
        r = ref.push(pcm, ticks_valid=tv, denoised=True)
        outputs_equal(o, r, tv, (mode, p))
        # the packed array as the C ABI delivers it (one layout when the rates agree), whole: zeros past ticks_valid too
        raw, s = eng._alloc_out(T, True)
        assert fvad_mod.lib().fvad_engine_fetch(eng.h, T, C.byref(s)) == 0
        packed = raw["denoised"][: T * 3 * Ch * 160].reshape(T, 3, Ch, 160)
        for k, v in enumerate(tv):
            assert np.array_equal(bits(packed[:v, k]), bits(r["denoised"][:v, k])), (mode, p, k)
            assert not packed[v:, k].any() and not r["denoised"][v:, k].any(), (mode, p, k)
            assert np.array_equal(bits(o["denoised"][k]), bits(packed[:, k])), (mode, p, k)


# ---------------------------------------------------------------------------
# 4. the round trip, and the rest of the engine
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["submit", "push"])
def test_round_trip_end_to_end(fvad_mod, model, how):
    """8 kHz in, 8 kHz out, per leg, one engine: per-stream rates on both sides, machines,
    events and a capture of the input, against the engine without the output marker"""
    import test_gpu_capture as tc
    rates, T, depth = [16000, 48000, 8000], 100, 3
    streams, _ = pu.make_streams(fvad_mod, [0, 1, 0], tc.SECS)
    n_push = int(tc.SECS * 100) // T
    feed = Feed(fvad_mod, rates, 2, 1)
    for s, r in enumerate(rates):  # every 48000 / r-th sample: a signal at r, as exact 16-bit samples
        k = np.round(np.ascontiguousarray(streams[s][:, ::48000 // r]) * 32768.0).clip(-32768, 32767).astype(np.int16)
        feed.src[s] = (k.astype(np.float32) * np.float32(1.0 / 32768.0), k)

    def engine(**kw):
        e = fvad_mod.Engine(model, 3, 2, max_ticks=T, bands=tc.BANDS, want_denoised=True, input_rate="per_stream",
                            input_rate_max=48000, **kw)
        e.set_stream_rates([0, 2], [16000, 8000])
        e.attach_vadm(tc.make_cfgs(fvad_mod))
        e.enable_events()
        e.enable_capture(0, tc.HIST, tc.POOL)
        return e

    eng, ref = engine(denoised_rate="per_stream", denoised_rate_max=48000), engine()
    eng.set_stream_denoised_rates([0, 2], [16000, 8000])
    assert eng.stream_denoised_rates() == rates and eng.stream_rates() == rates
    mir = Mirror(fvad_mod, rates, 2)
    ev, clips, outs = ([], []), ([], []), ([], [])
    tv = [T] * 3

    def after(i, e, o):
        outs[i].append(o)
        ev[i].extend(e.poll_events()[0])
        clips[i].extend(e.poll_clips())

    for p in range(n_push):
        rows, _, _ = feed.push(T, tv)
        for i, e in enumerate((eng, ref)):
            pcm = e.pack_input(rows)
            if how == "push":
                after(i, e, e.push(pcm, denoised=True))
            else:  # three pushes in flight
                e.submit(pcm)
                if p >= depth - 1:
                    after(i, e, e.collect(denoised=True))
    if how == "submit":
        for i, e in enumerate((eng, ref)):
            for _ in range(min(depth - 1, n_push)):
                after(i, e, e.collect(denoised=True))
    for i, e in enumerate((eng, ref)):
        e.sync()
        e.capture_flush()
        ev[i].extend(tc.drain_events(e))
        clips[i].extend(e.poll_clips())
        assert e.capture_lost() == 0
    assert len(outs[0]) == len(outs[1]) == n_push
    for p in range(n_push):
        outputs_equal(outs[0][p], outs[1][p], tv, (how, p))
        den_equal(outs[0][p]["denoised"], mir.push(outs[1][p]["denoised"], tv), tv, (how, p))
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
    assert all(outs[0][-1]["denoised"][s].any() for s in range(3))


# ---------------------------------------------------------------------------
# 5. a rate change with pushes in flight
# ---------------------------------------------------------------------------
def test_rate_change_with_pushes_in_flight(fvad_mod, model):
    old, new, Ch = [48000, 16000, 8000, 44100], [8000, 16000, 48000, 44100], 2
    inp, mir = Input48(4, Ch, 21, seed=3), Mirror(fvad_mod, old, Ch)
    eng = make(fvad_mod, model, old, Ch, 4, rate_max=48000)
    same = make(fvad_mod, model, old, Ch, 4, rate_max=48000)  # never retargeted
    ref = twin(fvad_mod, model, 4, Ch, 4)
    tvs = ([4, 3, 4, 2], [4, 4, 2, 3], [3, 0, 4, 4], [3, 4, 4, 4])
    pcms = [inp.push(4, tv) for tv in tvs]
    rs = [ref.push(pcm, ticks_valid=tv, denoised=True) for pcm, tv in zip(pcms, tvs)]
    ss = [same.push(pcm, ticks_valid=tv, denoised=True) for pcm, tv in zip(pcms, tvs)]
    o0 = eng.push(pcms[0], ticks_valid=tvs[0], denoised=True)  # (histories that are not zeros)
    den_equal(o0["denoised"], mir.push(rs[0]["denoised"], tvs[0]), tvs[0], "before")
    eng.submit(pcms[1], ticks_valid=tvs[1])
    eng.submit(pcms[2], ticks_valid=tvs[2])
    lay_old = eng.denoised_layout()
    eng.set_stream_denoised_rates([0, 2], [new[0], new[2]])
    # the new state right after the call, two pushes still in flight
    assert eng.stream_denoised_rates() == new
    assert np.array_equal(eng.denoised_layout(), fvad_mod.denoised_layout(new, Ch))
    assert not np.array_equal(eng.denoised_layout(), lay_old)
    eng.submit(pcms[3], ticks_valid=tvs[3])
    for p in (1, 2):  # the old layout, unpacked by collect with the layout taken at submit
        o = eng.collect(denoised=True)
        outputs_equal(o, rs[p], tvs[p], ("old", p))
        den_equal(o["denoised"], mir.push(rs[p]["denoised"], tvs[p]), tvs[p], ("old layout", p))
        assert [x.shape[2] for x in o["denoised"]] == [r // 100 for r in old]
    # what the changed rows' first tick at the new rate must continue from: the true last samples
    before = {s: mir.hist[s].copy() for s in (0, 2)}
    assert all(before[s].any() for s in before)
    mir.rates = list(new)
    o = eng.collect(denoised=True)
    want = mir.push(rs[3]["denoised"], tvs[3])
    outputs_equal(o, rs[3], tvs[3], "new")
    den_equal(o["denoised"], want, tvs[3], "new layout")
    assert [x.shape[2] for x in o["denoised"]] == [r // 100 for r in new]
    # 48000 -> 8000: the first new-rate tick is the mirror fed the true last K - 1 samples, and no zero-tail run
    for c in range(Ch):
        y = np.ascontiguousarray(rs[3]["denoised"][:1, 0, c]).reshape(-1)
        tail = before[0][c].copy()  # (K - 1 = 287 at 8 kHz: the whole history)
        assert np.array_equal(bits(o["denoised"][0][0, c]), bits(fvad_mod.resample_out_host(8000, y, tail)))
        assert not np.array_equal(bits(o["denoised"][0][0, c]), bits(fvad_mod.resample_out_host(8000, y)))
    # 8000 -> 48000: the rows themselves
    assert np.array_equal(bits(o["denoised"][2][:4]), bits(rs[3]["denoised"][:4, 2]))
    # the unlisted streams: an engine that was never retargeted, bit for bit
    for s in (1, 3):
        assert np.array_equal(bits(o["denoised"][s]), bits(ss[3]["denoised"][s])), s
    # and back again: 8000 -> 16000 and 48000 -> 44100 continue over their history too
    eng.set_stream_denoised_rates([0, 2], [16000, 44100])
    mir.rates[0], mir.rates[2] = 16000, 44100
    pcm = inp.push(4, [4, 4, 4, 4])
    r = ref.push(pcm, denoised=True)
    den_equal(eng.push(pcm, denoised=True)["denoised"], mir.push(r["denoised"], [4] * 4), [4] * 4, "second change")


# ---------------------------------------------------------------------------
# 6. reset and blobs
# ---------------------------------------------------------------------------
def test_reset_streams_and_reset_keep_the_rates(fvad_mod, model):
    rates, Ch = [8000, 44100, 48000, 96000], 2
    inp, mir = Input48(4, Ch, 13, seed=5), Mirror(fvad_mod, rates, Ch)
    eng, ref = make(fvad_mod, model, rates, Ch, 4), twin(fvad_mod, model, 4, Ch, 4)
    layout = eng.denoised_layout()

    def step(tv, what):
        pcm = inp.push(4, tv)
        r = ref.push(pcm, ticks_valid=tv, denoised=True)
        o = eng.push(pcm, ticks_valid=tv, denoised=True)
        outputs_equal(o, r, tv, what)
        den_equal(o["denoised"], mir.push(r["denoised"], tv), tv, what)

    step([4, 4, 4, 3], "before")
    for e in (eng, ref):
        e.reset_streams([1, 2])
    mir.reset([1, 2])
    assert eng.stream_denoised_rates() == rates and np.array_equal(eng.denoised_layout(), layout)
    step([4, 2, 4, 4], "after reset_streams")  # (streams 0 and 3 continue over their history: the mirror's)
    for e in (eng, ref):
        e.reset()
    mir.reset(range(4))
    assert eng.stream_denoised_rates() == rates
    step([4, 4, 4, 4], "after reset")


def test_save_restore_moves_rates_and_history(fvad_mod, model):
    Ch, keys = 2, KEYS
    inp = Input48(7, Ch, 13, seed=6)
    A = make(fvad_mod, model, ALL, Ch, 4)
    for tv in (TV7[0], TV7[4]):
        A.push(inp.push(4, tv), ticks_valid=tv)
    saved = [0, 4, 5]  # 8000, 44100, 48000
    blob = A.save_streams(saved)
    assert fvad_mod.stream_blob_info(blob)["count"] == 3
    assert int(np.frombuffer(blob.tobytes()[80:84], np.uint32)[0]) == 0xFFFFFFFF  # reserved[1]
    # the target: another n_streams, max_ticks and denoised_rate_max; other slots, through index
    Bn = make(fvad_mod, model, [16000] * 5, Ch, 6, rate_max=48000)
    before = Bn.denoised_layout()
    Bn.restore_streams([4, 0, 2], blob, index=[2, 0, 1])
    ratesB = [8000, 16000, 44100, 16000, 48000]
    assert Bn.stream_denoised_rates() == ratesB
    assert np.array_equal(Bn.denoised_layout(), fvad_mod.denoised_layout(ratesB, Ch))
    assert not np.array_equal(Bn.denoised_layout(), before)
    for tv in (TV7[1], TV7[2]):
        pcm = inp.push(4, tv)
        oa = A.push(pcm, ticks_valid=tv, denoised=True)  # the unsaved twins
        pcmB, tvB = np.zeros((4, 5, Ch, FRAME), np.float32), [0] * 5
        for sa, sb in ((5, 4), (0, 0), (4, 2)):
            pcmB[:, sb], tvB[sb] = pcm[:, sa], tv[sa]
        ob = Bn.push(pcmB, ticks_valid=tvB, denoised=True)
        for sa, sb in ((5, 4), (0, 0), (4, 2)):
            v = tv[sa]
            assert np.array_equal(bits(oa["denoised"][sa]), bits(ob["denoised"][sb])), (sa, sb)
            for k in keys:
                assert np.array_equal(bits(oa[k][:v, sa]), bits(ob[k][:v, sb])), (k, sa)
        for sb in (1, 3):
            assert not ob["denoised"][sb].any()
    assert any(oa["denoised"][s].any() for s in saved)


def test_blob_refusals_leave_the_target_untouched(fvad_mod, model):
    Ch = 2
    big = make(fvad_mod, model, [96000, 8000], Ch, 4)
    inpb = Input48(2, Ch, 9, seed=7)
    big.push(inpb.push(4, [4, 4]))
    blob = big.save_streams([1, 0])  # record 1 is the 96000 stream
    fixed = fvad_mod.Engine(model, 2, Ch, max_ticks=4, want_denoised=True, denoised_rate=16000)
    plain = fvad_mod.Engine(model, 2, Ch, max_ticks=4, want_denoised=True)
    small = make(fvad_mod, model, [16000, 8000], Ch, 4, rate_max=16000)
    never = make(fvad_mod, model, [16000, 8000], Ch, 4, rate_max=16000)  # never sees a refused call
    inps = Input48(2, Ch, 9, seed=8)
    pcm = inps.push(4, [4, 4])
    for e in (small, never):
        e.push(pcm)

    def refused(call):
        with pytest.raises(fvad_mod.FvadError) as ei:
            call()
        assert ei.value.code == EFORMAT, ei.value

    refused(lambda: small.restore_streams([0, 1], blob))          # record 1 above denoised_rate_max
    refused(lambda: small.restore_streams([1], blob, index=[1]))
    refused(lambda: fixed.restore_streams([0], blob))             # per-stream -> fixed rate
    refused(lambda: plain.restore_streams([0], blob))             # per-stream -> 48 kHz
    refused(lambda: small.restore_streams([0], fixed.save_streams([0])))  # fixed rate -> per-stream
    refused(lambda: small.restore_streams([0], plain.save_streams([0])))
    assert small.stream_denoised_rates() == [16000, 8000]
    pcm = inps.push(4, [4, 3])
    o, n = (e.push(pcm, ticks_valid=[4, 3], denoised=True) for e in (small, never))
    outputs_equal(o, n, [4, 3], "after the refused restores")
    for s in range(2):
        assert np.array_equal(bits(o["denoised"][s]), bits(n["denoised"][s])), s
    small.restore_streams([0], blob, index=[0])  # the 8000 record fits
    assert small.stream_denoised_rates() == [8000, 8000]


def test_other_engines_blobs_keep_their_bytes(fvad_mod, model):
    """save_size and the blob of a plain and of a denoised_rate = 16000 engine: what the
    record layout of include/fvad.h gives without the new sections, and the same bytes
    whether or not the engine's creation names the new field"""
    Ch, fft = 2, 2048
    pad4 = lambda x: (x + 3) & ~3
    inp = Input48(2, Ch, 5, seed=9)
    pcm = inp.push(4, [4, 3])
    for kw, extra in ((dict(), 0), (dict(denoised_rate=16000), Ch * pad4(144 - 1))):
        blobs = []
        for new in (dict(), dict(denoised_rate_max=0)):
            e = fvad_mod.Engine(model, 2, Ch, max_ticks=4, want_denoised=True, fft_size=fft, **kw, **new)
            e.push(pcm, ticks_valid=[4, 3])
            blobs.append(e.save_streams([1, 0]))
            info = fvad_mod.stream_blob_info(blobs[-1])
            words = info["state_words"] + Ch * pad4(fft - 1) + extra
            assert info["stream_bytes"] == 4 * words, (kw, info)
            assert fvad_mod.lib().fvad_engine_save_size(e.h, 2) == info["header_bytes"] + 2 * 4 * words == blobs[-1].size
        assert np.array_equal(blobs[0], blobs[1]), kw


# ---------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------
def test_refusals(fvad_mod, model):
    import test_gpu_capture as tc
    rates, Ch = [8000, 16000, 16000], 2

    def refused(code, call):
        with pytest.raises(fvad_mod.FvadError) as ei:
            call()
        assert ei.value.code == code, ei.value

    def create(**kw):
        return fvad_mod.Engine(model, 3, Ch, max_ticks=4, bands=tc.BANDS, **kw)

    ps = dict(denoised_rate="per_stream", denoised_rate_max=16000)
    refused(EINVAL, lambda: create(**ps))                                  # the marker without want_denoised
    refused(EINVAL, lambda: create(want_denoised="device", **ps))
    refused(EINVAL, lambda: create(want_denoised=True, use_denoiser=False, **ps))
    for kw in (dict(), dict(denoised_rate=16000), dict(denoised_rate=48000)):  # denoised_rate_max without the marker
        refused(ERATE, lambda: create(want_denoised=True, denoised_rate_max=16000, **kw))
    refused(ERATE, lambda: create(want_denoised=True, denoised_rate="per_stream"))
    refused(ERATE, lambda: create(want_denoised=True, denoised_rate="per_stream", denoised_rate_max=22050))
    for kw in (dict(), dict(denoised_rate=16000)):
        other = create(want_denoised=True, **kw)
        refused(EINVAL, lambda: other.set_stream_denoised_rates([0], [16000]))
        refused(EINVAL, lambda: other.stream_denoised_rates())
        refused(EINVAL, lambda: other.denoised_layout())

    def engine():
        e = create(want_denoised=True, denoised_rate="per_stream", denoised_rate_max=32000)
        e.set_stream_denoised_rates(range(3), rates)
        e.attach_vadm(tc.make_cfgs(fvad_mod))
        e.enable_events()
        return e

    eng, never = engine(), engine()
    inp = Input48(3, Ch, 9, seed=10)
    pcm = inp.push(4, [4, 4, 4])
    for e in (eng, never):
        e.push(pcm)
    refused(ERATE, lambda: eng.set_stream_denoised_rates([0], [11025]))
    refused(ERATE, lambda: eng.set_stream_denoised_rates([0, 1], [8000, 44100]))  # above the max: nothing touched
    refused(ERATE, lambda: eng.set_stream_denoised_rates([1, 0], [8000, 48000]))
    refused(EINVAL, lambda: eng.set_stream_denoised_rates([1, 1], [8000, 8000]))
    refused(EINVAL, lambda: eng.set_stream_denoised_rates([3], [8000]))
    refused(EINVAL, lambda: eng.set_stream_denoised_rates([-1], [8000]))
    eng.set_stream_denoised_rates([], [])  # a no-op
    assert eng.stream_denoised_rates() == rates
    refused(EINVAL, lambda: eng.enable_capture(0, tc.HIST, tc.POOL, source="denoised"))
    assert fvad_mod.lib().fvad_engine_denoised_frame(eng.h) == EINVAL and eng.frame_out is None
    pcm = inp.push(4, [4, 2, 4])
    o, n = (e.push(pcm, ticks_valid=[4, 2, 4], denoised=True) for e in (eng, never))
    outputs_equal(o, n, [4, 2, 4], "the push after the refusals")
    for s in range(3):
        assert o["denoised"][s].shape == (4, Ch, rates[s] // 100)
        assert np.array_equal(bits(o["denoised"][s]), bits(n["denoised"][s])), s
    eng.enable_capture(0, tc.HIST, tc.POOL)  # a capture of the input works
    assert eng.resample_out_times()[1] >= 1   # and the launches are timed together
