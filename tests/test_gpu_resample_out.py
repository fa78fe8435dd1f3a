"""The denoised PCM at another rate on the GPU (fvad_engine_config.denoised_rate;
k_resample_out, csrc/fvad_resample_out.hip).

The oracle for the kernel is the host mirror fvad_resample_out_host, which
tests/test_resample_out_cpu.py holds to an independent f64 computation: a twin
engine without denoised_rate runs the same pushes and gives the 48 kHz denoised
rows; the mirror, applied per (stream, channel) over each stream's valid ticks
with a carried tail, must equal the denoised_rate engine's rows by the bits,
and every other output must equal the twin's.

Unless said otherwise an engine has 3 streams, 2 channels, max_ticks 4 and
runs PUSHES: ragged ticks_valid, a stream that skips a push, a push of one
tick, so a tail is taken from a single tick and carried over a skipped push.
The slots past a stream's ticks_valid hold noise, which nothing may read."""
import numpy as np
import pytest

import test_gpu_resample as tr

pytestmark = pytest.mark.gpu

FRAME = 480
RATES = (8000, 16000, 24000, 32000, 44100, 96000)
# (n_ticks of the push, ticks_valid)
PUSHES = ((4, [4, 2, 0]), (3, [1, 0, 3]), (1, [1, 1, 0]), (4, [4, 4, 4]), (4, [3, 4, 1]), (2, [2, 2, 2]))
KEYS = tr.KEYS
EINVAL, EFORMAT = -1, -5
bits = tr.bits


@pytest.fixture(scope="module")
def model(fvad_mod):
    return fvad_mod.Model(seed=1)


def source48(B, C, ticks, seed=0):
    """[B][C][ticks * 480] float32 at 48 kHz whose values are exact 16-bit
    samples k / 32768, and the k as int16."""
    rng = np.random.default_rng(77 + seed)
    t = np.arange(ticks * FRAME, dtype=np.float64)
    x = 0.2 * rng.uniform(-1.0, 1.0, (B, C, t.size))
    for s in range(B):
        for c in range(C):
            x[s, c] += 0.4 * np.sin(2.0 * np.pi * (310.0 + 97.0 * s + 41.0 * c) * t / 48000.0)
    k = np.round(x * 32768.0).astype(np.int16)
    return k.astype(np.float32) * np.float32(1.0 / 32768.0), k


class Cut:
    """Cuts a 48 kHz source into pushes [nt][B][C][480] by ticks_valid; noise past them."""

    def __init__(self, src, src16=None):
        self.src, self.src16 = src, src16
        self.B, self.C = src.shape[:2]
        self.pos = [0] * self.B
        self.noise = np.random.default_rng(9)

    def push(self, nt, valid):
        k = self.noise.integers(-20000, 20000, (nt, self.B, self.C, FRAME)).astype(np.int16)
        pcm = k.astype(np.float32) * np.float32(1.0 / 32768.0)
        for s in range(self.B):
            v, a = int(valid[s]), self.pos[s] * FRAME
            for c in range(self.C):
                pcm[:v, s, c] = self.src[s, c, a:a + v * FRAME].reshape(v, FRAME)
                if self.src16 is not None:
                    k[:v, s, c] = self.src16[s, c, a:a + v * FRAME].reshape(v, FRAME)
            self.pos[s] += v
        return pcm, k


class Mirror:
    """fvad_resample_out_host over each row's valid ticks, the tails carried."""

    def __init__(self, fvad, rate, B, C):
        d = fvad.resample_out_info(rate)
        self.fvad, self.rate, self.n_out = fvad, rate, d["frame_out"]
        self.tail = np.zeros((B, C, d["taps_per_phase"] - 1), np.float32)

    def __call__(self, den48, valid):
        nt, B, C = den48.shape[:3]
        out = np.zeros((nt, B, C, self.n_out), np.float32)
        for s in range(B):
            v = int(valid[s])
            for c in range(C):
                if v:
                    tail = self.tail[s, c].copy()
                    out[:v, s, c] = self.fvad.resample_out_host(self.rate, den48[:v, s, c], tail).reshape(v, self.n_out)
                    self.tail[s, c] = tail
        return out


def check_push(o, ref, mir, tv, what):
    """o: the denoised_rate engine's outputs, ref: the twin's, mir: the mirror of the twin's denoised rows"""
    tr.outputs_equal(o, ref, tv, what)
    got = o["denoised"]
    assert got.shape == mir.shape, (what, got.shape, mir.shape)
    for s, v in enumerate(tv):
        assert np.array_equal(bits(got[:v, s]), bits(mir[:v, s])), (what, s, tr.pu.first_mismatch(got[:v, s], mir[:v, s]))
        assert not got[v:, s].any(), (what, s, "slots past ticks_valid are zeros")
    assert any(v > 0 and got[:v, s].any() for s, v in enumerate(tv)) or not any(tv)


def run_vs_mirror(fvad, model, rate, B=3, C=2, pushes=PUSHES, max_ticks=4, **kw):
    src, _ = source48(B, C, sum(max(tv) for _, tv in pushes) + 1, seed=rate // 1000)
    cut = Cut(src)
    eng = fvad.Engine(model, B, C, max_ticks=max_ticks, want_denoised=True, denoised_rate=rate, **kw)
    twin = fvad.Engine(model, B, C, max_ticks=max_ticks, want_denoised=True, **kw)
    assert eng.frame_out == rate // 100 and twin.frame_out == FRAME
    mirror = Mirror(fvad, rate, B, C)
    for p, (nt, tv) in enumerate(pushes):
        pcm, _ = cut.push(nt, tv)
        o = eng.push(pcm, ticks_valid=tv, denoised=True)
        r = twin.push(pcm, ticks_valid=tv, denoised=True)
        check_push(o, r, mirror(r["denoised"], tv), tv, (rate, kw, p))
    ms, n = eng.resample_out_times()
    assert n >= 1 and ms > 0.0


# ---------------------------------------------------------------------------
# 1. kernel = mirror, every rate
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_kernel_equals_mirror(fvad_mod, model, rate):
    run_vs_mirror(fvad_mod, model, rate)


@pytest.mark.parametrize("rate", [8000, 44100])
@pytest.mark.parametrize("B,C", [(1, 1), (65, 3)])
def test_kernel_equals_mirror_other_shapes(fvad_mod, model, rate, B, C):
    """One unit (less than a packed workgroup's four or eight) and 195 rows: a
    last group that is partly empty, more than one block."""
    rng = np.random.default_rng(B)
    pushes = [(4, list(rng.integers(0, 5, B))) for _ in range(2)] + [(1, [1] * B), (3, [3] * B)]
    run_vs_mirror(fvad_mod, model, rate, B, C, pushes)


# ---------------------------------------------------------------------------
# 2. every mode that fills the denoised rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode,rate", [("staged", 16000), ("fused", 44100), ("fp16", 16000), ("fp16_fused", 44100),
                                       ("f32_fast", 8000), ("fused", 96000)])
def test_modes(fvad_mod, model, mode, rate):
    run_vs_mirror(fvad_mod, model, rate, mode=mode)


# ---------------------------------------------------------------------------
# 3. every path that delivers denoised rows
# ---------------------------------------------------------------------------
def test_paths(fvad_mod, model):
    rate, B, C = 16000, 3, 2
    src, src16 = source48(B, C, 14, seed=3)
    cut = Cut(src, src16)
    pushes = [(4, tv) + cut.push(4, tv) for _, tv in (PUSHES[0], PUSHES[3], PUSHES[4])]
    keys = KEYS + ("denoised",)

    def make():
        return fvad_mod.Engine(model, B, C, max_ticks=4, want_denoised=True, denoised_rate=rate)

    sync = make()
    want = [sync.push(pcm, ticks_valid=tv, denoised=True) for _, tv, pcm, _ in pushes]
    assert want[0]["denoised"].shape == (4, B, C, 160)
    for i16 in (False, True):
        eng = make()
        for _, tv, pcm, k in pushes:  # three pushes in flight
            slot = eng.input_slot_i16() if i16 else eng.input_slot()
            slot[:] = k if i16 else pcm
            (eng.submit_i16 if i16 else eng.submit)(slot, ticks_valid=tv)
        for p, (_, tv, _, _) in enumerate(pushes):
            o = eng.collect(denoised=True)
            assert o["denoised"].shape == (4, B, C, 160)
            tr.outputs_equal(o, want[p], tv, ("collect", i16, p), keys)
            for s, v in enumerate(tv):
                assert not o["denoised"][v:, s].any()
    # fetch after run_resident on a synthetic 48 kHz engine: two runs, the tails carried
    eng, twin = make(), fvad_mod.Engine(model, B, C, max_ticks=4, want_denoised=True)
    mirror = Mirror(fvad_mod, rate, B, C)
    for e in (eng, twin):
        e.load_synthetic(4, base=5)
    for run in range(2):
        for e in (eng, twin):
            e.run_resident(4)
        o, r = eng.fetch(4, denoised=True), twin.fetch(4, denoised=True)
        check_push(o, r, mirror(r["denoised"], [4] * B), [4] * B, ("resident", run))


# ---------------------------------------------------------------------------
# 4. together with input_rate
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rate_in,rate_out", [(16000, 16000), (44100, 8000)])
def test_with_input_rate(fvad_mod, model, rate_in, rate_out):
    """resample_host -> the 48 kHz engine's rows -> resample_out_host"""
    B, C = 3, 2
    src, _ = tr.source(fvad_mod, rate_in, B, C, 20, seed=8)
    feed = tr.Feed(fvad_mod, rate_in, src)
    eng = fvad_mod.Engine(model, B, C, max_ticks=4, want_denoised=True, input_rate=rate_in, denoised_rate=rate_out)
    twin = fvad_mod.Engine(model, B, C, max_ticks=4, want_denoised=True)
    assert (eng.frame_in, eng.frame_out) == (rate_in // 100, rate_out // 100)
    mirror = Mirror(fvad_mod, rate_out, B, C)
    for p, tv in enumerate(tr.TV):
        raw, _, pcm48 = feed.push(4, tv)
        o = eng.push(raw, ticks_valid=tv, denoised=True)
        r = twin.push(pcm48, ticks_valid=tv, denoised=True)
        check_push(o, r, mirror(r["denoised"], tv), tv, (rate_in, rate_out, p))


# ---------------------------------------------------------------------------
# 5. reset_streams and reset
# ---------------------------------------------------------------------------
def test_reset_streams_and_reset(fvad_mod, model):
    rate, B, C = 8000, 3, 2
    src, _ = source48(B, C, 20, seed=4)
    keys = KEYS + ("denoised",)
    TV = tr.TV

    def run(action, first=0):
        """pushes first.. of TV's schedule on a new engine, `action` after the first of them"""
        cut = Cut(src)
        for tv in TV[:first]:  # (a fresh engine starts where the others are after `first` pushes)
            for s in range(B):
                cut.pos[s] += tv[s]
        eng = fvad_mod.Engine(model, B, C, max_ticks=4, want_denoised=True, denoised_rate=rate)
        out = []
        for p, tv in enumerate(TV[first:], first):
            out.append(eng.push(cut.push(4, tv)[0], ticks_valid=tv, denoised=True))
            if p == first and action:
                action(eng)
        return out

    plain = run(None)
    fresh = run(None, first=1)
    one = run(lambda e: e.reset_streams([1]))
    every = run(lambda e: e.reset())
    for p in range(1, len(TV)):
        tv = TV[p]
        for k in keys:
            for s in range(B):
                v = tv[s]
                want_one = fresh[p - 1] if s == 1 else plain[p]
                assert np.array_equal(bits(one[p][k][:v, s]), bits(want_one[k][:v, s])), ("reset_streams", p, k, s)
                assert np.array_equal(bits(every[p][k][:v, s]), bits(fresh[p - 1][k][:v, s])), ("reset", p, k, s)
    # the reset changed something: stream 1's first denoised tick after it
    p = next(p for p in range(1, len(TV)) if TV[p][1] > 0)
    assert not np.array_equal(one[p]["denoised"][0, 1], plain[p]["denoised"][0, 1])


# ---------------------------------------------------------------------------
# 6. save / restore, blob compatibility
# ---------------------------------------------------------------------------
def test_save_restore_moves_the_tails(fvad_mod, model):
    rate, K = 16000, 144
    TV = tr.TV
    src, _ = source48(3, 2, 20, seed=5)
    cut = Cut(src)
    keys = KEYS + ("denoised",)
    A = fvad_mod.Engine(model, 3, 2, max_ticks=4, want_denoised=True, denoised_rate=rate)
    for tv in TV[:2]:
        A.push(cut.push(4, tv)[0], ticks_valid=tv)
    blob = A.save_streams([0, 2])
    info = fvad_mod.stream_blob_info(blob)
    plain = fvad_mod.Engine(model, 3, 2, max_ticks=4, want_denoised=True)
    pblob = plain.save_streams([0])
    pinfo = fvad_mod.stream_blob_info(pblob)
    reserved = np.frombuffer(blob.tobytes()[76:128], np.uint32)
    assert reserved[0] == 0 and reserved[1] == rate and not reserved[2:].any()
    assert not np.frombuffer(pblob.tobytes()[76:128], np.uint32).any()
    words = pinfo["state_words"] + 2 * ((2048 - 1 + 3) & ~3)
    assert pinfo["stream_bytes"] == 4 * words
    # per channel (K + 2) & ~3 words behind the plain record
    assert info["stream_bytes"] == 4 * (words + 2 * ((K + 2) & ~3)) and info["config_hash"] != pinfo["config_hash"]
    assert info["count"] == 2 and fvad_mod.lib().fvad_engine_save_size(A.h, 2) == blob.size
    # with input tails too: the output tails stand behind them
    both = fvad_mod.Engine(model, 3, 2, max_ticks=4, want_denoised=True, input_rate=16000, denoised_rate=rate)
    binfo = fvad_mod.stream_blob_info(both.save_streams([1]))
    assert binfo["stream_bytes"] == 4 * (words + 2 * 48 + 2 * ((K + 2) & ~3))

    # refused by an engine of another denoised_rate and by a plain one, which stay as they were;
    # a plain engine's blob is refused by A
    other = fvad_mod.Engine(model, 3, 2, max_ticks=4, want_denoised=True, denoised_rate=8000)
    twin = fvad_mod.Engine(model, 3, 2, max_ticks=4, want_denoised=True)
    mirror = Mirror(fvad_mod, 8000, 3, 2)
    src8, _ = source48(3, 2, 9, seed=6)
    cut8 = Cut(src8)
    for p in range(2):
        if p == 1:
            for e, b in ((other, blob), (twin, blob), (other, pblob)):
                with pytest.raises(fvad_mod.FvadError) as ei:
                    e.restore_streams([0, 1] if b is blob else [0], b)
                assert ei.value.code == EFORMAT
        pcm, _ = cut8.push(4, [4, 3, 4])
        o = other.push(pcm, ticks_valid=[4, 3, 4], denoised=True)
        r = twin.push(pcm, ticks_valid=[4, 3, 4], denoised=True)
        check_push(o, r, mirror(r["denoised"], [4, 3, 4]), [4, 3, 4], ("after the refused restore", p))
    with pytest.raises(fvad_mod.FvadError) as ei:
        A.restore_streams([0], pblob)
    assert ei.value.code == EFORMAT

    # into other slots of an engine of another size: the streams continue by the bits
    Bn = fvad_mod.Engine(model, 5, 2, max_ticks=6, want_denoised=True, denoised_rate=rate)
    Bn.restore_streams([3, 1], blob)
    tv = TV[2]
    pcm, _ = cut.push(4, tv)
    oa = A.push(pcm, ticks_valid=tv, denoised=True)
    pcmb = np.zeros((4, 5, 2, FRAME), np.float32)
    pcmb[:, 3], pcmb[:, 1] = pcm[:, 0], pcm[:, 2]
    ob = Bn.push(pcmb, ticks_valid=[0, tv[2], 0, tv[0], 0], denoised=True)
    assert ob["denoised"].shape == (4, 5, 2, 160)
    for sa, sb in ((0, 3), (2, 1)):
        v = tv[sa]
        assert v > 0 and oa["denoised"][:v, sa].any()
        for k in keys:
            assert np.array_equal(bits(oa[k][:v, sa]), bits(ob[k][:v, sb])), (k, sa)
    # a restored stream differs from one that starts with empty tails (the equality is not empty)
    fresh = fvad_mod.Engine(model, 3, 2, max_ticks=4, want_denoised=True, denoised_rate=rate)
    of = fresh.push(pcm, ticks_valid=tv, denoised=True)
    assert not np.array_equal(of["denoised"][0, 0], oa["denoised"][0, 0])


# ---------------------------------------------------------------------------
# 7. plain engines are what they were
# ---------------------------------------------------------------------------
def kernel_names(fvad, eng):
    names, i = [], 0
    while True:
        nm = fvad.lib().fvad_engine_kernel_name(eng.h, i)
        if nm is None:
            return names
        names.append(nm.decode())
        i += 1


@pytest.mark.parametrize("mode", ["staged", "fused"])
def test_plain_engines_unchanged(fvad_mod, model, mode):
    engs = [fvad_mod.Engine(model, 3, 2, max_ticks=4, want_denoised=True, mode=mode, denoised_rate=r)
            for r in (0, 48000, 16000)]
    zero, same, rated = engs
    assert zero.cfg.denoised_rate == 0 and same.cfg.denoised_rate == 48000
    names = kernel_names(fvad_mod, zero)
    assert len(names) >= 2 and not any("resample" in n for n in names)
    words = fvad_mod.stream_blob_info(zero.save_streams([0]))["state_words"] + 2 * ((2048 - 1 + 3) & ~3)
    for e in (zero, same):
        assert e.frame_out == FRAME
        assert kernel_names(fvad_mod, e) == names
        assert fvad_mod.lib().fvad_engine_save_size(e.h, 3) == 128 + 3 * 4 * words
        with pytest.raises(fvad_mod.FvadError) as ei:
            e.resample_out_times()
        assert ei.value.code == EINVAL
    assert np.array_equal(zero.save_streams([0, 1]), same.save_streams([0, 1]))  # header, hash and records
    # the list of a push's pipeline kernels is the same with the field set
    assert kernel_names(fvad_mod, rated) == names and rated.frame_out == 160
    src, _ = source48(3, 2, 5, seed=7)
    pcm, _ = Cut(src).push(4, [4, 4, 4])
    o0, o1 = (e.push(pcm, denoised=True) for e in (zero, same))
    assert o0["denoised"].shape == (4, 3, 2, FRAME)
    tr.outputs_equal(o0, o1, [4, 4, 4], mode, KEYS + ("denoised",))
