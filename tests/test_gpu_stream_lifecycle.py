"""Per-stream lifecycle of the batched engine: fvad_engine_reset_streams,
fvad_engine_save_streams and fvad_engine_restore_streams.

"Equal" is np.array_equal on every per-tick output (vad, ratio, win_flag,
win_ratio, win_vad, band, denoised) and == on the machines' snapshot, rolling
buffers and segments.  The bit-exact modes (staged, fused) are compared with
the CPU oracle fed what the slot's current stream was fed; the tolerance modes
(f32_fast, fp16) with a control engine of the same mode that never resets or
moves a stream -- their outputs are not the oracle's bit for bit, so neither is
their machine state, and the control is the reference for both."""
import numpy as np
import pytest

import parity_util as pu

pytestmark = pytest.mark.gpu

FRAME = 480
KEYS = ("vad", "ratio", "win_flag", "win_ratio", "win_vad", "band", "denoised")
BANDS2 = ((4, 64), (13, 128))


def alt_config(mod):
    alt = mod.VadmConfig.default()
    alt.speech_min_freq, alt.speech_max_freq = 300.0, 3000.0
    alt.min_vad_duration_sec = 0.3
    return alt


_audio = {}


def audio(fvad_mod, sid, ticks):
    """ticks * 480 samples of synthetic stream sid, stereo (cached)."""
    if (sid, ticks) not in _audio:
        _audio[(sid, ticks)] = fvad_mod.synth_stream(sid, ticks * FRAME, 2)[0]
    return _audio[(sid, ticks)]


class Slots:
    """Feeds each slot of an engine its own audio and keeps each slot's outputs."""

    def __init__(self, eng, denoised=True):
        self.eng, self.den = eng, denoised
        self.x = [None] * eng.B
        self.pos = [0] * eng.B
        self.out = [[] for _ in range(eng.B)]

    def assign(self, s, x, pos=0):
        """slot s reads x from tick pos on; its kept outputs start again"""
        self.x[s], self.pos[s], self.out[s] = x, pos, []

    def _pcm(self, nt):
        B, C = self.eng.B, self.eng.C
        pcm = np.zeros((nt, B, C, FRAME), np.float32)
        valid = np.zeros(B, np.int32)
        for s in range(B):
            if self.x[s] is None:
                continue
            v = max(0, min(nt, self.x[s].shape[1] // FRAME - self.pos[s]))
            valid[s] = v
            if v:
                a = self.pos[s] * FRAME
                pcm[:v, s] = self.x[s][:, a:a + v * FRAME].reshape(C, v, FRAME).transpose(1, 0, 2)
            self.pos[s] += v
        return pcm, valid

    def _keep(self, o, valid):
        for s in range(self.eng.B):
            v = int(valid[s])
            self.out[s].append({k: o[k][:v, s] for k in o})

    def push(self, nt):
        pcm, valid = self._pcm(nt)
        self._keep(self.eng.push(pcm, ticks_valid=valid, denoised=self.den), valid)

    def submit(self, nt):
        pcm, valid = self._pcm(nt)
        self.eng.submit(pcm, ticks_valid=valid)
        return valid

    def collect(self, valid):
        self._keep(self.eng.collect(denoised=self.den), valid)

    def run(self, pushes):
        for nt in pushes:
            self.push(nt)

    def result(self, s):
        """slot s's outputs since its last assign: per tick, and per completed window"""
        W = self.eng.wpt
        cat = lambda k: np.concatenate([o[k] for o in self.out[s]])
        cnt = [o["win_flag"] for o in self.out[s]]
        r = {"vad": cat("vad"), "ratio": cat("ratio"), "win_flag": cat("win_flag")}
        for k in ("win_ratio", "win_vad", "band"):
            r[k] = np.concatenate([pu.tick_windows(o[k], c, W) for o, c in zip(self.out[s], cnt)])
        if self.den:
            r["denoised"] = cat("denoised").transpose(1, 0, 2).reshape(self.eng.C, -1)
        return r


def machines(eng, s, n_mach):
    return [(eng.vadm_snapshot(s, m), [eng.vadm_rolling(s, w, m).tobytes() for w in range(3)], eng.segments(s, m))
            for m in range(n_mach)]


_oracle = {}


def oracle_stream(fvad_mod, oracle_mod, x, key, fft_size=2048, use_denoiser=True, alt=True, trace=True):
    """The oracle over the whole of x: per-tick / per-window trace, denoised, and
    the machines' snapshot, rolling buffers and segments (main, then alt)."""
    key = (key, x.shape[1], fft_size, use_denoiser, alt, trace)
    if key in _oracle:
        return _oracle[key]
    om = oracle_mod.Model(seed=1)
    frames = x.shape[1] // FRAME
    alts = [alt_config(oracle_mod)] if alt else []
    p = oracle_mod.Pipeline(2, om, fft_size=fft_size, use_denoiser=use_denoiser, alt_cfgs=alts,
                            trace_frames=frames + 1 if trace else 0,
                            trace_windows=x.shape[1] // fft_size + 2 if trace else 0,
                            trace_denoised=frames * FRAME if trace and use_denoiser else 0)
    for k in range(0, x.shape[1], 48000):
        p.push([x[c, k:k + 48000] for c in range(2)])
    r = {"mach": [(p.vadm_snapshot(a), [p.vadm_rolling(w, a).tobytes() for w in range(3)], p.segments(a))
                  for a in ([-1, 0] if alt else [-1])]}
    if trace:
        r["frames"], r["windows"] = p.trace()
        r["denoised"] = p.tden[:, :frames * FRAME].copy() if use_denoiser else None
    _oracle[key] = r
    return r


def flags_from(tick0, n, fft_size):
    """windows completed in each of ticks [tick0, tick0 + n) of a stream"""
    t = np.arange(tick0, tick0 + n, dtype=np.int64)
    return (((t + 1) * FRAME) // fft_size - (t * FRAME) // fft_size).astype(np.int32)


def assert_oracle(ref, got, tick0=0, fft_size=2048, what=None):
    """got: a slot's outputs from tick tick0 of the stream ref is the oracle of"""
    fr, wi = ref["frames"], ref["windows"]
    n = len(got["vad"])
    assert n > 0 and tick0 + n <= len(fr), (what, n, tick0, len(fr))
    assert np.array_equal(fr["vad"][tick0:tick0 + n], got["vad"]), (what, pu.first_mismatch(fr["vad"][tick0:], got["vad"]))
    assert np.array_equal(fr["ratio"][tick0:tick0 + n], got["ratio"]), what
    assert np.array_equal(flags_from(tick0, n, fft_size), got["win_flag"]), what
    w0, w1 = tick0 * FRAME // fft_size, (tick0 + n) * FRAME // fft_size
    assert w1 <= len(wi) and w1 - w0 == len(got["win_ratio"]), (what, w0, w1, len(wi))
    assert np.array_equal(wi["band"][w0:w1, :2], got["band"][:, :, 0]), what
    assert np.array_equal(wi["ratio"][w0:w1], got["win_ratio"]), what
    assert np.array_equal(wi["vad"][w0:w1], got["win_vad"]), what
    if "denoised" in got and ref.get("denoised") is not None:
        assert np.array_equal(ref["denoised"][:, tick0 * FRAME:(tick0 + n) * FRAME], got["denoised"]), what


def assert_same(a, b, what=None):
    for k in KEYS:
        if k in a or k in b:
            assert np.array_equal(a[k], b[k]), (what, k, pu.first_mismatch(a[k], b[k]))


# ---------------------------------------------------------------------------
# 1. reset parity
# ---------------------------------------------------------------------------
P1 = [37, 13, 37, 29, 37, 37, 37, 23]  # 250 ticks (2.5 s), ragged
P2 = [37] * 9 + [17]                   # 350 ticks (3.5 s)
RESET = [0, 7, 8, 10]  # first slot, last of k_rnn3's group 0, first of group 1, the last


@pytest.mark.parametrize("mode", ["staged", "fused", "f32_fast", "fp16"])
def test_reset_streams_parity(fvad_mod, oracle_mod, mode):
    assert sum(P1) == 250 and sum(P2) == 350
    m = fvad_mod.Model(seed=1)
    B, n_mach = 11, 0 if mode == "fused" else 2
    old = [audio(fvad_mod, 100 + s, 600) for s in range(B)]
    new = {s: audio(fvad_mod, 200 + i, 350) for i, s in enumerate(RESET)}

    def engine():
        e = fvad_mod.Engine(m, B, 2, max_ticks=37, want_denoised=True, mode=mode, bands=BANDS2)
        if n_mach:
            e.attach_vadm([fvad_mod.VadmConfig.default(), alt_config(fvad_mod)])
        return e

    eng = engine()
    sl = Slots(eng)
    for s in range(B):
        sl.assign(s, old[s])
    sl.run(P1)
    eng.reset_streams(RESET)
    for s in RESET:
        sl.assign(s, new[s])
    sl.run(P2)
    if mode in ("staged", "fused"):
        for s in range(B):
            ref = oracle_stream(fvad_mod, oracle_mod, new[s] if s in RESET else old[s],
                                (200 + RESET.index(s)) if s in RESET else 100 + s)
            assert_oracle(ref, sl.result(s), what=(mode, s))
            if n_mach:
                assert machines(eng, s, 2) == ref["mach"], (mode, s)
    else:
        ctl = Slots(engine())  # never resets: the untouched slots' reference
        for s in range(B):
            ctl.assign(s, old[s])
        ctl.run(P1 + P2)
        fresh = Slots(engine())  # a fresh engine fed only the new audio, in the same slots
        for s in RESET:
            fresh.assign(s, new[s])
        fresh.run(P2)
        for s in range(B):
            ref = fresh if s in RESET else ctl
            assert_same(ref.result(s), sl.result(s), (mode, s))
            assert machines(eng, s, 2) == machines(ref.eng, s, 2), (mode, s)


@pytest.mark.parametrize("mode", ["staged", "fused"])
def test_reset_all_equals_reset_and_reset_before_first_push(fvad_mod, oracle_mod, mode):
    m = fvad_mod.Model(seed=1)
    B = 3
    xs = [audio(fvad_mod, 100 + s, 100) for s in range(B)]
    ys = [audio(fvad_mod, 200 + s, 100) for s in range(B)]
    res = []
    for how in ("streams", "all"):
        eng = fvad_mod.Engine(m, B, 2, max_ticks=37, want_denoised=True, mode=mode)
        if mode == "staged":
            eng.attach_vadm()
        eng.reset_streams([2, 0])  # before the first push: changes nothing
        eng.reset_streams([])
        sl = Slots(eng)
        for s in range(B):
            sl.assign(s, xs[s])
        sl.run([37, 37, 26])
        first = [sl.result(s) for s in range(B)]
        eng.reset_streams(range(B)) if how == "streams" else eng.reset()
        for s in range(B):
            sl.assign(s, ys[s])
        sl.run([37, 37, 26])
        res.append((first, [sl.result(s) for s in range(B)],
                    [machines(eng, s, 1) for s in range(B)] if mode == "staged" else None))
    for s in range(B):
        for ph in (0, 1):
            assert_same(res[0][ph][s], res[1][ph][s], (mode, s, ph))
        assert_oracle(oracle_stream(fvad_mod, oracle_mod, xs[s], 100 + s, alt=False), res[0][0][s], what=(mode, s))
        assert_oracle(oracle_stream(fvad_mod, oracle_mod, ys[s], 200 + s, alt=False), res[0][1][s], what=(mode, s))
    assert res[0][2] == res[1][2]


def test_reset_streams_refused_under_lt_full(fvad_mod):
    eng = fvad_mod.Engine(fvad_mod.Model(seed=1), 2, 2, max_ticks=10)
    eng.attach_vadm()
    eng.set_debug(fvad_mod.DEBUG_VADM_LT_FULL, 1)
    with pytest.raises(fvad_mod.FvadError) as ei:
        eng.reset_streams([0])
    assert ei.value.code == fvad_mod.EINVAL
    eng.set_debug(fvad_mod.DEBUG_VADM_LT_FULL, 0)
    eng.reset_streams([0])


# ---------------------------------------------------------------------------
# 2. ordering without syncs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["plain", "defer_max_5", "group"])
def test_reset_lands_between_pushes_without_syncs(fvad_mod, oracle_mod, flavour):
    m = fvad_mod.Model(seed=1)
    B, T = 6, 50
    reset = [4] if flavour == "group" else [1, 4]
    old = [audio(fvad_mod, 100 + s, 3 * T) for s in range(B)]
    new = {s: audio(fvad_mod, 200 + s, T) for s in reset}

    if flavour == "group":
        grp = fvad_mod.EngineGroup(m, B, 2, groups=2, vadm=True, max_ticks=T)
        engs, first = grp.engines, grp.first
    else:
        e = fvad_mod.Engine(m, B, 2, max_ticks=T)
        e.attach_vadm()
        if flavour == "defer_max_5":
            e.set_debug(fvad_mod.DEBUG_VADM_DEFER_MAX, 5)
        grp, engs, first = None, [e], [0]
    sls = [Slots(e, denoised=False) for e in engs]
    where = lambda s: max(g for g, f in enumerate(first) if f <= s)
    for s in range(B):
        sls[where(s)].assign(s - first[where(s)], old[s])
    pend = [[sl.submit(T) for sl in sls] for _ in range(2)]  # p0, p1 of every engine
    if grp:
        grp.reset_streams(reset)
    else:
        engs[0].reset_streams(reset)
    for s in reset:
        sls[where(s)].out[s - first[where(s)]] = []  # (outputs are kept from the collects below)
        sls[where(s)].x[s - first[where(s)]] = new[s]
        sls[where(s)].pos[s - first[where(s)]] = 0
    pend.append([sl.submit(T) for sl in sls])  # p2
    for valids in pend:  # collect x 3, no sync anywhere
        for sl, v in zip(sls, valids):
            sl.collect(v)
    for s in range(B):
        g = where(s)
        r = sls[g].result(s - first[g])
        if s in reset:
            # p0, p1: the old stream, untouched by the reset queued behind them; p2: a fresh stream
            assert len(r["vad"]) == 3 * T
            cut = lambda d, a, b: {"vad": d["vad"][a:b], "ratio": d["ratio"][a:b], "win_flag": d["win_flag"][a:b]}
            ro = oracle_stream(fvad_mod, oracle_mod, old[s], 100 + s, alt=False)
            rn = oracle_stream(fvad_mod, oracle_mod, new[s], 200 + s, alt=False)
            for ref, a, b, t0 in ((ro, 0, 2 * T, 0), (rn, 2 * T, 3 * T, 0)):
                assert np.array_equal(ref["frames"]["vad"][t0:t0 + b - a], r["vad"][a:b]), (flavour, s, a)
                assert np.array_equal(ref["frames"]["ratio"][t0:t0 + b - a], r["ratio"][a:b]), (flavour, s, a)
                assert np.array_equal(flags_from(0, b - a, 2048), r["win_flag"][a:b]), (flavour, s, a)
            nw_old = 2 * T * FRAME // 2048
            wi = np.concatenate([ro["windows"][:nw_old], rn["windows"][:T * FRAME // 2048]])
            assert np.array_equal(wi["band"][:, :2], r["band"][:, :, 0]), (flavour, s)
            assert np.array_equal(wi["ratio"], r["win_ratio"]) and np.array_equal(wi["vad"], r["win_vad"]), (flavour, s)
            ref_mach = rn["mach"]
        else:
            ref = oracle_stream(fvad_mod, oracle_mod, old[s], 100 + s, alt=False)
            assert_oracle(ref, r, what=(flavour, s))
            ref_mach = ref["mach"]
        assert machines(engs[g], s - first[g], 1) == ref_mach, (flavour, s)


# ---------------------------------------------------------------------------
# 3. migration
# ---------------------------------------------------------------------------
def test_migration_to_another_engine(fvad_mod, oracle_mod):
    m = fvad_mod.Model(seed=1)
    ids = [0, 3, 19, 39, 7, 12, 42, 4]
    total, cut = 2000, 1050  # ticks: 20 s, moved at 10.5 s
    xs = [audio(fvad_mod, i, total) for i in ids]
    cfgs = lambda: [fvad_mod.VadmConfig.default(), alt_config(fvad_mod)]
    A = fvad_mod.Engine(m, 8, 2, max_ticks=50, bands=BANDS2, want_denoised=True)
    A.attach_vadm(cfgs(), seg_capacity=256)
    sa = Slots(A)
    for s in range(8):
        sa.assign(s, xs[s])
    sa.run([50] * 21)
    src, dst, index = [1, 2, 5, 7], [4, 0, 2, 3], [2, 0, 3, 1]
    blob = A.save_streams(src)
    info = fvad_mod.stream_blob_info(blob)
    assert info["count"] == 4 and info["seg_capacity"] == 256 and info["n_machines"] == 2
    assert blob.size == 128 + 4 * info["stream_bytes"]

    # preconditions, from the oracle itself
    moved = {d: src[i] for d, i in zip(dst, index)}  # B's slot -> A's slot
    at_cut = {a: oracle_stream(fvad_mod, oracle_mod, np.ascontiguousarray(xs[a][:, :cut * FRAME]), ("cut", ids[a]),
                               trace=False)["mach"][0] for a in src}
    full = {a: oracle_stream(fvad_mod, oracle_mod, xs[a], ids[a]) for a in src}
    assert any(at_cut[a][0]["speech_state"] != 0 for a in src)
    assert any(at_cut[a][0]["n_segments"] >= 1 for a in src)
    assert all(full[a]["mach"][0][0]["n_segments"] > at_cut[a][0]["n_segments"] for a in src)
    assert cut * FRAME % 2048 == 192  # the pending window part is not empty

    Bn = fvad_mod.Engine(m, 5, 2, max_ticks=37, bands=BANDS2, want_denoised=True)
    Bn.attach_vadm(cfgs(), seg_capacity=8)
    sb = Slots(Bn)
    own = audio(fvad_mod, 77, 100 + total - cut)
    for s in range(5):  # unrelated audio first: the restore overwrites dirty state
        sb.assign(s, own if s == 1 else audio(fvad_mod, 90 + s, 100))
    sb.run([37, 37, 26])
    Bn.restore_streams(dst, blob, index=index)
    for d, a in moved.items():
        sb.assign(d, xs[a], pos=cut)
    rest = total - cut
    sb.run([37] * (rest // 37) + ([rest % 37] if rest % 37 else []))
    for d, a in moved.items():
        assert_oracle(full[a], sb.result(d), tick0=cut, what=(d, a))
        got = machines(Bn, d, 2)
        for mi in range(2):
            snap, rolling, segs = full[a]["mach"][mi]
            assert got[mi][0] == snap and got[mi][1] == rolling, (d, a, mi)
            assert got[mi][2] == segs[:8], (d, a, mi)  # (the target keeps the first seg_capacity)
    r1 = oracle_stream(fvad_mod, oracle_mod, own, 77)
    assert_oracle(r1, sb.result(1), what="slot 1")
    assert machines(Bn, 1, 2) == r1["mach"]


@pytest.mark.parametrize("fft_size,bins", [(1000, (2, 31)), (200, (0, 6))])
def test_migration_other_fft_sizes(fvad_mod, oracle_mod, fft_size, bins):
    """fft_size 1000: the k_ola / k_winmeta / k_fftb tail; 200: several windows per tick"""
    m = fvad_mod.Model(seed=1)
    total, cut = 600, 251
    xs = [audio(fvad_mod, i, total) for i in (3, 19, 12)]
    A = fvad_mod.Engine(m, 3, 2, max_ticks=50, fft_size=fft_size, bands=(bins,), want_denoised=True)
    A.attach_vadm()
    sa = Slots(A)
    for s in range(3):
        sa.assign(s, xs[s])
    sa.run([50] * 5 + [1])
    blob = A.save_streams([2, 0])
    assert cut * FRAME % fft_size != 0
    Bn = fvad_mod.Engine(m, 2, 2, max_ticks=37, fft_size=fft_size, bands=(bins,), want_denoised=True)
    Bn.attach_vadm(seg_capacity=16)
    sb = Slots(Bn)
    for s in range(2):
        sb.assign(s, audio(fvad_mod, 90 + s, 40))
    sb.run([37, 3])
    Bn.restore_streams([0, 1], blob)  # record 0 = A's slot 2, record 1 = A's slot 0
    sb.assign(0, xs[2], pos=cut)
    sb.assign(1, xs[0], pos=cut)
    rest = total - cut
    sb.run([37] * (rest // 37) + [rest % 37])
    assert sb.pos == [total, total]
    for d, a, sid in ((0, 2, 12), (1, 0, 3)):
        ref = oracle_stream(fvad_mod, oracle_mod, xs[a], sid, fft_size=fft_size, alt=False)
        assert_oracle(ref, sb.result(d), tick0=cut, fft_size=fft_size, what=(fft_size, d))
        assert Bn.vadm_snapshot(d) == ref["mach"][0][0], (fft_size, d)


# ---------------------------------------------------------------------------
# 4. use_denoiser = 0: the sample counter is not a multiple of 480 at the save
# ---------------------------------------------------------------------------
def test_migration_without_denoiser_mid_tick(fvad_mod, oracle_mod):
    m = fvad_mod.Model(seed=1)
    n = 4 * 48000
    xs = [fvad_mod.synth_stream(i, n, 2)[0] for i in (3, 19)]
    cut = 150 * FRAME + 133  # samples consumed before the save

    def feed(eng, slot_x, a, b, wins):
        """samples [a, b) of every slot's stream, the last tick partial"""
        B = eng.B
        for p0 in range(a, b, 50 * FRAME):
            p1 = min(b, p0 + 50 * FRAME)
            k = p1 - p0
            nt = (k + FRAME - 1) // FRAME
            pcm = np.zeros((nt, B, 2, FRAME), np.float32)
            for s, x in enumerate(slot_x):
                seg = np.zeros((2, nt * FRAME), np.float32)
                seg[:, :k] = x[:, p0:p1]
                pcm[:, s] = seg.reshape(2, nt, FRAME).transpose(1, 0, 2)
            o = eng.push(pcm, ticks_valid=np.full(B, nt, np.int32),
                         last_tick_samples=np.full(B, k - (nt - 1) * FRAME, np.int32))
            for s in range(B):
                wf = o["win_flag"][:, s].astype(bool)
                wins[s].append((o["band"][:, s][wf, :, 0], o["win_ratio"][:, s][wf]))

    A = fvad_mod.Engine(m, 2, 2, max_ticks=50, use_denoiser=False)
    A.attach_vadm()
    wa = [[], []]
    feed(A, xs, 0, cut, wa)
    blob = A.save_streams([0, 1])
    Bn = fvad_mod.Engine(m, 3, 2, max_ticks=64, use_denoiser=False)
    Bn.attach_vadm(seg_capacity=32)
    junk = fvad_mod.synth_stream(90, n, 2)[0]
    feed(Bn, [junk] * 3, 0, 700, [[], [], []])
    Bn.restore_streams([2, 0], blob)  # A's slot 0 -> slot 2, slot 1 -> slot 0
    wb = [[], [], []]
    # up to the last whole window, so that the oracle's count is the engine's
    end = n // 2048 * 2048
    feed(Bn, [xs[1], junk, xs[0]], cut, end, wb)
    for d, a in ((2, 0), (0, 1)):
        x = np.ascontiguousarray(xs[a][:, :end])
        ref = oracle_stream(fvad_mod, oracle_mod, x, ("nd", a), use_denoiser=False, alt=False)
        wi = ref["windows"]
        band = np.concatenate([b for b, _ in wa[a]] + [b for b, _ in wb[d]])
        ratio = np.concatenate([r for _, r in wa[a]] + [r for _, r in wb[d]])
        assert len(wi) == len(band) == end // 2048 and len(wa[a]) > 0
        assert np.array_equal(wi["band"][:, :2], band), d
        assert np.array_equal(wi["ratio"], ratio), d
        assert machines(Bn, d, 1) == ref["mach"], d


# ---------------------------------------------------------------------------
# 5. slot independence of the tolerance modes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32_fast", "fp16"])
def test_restore_into_other_slots_same_mode(fvad_mod, mode):
    m = fvad_mod.Model(seed=1)
    B, total, cut = 11, 300, 124
    xs = [audio(fvad_mod, 100 + s, total) for s in range(B)]

    def engine():
        e = fvad_mod.Engine(m, B, 2, max_ticks=37, want_denoised=True, mode=mode)
        e.attach_vadm()
        return e

    ctl = Slots(engine())
    for s in range(B):
        ctl.assign(s, xs[s])
    ctl.run([37, 37, 37, 13])
    for s in range(B):
        ctl.out[s] = []
    ctl.run([37] * 4 + [28])
    eng = engine()
    sl = Slots(eng)
    for s in range(B):
        sl.assign(s, xs[s])
    sl.run([37, 37, 37, 13])
    src, dst = [0, 3, 8, 10], [9, 7, 1, 4]  # across k_rnn3's groups of 8, both ways
    blob = eng.save_streams(src)
    eng.restore_streams(dst, blob)
    for s in range(B):
        sl.assign(s, xs[s], pos=cut)  # the other slots go on with their own streams
    for a, d in zip(src, dst):
        sl.assign(d, xs[a], pos=cut)
    sl.run([37] * 4 + [28])
    for a, d in zip(src, dst):
        assert_same(ctl.result(a), sl.result(d), (mode, a, d))
        assert machines(eng, d, 1) == machines(ctl.eng, a, 1), (mode, a, d)
    for s in set(range(B)) - set(dst):
        assert_same(ctl.result(s), sl.result(s), (mode, s))


# ---------------------------------------------------------------------------
# 6. blob and argument checks
# ---------------------------------------------------------------------------
def test_blob_and_argument_checks(fvad_mod):
    m = fvad_mod.Model(seed=1)
    B, total = 4, 150
    xs = [audio(fvad_mod, 100 + s, total) for s in range(B)]

    def engine(model=m, **kw):
        cfg = kw.pop("cfg", None)
        args = dict(max_ticks=50, want_denoised=True)
        args.update(kw)
        e = fvad_mod.Engine(model, B, args.pop("n_channels", 2), **args)
        if args.get("mode") != "fused":
            e.attach_vadm([cfg] if cfg is not None else None)
        return e

    ctl = Slots(engine())
    eng = engine()
    sl = Slots(eng)
    for s in range(B):
        ctl.assign(s, xs[s])
        sl.assign(s, xs[s])
    ctl.run([50])
    sl.run([50])
    blob = eng.save_streams([0, 1, 2, 3])
    eng.restore_streams([0, 1, 2, 3], blob)  # the identity
    step = [0]

    def next_push_equals_control():
        ctl.run([25])
        sl.run([25])
        step[0] += 1
        for s in range(B):
            assert_same(ctl.result(s), sl.result(s), (step[0], s))
            assert machines(eng, s, 1) == machines(ctl.eng, s, 1), (step[0], s)

    next_push_equals_control()

    def refused(code, ids, b, index=None, target=None):
        with pytest.raises(fvad_mod.FvadError) as ei:
            (target or eng).restore_streams(ids, b, index=index)
        assert ei.value.code == code, ei.value

    # blobs of engines that differ in one field
    slow = fvad_mod.VadmConfig.default()
    slow.max_speech_gap_sec += 0.25
    others = [dict(fft_size=1000, bands=((2, 31),)), dict(mode="f32_fast"), dict(model=fvad_mod.Model(seed=2)),
              dict(cfg=slow), dict(bands=BANDS2)]
    for kw in others:
        o = engine(**kw)
        o.push(np.zeros((5, B, 2, FRAME), np.float32))
        refused(fvad_mod.EFORMAT, [0, 1], o.save_streams([2, 3]))
    mono = fvad_mod.Engine(m, B, 1, max_ticks=50)
    mono.attach_vadm()
    refused(fvad_mod.EFORMAT, [0], mono.save_streams([0]))
    nomach = fvad_mod.Engine(m, B, 2, max_ticks=50)
    refused(fvad_mod.EFORMAT, [0], nomach.save_streams([0]))
    refused(fvad_mod.EFORMAT, [0], blob, target=nomach)
    # damaged blobs
    refused(fvad_mod.EFORMAT, [0, 1, 2, 3], blob[:-1])
    refused(fvad_mod.EFORMAT, [0], blob[:100])
    for off, val in ((0, 0x42535647), (4, 2), (8, 64)):  # magic, version, header_bytes
        bad = blob.copy()
        bad[off:off + 4] = np.frombuffer(np.uint32(val).tobytes(), np.uint8)
        refused(fvad_mod.EFORMAT, [0], bad)
    info = fvad_mod.stream_blob_info(blob)
    bad = blob.copy()  # a negative tick counter in record 1: only a restore that uses it refuses
    fd = 128 + info["stream_bytes"] + 4 * (1728 + 480 + 8 * 22 + 22 + 3 * 128 + 2 + 3)
    bad[fd:fd + 4] = np.frombuffer(np.int32(-480).tobytes(), np.uint8)
    refused(fvad_mod.EFORMAT, [0], bad, index=[1])
    # arguments
    refused(fvad_mod.EINVAL, [1, 1], blob)
    refused(fvad_mod.EINVAL, [0, B], blob)
    refused(fvad_mod.EINVAL, [-1], blob)
    refused(fvad_mod.EINVAL, [0], blob, index=[4])
    refused(fvad_mod.EINVAL, [0], blob, index=[-1])
    for ids in ([2, 2], [B], [-1]):
        with pytest.raises(fvad_mod.FvadError) as ei:
            eng.save_streams(ids)
        assert ei.value.code == fvad_mod.EINVAL
        with pytest.raises(fvad_mod.FvadError) as ei:
            eng.reset_streams(ids)
        assert ei.value.code == fvad_mod.EINVAL
    L, I32P = fvad_mod.lib(), fvad_mod.I32P
    ids = np.array([0, 1], np.int32)
    small = np.zeros(L.fvad_engine_save_size(eng.h, 2) - 1, np.uint8)
    assert L.fvad_engine_save_size(eng.h, 2) == 128 + 2 * info["stream_bytes"]
    assert L.fvad_engine_save_streams(eng.h, ids.ctypes.data_as(I32P), 2, small.ctypes.data, small.size) == fvad_mod.EINVAL
    assert not small.any()
    # n = 0
    assert L.fvad_engine_save_streams(eng.h, None, 0, None, 0) == 0
    assert L.fvad_engine_restore_streams(eng.h, None, 0, None, 0, None) == 0
    assert L.fvad_engine_reset_streams(eng.h, None, 0) == 0
    # nothing above touched the engine
    next_push_equals_control()
    # and the blob still restores: every slot back to tick 50, fed again from there
    eng.restore_streams([0, 1, 2, 3], bad, index=[0, 0, 2, 3])  # (record 1, the damaged one, is not used)
    for s, a in enumerate([0, 0, 2, 3]):
        sl.assign(s, xs[a], pos=50)
    sl.run([50])
    for s, a in enumerate([0, 0, 2, 3]):
        r = ctl.result(a)
        assert np.array_equal(r["vad"][50:100], sl.result(s)["vad"]), s
        assert np.array_equal(r["denoised"][:, 50 * FRAME:100 * FRAME], sl.result(s)["denoised"]), s
