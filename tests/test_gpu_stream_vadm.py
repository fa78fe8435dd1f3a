"""Per-stream VADMachine configs in the batched engine
(fvad_engine_attach_vadm_ex / fvad_engine_set_stream_vadm; DESIGN.md section
7, "Per-stream configs").  The oracle is the host fvad.VADMachine fed the
engine's own push outputs, a fresh machine per (stream, config) with window w
entering at sample index w * 2048 (test_gpu_vadm.py's host_segments); final
states are a host-only Sweep lane's snapshot.  The pipeline's outputs do not
depend on the machines, so each scene's pushes run once on a machine-less
engine (the scene fixtures), every test checks that its own engine returned
those outputs again, and the host references are computed once per scene."""
import ctypes as C

import numpy as np
import pytest

import sweep_util as su

pytestmark = pytest.mark.gpu

BANDS = ((4, 64), (13, 128))  # 100..1500 Hz (slot 0), 300..3000 Hz (slot 1)
FFT = 2048
OUT_KEYS = ("vad", "ratio", "win_flag", "win_ratio", "win_vad", "band")


def cfg(fvad, second_band=False, **kw):
    c = fvad.VadmConfig.default()
    if second_band:
        c.speech_min_freq, c.speech_max_freq = 300.0, 3000.0
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def quick(fvad, second_band=False, **kw):
    """test_gpu_events' configs: open after 0.1 s, close after 0.2 s, segments from
    0.3 s -- several speeches within a few seconds of a synthetic stream."""
    base = dict(min_consecutive_sec_to_open=0.1, max_speech_gap_sec=0.2, min_vad_duration_sec=0.3)
    base.update(kw)
    return cfg(fvad, second_band, **base)


def slot_of(c):
    return 1 if c.speech_min_freq == 300.0 else 0


def fields(c):
    return tuple(getattr(c, n) for n, _ in c._fields_)


def pushes_of(streams, chunk):
    """Ragged pushes of `chunk` ticks: [(pcm [nt][B][C][480], valid [B])]."""
    B, Ch = len(streams), streams[0].shape[0]
    lens = [x.shape[1] // 480 for x in streams]
    out = []
    for t0 in range(0, max(lens), chunk):
        nt = min(chunk, max(lens) - t0)
        pcm = np.zeros((nt, B, Ch, 480), np.float32)
        valid = np.zeros(B, np.int32)
        for s, x in enumerate(streams):
            v = max(0, min(nt, lens[s] - t0))
            valid[s] = v
            if v:
                pcm[:v, s] = x[:, t0 * 480:(t0 + v) * 480].reshape(Ch, v, 480).transpose(1, 0, 2)
        out.append((pcm, valid))
    return out


def windows_of(outs, s):
    """Stream s's completed windows over the pushes: band [W][C][bands], vad [W], ratio [W]."""
    band, vad, vr = [], [], []
    for o, valid in outs:
        v = valid[s]
        f = o["win_flag"][:v, s].astype(bool)
        band.append(o["band"][:v, s][f])
        vad.append(o["win_vad"][:v, s][f])
        vr.append(o["win_ratio"][:v, s][f])
    return np.concatenate(band), np.concatenate(vad), np.concatenate(vr)


def host_machine(fvad, wins, c, w_from=0, w_to=None, states=None):
    """A fresh host VADMachine of c over windows [w_from, w_to), window w at index
    w * 2048: its segments (states, a list: the speech state after every window)."""
    band, vad, vr = wins
    vm = fvad.VADMachine(c, n_channels=band.shape[1])
    slot = slot_of(c)
    for w in range(w_from, len(vr) if w_to is None else w_to):
        vm.run(w * FFT, band[w, :, slot], float(vad[w]), float(vr[w]))
        if states is not None:
            states.append(vm.state()[0])
    return vm.segments()


def host_snapshot(fvad, wins, c):
    band, vad, vr = wins
    sw = fvad.Sweep(1, band.shape[1], device=-1, bands=BANDS)
    sw.set_windows(0, band, vr, vad)
    sw.run([c])
    return sw.snapshot(0, 0)


class Scene:
    """Streams cut into pushes, and what a machine-less engine made of them."""

    def __init__(self, fvad, model, streams, chunk):
        self.fvad, self.model, self.chunk = fvad, model, chunk
        self.B, self.C = len(streams), streams[0].shape[0]
        self.pushes = pushes_of(streams, chunk)
        eng = self.engine()
        self.outs = [(eng.push(pcm, ticks_valid=valid), valid) for pcm, valid in self.pushes]
        self.wins = [windows_of(self.outs, s) for s in range(self.B)]
        self._segs, self._snaps = {}, {}

    def engine(self):
        return self.fvad.Engine(self.model, self.B, self.C, max_ticks=self.chunk, bands=BANDS)

    def run(self, eng, sync_each=False, after=None, upto=None):
        """The scene's pushes through eng, which must return the scene's outputs;
        after(k) runs behind push k."""
        for k, (pcm, valid) in enumerate(self.pushes[:upto]):
            o = eng.push(pcm, ticks_valid=valid)
            for key in OUT_KEYS:  # (a stream's rows past its valid ticks are not outputs)
                for s in range(self.B):
                    assert np.array_equal(o[key][:valid[s], s], self.outs[k][0][key][:valid[s], s]), (k, key, s)
            if sync_each:
                eng.sync()
            if after:
                after(k)

    def segs(self, s, c):
        key = (s, fields(c))
        if key not in self._segs:
            self._segs[key] = host_machine(self.fvad, self.wins[s], c)
        return self._segs[key]

    def snap(self, s, c):
        key = (s, fields(c))
        if key not in self._snaps:
            self._snaps[key] = host_snapshot(self.fvad, self.wins[s], c)
        return self._snaps[key]


@pytest.fixture(scope="module")
def model(fvad_mod):
    return fvad_mod.Model(seed=1)


# ---------------------------------------------------------------------------
# 1. parity with distinct rows
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene5(fvad_mod, model):
    ids, secs = [0, 4, 19, 42, 7], [40.0, 33.5, 25.0, 38.0, 12.0]
    return Scene(fvad_mod, model, [fvad_mod.synth_stream(i, int(48000 * s), 2)[0] for i, s in zip(ids, secs)], 64)


def rows5(fvad, no_init):
    """rows[m][s]: long-term 180 s, 10 s (234 entries: wraps) and 2 s (46 entries, not more
    than k_vadm_par's 48 windows: the in-kernel serial walk), other short-term and ratio
    lengths, threshold factors, minimum durations, and both band slots in each machine."""
    m0 = [cfg(fvad),
          cfg(fvad, True, long_term_speech_avg_sec=10.0, min_vad_duration_sec=0.3),
          cfg(fvad, long_term_speech_avg_sec=2.0, speech_threshold_factor=6.0, short_term_speech_avg_sec=0.5),
          cfg(fvad, True, speech_threshold_factor=40.0, channel_vol_ratio_avg_sec=1.0, min_vad_duration_sec=1.5),
          cfg(fvad, long_term_speech_avg_sec=10.0, speech_threshold_factor=8.0, min_vad_duration_sec=0.2)]
    m1 = [cfg(fvad, True, long_term_speech_avg_sec=10.0, min_vad_duration_sec=0.3),
          cfg(fvad, speech_threshold_factor=30.0, min_vad_duration_sec=1.2),
          cfg(fvad, True, long_term_speech_avg_sec=2.0, speech_threshold_factor=12.0),
          cfg(fvad, long_term_speech_avg_sec=10.0, short_term_speech_avg_sec=0.5, min_vad_duration_sec=0.4,
              has_initial_long_term_avg=0 if no_init else 1),
          cfg(fvad, True, speech_threshold_factor=9.0, channel_vol_ratio_avg_sec=0.25)]
    return [m0, m1]


@pytest.mark.parametrize("flavour", ["no_sync", "sync_each", "always_par_serial_2", "one_row_no_init", "defer_max_1",
                                     "bound_open"])
def test_distinct_rows_match_host(fvad_mod, scene5, flavour):
    """no_sync: k_vadm_hbm_ps between pushes, the last push's pass at the reader's sync
    point; sync_each: every push's pass at a sync point, k_vadm_par_ps (every row has an
    initial average); always_par_serial_2: k_vadm_par_ps for every push with every second
    stream on its in-kernel serial walk; one_row_no_init: a row without an initial
    average sends the sync points to k_vadm_hbm_ps; defer_max_1 / bound_open: the lazy
    walk's hooks, as in test_gpu_vadm.py."""
    fvad, sc = fvad_mod, scene5
    rows = rows5(fvad, flavour == "one_row_no_init")
    eng = sc.engine()
    eng.attach_vadm([cfg(fvad), cfg(fvad, True)], room=rows[0] + rows[1])
    for m in range(2):
        eng.set_stream_vadm(range(sc.B), rows[m], machine=m)
    if flavour == "always_par_serial_2":
        eng.set_debug(fvad.DEBUG_VADM_ALWAYS_PAR, 1)
        eng.set_debug(fvad.DEBUG_VADM_PAR_SERIAL_EVERY, 2)
    if flavour == "defer_max_1":
        eng.set_debug(fvad.DEBUG_VADM_DEFER_MAX, 1)
    if flavour == "bound_open":
        eng.set_debug(fvad.DEBUG_VADM_BOUND_SCALE, -1)
    if flavour in ("bound_open", "no_sync"):
        eng.set_debug(fvad.DEBUG_VADM_COUNT, 1)
    sc.run(eng, sync_each=flavour in ("sync_each", "one_row_no_init"))
    total, differ = 0, set()
    for s in range(sc.B):
        for m in range(2):
            ref = sc.segs(s, rows[m][s])
            got = eng.segments(s, m)
            assert got == ref, (s, m, got[:3], ref[:3])
            assert eng.vadm_snapshot(s, m) == sc.snap(s, rows[m][s]), (s, m)
            assert fields(eng.stream_vadm_config(s, m)) == fields(rows[m][s]), (s, m)
            total += len(ref)
            if s and ref != sc.segs(s, rows[m][0]):  # an engine that ran stream 0's row everywhere differs here
                differ.add(s)
    print(flavour, "segments", total, "streams that need their own row", sorted(differ))
    assert total > 0
    assert len(differ) >= 2, differ
    kt = eng.kernel_times()["kernels"]
    print({k: v for k, v in kt.items() if k.startswith("k_vadm")})
    assert "k_vadm_hbm_ps" in kt and "k_vadm_par_ps" in kt and "k_vadm_hbm" not in kt, sorted(kt)
    if flavour in ("sync_each", "always_par_serial_2"):
        assert kt["k_vadm_par_ps"] > 0 and kt["k_vadm_hbm_ps"] == 0, kt
    if flavour == "one_row_no_init":
        assert kt["k_vadm_hbm_ps"] > 0 and kt["k_vadm_par_ps"] == 0, kt
    if flavour == "bound_open":
        cnt = eng.debug_counts()
        assert cnt["open"] > 0 and cnt["settled"] == 0, cnt
    if flavour == "no_sync":
        # the lazy walk ran, so k_vadm_hbm_ps did between the pushes: the reader's k_vadm_par_ps
        # pass has stream 0 alone, both machines window-parallel, which counts nothing
        cnt = eng.debug_counts()
        assert cnt["settled"] > 0, cnt


# ---------------------------------------------------------------------------
# 2. identical rows equal the plain engine
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene5s(fvad_mod, model):
    ids, secs = [0, 4, 19, 42, 7], [25.0, 20.5, 14.0, 22.0, 9.0]
    return Scene(fvad_mod, model, [fvad_mod.synth_stream(i, int(48000 * s), 2)[0] for i, s in zip(ids, secs)], 64)


@pytest.mark.parametrize("sync_each", [False, True])
def test_identical_rows_equal_plain_engine(fvad_mod, scene5s, sync_each):
    fvad, sc = fvad_mod, scene5s
    cfgs = [cfg(fvad), cfg(fvad, True, long_term_speech_avg_sec=10.0, min_vad_duration_sec=0.3)]
    plain, ex = sc.engine(), sc.engine()
    plain.attach_vadm(cfgs)
    ex.attach_vadm(cfgs, room=[])
    sc.run(plain, sync_each)
    sc.run(ex, sync_each)
    assert "k_vadm_hbm" in plain.kernel_times()["kernels"] and "k_vadm_hbm_ps" in ex.kernel_times()["kernels"]
    total = 0
    for s in range(sc.B):
        for m in range(2):
            a, b = plain.segments(s, m), ex.segments(s, m)
            assert a == b and [su.bits(x[2:]) for x in a] == [su.bits(x[2:]) for x in b], (s, m)
            sa, sb = plain.vadm_snapshot(s, m), ex.vadm_snapshot(s, m)
            assert sa == sb and su.bits(sa["avg"]) == su.bits(sb["avg"]), (s, m, sa, sb)
            for which in range(3):
                ra, rb = plain.vadm_rolling(s, which, m), ex.vadm_rolling(s, which, m)
                assert ra.shape == rb.shape and su.bits(ra) == su.bits(rb), (s, m, which)
            total += len(a)
    assert total > 0


# ---------------------------------------------------------------------------
# 3. retarget between pushes
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene6(fvad_mod, model):
    ids = [0, 3, 19, 39, 7, 12]
    return Scene(fvad_mod, model, [fvad_mod.synth_stream(i, int(48000 * 30.0), 2)[0] for i in ids], 50)


RETARGETED = (1, 2, 4)


def scene6_cfgs(fvad):
    old = [quick(fvad), quick(fvad, True)]
    # what streams 1, 2 and 4 move to, per machine: another band slot, a 10 s and a 2 s
    # long-term buffer, other thresholds
    new = [[quick(fvad, True, long_term_speech_avg_sec=10.0, speech_threshold_factor=10.0),
            quick(fvad, long_term_speech_avg_sec=2.0, speech_threshold_factor=8.0, min_vad_duration_sec=0.2),
            quick(fvad, speech_threshold_factor=30.0, short_term_speech_avg_sec=0.5)],
           [quick(fvad, long_term_speech_avg_sec=10.0, speech_threshold_factor=25.0),
            quick(fvad, True, speech_threshold_factor=9.0, min_vad_duration_sec=0.5),
            quick(fvad, True, long_term_speech_avg_sec=2.0, channel_vol_ratio_avg_sec=0.25)]]
    return old, new


def push_with_speech_in_progress(sc, c):
    """The first push k >= 10 (not the last) after which, under c, a retargeted stream's
    machine is Open or Closing; the windows each stream has done by then."""
    done = np.cumsum([[int(o["win_flag"][:valid[s], s].sum()) for s in range(sc.B)] for o, valid in sc.outs], axis=0)
    states = {}
    for s in RETARGETED:
        states[s] = []
        host_machine(sc.fvad, sc.wins[s], c, states=states[s])
    for k in range(10, len(sc.outs) - 10):
        if any(done[k][s] and states[s][done[k][s] - 1] in (2, 3) for s in RETARGETED):
            return k, done[k]
    raise AssertionError("no push leaves a retargeted stream in a speech")


@pytest.mark.parametrize("flavour", ["no_sync", "snapshot_before"])
def test_retarget_between_pushes(fvad_mod, scene6, flavour):
    """no_sync: nothing waits for the device from the first push to the readers at the
    end, the feed on; snapshot_before: a vadm_snapshot right before the call shows a
    retargeted machine in a speech (abandoned: no segment, no SEGMENT event), clip
    capture on as well."""
    fvad, sc = fvad_mod, scene6
    old, new = scene6_cfgs(fvad)
    k, done = push_with_speech_in_progress(sc, old[0])
    eng = sc.engine()
    eng.attach_vadm(old, room=new[0] + new[1])
    eng.enable_events()
    if flavour == "snapshot_before":
        eng.enable_capture(0, 14.0, 8 << 20)

    def after(p):
        if p != k:
            return
        if flavour == "snapshot_before":
            st = [eng.vadm_snapshot(s, 0) for s in RETARGETED]
            assert [x["windows"] for x in st] == [done[s] for s in RETARGETED]
            assert any(x["speech_state"] in (2, 3) for x in st), st
        for m in range(2):
            eng.set_stream_vadm(RETARGETED, new[m], machine=m)

    sc.run(eng, after=after)
    expect = {}
    for s in range(sc.B):
        for m in range(2):
            if s in RETARGETED:
                w0 = int(done[s])
                expect[s, m] = host_machine(fvad, sc.wins[s], old[m], 0, w0) + \
                    host_machine(fvad, sc.wins[s], new[m][RETARGETED.index(s)], w0)
            else:
                expect[s, m] = sc.segs(s, old[m])  # a run that never retargets
            assert eng.segments(s, m) == expect[s, m], (s, m)
            want = new[m][RETARGETED.index(s)] if s in RETARGETED else old[m]
            assert fields(eng.stream_vadm_config(s, m)) == fields(want)
    assert sum(len(v) for v in expect.values()) > 0
    # the abandoned speech: the old machine alone would have gone on to a segment there
    assert any(expect[s, 0] != sc.segs(s, old[0]) for s in RETARGETED)
    eng.sync()
    events = []
    while True:
        ev, lost = eng.poll_events(4096)
        assert lost == 0
        events += ev
        if not ev:
            break
    for (s, m), segs in expect.items():
        got = [e for e in events if e["kind"] == fvad.EVENT_SEGMENT and e["stream"] == s and e["machine"] == m]
        assert [e["seq"] for e in got] == list(range(len(segs))), (s, m)
        assert [(e["sample_from"], e["sample_to"], e["debug_rnn_vad"], e["debug_avg_speech_vol_ratio"])
                for e in got] == segs, (s, m)
    if flavour == "snapshot_before":
        clips = eng.poll_clips()
        assert clips
        for d, _ in clips:
            assert (d["sample_from"], d["sample_to"]) in {(g[0], g[1]) for g in expect[d["stream"], 0]}, d


# ---------------------------------------------------------------------------
# 4. more rows than one launch carries, and more than kListMax
# ---------------------------------------------------------------------------
def test_retarget_260_streams_in_one_call(fvad_mod, model):
    fvad, B, T = fvad_mod, 260, 50
    eng = fvad.Engine(model, B, 1, max_ticks=T, bands=BANDS)
    eng.attach_vadm([cfg(fvad)], room=[])
    rows = [quick(fvad, s % 3 == 1, min_vad_duration_sec=0.1 + 0.01 * (s % 40), speech_threshold_factor=4.0 + s % 23)
            for s in range(B)]
    ids = [(s * 7) % B for s in range(B)]  # not in order: 7 and 260 are coprime
    eng.set_stream_vadm(ids, [rows[s] for s in ids])
    outs = []
    for p in range(4):
        pcm = fvad.synth_ticks(0, B, 1, 4 * T, tick0=p * T, n_ticks=T)
        outs.append((eng.push(pcm), np.full(B, T, np.int32)))
    total = 0
    for s in range(B):
        assert fields(eng.stream_vadm_config(s)) == fields(rows[s]), s
        states = []
        ref = host_machine(fvad, windows_of(outs, s), rows[s], states=states)
        assert eng.segments(s) == ref, s
        total += len(ref)
    snap = eng.vadm_snapshot(B - 1)
    assert snap["windows"] == len(states) and snap["speech_state"] == states[-1]
    print("segments over 260 streams:", total)


# ---------------------------------------------------------------------------
# 5. resets
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene4(fvad_mod, model):
    ids = [0, 19, 7, 12]
    return Scene(fvad_mod, model, [fvad_mod.synth_stream(i, int(48000 * 12.0), 2)[0] for i in ids], 50)


def test_resets_keep_the_rows(fvad_mod, scene4):
    fvad, sc = fvad_mod, scene4
    old = [quick(fvad)]
    rows = {1: quick(fvad, True, long_term_speech_avg_sec=10.0, speech_threshold_factor=10.0),
            2: quick(fvad, long_term_speech_avg_sec=2.0, speech_threshold_factor=8.0)}
    eng = sc.engine()
    eng.attach_vadm(old, room=list(rows.values()))
    sc.run(eng, upto=6)
    eng.set_stream_vadm(list(rows), list(rows.values()))
    for pcm, valid in sc.pushes[6:]:
        eng.push(pcm, ticks_valid=valid)
    now = [rows.get(s, old[0]) for s in range(sc.B)]
    # stream 1 alone starts again and is replayed from its start
    eng.reset_streams([1])
    others = eng.segments(0), eng.segments(2), eng.segments(3)
    for pcm, valid in sc.pushes:
        only = np.where(np.arange(sc.B) == 1, valid, 0).astype(np.int32)
        eng.push(pcm, ticks_valid=only)
    assert eng.segments(1) == sc.segs(1, now[1])
    assert eng.vadm_snapshot(1) == sc.snap(1, now[1])
    assert (eng.segments(0), eng.segments(2), eng.segments(3)) == others
    assert fields(eng.stream_vadm_config(1)) == fields(now[1])
    # fvad_engine_reset: every stream a fresh machine of its current config
    eng.reset()
    sc.run(eng)
    total = 0
    for s in range(sc.B):
        assert eng.segments(s) == sc.segs(s, now[s]), s
        assert eng.vadm_snapshot(s) == sc.snap(s, now[s]), s
        total += len(sc.segs(s, now[s]))
    assert total > 0
    assert any(sc.segs(s, now[s]) != sc.segs(s, old[0]) for s in rows)


# ---------------------------------------------------------------------------
# 6. closing the loop: sweep, pick per stream, serve
# ---------------------------------------------------------------------------
def test_sweep_pick_served_per_stream(fvad_mod, scene4):
    fvad, sc = fvad_mod, scene4
    cfgs = [quick(fvad, i % 2 == 1, long_term_speech_avg_sec=(180.0, 10.0, 2.0, 60.0)[i % 4],
                  speech_threshold_factor=(18.0, 6.0, 30.0, 10.0, 14.0, 4.0, 22.0, 8.0)[i],
                  min_vad_duration_sec=0.2 + 0.05 * i) for i in range(8)]
    sw = fvad.Sweep(sc.B, sc.C, device=0, bands=BANDS)
    for o, valid in sc.outs:  # an engine's pushes
        sw.append_outputs(o, valid)
    sw.run(cfgs)
    pick = [(7 * s + 3) % 8 for s in range(sc.B)]
    eng = sc.engine()
    eng.attach_vadm([cfgs[0]], room=cfgs)
    eng.set_stream_vadm(range(sc.B), [cfgs[p] for p in pick])
    sc.run(eng)
    total = 0
    for s in range(sc.B):
        n, segs = sw.segments(s, pick[s])
        assert n == len(segs) and eng.segments(s) == segs, (s, pick[s])
        assert eng.vadm_snapshot(s) == sw.snapshot(s, pick[s]), (s, pick[s])
        total += n
    assert total > 0


# ---------------------------------------------------------------------------
# 7. refusals leave the engine as it was
# ---------------------------------------------------------------------------
def refused(fvad, call, needle=None):
    with pytest.raises(fvad.FvadError) as ei:
        call()
    assert ei.value.code == fvad.EINVAL, ei.value
    if needle:
        for n in needle:
            assert n in str(ei.value), (n, str(ei.value))


def test_refusals_leave_the_engine_as_it_was(fvad_mod, scene4):
    fvad, sc = fvad_mod, scene4
    base = quick(fvad)
    small = quick(fvad, long_term_speech_avg_sec=10.0)  # the room: 234 long-term entries
    other = quick(fvad, True, long_term_speech_avg_sec=10.0, speech_threshold_factor=9.0)

    def check(eng, rows, first=0):
        """the scene's pushes from `first` on give the host's segments"""
        for pcm, valid in sc.pushes[first:]:
            eng.push(pcm, ticks_valid=valid)
        for s in range(sc.B):
            assert eng.segments(s) == sc.segs(s, rows[s]), s
            assert eng.vadm_snapshot(s) == sc.snap(s, rows[s]), s

    # a plain engine
    plain = sc.engine()
    plain.attach_vadm([base])
    sc.run(plain, upto=3)
    refused(fvad, lambda: plain.set_stream_vadm([0], [other]), ["fvad_engine_attach_vadm_ex"])
    check(plain, [base] * sc.B, 3)
    # an engine with room for 10 s, every stream on `small` but stream 2 on `other`
    eng = sc.engine()
    eng.attach_vadm([small], room=[])
    eng.set_stream_vadm([2], [other])
    rows = [small, small, other, small]
    sc.run(eng, upto=3)  # the refusals come with a machine pass pending
    refused(fvad, lambda: eng.set_stream_vadm([1, 3], [other, base]), ["stream 3", "long-term", "4218", "234"])
    refused(fvad, lambda: eng.set_stream_vadm([1, 3], [other, quick(fvad, long_term_speech_avg_sec=10.0,
                                                                    short_term_speech_avg_sec=0.5)]),
            ["stream 3", "short-term", "11", "4"])
    outside = quick(fvad, long_term_speech_avg_sec=10.0)
    outside.speech_min_freq, outside.speech_max_freq = 500.0, 2000.0
    refused(fvad, lambda: eng.set_stream_vadm([1, 3], [other, outside]), ["stream 3", "band"])
    refused(fvad, lambda: eng.set_stream_vadm([1, 1], [other, other]), ["duplicate"])
    refused(fvad, lambda: eng.set_stream_vadm([1, sc.B], [other, other]), ["out of range"])
    refused(fvad, lambda: eng.set_stream_vadm([-1], [other]), ["out of range"])
    refused(fvad, lambda: eng.set_stream_vadm([1], [other], machine=1))
    refused(fvad, lambda: eng.set_stream_vadm([1], [other], machine=-1))
    eng.set_stream_vadm([], [])  # n == 0: FVAD_OK
    for s in range(sc.B):
        assert fields(eng.stream_vadm_config(s)) == fields(rows[s]), s
    check(eng, rows, 3)
    # under FVAD_DEBUG_VADM_LT_FULL (a timing hook: setting and clearing it restarts the machines)
    eng.reset()
    eng.set_debug(fvad.DEBUG_VADM_LT_FULL, 1)
    refused(fvad, lambda: eng.set_stream_vadm([1], [other]), ["LT_FULL"])
    eng.set_debug(fvad.DEBUG_VADM_LT_FULL, 0)
    assert fields(eng.stream_vadm_config(1)) == fields(small)
    check(eng, rows)


def test_save_restore_refused_with_per_stream_configs(fvad_mod, scene4):
    fvad, sc = fvad_mod, scene4
    plain, ex = sc.engine(), sc.engine()
    plain.attach_vadm([quick(fvad)])
    ex.attach_vadm([quick(fvad)], room=[])
    sc.run(plain, upto=8)
    sc.run(ex, upto=8)
    blob = plain.save_streams([0, 2])  # works as before on a plain engine
    assert fvad.stream_blob_info(blob)["count"] == 2
    refused(fvad, lambda: ex.save_streams([0, 2]), ["fvad_engine_attach_vadm_ex"])
    refused(fvad, lambda: ex.restore_streams([0, 2], blob), ["fvad_engine_attach_vadm_ex"])
    # a plain engine takes its streams back where they were and goes on; the
    # refused engine goes on as if nothing had been asked
    plain.reset_streams([0, 2])
    plain.restore_streams([0, 2], blob)
    for eng in (plain, ex):
        for pcm, valid in sc.pushes[8:]:
            eng.push(pcm, ticks_valid=valid)
        for s in range(sc.B):
            assert eng.segments(s) == sc.segs(s, quick(fvad)), s
