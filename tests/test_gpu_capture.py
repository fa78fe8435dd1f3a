"""Clip capture (fvad_engine_enable_capture / poll_clip / capture_flush;
csrc/fvad_capture.hip) on the GPU.

Workload W: streams 0..7 of parity_util.make_streams, stereo, 14 s, in seven
pushes of 200 ticks, Model(seed=1), bands ((4, 64), (13, 128)), the two machine
configs of test_gpu_events.make_cfgs (restated here), capture on machine 0.

The expected list of a run is built by `Sim`, a direct model of the contract
in include/fvad.h, from three things only: the engine's own machine-0 SEGMENT
events (which test_gpu_events.py checks), the samples each stream holds at the
end of every push, and the input.  The completing push comes from sample_to
and the counts, the channel from oracle.recording_channel over the delivered
range, the audio from the input array.  Every field is compared exactly and
every sample bit for bit."""
import ctypes as C
import types

import numpy as np
import pytest

import parity_util as pu

pytestmark = pytest.mark.gpu

B, CH, SECS, T = 8, 2, 14.0, 200
NP = int(SECS * 100) // T  # 7 pushes
PUSH = T * 480             # samples of a stream in a push
BANDS = ((4, 64), (13, 128))
HIST = 14.0
POOL = 8 << 20
EINVAL = -1
HEAD, TAIL, NOAUDIO = 1, 2, 4


def make_cfgs(mod):
    """test_gpu_events.make_cfgs: the default config opening after 0.1 s, closing
    after 0.2 s, segments from 0.3 s; the same on 300-3000 Hz."""
    out = []
    for band in (None, (300.0, 3000.0)):
        c = mod.VadmConfig.default()
        c.min_consecutive_sec_to_open = 0.1
        c.max_speech_gap_sec = 0.2
        c.min_vad_duration_sec = 0.3
        if band:
            c.speech_min_freq, c.speech_max_freq = band
        out.append(c)
    return out


def new_engine(fvad, model, n_streams=B, mode="staged", capture=True, history=HIST, pool=POOL):
    eng = fvad.Engine(model, n_streams, CH, max_ticks=T, bands=BANDS, mode=mode)
    eng.attach_vadm(make_cfgs(fvad))
    eng.enable_events()
    if capture:
        eng.enable_capture(0, history, pool)
    return eng


def drain_events(eng):
    got = []
    while True:
        ev, lost = eng.poll_events(4096)
        assert lost == 0
        got += ev
        if not ev:
            return got


def seg0(events):
    """Machine 0's SEGMENT events, in feed order."""
    return [e for e in events if e["kind"] == 2 and e["machine"] == 0]


def split_pushes(x):
    """[streams][CH][n] -> NP arrays [T][streams][CH][480]."""
    n = x.shape[0]
    return [np.ascontiguousarray(x[:, :, p * PUSH:(p + 1) * PUSH].reshape(n, CH, T, 480).transpose(2, 0, 1, 3))
            for p in range(NP)]


class Sim:
    """The contract, step by step: pass_(p, events, counts) after push p,
    flush(streams, counts), read() when the host has polled everything,
    drop(s) for a reset or restored stream.  audio(s) -> [CH][n] indexed by the
    stream's own sample index; base[s]: its first held sample."""

    def __init__(self, oracle, n_streams, audio, history=HIST, pool_cap=None):
        self.oracle, self.audio = oracle, audio
        self.hist = int(np.floor(48000 * history))
        self.pend = {s: [] for s in range(n_streams)}
        self.base = {s: 0 for s in range(n_streams)}
        self.pool_cap, self.pool_wr, self.pool_rd = pool_cap, 0, 0
        self.lost = 0
        self.out = []  # (descriptor dict, samples)

    def _cut(self, e, p, n_now):
        s = e["stream"]
        lo = max(self.base[s], n_now - min(n_now, self.hist))
        first, end = max(e["sample_from"], lo), min(e["sample_to"], n_now)
        flags = (HEAD if e["sample_from"] < lo else 0) | (TAIL if e["sample_to"] > n_now else 0)
        n = max(0, end - first)
        if n == 0:
            flags |= NOAUDIO
            first = min(first, n_now)
        return dict(stream=s, seq=e["seq"], channel=-1, flags=flags, push=p, sample_from=e["sample_from"],
                    sample_to=e["sample_to"], first_sample=first, n_samples=n, reserved=0)

    def _place(self, due):
        room = self.pool_cap - (self.pool_wr - self.pool_rd) if self.pool_cap else None
        before = 0
        for d in due:
            want = d["n_samples"]
            if want and room is not None and before + want > room:
                d["n_samples"] = 0
                d["flags"] |= NOAUDIO
            if d["n_samples"] == 0:
                self.lost += 1
                pcm = np.zeros(0, np.float32)
            else:
                a = self.audio(d["stream"])[:, d["first_sample"]:d["first_sample"] + want]
                assert a.shape[1] == want
                d["channel"] = self.oracle.recording_channel([a[c] for c in range(a.shape[0])])
                pcm = np.array(a[d["channel"]], np.float32)
                self.pool_wr += want
            before += want
            self.out.append((d, pcm))

    def pass_(self, p, events, counts):
        for e in events:
            if e["push"] != p:
                continue
            q = self.pend[e["stream"]]
            if len(q) < 4:
                q.append(e)
            else:
                self.lost += 1
        due = []
        for s in sorted(self.pend):
            keep = []
            for e in self.pend[s]:
                if e["sample_to"] <= counts[s]:
                    due.append(self._cut(e, p, counts[s]))
                else:
                    keep.append(e)
            self.pend[s] = keep
        self._place(due)

    def flush(self, streams, p, counts):
        due = []
        for s in sorted(self.pend):
            if streams is None or s in streams:
                due += [self._cut(e, p, counts[s]) for e in self.pend[s]]
                self.pend[s] = []
        self._place(due)

    def read(self):
        self.pool_rd = self.pool_wr

    def drop(self, s, base):
        self.pend[s] = []
        self.base[s] = base


def even_counts(n_streams=B):
    return [[(p + 1) * PUSH] * n_streams for p in range(NP)]


def expected_w(oracle, events, audio, history=HIST, n_streams=B):
    """W's list: seven passes, then a flush of every stream.  (clips, how many before the flush)"""
    sim = Sim(oracle, n_streams, audio, history)
    counts = even_counts(n_streams)
    for p in range(NP):
        sim.pass_(p, events, counts[p])
    k = len(sim.out)
    sim.flush(None, NP - 1, counts[-1])
    return sim.out, k


def same_clip(got, want):
    return got[0] == want[0] and got[1].dtype == np.float32 and got[1].shape == want[1].shape and \
        np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def assert_clips(got, want, what=""):
    for i, (g, e) in enumerate(zip(got, want)):
        assert g[0] == e[0], (what, i, g[0], e[0])
        assert same_clip(g, e), (what, i, g[0], "samples differ")
    assert len(got) == len(want), (what, len(got), len(want))


def check_not_vacuous(clips, events):
    """The expected list exercises what the tests are about."""
    produced = {(e["stream"], e["seq"]): e["push"] for e in events}
    d = [c[0] for c in clips]
    assert len(d) >= 8
    assert {c["channel"] for c in d if c["n_samples"]} == {0, 1}
    assert any(c["push"] == produced[(c["stream"], c["seq"])] and not c["flags"] & TAIL for c in d)
    assert any(c["push"] > produced[(c["stream"], c["seq"])] for c in d)
    assert any(c["flags"] & TAIL for c in d)
    assert any(c["sample_from"] == 0 for c in d)


@pytest.fixture(scope="module")
def world(fvad_mod, oracle_mod):
    fvad = fvad_mod
    model = fvad.Model(seed=1)
    streams, _ = pu.make_streams(fvad, list(range(B)), SECS)
    x = np.stack(streams)  # [B][CH][n]
    pcm = split_pushes(x)
    for a in pcm:
        a.setflags(write=False)
    twin = new_engine(fvad, model, capture=False)  # events, no capture: the reference outputs and feed
    outs = [twin.push(a) for a in pcm]
    twin.sync()
    events = drain_events(twin)
    segs = seg0(events)
    clips, k = expected_w(oracle_mod, segs, lambda s: x[s])
    print("W: %d machine-0 segments; clips %s" % (len(segs), [(c["stream"], c["seq"], c["push"], c["flags"], c["channel"],
                                                                c["first_sample"], c["n_samples"]) for c, _ in clips]))
    return types.SimpleNamespace(fvad=fvad, oracle=oracle_mod, model=model, x=x, pcm=pcm, outs=outs, events=events,
                                 segs=segs, clips=clips, before_flush=k)


def same_outputs(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("vad", "ratio", "win_flag", "win_ratio", "win_vad", "band"))


def test_sync_pushes_poll_each(world):
    """Case 1: a poll after every synchronous push delivers a prefix; after sync
    everything completed; capture_flush the rest, TAIL_SHORT.  Keyed by (stream,
    seq) the clips are oracle.recordings of the oracle pipeline's segments; the
    outputs and the event feed are a twin engine's without capture."""
    w, fvad, oracle = world, world.fvad, world.oracle
    check_not_vacuous(w.clips, w.segs)
    eng = new_engine(fvad, w.model)
    got, events = [], []
    for p in range(NP):
        assert same_outputs(eng.push(w.pcm[p]), w.outs[p]), p
        got += eng.poll_clips()
        events += eng.poll_events()[0]
        assert_clips(got, w.clips[:len(got)], "push %d" % p)
        assert all(c["push"] < p for c, _ in got), p  # push p's pass is not even enqueued yet
    eng.sync()
    got += eng.poll_clips()
    assert_clips(got, w.clips[:w.before_flush], "after sync")
    eng.capture_flush()
    got += eng.poll_clips()
    assert_clips(got, w.clips, "after flush")
    assert eng.capture_lost() == 0 and eng.poll_clips() == []
    assert all(c["flags"] == TAIL for c, _ in got[w.before_flush:]) and len(got) > w.before_flush
    assert events + drain_events(eng) == w.events
    # the reference's recorder over the oracle pipeline's own segments
    om = oracle.Model(seed=1)
    cfg = make_cfgs(oracle)[0]
    ref = {}
    for s in range(B):
        p = oracle.Pipeline(CH, om, main_cfg=cfg)
        for k in range(0, w.x.shape[2], 48000):
            p.push([w.x[s, 0, k:k + 48000], w.x[s, 1, k:k + 48000]])
        for seq, (start, ch, a) in enumerate(oracle.recordings([w.x[s, 0], w.x[s, 1]], p.segments())):
            ref[(s, seq)] = (start, ch, a)
    mine = {(c["stream"], c["seq"]): (c["first_sample"], c["channel"], a) for c, a in got}
    assert sorted(mine) == sorted(ref) and len(ref) == 11
    for key, (start, ch, a) in ref.items():
        assert mine[key][:2] == (start, ch), key
        assert np.array_equal(mine[key][2].view(np.uint32), a.view(np.uint32)), key


def test_ragged_pushes(world):
    """Case 2: stream 3 gets no tick in push 2, stream 5 gets 137 of 200 in
    push 1; each stream consumes its own audio in order, and clips are cut from
    that."""
    w, fvad = world, world.fvad
    check_not_vacuous(w.clips, w.segs)
    valid = np.full((NP, B), T, np.int32)
    valid[2, 3], valid[1, 5] = 0, 137
    eng = new_engine(fvad, w.model)
    at = np.zeros(B, np.int64)  # ticks consumed
    counts = []
    for p in range(NP):
        a = np.zeros((T, B, CH, 480), np.float32)
        for s in range(B):
            v = valid[p, s]
            a[:v, s] = w.x[s, :, at[s] * 480:(at[s] + v) * 480].reshape(CH, v, 480).transpose(1, 0, 2)
            at[s] += v
        eng.push(a, ticks_valid=valid[p])
        counts.append([int(t) * 480 for t in at])
    eng.sync()
    got = eng.poll_clips()
    eng.capture_flush()
    got += eng.poll_clips()
    segs = seg0(drain_events(eng))
    sim = Sim(w.oracle, B, lambda s: w.x[s])
    for p in range(NP):
        sim.pass_(p, segs, counts[p])
    sim.flush(None, NP - 1, counts[-1])
    check_not_vacuous(sim.out, segs)
    assert any(c["stream"] == 3 for c, _ in sim.out) and any(c["stream"] == 5 for c, _ in sim.out)
    assert_clips(got, sim.out)
    assert eng.capture_lost() == 0


def test_short_history(world):
    """Case 3: history_sec = 6: whole clips and HEAD_SHORT clips, the latter
    starting 288 000 samples before the completing push's end."""
    w, fvad = world, world.fvad
    check_not_vacuous(w.clips, w.segs)
    want, _ = expected_w(w.oracle, w.segs, lambda s: w.x[s], history=6.0)
    short = [c for c, _ in want if c["flags"] & HEAD]
    assert short and any(c["flags"] == 0 for c, _ in want)
    for c in short:
        assert c["first_sample"] == (c["push"] + 1) * PUSH - 288000 > c["sample_from"]
    eng = new_engine(fvad, w.model, history=6.0)
    for p in range(NP):
        eng.push(w.pcm[p])
    eng.sync()
    got = eng.poll_clips()
    eng.capture_flush()
    got += eng.poll_clips()
    assert seg0(drain_events(eng)) == w.segs
    assert_clips(got, want)


@pytest.mark.parametrize("poll_each", [False, True])
@pytest.mark.parametrize("schedule", ["in_flight", "resident"])
def test_schedules_give_the_same_list(world, schedule, poll_each):
    """Case 4: submit / collect with three pushes in flight, and seven
    run_resident calls over load_synthetic_ex(200, 7) with no sync: case 1's list
    exactly, polled once at the end or after every push."""
    w, fvad = world, world.fvad
    check_not_vacuous(w.clips, w.segs)
    eng = new_engine(fvad, w.model)
    if schedule == "resident":
        eng.load_synthetic(T, base=0, pushes=NP)
    got = []
    for p in range(NP):
        if schedule == "resident":
            eng.run_resident(T)
        else:
            eng.submit(w.pcm[p])
            if p >= 2:
                eng.collect(want=False)
        if poll_each:
            got += eng.poll_clips()
            assert_clips(got, w.clips[:len(got)], "push %d" % p)
    if schedule == "in_flight":
        eng.collect(want=False)
        eng.collect(want=False)
    eng.sync()
    got += eng.poll_clips()
    assert_clips(got, w.clips[:w.before_flush], "after sync")
    eng.capture_flush()
    got += eng.poll_clips()
    assert_clips(got, w.clips)
    assert drain_events(eng) == w.events and eng.capture_lost() == 0


def test_submit_i16_equals_float(world):
    """Case 5: submit_i16 of the streams quantised to 16 bits gives the clips of
    a float engine fed k / 32768, which are the model's over that input."""
    w, fvad = world, world.fvad
    check_not_vacuous(w.clips, w.segs)
    q = np.clip(np.rint(w.x * 32768.0), -32768, 32767).astype(np.int16)
    xf = (q.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    runs = []
    for pcm, sub in ((split_pushes(q), "submit_i16"), (split_pushes(xf), "submit")):
        eng = new_engine(fvad, w.model)
        for p in range(NP):
            getattr(eng, sub)(pcm[p])
            eng.collect(want=False)
        eng.sync()
        got = eng.poll_clips()
        eng.capture_flush()
        runs.append((got + eng.poll_clips(), seg0(drain_events(eng))))
    (a, ea), (b, eb) = runs
    assert ea == eb
    want, _ = expected_w(w.oracle, eb, lambda s: xf[s])
    check_not_vacuous(want, eb)
    assert_clips(b, want, "float")
    assert_clips(a, want, "i16")


def test_pool_overflow(world):
    """Case 6: a pool of 600 000 samples and no poll until the end: the clips
    that fit are intact, the newest are NO_AUDIO and counted, nothing unread is
    overwritten; after polling, a later pass (the flush) has room again."""
    w, fvad = world, world.fvad
    check_not_vacuous(w.clips, w.segs)
    sim = Sim(w.oracle, B, lambda s: w.x[s], pool_cap=600000)
    counts = even_counts()
    for p in range(NP):
        sim.pass_(p, w.segs, counts[p])
    k = len(sim.out)
    sim.read()
    sim.flush(None, NP - 1, counts[-1])
    want = sim.out
    kept = [c for c, _ in want[:k] if c["n_samples"]]
    lost = [c for c, _ in want[:k] if c["flags"] & NOAUDIO]
    assert kept and len(lost) >= 2 and sum(c["n_samples"] for c in kept) <= 600000
    assert lost[0]["n_samples"] == 0 and lost[0]["channel"] == -1
    assert any(c["n_samples"] for c, _ in want[k:])  # the flush found room again
    eng = new_engine(fvad, w.model, pool=600000)
    for p in range(NP):
        eng.submit(w.pcm[p])
        eng.collect(want=False)
    eng.sync()
    got = eng.poll_clips()
    assert_clips(got, want[:k], "before the flush")
    assert eng.capture_lost() == len(lost)
    eng.capture_flush()
    got += eng.poll_clips()
    assert_clips(got, want)
    assert eng.capture_lost() == sim.lost


def test_lifecycle(world):
    """Case 7: reset_streams drops a pending clip and restarts the stream's
    positions; capture_flush before it delivers the clip TAIL_SHORT;
    fvad_engine_reset discards; a stream saved after push 3 and restored into
    another slot of a second engine continues with nothing held."""
    w, fvad = world, world.fvad
    check_not_vacuous(w.clips, w.segs)
    produced = {(e["stream"], e["seq"]): e["push"] for e in w.segs}
    # a clip pending after the push that produced it, with three pushes left after it;
    # the slot then takes another stream from its start, one whose first clip completes within those
    s0, k = next((c["stream"], produced[(c["stream"], c["seq"])]) for c, _ in w.clips
                 if c["push"] > produced[(c["stream"], c["seq"])] and produced[(c["stream"], c["seq"])] <= NP - 4)
    donor = next(c["stream"] for c, _ in w.clips if c["sample_to"] <= 3 * PUSH and c["stream"] != s0)
    counts = even_counts()

    def run(flush_first):
        """Pushes 0..k, [flush s0,] reset s0, then the donor's audio from its start in slot s0."""
        eng = new_engine(fvad, w.model)
        sim = Sim(w.oracle, B, lambda s: w.x[s])
        mine, got = [list(c) for c in counts], []
        for p in range(NP):
            a = w.pcm[p]
            if p > k:
                a = a.copy()
                a[:, s0] = w.pcm[p - k - 1][:, donor]
                mine[p][s0] = (p - k) * PUSH
            eng.push(a)
            if p == k:
                if flush_first:
                    eng.capture_flush([s0])
                eng.reset_streams([s0])
        eng.sync()
        got += eng.poll_clips()
        eng.capture_flush()
        got += eng.poll_clips()
        segs = seg0(drain_events(eng))
        for p in range(NP):
            sim.pass_(p, segs, mine[p])
            if p == k:
                if flush_first:
                    sim.flush([s0], k, mine[k])
                sim.drop(s0, 0)
                sim.audio = lambda s: w.x[donor if s == s0 else s]
        sim.flush(None, NP - 1, mine[-1])
        return got, sim.out, segs

    got, want, segs = run(False)
    assert_clips(got, want, "reset")
    # the pending clip is gone, and s0's later clips count from 0 again
    pending = [e for e in segs if e["stream"] == s0 and e["push"] <= k and e["sample_to"] > (k + 1) * PUSH]
    assert pending and all((s0, e["seq"], e["sample_from"]) not in {(c["stream"], c["seq"], c["sample_from"])
                                                                    for c, _ in got if c["push"] <= k} for e in pending)
    again = [c for c, _ in got if c["stream"] == s0 and c["push"] > k]
    first = [c for c, _ in w.clips if c["stream"] == donor]
    assert again and again[0]["seq"] == 0 and again[0]["sample_from"] == first[0]["sample_from"]
    assert again[0]["flags"] == 0 and again[0]["n_samples"] == first[0]["n_samples"]
    got2, want2, _ = run(True)
    assert_clips(got2, want2, "flush, then reset")
    cut = [c for c, _ in got2 if c["stream"] == s0 and c["push"] == k and c["flags"] & TAIL]
    assert len(cut) == len(pending) and cut[0]["first_sample"] + cut[0]["n_samples"] == (k + 1) * PUSH
    assert len(got2) == len(got) + len(cut)

    # fvad_engine_reset: pending and unpolled clips are gone, the counts zero
    eng = new_engine(fvad, w.model, pool=600000)
    for p in range(NP):
        eng.push(w.pcm[p])
    eng.sync()
    eng.reset()
    assert eng.poll_clips() == [] and eng.capture_lost() == 0
    eng.capture_flush()
    assert eng.poll_clips() == []
    sim = Sim(w.oracle, B, lambda s: w.x[s], pool_cap=600000)
    for p in range(3):
        eng.push(w.pcm[p])
        sim.pass_(p, w.segs, counts[p])
    eng.sync()
    assert sim.out and any(c["n_samples"] for c, _ in sim.out)
    assert_clips(eng.poll_clips(), sim.out, "after fvad_engine_reset")
    assert eng.capture_lost() == sim.lost

    # save after push 3, restore into slot 2 of a three-stream engine
    at = 4 * PUSH
    sv = next(e["stream"] for e in w.segs if e["push"] >= 4 and e["sample_from"] < at)
    A = new_engine(fvad, w.model)
    for p in range(4):
        A.push(w.pcm[p])
    blob = A.save_streams([sv])
    Bn = new_engine(fvad, w.model, n_streams=3)
    Bn.restore_streams([2], blob)
    for p in range(4, NP):
        a = np.zeros((T, 3, CH, 480), np.float32)
        a[:, 2] = w.pcm[p][:, sv]
        Bn.push(a)
    Bn.sync()
    got = Bn.poll_clips()
    Bn.capture_flush()
    got += Bn.poll_clips()
    segs = seg0(drain_events(Bn))
    assert [(e["seq"], e["sample_from"], e["sample_to"]) for e in segs] == \
        [(e["seq"], e["sample_from"], e["sample_to"]) for e in w.segs if e["stream"] == sv and e["push"] >= 4]
    sim = Sim(w.oracle, 3, lambda s: w.x[sv])
    sim.drop(2, at)
    for q in range(NP - 4):
        sim.pass_(q, segs, [0, 0, at + (q + 1) * PUSH])
    sim.flush(None, NP - 5, [0, 0, at + (NP - 4) * PUSH])
    assert_clips(got, sim.out, "restored")
    assert got and all(c["first_sample"] >= at for c, _ in got)
    assert any(c["flags"] & HEAD and c["first_sample"] == at for c, _ in got)


def test_enable_after_pushes(world):
    """Capture enabled on a running engine (two pushes in): the streams hold
    nothing from before, so clips start at the enabling position at the
    earliest, and segments emitted before it are not recorded."""
    w, fvad = world, world.fvad
    check_not_vacuous(w.clips, w.segs)
    eng = new_engine(fvad, w.model, capture=False)
    for p in range(2):
        eng.push(w.pcm[p])
    eng.enable_capture(0, HIST, POOL)
    for p in range(2, NP):
        eng.push(w.pcm[p])
    eng.sync()
    got = eng.poll_clips()
    eng.capture_flush()
    got += eng.poll_clips()
    assert drain_events(eng) == w.events
    sim = Sim(w.oracle, B, lambda s: w.x[s])
    counts = even_counts()
    later = [e for e in w.segs if e["push"] >= 2]
    for s in range(B):
        sim.drop(s, 2 * PUSH)
    for p in range(2, NP):
        sim.pass_(p, later, counts[p])
    sim.flush(None, NP - 1, counts[-1])
    assert_clips(got, sim.out)
    assert any(c["flags"] & HEAD and c["first_sample"] == 2 * PUSH for c, _ in got)
    assert any(c["flags"] == 0 for c, _ in got)


@pytest.mark.parametrize("mode", ["f32_fast", "fp16"])
def test_other_modes(world, mode):
    """Case 8: the clips of an f32_fast and an fp16 engine are the model's over
    that engine's own events and the input."""
    w, fvad = world, world.fvad
    check_not_vacuous(w.clips, w.segs)
    eng = new_engine(fvad, w.model, mode=mode)
    for p in range(NP):
        eng.submit(w.pcm[p])
        eng.collect(want=False)
    eng.sync()
    got = eng.poll_clips()
    eng.capture_flush()
    got += eng.poll_clips()
    segs = seg0(drain_events(eng))
    want, _ = expected_w(w.oracle, segs, lambda s: w.x[s])
    assert len(want) >= 8
    assert_clips(got, want, mode)
    assert eng.capture_lost() == 0


def test_argument_checks(world):
    """Case 9."""
    w, fvad = world, world.fvad
    L = fvad.lib()
    info, lost = fvad.Clip(), C.c_uint64()

    def engine(**kw):
        e = fvad.Engine(w.model, 2, CH, max_ticks=T, bands=BANDS, **kw)
        e.attach_vadm(make_cfgs(fvad))
        return e

    eng = engine()
    assert L.fvad_engine_enable_capture(eng.h, 0, 10.0, 1 << 20) == EINVAL  # before enable_events
    assert L.fvad_engine_poll_clip(eng.h, C.byref(info), None, 0, C.byref(lost)) == EINVAL  # not enabled
    assert L.fvad_engine_capture_flush(eng.h, None, 0) == EINVAL
    eng.enable_events()
    assert L.fvad_engine_enable_capture(eng.h, 0, 3.99, 1 << 20) == EINVAL  # history_sec < 4
    assert L.fvad_engine_enable_capture(eng.h, 2, 10.0, 1 << 20) == EINVAL  # no such machine
    pcm = np.zeros((T, 2, CH, 480), np.float32)
    eng.submit(pcm)
    assert L.fvad_engine_enable_capture(eng.h, 0, 10.0, 1 << 20) == EINVAL  # a push not collected yet
    eng.collect(want=False)
    assert L.fvad_engine_enable_capture(eng.h, 0, 4.0, 1 << 20) == 0
    assert L.fvad_engine_enable_capture(eng.h, 0, 4.0, 1 << 20) == EINVAL  # twice
    assert L.fvad_engine_poll_clip(eng.h, C.byref(info), None, 0, None) == 0  # nothing yet
    fused = fvad.Engine(w.model, 2, CH, max_ticks=T, mode="fused")
    assert L.fvad_engine_enable_capture(fused.h, 0, 10.0, 1 << 20) == EINVAL
    nod = engine(use_denoiser=False)
    nod.enable_events()
    assert L.fvad_engine_enable_capture(nod.h, 0, 10.0, 1 << 20) == EINVAL
    # a short buffer reports n_samples and keeps the clip
    eng = new_engine(fvad, w.model)
    for p in range(NP):
        eng.push(w.pcm[p])
    eng.sync()
    first, audio = w.clips[0]
    n = first["n_samples"]
    assert n > 1
    buf = np.full(n, 7.0, np.float32)
    assert L.fvad_engine_poll_clip(eng.h, C.byref(info), buf.ctypes.data_as(C.c_void_p), n - 1, C.byref(lost)) == EINVAL
    assert info.as_dict() == first and np.all(buf == 7.0)
    assert L.fvad_engine_poll_clip(eng.h, C.byref(info), buf.ctypes.data_as(C.c_void_p), n, C.byref(lost)) == 1
    assert info.as_dict() == first and np.array_equal(buf.view(np.uint32), audio.view(np.uint32)) and lost.value == 0
    rest = eng.poll_clips()
    assert_clips(rest, w.clips[1:w.before_flush])
    ms, runs = eng.capture_times()
    assert set(ms) == {"k_hist_append", "capture_pass"} and runs >= 0
