"""The speech event feed (fvad_engine_enable_events / fvad_engine_poll_events,
k_vadm_events) against the host VADMachine fed the engine's own window
outputs: 40 stereo streams of 14 s in seven pushes of 200 ticks, two machines
(a fast-opening variant of the default config, and the same on the 300-3000 Hz
band).  An OPEN is expected wherever the host machine's state() goes 1 -> 2, a
SEGMENT wherever its segment count grows; the feed must equal that list
exactly -- every field, floats bit for bit, in (push, stream, machine,
production) order -- on k_vadm_hbm and on k_vadm_par, for any compaction chunk,
past seg_capacity, across ring overflow, per-stream reset, migration to another
engine, a whole-engine reset and an EngineGroup's merged feed.

The workload, the twin engine's outputs (no events) and the expected list are
computed once per module."""
import ctypes as C
import types

import numpy as np
import pytest

import parity_util as pu

pytestmark = pytest.mark.gpu

B, CH, SECS, T = 40, 2, 14.0, 200
NP = int(SECS * 100) // T  # 7 pushes
BANDS = ((4, 64), (13, 128))
SLOTS = (0, 1)
EINVAL = -1


def make_cfgs(mod):
    """[the default config opening after 0.1 s, closing after 0.2 s, segments
    from 0.3 s; the same on 300-3000 Hz] as mod's VadmConfig (fvad or oracle)."""
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


def host_events(fvad, outs, n_streams, push0=0):
    """The expected feed of `outs` (one output dict per push, every stream
    with all its ticks): (events, states) -- states[p][(s, m)] the host
    machine's speech state after push p."""
    cfgs = make_cfgs(fvad)
    L = fvad.lib()
    vms = [[fvad.VADMachine(c, n_channels=CH) for c in cfgs] for _ in range(n_streams)]
    wd = [0] * n_streams
    events, states = [], []
    for p, o in enumerate(outs):
        for s in range(n_streams):
            per_m = [[] for _ in cfgs]
            for t in np.nonzero(o["win_flag"][:, s])[0]:
                index = wd[s] * 2048
                for mi, vm in enumerate(vms[s]):
                    before = vm.state()[0]
                    nseg = L.fvad_vadm_segments(vm.h, None, 0)
                    vm.run(index, o["band"][t, s, :, SLOTS[mi]], float(o["win_vad"][t, s]),
                           float(o["win_ratio"][t, s]))
                    st, start, _ = vm.state()
                    base = {"stream": s, "machine": mi, "seq": nseg, "push": push0 + p}
                    if before == 1 and st == 2:
                        per_m[mi].append(dict(base, kind=fvad.EVENT_SPEECH_OPEN, sample_from=start, sample_to=index,
                                              debug_rnn_vad=0.0, debug_avg_speech_vol_ratio=0.0))
                    if L.fvad_vadm_segments(vm.h, None, 0) > nseg:
                        a, b, v, r = vm.segments()[-1]
                        per_m[mi].append(dict(base, kind=fvad.EVENT_SEGMENT, sample_from=a, sample_to=b,
                                              debug_rnn_vad=v, debug_avg_speech_vol_ratio=r))
                wd[s] += 1
            for ev in per_m:
                events.extend(ev)
        states.append({(s, mi): vms[s][mi].state()[0] for s in range(n_streams) for mi in range(len(cfgs))})
    return events, states


def new_engine(fvad, model, n_streams=B, seg_capacity=256):
    eng = fvad.Engine(model, n_streams, CH, max_ticks=T, bands=BANDS)
    eng.attach_vadm(make_cfgs(fvad), seg_capacity=seg_capacity)
    return eng


def drain(eng, step=4096):
    got = []
    while True:
        ev, lost = eng.poll_events(step)
        assert len(ev) <= step
        got += ev
        if not ev:
            return got, lost


def same_outputs(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("vad", "ratio", "win_flag", "win_ratio", "win_vad", "band"))


def seg_tuples(events, s, m):
    return [(e["sample_from"], e["sample_to"], e["debug_rnn_vad"], e["debug_avg_speech_vol_ratio"])
            for e in events if e["kind"] == 2 and e["stream"] == s and e["machine"] == m]


@pytest.fixture(scope="module")
def world(fvad_mod):
    fvad = fvad_mod
    model = fvad.Model(seed=1)
    streams, _ = pu.make_streams(fvad, list(range(B)), SECS)
    x = np.stack(streams)  # [B][CH][n]
    pcm = [np.ascontiguousarray(x[:, :, p * T * 480:(p + 1) * T * 480].reshape(B, CH, T, 480).transpose(2, 0, 1, 3))
           for p in range(NP)]
    twin = new_engine(fvad, model)  # no events: the reference outputs and segments
    outs = [twin.push(a) for a in pcm]
    segs = {(s, m): twin.segments(s, m) for s in range(B) for m in range(2)}
    expected, states = host_events(fvad, outs, B)
    w = types.SimpleNamespace(fvad=fvad, model=model, streams=streams, pcm=pcm, outs=outs, segs=segs,
                              expected=expected, states=states)
    for a in pcm:
        a.setflags(write=False)
    return w


@pytest.fixture(scope="module")
def oracle_segments(world, oracle_mod):
    """Machine 0's segments from the CPU oracle's pipeline with that config."""
    om = oracle_mod.Model(seed=1)
    cfg = make_cfgs(oracle_mod)[0]
    out = []
    for x in world.streams:
        p = oracle_mod.Pipeline(CH, om, main_cfg=cfg)
        for k in range(0, x.shape[1], 48000):
            p.push([x[0, k:k + 48000], x[1, k:k + 48000]])
        out.append(p.segments())
    return out


def check_not_vacuous(expected):
    """The expected list exercises what the tests are about."""
    for m in range(2):
        assert sum(1 for e in expected if e["machine"] == m) >= 50, m
    per = {}
    for e in expected:
        key = (e["push"], e["stream"] * 2 + e["machine"])
        per[key] = per.get(key, 0) + 1
    pushes = {p for p, _ in per}
    assert any(any(q == p and l < 64 for q, l in per) and any(q == p and l >= 64 for q, l in per) for p in pushes)
    assert max(per.values()) >= 2
    assert {e["kind"] for e in expected} == {1, 2}


@pytest.mark.parametrize("chunk", [0, 64])
@pytest.mark.parametrize("schedule", ["default", "always_par", "sync_each"])
def test_feed_equals_host_machines(world, oracle_segments, schedule, chunk):
    """default: submit / collect / poll, the machines of a push on k_vadm_hbm
    beside the next one, the last on k_vadm_par; always_par: every pass on
    k_vadm_par; sync_each: a sync point after every push.  chunk 64: the
    compaction walks the 80 lanes in two chunks (the carried base)."""
    w, fvad = world, world.fvad
    check_not_vacuous(w.expected)
    eng = new_engine(fvad, w.model)
    eng.enable_events()
    eng.set_debug(fvad.DEBUG_EVENTS_CHUNK, chunk)
    if schedule == "always_par":
        eng.set_debug(fvad.DEBUG_VADM_ALWAYS_PAR, 1)
    got = []
    for p in range(NP):
        if schedule == "sync_each":
            out = eng.push(w.pcm[p])
            eng.sync()
        else:
            eng.submit(w.pcm[p])
            out = eng.collect()
        assert same_outputs(out, w.outs[p]), p
        ev, lost = eng.poll_events()
        assert lost == 0
        got += ev
        assert got == w.expected[:len(got)], p
        if schedule == "sync_each":  # everything submitted so far is delivered
            assert len(got) == sum(1 for e in w.expected if e["push"] <= p), p
    eng.sync()
    ev, lost = drain(eng)
    got += ev
    assert lost == 0
    assert len(got) == len(w.expected)
    for i, (g, e) in enumerate(zip(got, w.expected)):
        assert g == e, (i, g, e)
    for s in range(B):
        for m in range(2):
            mine = eng.segments(s, m)
            assert mine == w.segs[(s, m)], (s, m)
            assert seg_tuples(got, s, m) == mine, (s, m)
            assert [e["seq"] for e in got if e["kind"] == 2 and e["stream"] == s and e["machine"] == m] == \
                list(range(len(mine))), (s, m)
        assert w.segs[(s, 0)] == oracle_segments[s], s
        assert eng.vadm_snapshot(s, 1)["n_segments"] == len(w.segs[(s, 1)])


def test_feed_past_seg_capacity(world):
    """seg_capacity 1: the list keeps the first segment and the true total,
    the feed carries every one with its index."""
    w, fvad = world, world.fvad
    check_not_vacuous(w.expected)
    assert max(len(v) for v in w.segs.values()) >= 2
    eng = new_engine(fvad, w.model, seg_capacity=1)
    eng.enable_events()
    for p in range(NP):
        eng.submit(w.pcm[p])
        eng.collect(want=False)
    eng.sync()
    got, lost = drain(eng)
    assert lost == 0 and got == w.expected
    L = fvad.lib()
    for (s, m), ref in w.segs.items():
        buf = (fvad.Segment * 4)()
        total = L.fvad_engine_segments(eng.h, s, m, buf, 4)
        assert total == len(ref), (s, m)
        kept = [(g.sample_from, g.sample_to, g.debug_rnn_vad, g.debug_avg_speech_vol_ratio) for g in buf[:min(total, 1)]]
        assert kept == ref[:1], (s, m)
        assert seg_tuples(got, s, m) == ref, (s, m)


def test_no_polling_then_drain(world):
    """Seven pushes with no poll, a sync, then slices of 7: the whole list,
    nothing lost.  Then, after fvad_engine_reset, the same pushes with a poll
    right after every submit: whatever has finished by then is a prefix (no
    timing is asserted), and the push ordinals start again at 0."""
    w, fvad = world, world.fvad
    check_not_vacuous(w.expected)
    eng = new_engine(fvad, w.model)
    eng.enable_events()
    for p in range(NP):
        eng.submit(w.pcm[p])
        assert same_outputs(eng.collect(), w.outs[p]), p
    eng.sync()
    got, lost = drain(eng, step=7)
    assert lost == 0 and got == w.expected
    eng.reset()
    got = []
    for p in range(NP):
        eng.submit(w.pcm[p])
        ev, lost = eng.poll_events()
        got += ev
        assert lost == 0 and got == w.expected[:len(got)], p
        assert all(e["push"] < p for e in ev), p  # push p's machines are not even enqueued yet
        eng.collect(want=False)
    eng.sync()
    ev, lost = drain(eng, step=7)
    assert lost == 0 and got + ev == w.expected


def test_ring_overflow(world):
    """A ring of 8 and no poll: the first 8 events survive, the rest are
    counted; unpolled events are never overwritten.  After reset_streams of
    every stream the audio again, polled after every push (a sync point each,
    so a batch is one pass's): a pass writes the first 8 of its push."""
    w, fvad = world, world.fvad
    check_not_vacuous(w.expected)
    eng = new_engine(fvad, w.model)
    eng.enable_events(8)
    for p in range(NP):
        eng.submit(w.pcm[p])
        eng.collect(want=False)
    eng.sync()
    got, lost = drain(eng)
    assert got == w.expected[:8]
    assert lost == len(w.expected) - 8
    eng.reset_streams(list(range(B)))
    over = 0
    for p in range(NP):
        assert same_outputs(eng.push(w.pcm[p]), w.outs[p]), p
        eng.sync()
        ev, lost2 = drain(eng)
        mine = [dict(e, push=e["push"] + NP) for e in w.expected if e["push"] == p]
        assert ev == mine[:8], p
        lost += max(0, len(mine) - 8)
        assert lost2 == lost, p
        over += len(mine) > 8
    assert over >= 2  # (pushes that overflowed the emptied ring again)
    for (s, m), ref in w.segs.items():  # the machines themselves lost nothing
        assert eng.segments(s, m) == ref, (s, m)


def test_reset_streams_restarts_seq(world):
    """reset_streams([3, 17]) after three pushes, then those two from the start
    of their audio: their events repeat the first pushes' with seq from 0 and
    sample indices from 0, beside everyone else's unchanged."""
    w, fvad = world, world.fvad
    check_not_vacuous(w.expected)
    back = (3, 17)
    for s in back:  # each has events to repeat, from seq 0
        assert any(e["stream"] == s and e["push"] < NP - 3 and e["seq"] == 0 for e in w.expected), s
    eng = new_engine(fvad, w.model)
    eng.enable_events()
    got = []
    for p in range(NP):
        if p == 3:
            eng.reset_streams(back)
        a = w.pcm[p]
        if p >= 3:
            a = a.copy()
            for s in back:
                a[:, s] = w.pcm[p - 3][:, s]
        eng.submit(a)
        eng.collect(want=False)
        got += eng.poll_events()[0]
    eng.sync()
    got += drain(eng)[0]
    want = []
    for p in range(NP):
        now = [e for e in w.expected if e["push"] == p and (p < 3 or e["stream"] not in back)]
        if p >= 3:
            now += [dict(e, push=p) for e in w.expected if e["push"] == p - 3 and e["stream"] in back]
        want += sorted(now, key=lambda e: e["stream"])  # (stable: machine and production order stay)
    assert got == want


def test_restore_continues_seq_without_second_open(world):
    """Five streams saved after four pushes -- one of them Open at that point
    by the host machine -- restored into a second engine with events enabled:
    its feed is the tail of the expected list for those streams, seq carrying
    on from the blob's segment count, no OPEN for the speech already open."""
    w, fvad = world, world.fvad
    check_not_vacuous(w.expected)
    st = w.states[3]
    # lanes Open after push 3 whose speech ends within the remaining pushes
    open_now = [(s, m) for s in range(B) for m in range(2) if st[(s, m)] == 2 and
                any(e["stream"] == s and e["machine"] == m and e["push"] >= 4 for e in w.expected)]
    assert open_now, "no machine is Open after push 3"
    s_open, m_open = open_now[0]
    moved = sorted(set([s_open] + [s for s in (1, 8, 22, 31, 39, 5) if s != s_open][:4]))
    assert len(moved) == 5
    tail = [dict(e, push=e["push"] - 4, stream=moved.index(e["stream"])) for e in w.expected
            if e["push"] >= 4 and e["stream"] in moved]
    assert any(e["seq"] > 0 for e in tail)
    # the open speech ends in the tail: a SEGMENT that no OPEN of the tail precedes
    first = next(e for e in tail if e["stream"] == moved.index(s_open) and e["machine"] == m_open)
    assert first["kind"] == fvad.EVENT_SEGMENT
    A = new_engine(fvad, w.model)
    for p in range(4):
        A.submit(w.pcm[p])
        A.collect(want=False)
    blob = A.save_streams(moved)
    Bn = new_engine(fvad, w.model, n_streams=5)
    Bn.enable_events()
    Bn.restore_streams(list(range(5)), blob)
    got = []
    for p in range(4, NP):
        out = Bn.push(np.ascontiguousarray(w.pcm[p][:, moved]))
        assert np.array_equal(out["band"], w.outs[p]["band"][:, moved]), p
        got += Bn.poll_events()[0]
    Bn.sync()
    got += drain(Bn)[0]
    assert got == tail


def test_engine_reset_empties_feed(world):
    w, fvad = world, world.fvad
    check_not_vacuous(w.expected)
    first = [e for e in w.expected if e["push"] == 0]
    assert first
    eng = new_engine(fvad, w.model)
    eng.enable_events(4)
    eng.push(w.pcm[0])
    eng.push(w.pcm[1])
    eng.sync()  # unpolled events in the ring, some lost
    eng.reset()
    assert eng.poll_events() == ([], 0)
    eng.push(w.pcm[0])
    eng.sync()
    ev, lost = drain(eng)
    assert ev == first[:4] and lost == len(first) - 4


def test_argument_checks(world):
    w, fvad = world, world.fvad
    L = fvad.lib()
    n, lost = C.c_size_t(9), C.c_uint64(9)
    plain = fvad.Engine(w.model, 2, CH, max_ticks=10)
    assert L.fvad_engine_enable_events(plain.h, 0) == EINVAL  # no machines
    assert L.fvad_engine_poll_events(plain.h, None, 0, C.byref(n), C.byref(lost)) == EINVAL  # not enabled
    fused = fvad.Engine(w.model, 2, CH, max_ticks=10, mode="fused")
    assert L.fvad_engine_enable_events(fused.h, 0) == EINVAL
    eng = fvad.Engine(w.model, 2, CH, max_ticks=10)
    eng.attach_vadm()
    pcm = np.zeros((10, 2, CH, 480), np.float32)
    eng.submit(pcm)
    assert L.fvad_engine_enable_events(eng.h, 0) == EINVAL  # a push not collected yet
    eng.collect(want=False)
    assert L.fvad_engine_enable_events(eng.h, 16) == 0
    assert L.fvad_engine_enable_events(eng.h, 16) == EINVAL  # twice
    eng.push(pcm)
    eng.sync()
    assert L.fvad_engine_poll_events(eng.h, None, 0, C.byref(n), C.byref(lost)) == 0
    assert n.value == 0 and lost.value == 0
    buf = (fvad.Event * 2)()
    assert L.fvad_engine_poll_events(eng.h, None, 2, C.byref(n), C.byref(lost)) == EINVAL  # no buffer
    assert L.fvad_engine_poll_events(eng.h, buf, 2, None, None) == EINVAL
    assert L.fvad_engine_poll_events(eng.h, buf, 2, C.byref(n), None) == 0 and n.value == 0  # silence: no events


def test_group_merged_feed(world):
    """EngineGroup(groups=2) over the 40 streams, machine passes of both
    engines on one shared side stream: the merged feed is the single
    engine's."""
    w, fvad = world, world.fvad
    check_not_vacuous(w.expected)
    grp = fvad.EngineGroup(w.model, B, CH, groups=2, vadm=make_cfgs(fvad), max_ticks=T, bands=BANDS)
    grp.enable_events()
    got = []
    for p in range(NP):
        for e, f, n in zip(grp.engines, grp.first, grp.sizes):
            e.submit(np.ascontiguousarray(w.pcm[p][:, f:f + n]))
        for e in grp.engines:
            e.collect(want=False)
        ev, lost = grp.poll_events()
        got += ev
        assert lost == 0 and got == w.expected[:len(got)], p
    grp.sync()
    ev, lost = grp.poll_events()
    assert lost == 0 and got + ev == w.expected
    assert grp.poll_events() == ([], 0)
