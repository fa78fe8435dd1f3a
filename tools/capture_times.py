"""Times clip capture on the bench workload, built the way bench.py's measure()
builds it: 2048 stereo streams, 50-tick pushes of resident synthetic input (20
distinct pushes), device VADMachines, model seed 1, the speech event feed on.
Two staged engines live in one process, one with capture enabled (machine 0,
10 s of history) and its clips polled after every push, and take turns: each
repeat times `steps` pushes of each (the order alternates between repeats), so
both see the same box, clocks and neighbours.  The polling host thread copies
every clip out of the pinned pool into one reused buffer; the time it spends
in those calls is reported beside the push time it is part of.
Writes one JSON object (also printed): ms per push of both (every repeat and
the median), k_hist_append's and the capture pass's own times by HIP events
(fvad_engine_capture_times, the engine's sampled pushes), clips, samples and
bytes per push, clips lost, and the memory capture holds.

Usage: python3 tools/capture_times.py [--repeats 5] [--steps 20] [--warmup 5] [--pool SAMPLES]
       [--out profiles/capture_times.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "formula-vad_amd"))
import fvad


class Poller:
    """fvad_engine_poll_clip into one reused buffer: (clips, samples, without audio) of a drain."""

    def __init__(self, eng):
        self.eng, self.buf, self.info, self.lost = eng, np.zeros(1 << 20, np.float32), fvad.Clip(), C.c_uint64()
        self.seconds = 0.0

    def drain(self):
        L, clips, samples, bare = fvad.lib(), 0, 0, 0
        t0 = time.perf_counter()
        while True:
            rc = L.fvad_engine_poll_clip(self.eng.h, C.byref(self.info), self.buf.ctypes.data_as(C.c_void_p),
                                         self.buf.size, C.byref(self.lost))
            if rc == fvad.EINVAL and self.info.n_samples > self.buf.size:
                self.buf = np.zeros(int(self.info.n_samples), np.float32)
                continue
            if rc < 0:
                raise fvad.FvadError("fvad_engine_poll_clip failed (%d): %s" % (rc, fvad.last_error()))
            if rc == 0:
                break
            clips += 1
            samples += self.info.n_samples
            bare += bool(self.info.flags & fvad.CLIP_NO_AUDIO)
        self.seconds += time.perf_counter() - t0
        return clips, samples, bare


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--history", type=float, default=10.0)
    ap.add_argument("--pool", type=int, default=0, help="pool_samples (0: the library's default, 64 Mi)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capture_times.json"))
    args = ap.parse_args()
    B, Ch, T, P = args.streams, 2, 50, 20
    model = fvad.Model(seed=1)
    kinds = ("off", "on")
    eng, poller = {}, None
    for k in kinds:
        e = fvad.Engine(model, B, Ch, device=0, max_ticks=T)
        e.attach_vadm()
        e.enable_events()
        if k == "on":
            e.enable_capture(0, args.history, args.pool)
            poller = Poller(e)
        e.load_synthetic(T, base=0, pushes=P)
        for _ in range(args.warmup):
            e.run_resident(T)
            if k == "on":
                poller.drain()
        e.sync()
        while e.poll_events()[0]:
            pass
        if k == "on":
            poller.drain()
        eng[k] = e
        print("engine '%s' ready" % k, file=sys.stderr, flush=True)
    ms = {k: [] for k in kinds}
    append_ms, pass_ms, poll_ms = [], [], []
    clips = samples = bare = 0
    for r in range(args.repeats):
        for k in (kinds if r % 2 == 0 else kinds[::-1]):
            e = eng[k]
            e.clear_times()
            e.sync()
            if k == "on":
                poller.seconds = 0.0
            t0 = time.perf_counter()
            for _ in range(args.steps):
                e.run_resident(T)
                e.poll_events()
                if k == "on":
                    c, n, b = poller.drain()
                    clips, samples, bare = clips + c, samples + n, bare + b
            e.sync()
            ms[k].append(1e3 * (time.perf_counter() - t0) / args.steps)
            while e.poll_events()[0]:  # (outside the timed region: the last passes')
                pass
            if k == "on":
                poll_ms.append(1e3 * poller.seconds / args.steps)
                c, n, b = poller.drain()
                clips, samples, bare = clips + c, samples + n, bare + b
                t, n_runs = e.capture_times()
                if n_runs:
                    append_ms.append(t["k_hist_append"])
                    pass_ms.append(t["capture_pass"])
    pushes = args.repeats * args.steps
    hist = int(48000 * args.history)
    H = (hist + T * 480 + 3) & ~3
    out = {"workload": {"streams": B, "channels": Ch, "ticks_per_push": T, "resident_pushes": P, "vadm": True,
                        "events": True, "model_seed": 1, "repeats": args.repeats, "steps_per_repeat": args.steps,
                        "history_sec": args.history},
           "history_ring_bytes": B * Ch * H * 4, "pool_bytes": (args.pool or 64 << 20) * 4,
           "clips_per_push": clips / pushes, "samples_per_push": samples / pushes, "bytes_per_push": 4 * samples / pushes,
           "clips_without_audio": bare, "clips_lost": poller.lost.value,
           "k_hist_append_ms": statistics.median(append_ms) if append_ms else None, "k_hist_append_ms_repeats": append_ms,
           "capture_pass_ms": statistics.median(pass_ms) if pass_ms else None, "capture_pass_ms_repeats": pass_ms,
           "host_poll_ms_per_push": statistics.median(poll_ms), "host_poll_ms_per_push_repeats": poll_ms}
    for k in kinds:
        out[k] = {"ms_per_push": statistics.median(ms[k]), "ms_per_push_repeats": ms[k]}
    out["on_minus_off_ms"] = out["on"]["ms_per_push"] - out["off"]["ms_per_push"]
    out["off_spread_ms"] = max(ms["off"]) - min(ms["off"])
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
