"""Times the speech event feed on the bench workload, built the way bench.py's
measure() builds it: 2048 stereo streams, 50-tick pushes of resident synthetic
input (20 distinct pushes), device VADMachines, model seed 1.  Two staged
engines live in one process, one with the feed enabled and polled after every
push, and take turns: each repeat times `steps` pushes of each (the order
alternates between repeats), so both see the same box, clocks and neighbours.
Writes one JSON object (also printed): ms per push of both (every repeat and
the median), k_vadm_events' own time by HIP events (the engine's sampled
passes), the machine kernels' times of both engines, and events per push.

Usage: python3 tools/event_times.py [--repeats 5] [--steps 40] [--warmup 5] [--out profiles/event_times.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "formula-vad_amd"))
import fvad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "event_times.json"))
    args = ap.parse_args()
    B, C, T, P = args.streams, 2, 50, 20
    model = fvad.Model(seed=1)
    kinds = ("off", "on")
    eng = {}
    for k in kinds:
        e = fvad.Engine(model, B, C, device=0, max_ticks=T)
        e.attach_vadm()
        if k == "on":
            e.enable_events()
        e.load_synthetic(T, base=0, pushes=P)
        for _ in range(args.warmup):
            e.run_resident(T)
        e.sync()
        if k == "on":
            while e.poll_events()[0]:
                pass
        eng[k] = e
    ms = {k: [] for k in kinds}
    vadm = {k: {} for k in kinds}
    pass_ms, n_events, lost, polls_empty = [], 0, 0, 0
    for r in range(args.repeats):
        for k in (kinds if r % 2 == 0 else kinds[::-1]):
            e = eng[k]
            e.clear_times()
            e.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                e.run_resident(T)
                if k == "on":
                    ev, lost = e.poll_events()
                    n_events += len(ev)
                    polls_empty += not ev
            e.sync()
            ms[k].append(1e3 * (time.perf_counter() - t0) / args.steps)
            if k == "on":
                while True:  # (outside the timed region: the last passes' events)
                    ev, lost = e.poll_events()
                    n_events += len(ev)
                    if not ev:
                        break
                t, n = e.event_times()
                if n:
                    pass_ms.append(t)
            for name, v in e.kernel_times()["kernels"].items():
                if name.startswith("k_vadm"):
                    vadm[k].setdefault(name, []).append(v)
    pushes = args.repeats * args.steps
    out = {"workload": {"streams": B, "channels": C, "ticks_per_push": T, "resident_pushes": P, "vadm": True,
                        "model_seed": 1, "repeats": args.repeats, "steps_per_repeat": args.steps},
           "events_per_push": n_events / pushes, "events_lost": lost,
           "polls_returning_nothing": polls_empty,
           "k_vadm_events_ms": statistics.median(pass_ms) if pass_ms else None, "k_vadm_events_ms_repeats": pass_ms}
    for k in kinds:
        out[k] = {"ms_per_push": statistics.median(ms[k]), "ms_per_push_repeats": ms[k],
                  "vadm_kernels_ms": {n: statistics.median(v) for n, v in vadm[k].items()}}
    out["on_minus_off_ms"] = out["on"]["ms_per_push"] - out["off"]["ms_per_push"]
    out["off_spread_ms"] = max(ms["off"]) - min(ms["off"])
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
