"""Times the f32_fast engine mode against the staged mode on the bench
workload, built the way bench.py's measure() builds it: 2048 stereo streams,
50-tick pushes of resident synthetic input (20 distinct pushes), device
VADMachines, model seed 1.  Both engines live in one process and take turns:
each repeat times `steps` staged pushes and `steps` f32_fast pushes (the order
alternates between repeats), so both modes see the same box, clocks and
neighbours.  Prints one JSON object: ms per push and kernel_times() of both
modes (every repeat and the median), and for each fused multiply-add kernel
(TWINS) its time beside its exact twin's with the spread of the pair over the
repeats.

Usage: python3 tools/mode_times.py [--repeats 5] [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "formula-vad_amd"))
import fvad

TWINS = {"k_rnn3f": "k_rnn3"}  # fused multiply-add kernel -> exact twin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--streams", type=int, default=2048)
    args = ap.parse_args()
    B, C, T, P = args.streams, 2, 50, 20
    model = fvad.Model(seed=1)
    modes = ("staged", "f32_fast")
    eng = {}
    for m in modes:
        e = fvad.EngineGroup(model, B, C, groups=1, vadm=True, device=0, max_ticks=T, mode=m)
        e.load_synthetic(T, base=0, pushes=P)
        for _ in range(args.warmup):
            e.run_resident(T)
        e.sync()
        eng[m] = e
    ms = {m: [] for m in modes}
    kern = {m: {} for m in modes}
    for r in range(args.repeats):
        for m in (modes if r % 2 == 0 else modes[::-1]):
            e = eng[m]
            e.clear_times()
            e.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                e.run_resident(T)
            e.sync()
            ms[m].append(1e3 * (time.perf_counter() - t0) / args.steps)
            for k, v in e.kernel_times()["kernels"].items():
                kern[m].setdefault(k, []).append(v)
    out = {"workload": {"streams": B, "channels": C, "ticks_per_push": T, "resident_pushes": P, "vadm": True,
                        "model_seed": 1, "repeats": args.repeats, "steps_per_repeat": args.steps}}
    for m in modes:
        out[m] = {"ms_per_push": statistics.median(ms[m]), "ms_per_push_repeats": ms[m],
                  "frames_per_s": B * C * T / (1e-3 * statistics.median(ms[m])),
                  "kernel_times_ms": {k: statistics.median(v) for k, v in kern[m].items()},
                  "kernel_times_ms_repeats": kern[m]}
    pairs = {}
    for f, x in TWINS.items():
        if f not in kern["f32_fast"] or x not in kern["staged"]:
            continue
        a, b = kern["staged"][x], kern["f32_fast"][f]
        spread = max(max(a) - min(a), max(b) - min(b))
        gain = statistics.median(a) - statistics.median(b)
        pairs[f] = {"exact_ms": statistics.median(a), "fast_ms": statistics.median(b), "gain_ms": gain,
                    "spread_ms": spread, "wins": gain > spread}
    out["pairs"] = pairs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
