"""Times per-stream VADMachine configs on the bench workload, built the way
bench.py's measure() builds it: 2048 stereo streams, 50-tick pushes of resident
synthetic input (20 distinct pushes), device VADMachines, model seed 1.  Three
staged engines live in one process and take turns (the order rotates between
repeats), so all see the same box, clocks and neighbours:
  A  attach_vadm(default)             k_vadm_hbm / k_vadm_par, constants in the argument block
  B  attach_vadm(default, room=[])    the _ps kernels over identical table rows
  C  room=[] and a row per stream: long_term_speech_avg_sec spread over 60..180 s,
     speech_threshold_factor and min_vad_duration_sec varied
Writes one JSON object (also printed): ms per push of each (every repeat and
the median), each engine's machine-kernel slots (the engine's sampled passes,
by HIP events), and the host wall time of one fvad_engine_set_stream_vadm call
for 256 and for all streams with the k_vadm_retarget launches it made, plus the
time until the device had finished them.

Usage: python3 tools/stream_vadm_times.py [--repeats 5] [--steps 20] [--warmup 5]
       [--out profiles/stream_vadm_times.json]"""
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

ROWS_PER_LAUNCH = 47  # kRetargetMax (fvad_lifecycle.h): the rows one 4 KB argument block carries


def row(s, B):
    c = fvad.VadmConfig.default()
    c.long_term_speech_avg_sec = 60.0 + 120.0 * s / max(1, B - 1)
    c.speech_threshold_factor = 12.0 + s % 13
    c.min_vad_duration_sec = 0.4 + 0.05 * (s % 9)
    return c


def time_set(eng, ids, cfgs):
    """One fvad_engine_set_stream_vadm call on an idle engine: (host ms, ms until the device is done)."""
    a = np.ascontiguousarray(ids, np.int32)
    arr = (fvad.VadmConfig * len(cfgs))(*cfgs)
    eng.sync()
    t0 = time.perf_counter()
    rc = fvad.lib().fvad_engine_set_stream_vadm(eng.h, a.ctypes.data_as(C.POINTER(C.c_int32)), a.size, 0, arr)
    t1 = time.perf_counter()
    eng.sync()
    t2 = time.perf_counter()
    assert rc == 0, fvad.last_error()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_vadm_times.json"))
    args = ap.parse_args()
    B, Ch, T, P = args.streams, 2, 50, 20
    model = fvad.Model(seed=1)
    kinds = ("A", "B", "C")
    rows = [row(s, B) for s in range(B)]
    eng, set_ms = {}, {}
    for k in kinds:
        e = fvad.Engine(model, B, Ch, device=0, max_ticks=T)
        e.attach_vadm(room=None if k == "A" else [])
        if k == "C":
            for n in sorted({min(256, B), B}):
                samples = [time_set(e, range(n), rows[:n]) for _ in range(5)]
                set_ms[str(n)] = {"host_ms": statistics.median(x[0] for x in samples),
                                  "host_ms_repeats": [x[0] for x in samples],
                                  "until_device_done_ms": statistics.median(x[1] for x in samples),
                                  "launches": -(-n // ROWS_PER_LAUNCH)}
        e.load_synthetic(T, base=0, pushes=P)
        for _ in range(args.warmup):
            e.run_resident(T)
        e.sync()
        eng[k] = e
    ms = {k: [] for k in kinds}
    vadm = {k: {} for k in kinds}
    for r in range(args.repeats):
        for k in kinds[r % 3:] + kinds[:r % 3]:
            e = eng[k]
            e.clear_times()
            e.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                e.run_resident(T)
            e.sync()
            ms[k].append(1e3 * (time.perf_counter() - t0) / args.steps)
            for name, v in e.kernel_times()["kernels"].items():
                if name.startswith("k_vadm"):
                    vadm[k].setdefault(name, []).append(v)
    out = {"workload": {"streams": B, "channels": Ch, "ticks_per_push": T, "resident_pushes": P, "vadm": True,
                        "model_seed": 1, "repeats": args.repeats, "steps_per_repeat": args.steps},
           "set_stream_vadm": set_ms}
    for k in kinds:
        out[k] = {"ms_per_push": statistics.median(ms[k]), "ms_per_push_repeats": ms[k],
                  "vadm_kernels_ms": {n: statistics.median(v) for n, v in vadm[k].items()}}
    out["B_minus_A_ms"] = out["B"]["ms_per_push"] - out["A"]["ms_per_push"]
    out["C_minus_A_ms"] = out["C"]["ms_per_push"] - out["A"]["ms_per_push"]
    out["A_spread_ms"] = max(ms["A"]) - min(ms["A"])
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
