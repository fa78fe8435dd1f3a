"""Times the two ways from recorded windows to a score per config, on
tools/sweep_times.py's workload and grid (64 streams x 20 000 windows x 1 024
configs) with each stream's bursts as its labels, at the smallest seg_capacity
(a multiple of 8) that holds every lane -- sweep_times.py's 64 does not, and
neither path scores a truncated lane:

  (a) run + score   Sweep.run (k_vadm_sweep, states and segments back), then
                    Sweep.score (the host evaluator, one thread, per lane)
  (b) run_score     Sweep.run_score (k_vadm_sweep and k_sweep_score per chunk;
                    states, statistics and status words back; the aggregates
                    on the host)

In one process, after one warm-up of each path: `repeats` interleaved repeats
of (a) and (b), each a wall clock around the calls (every one ends in a device
synchronise and its copy back, or is host code).  The kernel is not timed on
its own.  Also: score alone within (a), the bytes each path copies back
(fvad_sweep_last_run), and whether (b)'s aggregates equal (a)'s by their bits.

Writes one JSON object (also printed) to profiles/sweep_score_times.json.

Usage: python3 tools/sweep_score_times.py [--repeats 5] [--streams 64] [--windows 20000] [--out ...]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sweep_times import FFT, fvad, gen, grid  # noqa: E402  (the workload is sweep_times.py's)

STAT = dict(ignore_shorter_than_sec=0.5, extrude_start=0.5, extrude_end=1.0, fill_gaps=0.5)


def labels(s, W):
    """Stream s's bursts (sweep_times.gen) as (from_sec, to_sec)."""
    return [(w0 * FFT / 48000.0, min(W, w0 + 30 + 10 * (s % 4)) * FFT / 48000.0)
            for w0 in range(20 + 7 * s, W, 150 + 13 * (s % 16))]


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats_ms": ms}


def same_bits(a, b):
    """Aggregates as float32: equal bits wherever a is not NaN, NaN where it is."""
    x = np.frombuffer(b"".join(bytes(v) for v in a), np.float32)
    y = np.frombuffer(b"".join(bytes(v) for v in b), np.float32)
    nan = np.isnan(x)
    return bool(np.isnan(y[nan]).all() and np.array_equal(x[~nan].view(np.uint32), y[~nan].view(np.uint32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--windows", type=int, default=20000)
    ap.add_argument("--device", type=int, default=0, help="-1: a host-only sweep (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_score_times.json"))
    args = ap.parse_args()
    B, W = args.streams, args.windows
    cfgs = grid()
    refs = [labels(s, W) for s in range(B)]
    data = [gen(s, W) for s in range(B)]

    def sweep(cap):
        sw = fvad.Sweep(B, 2, device=args.device, seg_capacity=cap)
        for s, (band, vad, vr) in enumerate(data):
            sw.set_windows(s, band, vr, vad)
        return sw

    # sweep_times.py's seg_capacity 64 does not hold this workload's busiest lanes, and a truncated lane
    # cannot be scored by either path: the smallest multiple of 8 that holds them all
    sw = sweep(64)
    sw.run(cfgs)
    most = int(sw.counts().max())
    cap = max(64, (most + 7) // 8 * 8)
    if cap != 64:
        sw = sweep(cap)

    def path_a():
        t0 = time.perf_counter()
        sw.run(cfgs)
        t1 = time.perf_counter()
        agg = sw.score(refs, **STAT)
        t2 = time.perf_counter()
        return 1e3 * (t2 - t0), 1e3 * (t2 - t1), agg, sw.last_run()["bytes_back"]

    def path_b():
        t0 = time.perf_counter()
        agg = sw.run_score(cfgs, refs, stat=STAT)
        return 1e3 * (time.perf_counter() - t0), agg, sw.last_run()["bytes_back"]

    path_a()  # warm-up: the windows' upload, every buffer at its size
    path_b()
    a_ms, score_ms, b_ms = [], [], []
    same = True
    for _ in range(args.repeats):
        ta, ts, agg_a, back_a = path_a()
        tb, agg_b, back_b = path_b()
        a_ms.append(ta)
        score_ms.append(ts)
        b_ms.append(tb)
        same = same and same_bits(agg_a, agg_b)
    counts = sw.counts()
    out = {"workload": {"streams": B, "windows_per_stream": W, "configs": len(cfgs), "channels": 2, "fft_size": FFT,
                        "lanes": B * len(cfgs), "seg_capacity": cap, "device": args.device,
                        "segments_total": int(counts.sum()), "segments_most": most,
                        "labels_total": sum(len(r) for r in refs), "stat_config": STAT},
           "run_then_score": dict(spread(a_ms), bytes_back=back_a,
                                  how="wall clock around Sweep.run followed by Sweep.score (host evaluator, one thread)"),
           "score_alone": dict(spread(score_ms), how="the Sweep.score part of run_then_score"),
           "run_score": dict(spread(b_ms), bytes_back=back_b,
                             how="wall clock around Sweep.run_score (ends in a device synchronise and the copy back "
                                 "of states, statistics and status words, then the host aggregation); the kernel "
                                 "was not timed on its own"),
           "aggregates_equal_by_bits": bool(same),
           "method": "one process, one warm-up of each path, then %d interleaved repeats" % args.repeats}
    out["run_then_score_over_run_score"] = out["run_then_score"]["median_ms"] / out["run_score"]["median_ms"]
    text = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    if not same:
        sys.exit("run_score's aggregates differ from run + score's")


if __name__ == "__main__":
    main()
