"""Times the config sweep (fvad.Sweep, k_vadm_sweep) against the host loop on
one workload: 64 streams x 20 000 recorded windows (14.2 min of audio each at
fft_size 2048) x 1 024 configs, a grid over the default VadmConfig (long-term
60..240 s, short-term 0.1..0.5 s, threshold factor 6..40, ratio threshold
0.3..0.6, two opening times).  The windows are synthetic (seeded): background
band sums with bursts, as the sweep tests' generator makes them.

  device   wall time of Sweep.run (constants up, buffers cleared, k_vadm_sweep,
           states and segments back, all chunks), one warm-up run, then
           `repeats` runs: median, min, max.  The one-off upload of the windows
           with k_sweep_min is timed apart (the first run pays it).
  host     wall time of Sweep.run_host (the host VADMachine, up to 16 threads)
           on a sample of the lanes -- `host_streams` streams x every
           `host_cfg_step`-th config -- scaled by lanes to the whole workload;
           the sample's device results are compared with it lane by lane.
  engine   what the engine alone needs for the same answer: four machines per
           engine, so n_cfgs / 4 passes over the audio, each pass the
           workload's ticks at the bench's measured rate (ms per 2048-stream x
           50-tick push of profiles/r6_final8_bench.json, taken as scaling
           linearly down to 64 streams, which flatters this route).

Writes one JSON object (also printed) to profiles/sweep_times.json.

Usage: python3 tools/sweep_times.py [--repeats 5] [--streams 64] [--windows 20000] [--out ...]"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "formula-vad_amd"))
import fvad

FFT = 2048


def gen(s, W):
    rng = np.random.default_rng(1000 + s)
    band = (1e-3 * (1.0 + 0.5 * rng.random((W, 2)))).astype(np.float32)
    ub = rng.random(W)
    vad = np.full(W, 0.05, np.float32)
    vr = np.full(W, 0.2, np.float32)
    for w0 in range(20 + 7 * s, W, 150 + 13 * (s % 16)):
        w1 = min(W, w0 + 30 + 10 * (s % 4))
        c0 = (0.5 * (1.0 + ub[w0:w1])).astype(np.float32)
        band[w0:w1, 0] = c0
        band[w0:w1, 1] = np.float32(0.8) * c0
        vad[w0:w1] = 0.9
        vr[w0:w1] = 0.9
    return band.reshape(W, 2, 1), vad, vr


def grid():
    out = []
    for lt, st, thr, rt, mo in itertools.product((60.0, 120.0, 180.0, 240.0), (0.1, 0.2, 0.3, 0.5),
                                                 (6.0, 10.0, 14.0, 18.0, 22.0, 26.0, 30.0, 40.0),
                                                 (0.3, 0.4, 0.5, 0.6), (0.1, 0.2)):
        c = fvad.VadmConfig.default()
        c.long_term_speech_avg_sec, c.short_term_speech_avg_sec = lt, st
        c.speech_threshold_factor, c.channel_vol_ratio_threshold, c.min_consecutive_sec_to_open = thr, rt, mo
        out.append(c)
    return out


def lanes_of(sw, n_streams, n_cfgs):
    return [sw.segments(s, m) for s in range(n_streams) for m in range(n_cfgs)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--windows", type=int, default=20000)
    ap.add_argument("--host-streams", type=int, default=2)
    ap.add_argument("--host-cfg-step", type=int, default=32)
    ap.add_argument("--bench", default=os.path.join(ROOT, "profiles", "r6_final8_bench.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_times.json"))
    args = ap.parse_args()
    B, W = args.streams, args.windows
    cfgs = grid()
    data = [gen(s, W) for s in range(B)]
    sw = fvad.Sweep(B, 2, device=0, seg_capacity=64)
    for s, (band, vad, vr) in enumerate(data):
        sw.set_windows(s, band, vr, vad)
    t0 = time.perf_counter()
    sw.run(cfgs[:1])  # the windows' upload and k_sweep_min, one config's lanes, first-launch costs
    first_ms = 1e3 * (time.perf_counter() - t0)
    sw.run(cfgs)  # warm-up: every buffer at its size
    dev = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        sw.run(cfgs)
        dev.append(1e3 * (time.perf_counter() - t0))
    counts = sw.counts()
    # the host loop on a sample of the lanes, and the device's results on the same lanes
    hs, hc = min(args.host_streams, B), cfgs[::args.host_cfg_step]
    dev_sample = [sw.segments(s, m) for s in range(hs) for m in range(0, len(cfgs), args.host_cfg_step)]
    hsw = fvad.Sweep(hs, 2, device=-1, seg_capacity=64)
    for s in range(hs):
        hsw.set_windows(s, data[s][0], data[s][2], data[s][1])
    t0 = time.perf_counter()
    hsw.run(hc)
    host_ms = 1e3 * (time.perf_counter() - t0)
    same = lanes_of(hsw, hs, len(hc)) == dev_sample
    host_all_ms = host_ms * (B * len(cfgs)) / (hs * len(hc))
    with open(args.bench) as f:
        bench = json.loads(f.readline())
    push_ms, bs, bt = bench["ms_per_step"], bench["config"]["streams_per_gpu"], bench["config"]["ticks_per_step"]
    ticks = W * FFT / 480.0
    passes = (len(cfgs) + 3) // 4
    pass_ms = push_ms * (B * ticks) / (bs * bt)
    med = statistics.median(dev)
    out = {"workload": {"streams": B, "windows_per_stream": W, "configs": len(cfgs), "channels": 2, "fft_size": FFT,
                        "lanes": B * len(cfgs), "machine_bytes": sw.bytes(cfgs), "seg_capacity": 64,
                        "segments_total": int(counts.sum()), "lanes_with_segments": int((counts > 0).sum())},
           "device": {"run_ms": med, "run_ms_min": min(dev), "run_ms_max": max(dev), "run_ms_repeats": dev,
                      "first_run_one_config_ms": first_ms,
                      "how": "wall clock around Sweep.run (ends in a device synchronise and the copy back), "
                             "after one warm-up run",
                      "window_lane_steps_per_s": B * len(cfgs) * W / (med * 1e-3)},
           "host": {"sample_ms": host_ms, "sample_lanes": hs * len(hc), "threads": min(16, os.cpu_count() or 1),
                    "whole_workload_ms_scaled": host_all_ms, "sample_equals_device": bool(same),
                    "how": "wall clock around Sweep.run_host on %d streams x every %d-th config, scaled by lanes"
                           % (hs, args.host_cfg_step)},
           "engine_passes_equivalent": {"passes": passes, "ms_per_pass": pass_ms, "total_ms": passes * pass_ms,
                                 "bench_ms_per_push": push_ms, "bench": os.path.basename(args.bench),
                                 "how": "ceil(configs / 4) engine passes; a pass = streams x ticks at the bench's "
                                        "ms per %d-stream x %d-tick push, scaled linearly" % (bs, bt)}}
    out["host_over_device"] = host_all_ms / med
    out["engine_passes_over_device"] = passes * pass_ms / med
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    if not same:
        sys.exit("device and host disagree on the sampled lanes")


if __name__ == "__main__":
    main()
