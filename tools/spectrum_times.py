"""Times the window-spectrum tap and the spectral sweep, interleaved in one
process as the other tools do.  Writes one JSON object (also printed) to
profiles/spectrum_times.json.

  (a) push     the bench's workload (2048 stereo streams, 50-tick pushes of
               resident synthetic input, model seed 1): three staged engines --
               without the tap, with spectrum=(0, 1024), with spectrum=(4, 128)
               -- take turns; each repeat times `steps` run_resident calls and a
               sync of each (wall clock, ms per push; the order alternates).
               Also the k_olafb / k_olafb_spec event time of each
               (Engine.kernel_times) and the bytes the tap writes per push.
  (b) sweep    tools/sweep_times.py's workload and grid (64 streams x 20 000
               windows x 1 024 configs): Sweep.run on a plain sweep of one band
               against a spectral sweep over the bins 4..128 whose configs lie
               on 1, 64 and 1 024 distinct bands (wall clock round the call,
               one warm-up each, then interleaved repeats).
  (c) bandmin  k_sweep_bandmin alone in those runs, by events
               (Sweep.bandmin_ms), beside a device-to-device copy of the
               recorded spectra's bytes, by events too: what reading them once
               costs at the least.

Usage: python3 tools/spectrum_times.py [--repeats 5] [--steps 20] [--streams 2048] [--sweep-streams 64]
                                       [--windows 20000] [--out profiles/spectrum_times.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resample_times import d2d_copy_ms  # noqa: E402
from sweep_times import FFT, fvad, gen, grid  # noqa: E402  (the workload is sweep_times.py's)

SPEC = (4, 128)


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats_ms": ms}


def push_times(args):
    B, C, T = args.streams, 2, 50
    model = fvad.Model(seed=1)
    kinds = (("tap_off", None), ("tap_0_1024", (0, 1024)), ("tap_4_128", SPEC))
    eng = {}
    for name, rng in kinds:
        e = fvad.Engine(model, B, C, device=0, max_ticks=T, spectrum=rng)
        e.load_synthetic(T, base=0)
        for _ in range(args.warmup):
            e.run_resident(T)
        e.sync()
        e.clear_times()
        eng[name] = e
    names = [k[0] for k in kinds]
    ms = {k: [] for k in names}
    for r in range(args.repeats):
        for k in (names if r % 2 == 0 else names[::-1]):
            e = eng[k]
            e.run_resident(T)  # back into steady state, outside the timed region
            e.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                e.run_resident(T)
            e.sync()
            ms[k].append(1e3 * (time.perf_counter() - t0) / args.steps)
    out = {"workload": {"streams": B, "channels": C, "ticks_per_push": T, "model_seed": 1, "input": "resident synthetic",
                        "repeats": args.repeats, "steps_per_repeat": args.steps}}
    for name, rng in kinds:
        e = eng[name]
        o = dict(spread(ms[name]), how="wall clock round `steps` run_resident calls and a sync, per push")
        o["kernel_times"] = e.kernel_times()
        if rng is not None:
            o["n_spec"] = e.n_spec
            o["spectrum_bytes_per_push"] = T * B * C * e.n_spec * 4
            o["over_tap_off"] = o["median_ms"] / statistics.median(ms["tap_off"])
        out[name] = o
    return out


def spectra_of(band, s):
    """sweep_times.gen's band sums of the default band (bins 4..64) spread over the recorded
    bins: every bin 1 / 61 of the sum, times 1 + 0.2 u."""
    rng = np.random.default_rng(5000 + s)
    W = band.shape[0]
    n_spec = SPEC[1] - SPEC[0] + 1
    return (band.reshape(W, 2, 1) / np.float32(61.0) * (1.0 + 0.2 * rng.random((W, 2, n_spec), np.float32))).astype(np.float32)


def on_bands(cfgs, D):
    """The grid with config i on band i % D of 1 024 distinct bands inside SPEC (D = 1: the default band)."""
    out = []
    for i, c in enumerate(cfgs):
        d = fvad.VadmConfig()
        for n, _ in c._fields_:
            setattr(d, n, getattr(c, n))
        j = i % D
        lo, hi = (4, 64) if D == 1 else (4 + j % 32, 4 + j % 32 + 29 + j // 32)
        d.speech_min_freq, d.speech_max_freq = lo * 48000.0 / FFT, hi * 48000.0 / FFT
        out.append(d)
    return out


def sweep_times(args):
    B, W = args.sweep_streams, args.windows
    cfgs = grid()
    plain = fvad.Sweep(B, 2, device=0, seg_capacity=64)
    spec = fvad.Sweep(B, 2, device=0, seg_capacity=64, spectrum=SPEC)
    for s in range(B):
        band, vad, vr = gen(s, W)
        plain.set_windows(s, band, vr, vad)
        spec.set_spectra(s, spectra_of(band, s), vr, vad)
    runs = [("plain_1_band", plain, cfgs)] + [("spectral_%d_bands" % D, spec, on_bands(cfgs, D)) for D in (1, 64, 1024)]
    print("sweeps filled", file=sys.stderr, flush=True)
    first = {}
    for name, sw, c in runs:  # warm-up: the one-off upload of the windows, every buffer at its size
        t0 = time.perf_counter()
        sw.run(c)
        first[name] = 1e3 * (time.perf_counter() - t0)
    ms = {name: [] for name, _, _ in runs}
    bm = {name: [] for name, _, _ in runs}
    for r in range(args.repeats):
        for name, sw, c in (runs if r % 2 == 0 else runs[::-1]):
            t0 = time.perf_counter()
            sw.run(c)
            ms[name].append(1e3 * (time.perf_counter() - t0))
            if sw is spec:
                bm[name].append(sw.bandmin_ms())
    n_spec = SPEC[1] - SPEC[0] + 1
    spectra_bytes = B * W * 2 * n_spec * 4
    copy_ms = d2d_copy_ms(spectra_bytes)
    out = {"workload": {"streams": B, "windows_per_stream": W, "configs": len(cfgs), "channels": 2, "fft_size": FFT,
                        "spectrum": list(SPEC), "n_spec": n_spec, "seg_capacity": 64, "repeats": args.repeats},
           "spectra_bytes": spectra_bytes, "d2d_copy_of_spectra_ms": copy_ms}
    for name, sw, c in runs:
        o = dict(spread(ms[name]), first_run_ms=first[name], segments_total=None,
                 how="wall clock round Sweep.run (ends in a device synchronise and the copy back)")
        if bm[name]:
            o["k_sweep_bandmin_ms"] = spread(bm[name])
            o["k_sweep_bandmin_over_d2d_copy"] = statistics.median(bm[name]) / copy_ms if copy_ms else None
            o["over_plain"] = o["median_ms"] / statistics.median(ms["plain_1_band"])
        out[name] = o
    for name, sw, c in runs[:2]:
        sw.run(c)
        out[name]["segments_total"] = int(sw.counts().sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--sweep-streams", type=int, default=64)
    ap.add_argument("--windows", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_times.json"))
    args = ap.parse_args()
    push = push_times(args)
    print("push timed", file=sys.stderr, flush=True)
    out = {"push": push, "sweep": sweep_times(args),
           "method": "one process; engines / sweeps take turns, the order alternating between repeats"}
    text = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
