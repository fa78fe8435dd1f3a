"""Times per-stream denoised rates at the bench's shape: 2048 stereo streams,
50-tick pushes, model seed 1, host-fed 16-bit 48 kHz samples in steady state
through the pinned input slot (input_slot_i16 / submit_i16 / collect, three
pushes in flight), every push returning its denoised rows to the pinned output
slot.  Three engines, each alone in a process of its own (this script starts
itself once per engine with --kind, one after the other, each under a time
limit):

  mixed     per-stream, half the streams at 8000 out and half at 16000
  ps16      per-stream, every stream at 16000 out
  fixed16   Engine(denoised_rate=16000)

For each: ms per push (every repeat, the median, the spread), the bytes of
denoised PCM a push brings back over PCIe, the output-resample launches' own
time by HIP events (fvad_engine_resample_out_times: all of a push's launches
together), and for the per-stream engines the host time of one
set_stream_denoised_rates call for 256 and for 2048 streams (it makes no device
call).  ps16 against fixed16 is the cost of the indirection, reported against
the spread of fixed16's own repeats; mixed against ps16 shows what a second
launch costs beside what the smaller copy saves.  Writes one JSON object (also
printed).

Usage: python3 tools/stream_denoised_rates_times.py [--repeats 5] [--steps 30] [--warmup 6]
                                                    [--out profiles/stream_denoised_rates_times.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "formula-vad_amd"))
import fvad

KINDS = ("mixed", "ps16", "fixed16")


def rates_of(kind, B):
    return [8000 if kind == "mixed" and s < B // 2 else 16000 for s in range(B)]


class Fed:
    """An engine kept in steady state: three pushes in flight, every submit
    from the pinned slot (filled while it is fresh: the slots cycle)."""

    def __init__(self, model, kind, B, C, T):
        self.T, self.sent, self.flight = T, 0, 0
        if kind == "fixed16":
            self.e = fvad.Engine(model, B, C, device=0, max_ticks=T, want_denoised=True, denoised_rate=16000)
            self.den_bytes = 4 * T * B * C * self.e.frame_out
        else:
            self.e = fvad.Engine(model, B, C, device=0, max_ticks=T, want_denoised=True, denoised_rate="per_stream",
                                 denoised_rate_max=16000)
            self.e.set_stream_denoised_rates(range(B), rates_of(kind, B))
            self.den_bytes = 4 * T * int(self.e.denoised_layout()[-1])
        self.samples = T * B * C * self.e.frame_in
        self.rng = np.random.default_rng(len(kind))

    def step(self):
        e = self.e
        slot = e.input_slot_i16()
        if self.sent < 3:
            t = np.arange(self.samples) / 480.0
            x = 0.3 * np.sin(2 * np.pi * 4.4 * t) + 0.1 * self.rng.uniform(-1, 1, self.samples)
            slot.reshape(-1)[:] = np.round(x * 32768).astype(np.int16)
        e.submit_i16(slot)
        self.sent += 1
        self.flight += 1
        if self.flight == 3:
            e.collect(want=False)  # (the rows are in the pinned slot: the copy to a caller's array is not timed)
            self.flight -= 1

    def drain(self):
        while self.flight:
            self.e.collect(want=False)
            self.flight -= 1


def set_rates_host_ms(e, n, calls=20):
    """median host time of one set_stream_denoised_rates call over n streams (to their own rates)"""
    ids = list(range(n))
    rates = e.stream_denoised_rates()[:n]
    e.sync()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        e.set_stream_denoised_rates(ids, rates)
        ms.append(1e3 * (time.perf_counter() - t0))
    e.sync()
    return statistics.median(ms)


def one(args):
    B, C, T = args.streams, 2, 50
    f = Fed(fvad.Model(seed=1), args.kind, B, C, T)
    for _ in range(args.warmup):
        f.step()
    f.drain()
    ms = []
    for _ in range(args.repeats):
        for _ in range(3):  # back into steady state, outside the timed region
            f.step()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            f.step()
        ms.append(1e3 * (time.perf_counter() - t0) / args.steps)
        f.drain()
    t, n = f.e.resample_out_times()
    o = {"ms_per_push": statistics.median(ms), "ms_per_push_repeats": ms, "spread_ms": max(ms) - min(ms),
         "pcie_denoised_bytes_per_push": f.den_bytes, "resample_out_ms": t, "resample_out_runs": n}
    if f.e.per_stream_out:
        o["set_stream_denoised_rates_host_ms"] = {str(k): set_rates_host_ms(f.e, min(k, B)) for k in (256, 2048)}
    print("RESULT " + json.dumps(o))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--kind", choices=KINDS, help="time this engine in this process (what the script starts itself with)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_denoised_rates_times.json"))
    args = ap.parse_args()
    if args.kind:
        return one(args)
    out = {"workload": {"streams": args.streams, "channels": 2, "ticks_per_push": 50, "model_seed": 1, "in_flight": 3,
                        "input": "int16 at 48 kHz", "denoised": "to the pinned output slot", "repeats": args.repeats,
                        "steps_per_repeat": args.steps, "one_engine_per_process": True}}
    for kind in KINDS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--kind", kind, "--repeats", str(args.repeats),
                            "--steps", str(args.steps), "--warmup", str(args.warmup), "--streams", str(args.streams)],
                           capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit("engine %s failed (%d): not going on" % (kind, r.returncode))
        out[kind] = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])
    d = out["ps16"]["ms_per_push"] - out["fixed16"]["ms_per_push"]
    out["indirection"] = {"ps16_minus_fixed16_ms": d, "fixed16_spread_ms": out["fixed16"]["spread_ms"],
                          "within_fixed16_spread": abs(d) <= out["fixed16"]["spread_ms"],
                          "resample_out_ms_ps16_minus_fixed16": out["ps16"]["resample_out_ms"] - out["fixed16"]["resample_out_ms"]}
    out["second_rate"] = {"mixed_minus_ps16_ms": out["mixed"]["ms_per_push"] - out["ps16"]["ms_per_push"],
                          "resample_out_ms_mixed_minus_ps16": out["mixed"]["resample_out_ms"] - out["ps16"]["resample_out_ms"]}
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
