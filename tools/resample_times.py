"""Times the input resampling at the bench's shape: 2048 stereo streams,
50-tick pushes, model seed 1, host-fed in steady state through the pinned
input slots (input_slot[_i16] / submit[_i16] / collect, three pushes in
flight).  Four staged engines live in one process -- 48 kHz, 16 kHz and 8 kHz
fed 16-bit samples, 44.1 kHz fed float -- and take turns: each repeat times
`steps` pushes of each (the order alternates between repeats), so all see the
same box, clocks and neighbours.  Writes one JSON object (also printed): ms per
push of each (every repeat, the median, the spread), the bytes a push sends
over PCIe, the resample launches' own time by HIP events
(fvad_engine_resample_times), and beside it the time of a device-to-device copy
of the bytes k_resample writes, measured here with events too: a floor no
kernel writing those bytes can beat.  --kinds 16000_i16 builds and times that
engine alone (profiles/resample_times_single.json: each of the four in a
process of its own; four engines' streams share the process's hardware queues).

Usage: python3 tools/resample_times.py [--repeats 5] [--steps 30] [--warmup 6] [--kinds a,b]
                                       [--out profiles/resample_times.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "formula-vad_amd"))
import fvad

KINDS = (("48000_i16", 48000, True), ("16000_i16", 16000, True), ("8000_i16", 8000, True), ("44100_f32", 44100, False))


def d2d_copy_ms(n_bytes, repeats=20):
    """Median event time of a device-to-device copy of n_bytes (the HIP runtime
    libfvad.so already runs on, through ctypes)."""
    import ctypes as C
    fvad.lib()
    with open("/proc/self/maps") as f:  # the copy of the runtime this process has loaded
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = C.CDLL(path)

    def ok(rc):
        assert rc == 0, "HIP error %d" % rc

    src, dst, a, b = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipSetDevice(0))
    ok(hip.hipMalloc(C.byref(src), C.c_size_t(n_bytes)))
    ok(hip.hipMalloc(C.byref(dst), C.c_size_t(n_bytes)))
    ok(hip.hipMemset(src, 0, C.c_size_t(n_bytes)))
    ok(hip.hipEventCreate(C.byref(a)))
    ok(hip.hipEventCreate(C.byref(b)))
    ms = []
    for _ in range(repeats + 3):
        ok(hip.hipEventRecord(a, None))
        ok(hip.hipMemcpyAsync(dst, src, C.c_size_t(n_bytes), 3, None))  # hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(b, None))
        ok(hip.hipEventSynchronize(b))
        t = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(t), a, b))
        ms.append(t.value)
    for ev in (a, b):
        ok(hip.hipEventDestroy(ev))
    for p in (src, dst):
        ok(hip.hipFree(p))
    return statistics.median(ms[3:])


class Fed:
    """An engine kept in steady state: three pushes in flight, every submit
    from a pinned slot (filled once: the slots cycle), one collect per submit."""

    def __init__(self, model, B, C, T, rate, i16):
        self.e = fvad.Engine(model, B, C, device=0, max_ticks=T, input_rate=rate)
        self.i16, self.T, self.sent, self.flight = i16, T, 0, 0
        self.rng = np.random.default_rng(rate)
        self.bytes = T * B * C * self.e.frame_in * (2 if i16 else 4)

    def step(self):
        e = self.e
        slot = e.input_slot_i16() if self.i16 else e.input_slot()
        if self.sent < 3:
            t = np.arange(slot.shape[-1]) / (100.0 * slot.shape[-1])
            x = 0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.1 * self.rng.uniform(-1, 1, slot.shape[1:]).astype(np.float32)
            slot[:] = np.round(x * 32768).astype(np.int16) if self.i16 else x.astype(np.float32)
        (e.submit_i16 if self.i16 else e.submit)(slot)
        self.sent += 1
        self.flight += 1
        if self.flight == 3:
            e.collect(want=False)
            self.flight -= 1

    def drain(self):
        while self.flight:
            self.e.collect(want=False)
            self.flight -= 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_times.json"))
    ap.add_argument("--kinds", default=",".join(k[0] for k in KINDS),
                    help="the engines to build and interleave (default: all four)")
    args = ap.parse_args()
    B, C, T = args.streams, 2, 50
    model = fvad.Model(seed=1)
    kinds = [k for k in KINDS if k[0] in args.kinds.split(",")]
    fed = {}
    for name, rate, i16 in kinds:
        f = Fed(model, B, C, T, rate, i16)
        for _ in range(args.warmup):
            f.step()
        f.drain()
        fed[name] = f
    names = [k[0] for k in kinds]
    ms = {k: [] for k in names}
    for r in range(args.repeats):
        for k in (names if r % 2 == 0 else names[::-1]):
            f = fed[k]
            for _ in range(3):  # back into steady state, outside the timed region
                f.step()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                f.step()
            ms[k].append(1e3 * (time.perf_counter() - t0) / args.steps)
            f.drain()
    out_bytes = T * B * C * fvad.FRAME * 4
    copy_ms = d2d_copy_ms(out_bytes)
    out = {"workload": {"streams": B, "channels": C, "ticks_per_push": T, "model_seed": 1, "in_flight": 3,
                        "repeats": args.repeats, "steps_per_repeat": args.steps},
           "resample_output_bytes": out_bytes, "d2d_copy_of_output_ms": copy_ms}
    for k in names:
        f = fed[k]
        o = {"ms_per_push": statistics.median(ms[k]), "ms_per_push_repeats": ms[k],
             "spread_ms": max(ms[k]) - min(ms[k]), "pcie_bytes_per_push": f.bytes}
        if f.e.frame_in != fvad.FRAME:
            t, n = f.e.resample_times()
            o["resample_ms"], o["resample_runs"] = t, n
            o["resample_over_d2d_copy"] = t / copy_ms if copy_ms else None
        out[k] = o
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
