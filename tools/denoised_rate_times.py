"""Times a host-fed push that returns its denoised PCM, at the bench's shape:
2048 stereo streams, 50-tick pushes, model seed 1, staged engine, 16-bit input
through the pinned slots in steady state (input_slot_i16 / submit_i16 /
collect, three pushes in flight; the denoised rows arrive in the slot's pinned
buffer with every push).  Three engines are compared: want_denoised at 48 kHz,
denoised_rate 16000 and denoised_rate 8000.  EACH ENGINE RUNS ALONE IN A
PROCESS OF ITS OWN: this script starts one child per kind (engines interleaved
in one process gave a figure that did not reproduce) and
merges what they print.  Per kind: ms per push (every repeat, the median, the
spread), the denoised bytes a push returns over PCIe, and the event time of a
push's two output-resample launches (fvad_engine_resample_out_times).
A fourth kind, "none", is the same feed without want_denoised: the floor the
copy of the denoised rows stands on.

Usage: python3 tools/denoised_rate_times.py [--repeats 5] [--steps 30] [--warmup 6]
                                            [--out profiles/denoised_rate_times.json]
       python3 tools/denoised_rate_times.py --kind 16000   (one child: prints its JSON object)"""
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

KINDS = ("none", "48000", "16000", "8000")


def child(args):
    import fvad
    B, C, T = args.streams, 2, 50
    model = fvad.Model(seed=1)
    den = args.kind != "none"
    e = fvad.Engine(model, B, C, device=0, max_ticks=T, want_denoised=den,
                    denoised_rate=int(args.kind) if den else 0)
    rng = np.random.default_rng(48)
    state = {"sent": 0, "flight": 0}

    def step():
        slot = e.input_slot_i16()
        if state["sent"] < 3:  # filled once: the slots cycle
            t = np.arange(slot.shape[-1]) / (100.0 * slot.shape[-1])
            x = 0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.1 * rng.uniform(-1, 1, slot.shape[1:]).astype(np.float32)
            slot[:] = np.round(x * 32768).astype(np.int16)
        e.submit_i16(slot)
        state["sent"] += 1
        state["flight"] += 1
        if state["flight"] == 3:
            e.collect(want=False)
            state["flight"] -= 1

    def drain():
        while state["flight"]:
            e.collect(want=False)
            state["flight"] -= 1

    for _ in range(args.warmup):
        step()
    drain()
    ms = []
    for _ in range(args.repeats):
        for _ in range(3):  # back into steady state, outside the timed region
            step()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        ms.append(1e3 * (time.perf_counter() - t0) / args.steps)
        drain()
    o = {"ms_per_push": statistics.median(ms), "ms_per_push_repeats": ms, "spread_ms": max(ms) - min(ms),
         "denoised_frame": e.frame_out if den else 0,
         "denoised_bytes_per_push": T * B * C * e.frame_out * 4 if den else 0,
         "input_bytes_per_push": T * B * C * fvad.FRAME * 2}
    if e.frame_out != fvad.FRAME:
        t, n = e.resample_out_times()
        o["resample_out_ms"], o["resample_out_runs"] = t, n
    print("RESULT " + json.dumps(o))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--kind", choices=KINDS, default=None, help="run this engine in this process and print its figures")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoised_rate_times.json"))
    args = ap.parse_args()
    if args.kind:
        return child(args)
    out = {"what": "tools/denoised_rate_times.py: host-fed pushes (16-bit input, pinned slots, three in flight) that "
                   "return their denoised PCM, each engine alone in a process of its own, one after another",
           "workload": {"streams": args.streams, "channels": 2, "ticks_per_push": 50, "model_seed": 1, "mode": "staged",
                        "in_flight": 3, "repeats": args.repeats, "steps_per_repeat": args.steps}}
    for kind in KINDS:
        cmd = [sys.executable, os.path.abspath(__file__), "--kind", kind, "--repeats", str(args.repeats),
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--streams", str(args.streams)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:  # (a child that failed: nothing more is started)
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit("kind %s failed with status %d" % (kind, r.returncode))
        line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
        out["none" if kind == "none" else "denoised_%s" % kind] = json.loads(line[len("RESULT "):])
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
