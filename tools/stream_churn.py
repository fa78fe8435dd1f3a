"""What the per-stream lifecycle costs on the bench workload, built the way
bench.py's measure() builds it: 2048 stereo streams, 50-tick pushes of resident
synthetic input (20 distinct pushes), device VADMachines, model seed 1.

Churn against plain: one engine in one process; each repeat times a block of
`steps` plain pushes and a block of `steps` pushes with a
fvad_engine_reset_streams of `churn` rotating streams before each one (the
order alternates between repeats), so both see the same box, clocks and
neighbours.  Reported: the median ms per push of each, the pair's spread (the
larger of the two blocks' max - min over the repeats), and the reset launches'
own event time (FVAD_DEBUG_RESET_TIMES, in a block of its own after the timed
ones, so its event markers are in neither).  If churn - plain exceeds spread +
the launches' own time, a wait in the event graph is the cause and has to be
named.

Save and restore: one timed save and one timed restore of every stream, in ms
and GB/s of blob.

Prints one JSON object and writes it to --out (default
profiles/stream_churn.json).  Run it under a time limit:
  timeout 300 python3 tools/stream_churn.py [--repeats 5] [--steps 20] [--churn 64]"""
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--churn", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_churn.json"))
    args = ap.parse_args()
    B, C, T, P = args.streams, 2, 50, 20
    n = min(args.churn, B)
    model = fvad.Model(seed=1)
    e = fvad.Engine(model, B, C, device=0, max_ticks=T)
    e.attach_vadm()
    e.load_synthetic(T, base=0, pushes=P)
    for _ in range(args.warmup):
        e.run_resident(T)
    e.sync()
    rot = [0]

    def block(churn):
        e.clear_times()
        e.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            if churn:
                e.reset_streams([(rot[0] + i) % B for i in range(n)])
                rot[0] = (rot[0] + n) % B
            e.run_resident(T)
        e.sync()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    ms = {"plain": [], "churn": []}
    for r in range(args.repeats):
        for k in (("plain", "churn") if r % 2 == 0 else ("churn", "plain")):
            ms[k].append(block(k == "churn"))
    e.set_debug(fvad.DEBUG_RESET_TIMES, 1)
    block(True)
    rt_ms, rt_n = e.reset_times()
    e.set_debug(fvad.DEBUG_RESET_TIMES, 0)
    plain, churn = statistics.median(ms["plain"]), statistics.median(ms["churn"])
    spread = max(max(v) - min(v) for v in ms.values())
    own = sum(rt_ms.values())
    out = {"workload": {"streams": B, "channels": C, "ticks_per_push": T, "resident_pushes": P, "vadm": True,
                        "model_seed": 1, "repeats": args.repeats, "steps_per_repeat": args.steps,
                        "reset_streams_per_push": n},
           "plain_ms_per_push": plain, "churn_ms_per_push": churn, "ms_per_push_repeats": ms,
           "churn_minus_plain_ms": churn - plain, "pair_spread_ms": spread,
           "reset_launch_event_ms": rt_ms, "reset_launch_samples": rt_n, "reset_launches_ms": own,
           "within_spread_plus_launches": churn - plain <= spread + own}
    ids = list(range(B))
    e.sync()
    t0 = time.perf_counter()
    blob = e.save_streams(ids)
    t1 = time.perf_counter()
    e.restore_streams(ids, blob)
    t2 = time.perf_counter()
    out["save"] = {"streams": B, "blob_bytes": int(blob.size), "ms": 1e3 * (t1 - t0),
                   "GB_per_s": blob.size / (t1 - t0) / 1e9}
    out["restore"] = {"streams": B, "blob_bytes": int(blob.size), "ms": 1e3 * (t2 - t1),
                      "GB_per_s": blob.size / (t2 - t1) / 1e9}
    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
