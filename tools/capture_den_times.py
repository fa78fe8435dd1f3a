"""Times the four ways to get speech audio out of a host-fed engine, at the
bench's shape: 2048 stereo streams, 50-tick pushes, model seed 1, staged
engine, one device VADMachine per stream with the event feed on, 16-bit input
through the pinned slots in steady state (input_slot_i16 / submit_i16 /
collect, three pushes in flight), events and clips polled after every push.

  a  want_denoised = 1, denoised_rate 16000, no capture: every tick's denoised
     rows come back with every push, the host would cut the segments itself
  b  clip capture of the input (INPUT, f32, 48 kHz), want_denoised = 0
  c  want_denoised = 2, denoised_rate 16000, DENOISED s16 capture: the rows
     stay on the device, only the clips cross
  d  c at 8000
  n  neither: want_denoised = 0, no capture -- the floor the others stand on

EACH ENGINE RUNS ALONE IN A PROCESS OF ITS OWN (as tools/denoised_rate_times.py
does, and for its reason): this script starts one child per kind and merges
what they print.

The input.  The three pinned slots are filled once and cycle, so the signal
has a period of three pushes, 1.5 s.  Every third stream hears 1.0 s of a
synthetic stream's labelled speech, then 0.5 s of faint noise, the streams
spread evenly over the period's three phases; the others hear the faint noise
only.  With the machine opening after 0.1 s, closing after a gap of 0.2 s and
keeping segments from 0.3 s, a speaking stream gives about one segment a
period, and each clip carries the segment and its 2 s tail (clips overlap):
about a third of a second of clip per stream and push, the same for every
kind.  64 distinct streams, repeated over the 2048 slots; the parent process
builds the three slots' contents once and hands them to the children in a
temporary file.

Per kind: ms per push (every repeat, the median, the spread), the bytes a push
returns over PCIe as denoised rows and as clips, clips and clips lost, the
append's and the pass's own times (fvad_engine_capture_times: the DENOISED
append is timed on every push, the pass on the sampled ones, which in a
host-fed run are the sync points') and the memory capture holds.

Usage: python3 tools/capture_den_times.py [--repeats 5] [--steps 30] [--warmup 6]
                                          [--out profiles/capture_den_times.json]
       python3 tools/capture_den_times.py --kind c   (one child: prints its JSON object)"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "formula-vad_amd"))

KINDS = {"a": dict(den=True, rate=16000, capture=None),
         "b": dict(den=False, rate=0, capture=("input", "f32")),
         "c": dict(den="device", rate=16000, capture=("denoised", "s16")),
         "d": dict(den="device", rate=8000, capture=("denoised", "s16")),
         "n": dict(den=False, rate=0, capture=None)}
DISTINCT = 64


def period(fvad, B, T):
    """[3][T][B][2][480] int16: the three slots' contents."""
    n = T * 480
    rng = np.random.default_rng(48)
    src = np.zeros((3, min(B, DISTINCT), 2, n), np.float32)
    for sid in range(src.shape[1]):
        x, lab = fvad.synth_stream(sid, 10 * 48000, 2)
        at = 0
        for lo, hi in lab:
            if hi - lo >= 2.0 * n / 48000.0 + 0.05:
                at = int(lo * 48000) + 480
                break
        src[0, sid], src[1, sid] = x[:, at:at + n], x[:, at + n:at + 2 * n]
    src[2] = 1e-3 * rng.uniform(-1, 1, src[2].shape)
    q = np.clip(np.rint(src * 32768.0), -32768, 32767).astype(np.int16)
    # [3][sid][ch][T * 480] -> [3][T][sid][ch][480]
    q = q.reshape(3, q.shape[1], 2, T, 480).transpose(0, 3, 1, 2, 4)
    # slot k of stream s: part (k + s // 3) % 3 of the period for every third stream, the noise for the others
    s = np.arange(B)
    out = np.empty((3, T, B, 2, 480), np.int16)
    for k in range(3):
        part = np.where(s % 3 == 0, (k + s // 3) % 3, 2)
        out[k] = q[part, :, s % q.shape[2]].transpose(1, 0, 2, 3)
    return out


def child(args):
    import fvad
    kind = KINDS[args.kind]
    B, Ch, T = args.streams, 2, 50
    model = fvad.Model(seed=1)
    e = fvad.Engine(model, B, Ch, device=0, max_ticks=T, want_denoised=kind["den"], denoised_rate=kind["rate"])
    cfg = fvad.VadmConfig.default()
    cfg.min_consecutive_sec_to_open, cfg.max_speech_gap_sec, cfg.min_vad_duration_sec = 0.1, 0.2, 0.3
    e.attach_vadm([cfg])
    e.enable_events()
    s16 = False
    if kind["capture"]:
        source, fmt = kind["capture"]
        e.enable_capture(0, args.history, args.pool, source=source, fmt=fmt)
        s16 = fmt == "s16"
    content = np.load(args.content) if args.content else period(fvad, B, T)
    assert content.shape == (3, T, B, Ch, 480) and content.dtype == np.int16
    L = fvad.lib()
    poll = L.fvad_engine_poll_clip_s16 if s16 else L.fvad_engine_poll_clip
    st = {"sent": 0, "flight": 0, "clips": 0, "samples": 0, "bare": 0, "events": 0, "poll_s": 0.0,
          "buf": np.zeros(1 << 20, np.int16 if s16 else np.float32)}
    info, lost = fvad.Clip(), C.c_uint64()

    def drain_clips():
        if not kind["capture"]:
            return
        t0 = time.perf_counter()
        while True:
            buf = st["buf"]
            rc = poll(e.h, C.byref(info), buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(lost))
            if rc == fvad.EINVAL and info.n_samples > buf.size:
                st["buf"] = np.zeros(int(info.n_samples), buf.dtype)
                continue
            if rc < 0:
                raise fvad.FvadError("poll failed (%d): %s" % (rc, fvad.last_error()))
            if rc == 0:
                break
            st["clips"] += 1
            st["samples"] += info.n_samples
            st["bare"] += bool(info.flags & fvad.CLIP_NO_AUDIO)
        st["poll_s"] += time.perf_counter() - t0

    def step():
        slot = e.input_slot_i16()
        if st["sent"] < 3:  # filled once: the slots cycle
            slot[:] = content[st["sent"]]
        e.submit_i16(slot)
        st["sent"] += 1
        st["flight"] += 1
        if st["flight"] == 3:
            e.collect(want=False)
            st["flight"] -= 1
        st["events"] += len(e.poll_events()[0])
        drain_clips()

    def drain():
        while st["flight"]:
            e.collect(want=False)
            st["flight"] -= 1

    for _ in range(args.warmup):
        step()
    drain()
    e.sync()
    drain_clips()
    e.clear_times()
    ms, append_ms, pass_ms = [], [], []
    for k in ("clips", "samples", "bare", "events"):
        st[k] = 0
    st["poll_s"] = 0.0
    for _ in range(args.repeats):
        for _ in range(3):  # back into steady state, outside the timed region
            step()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        ms.append(1e3 * (time.perf_counter() - t0) / args.steps)
        drain()
        e.sync()
        drain_clips()
    pass_runs = 0
    if kind["capture"]:  # (averages since the clear_times behind the warm-up)
        t, pass_runs = e.capture_times()
        append_ms.append(t["k_hist_append"])
        if pass_runs:
            pass_ms.append(t["capture_pass"])
    pushes = args.repeats * (args.steps + 3)
    bytes_per = 2 if s16 else 4
    o = {"ms_per_push": statistics.median(ms), "ms_per_push_repeats": ms, "spread_ms": max(ms) - min(ms),
         "want_denoised": e.cfg.want_denoised, "denoised_rate": kind["rate"],
         "denoised_bytes_per_push": T * B * Ch * e.frame_out * 4 if kind["den"] is True else 0,
         "input_bytes_per_push": T * B * Ch * fvad.FRAME * 2, "events_per_push": st["events"] / pushes}
    if kind["capture"]:
        R = e.clip_rate()
        hist = int(R * args.history)
        H = (hist + T * (R // 100) + 3) & ~3
        o.update({"clip_rate": R, "clip_format": kind["capture"][1], "clips_per_push": st["clips"] / pushes,
                  "clip_samples_per_push": st["samples"] / pushes, "clip_bytes_per_push": bytes_per * st["samples"] / pushes,
                  "clips_without_audio": st["bare"], "clips_lost": lost.value,
                  "append_ms": append_ms[0] if append_ms else None,
                  "capture_pass_ms": pass_ms[0] if pass_ms else None, "capture_pass_runs": pass_runs,
                  "host_poll_ms_per_push": 1e3 * st["poll_s"] / pushes,
                  "history_ring_bytes": B * Ch * H * 4, "pool_bytes": (args.pool or 64 << 20) * bytes_per})
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
    ap.add_argument("--history", type=float, default=10.0)
    ap.add_argument("--pool", type=int, default=0, help="pool_samples (0: the library's default, 64 Mi)")
    ap.add_argument("--kind", choices=sorted(KINDS), default=None, help="run this engine in this process and print its figures")
    ap.add_argument("--content", default=None, help="(a child's) the slots' contents, a .npy file written by the parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capture_den_times.json"))
    args = ap.parse_args()
    if args.kind:
        return child(args)
    out = {"what": "tools/capture_den_times.py: host-fed pushes (16-bit input, pinned slots, three in flight, machines "
                   "and the event feed on, events and clips polled after every push), each engine alone in a process "
                   "of its own, one after another",
           "kinds": {"a": "want_denoised 1, denoised_rate 16000, no capture", "b": "INPUT f32 capture at 48 kHz",
                     "c": "want_denoised 2, denoised_rate 16000, DENOISED s16 capture", "d": "c at 8000", "n": "want_denoised 0, no capture"},
           "workload": {"streams": args.streams, "channels": 2, "ticks_per_push": 50, "model_seed": 1, "mode": "staged",
                        "in_flight": 3, "repeats": args.repeats, "steps_per_repeat": args.steps,
                        "history_sec": args.history, "pool_samples": args.pool or 64 << 20, "signal_period_pushes": 3}}
    import tempfile
    import fvad
    tmp = tempfile.TemporaryDirectory()
    content = os.path.join(tmp.name, "content.npy")
    np.save(content, period(fvad, args.streams, 50))
    for kind in sorted(KINDS):
        cmd = [sys.executable, os.path.abspath(__file__), "--kind", kind, "--repeats", str(args.repeats),
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--streams", str(args.streams),
               "--history", str(args.history), "--pool", str(args.pool), "--content", content]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:  # (a child that failed: nothing more is started)
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit("kind %s failed with status %d" % (kind, r.returncode))
        line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
        out[kind] = json.loads(line[len("RESULT "):])
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
