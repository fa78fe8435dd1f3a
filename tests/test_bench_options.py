"""bench.py's --full and --dump-outputs, CPU only: a plain run switches off
every leg beyond the timed steps, --full keeps them (each still switchable),
and dump_outputs writes the last push's arrays of a simulated engine group as
float32 / float64 .npy files, the same from call to call, with a fixed seeded
sample of the streams once the whole would pass its size cap."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

LEGS = ("cpu_baseline", "host_rate", "variants", "one_engine_leg")


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_has_no_extra_leg(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert not a.full and a.dump_outputs is None
    assert (a.steps, a.warmup) == (7, 2)
    assert [getattr(a, k) for k in LEGS] == [0, 0, 0, 0]
    # a leg's own switch does not bring it back without --full
    a = parse(monkeypatch, "--host-rate", "1", "--variants", "1")
    assert [getattr(a, k) for k in LEGS] == [0, 0, 0, 0]


def test_full_keeps_the_legs(monkeypatch):
    a = parse(monkeypatch, "--full")
    assert a.full and [getattr(a, k) for k in LEGS] == [1, 1, 1, 1]
    a = parse(monkeypatch, "--full", "--cpu-baseline", "0", "--variants", "0", "--dump-outputs", "d")
    assert [getattr(a, k) for k in LEGS] == [0, 1, 0, 1] and a.dump_outputs == "d"


class FakeEngine:
    def __init__(self, first, n, T, C):
        self.first, self.n, self.T, self.C = first, n, T, C

    def fetch(self, n_ticks):
        assert n_ticks == self.T
        s = np.arange(self.first, self.first + self.n, dtype=np.float32)
        tb = np.arange(self.T, dtype=np.float32)[:, None] * 1000 + s[None, :]
        return {"vad": tb, "ratio": tb + 0.5, "win_flag": (tb % 2).astype(np.int32), "win_ratio": tb + 0.25,
                "win_vad": tb + 0.75, "band": np.repeat(tb[:, :, None, None], self.C, axis=2)}


class FakeGroup:
    def __init__(self, T, sizes, C):
        self.sizes, self.B = sizes, sum(sizes)
        self.first = [sum(sizes[:g]) for g in range(len(sizes))]
        self.engines = [FakeEngine(f, n, T, C) for f, n in zip(self.first, sizes)]

    def segments(self, stream, machine=0):
        return [(480 * stream, 480 * stream + 960, 0.5, 0.25)] * (stream % 3)


class Args:
    ticks = 3
    dump_outputs = None


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_arrays(tmp_path):
    A = Args()
    A.dump_outputs = str(tmp_path / "a")
    grp = FakeGroup(A.ticks, [3, 2], 2)
    bench.dump_outputs(grp, A, 0, True)
    got = load(A.dump_outputs)
    assert sorted(got) == ["band", "ratio", "segments", "streams", "vad", "win_flag", "win_ratio", "win_vad"]
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert got["vad"].shape == (3, 5) and got["band"].shape == (3, 5, 2, 1)
    assert np.array_equal(got["vad"][2], 2000 + np.arange(5))  # engines joined on the stream axis
    assert np.array_equal(got["streams"], np.arange(5))
    want = [(s, 480 * s, 480 * s + 960, 0.5, 0.25) for s in range(5) for _ in range(s % 3)]
    assert np.array_equal(got["segments"], np.array(want, np.float64))
    # no machines: no segments file; another rank: its own names; same arrays again
    A.dump_outputs = str(tmp_path / "b")
    bench.dump_outputs(grp, A, 1, False)
    again = load(A.dump_outputs)
    assert sorted(again) == sorted(k + ".rank1" for k in got if k != "segments")
    assert all(np.array_equal(again[k + ".rank1"], got[k]) for k in got if k != "segments")


def test_dump_outputs_size_cap(tmp_path, monkeypatch):
    A = Args()
    grp = FakeGroup(A.ticks, [40, 24], 2)
    per_stream = A.ticks * 4 * (5 + 2) + 8
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 2 * 10 * per_stream)  # room for 10 of the 64 streams
    total = []
    for name in ("a", "b"):
        A.dump_outputs = str(tmp_path / name)
        bench.dump_outputs(grp, A, 0, True)
        got = load(A.dump_outputs)
        keep = got["streams"].astype(int)
        assert len(keep) == 10 and np.all(np.diff(keep) > 0) and keep.max() < 64
        assert np.array_equal(got["vad"][1], 1000 + keep)
        assert set(got["segments"][:, 0]) <= set(keep)
        assert sum(v.nbytes for v in got.values()) <= bench.DUMP_CAP_BYTES
        total.append(got)
    assert all(np.array_equal(total[0][k], total[1][k]) for k in total[0])  # the sample is fixed
