"""Denoised / 16-bit clip capture's host side, no GPU: the new calls are
exported, bound and declared in the header; fvad_capture_config_default's
values; a null engine is rejected; fvad_pcm_f32_to_s16 equals numpy.rint(x *
32768) clipped, value for value; fvad_clip_range equals ceil(x L / M) in
Python integers at all seven rates; and csrc/fvad_capture_core.h's clip-rate
arithmetic (cap::to_rate, due and cut in clip-rate units, cap::to_s16) agrees
with a direct model as a stand-alone program under AddressSanitizer and
UBSan."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "formula-vad_amd", "csrc")
CALLS = {"fvad_capture_config_default": "void", "fvad_engine_enable_capture_ex": "int",
         "fvad_engine_poll_clip_s16": "int", "fvad_engine_clip_rate": "int", "fvad_pcm_f32_to_s16": "void",
         "fvad_clip_range": "int"}
RATES = (48000, 8000, 16000, 24000, 32000, 44100, 96000)
EINVAL = -1


def header():
    return open(os.path.join(ROOT, "include", "fvad.h")).read()


def defines():
    return dict((k, int(v)) for k, v in re.findall(r"#define\s+(FVAD_[A-Z0-9_]+)\s+\(?(-?\d+)\)?", header()))


def test_symbols_exported(fvad_mod):
    L = fvad_mod.lib()
    hdr = header()
    bound = {name for name, _, _ in fvad_mod.SYMBOLS}
    for name, res in CALLS.items():
        assert hasattr(L, name), name
        assert name in bound, name
        assert re.search(r"\b%s\s+%s\s*\(" % (res, name), hdr), name
    for m in ("enable_capture", "poll_clips", "clip_rate"):
        assert callable(getattr(fvad_mod.Engine, m)), m
    assert callable(fvad_mod.pcm_f32_to_s16) and callable(fvad_mod.clip_range)
    d = defines()
    assert (d["FVAD_CLIP_SOURCE_INPUT"], d["FVAD_CLIP_SOURCE_DENOISED"]) == (0, 1) == \
        (fvad_mod.CLIP_SOURCE_INPUT, fvad_mod.CLIP_SOURCE_DENOISED)
    assert (d["FVAD_CLIP_F32"], d["FVAD_CLIP_S16"]) == (0, 1) == (fvad_mod.CLIP_F32, fvad_mod.CLIP_S16)
    # the header says that the filter delay is not compensated
    assert re.search(r"delay[^;]*NOT\s+compensated", hdr, re.S)


def test_config_default_and_layout(fvad_mod, tmp_path):
    c = fvad_mod.CaptureConfig()
    C.memset(C.byref(c), 0xff, C.sizeof(c))
    fvad_mod.lib().fvad_capture_config_default(C.byref(c))
    assert (c.machine, c.history_sec, c.pool_samples, c.source, c.format) == (0, 10.0, 0, 0, 0)
    fvad_mod.lib().fvad_capture_config_default(None)  # tolerated
    # the binding's layout is the header's own, through the C compiler
    src = tmp_path / "layout.c"
    checks = ["_Static_assert(sizeof(fvad_capture_config) == %d, \"size\");" % C.sizeof(c),
              "_Static_assert(sizeof(fvad_clip) == 64, \"clip\");"]
    for name, _ in fvad_mod.CaptureConfig._fields_:
        checks.append("_Static_assert(offsetof(fvad_capture_config, %s) == %d, \"%s\");"
                      % (name, getattr(fvad_mod.CaptureConfig, name).offset, name))
    src.write_text("#include <stddef.h>\n#include \"fvad.h\"\n" + "\n".join(checks) + "\nint main(void) { return 0; }\n")
    r = subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_calls_reject_null(fvad_mod):
    L = fvad_mod.lib()
    info, lost = fvad_mod.Clip(), C.c_uint64()
    c = fvad_mod.CaptureConfig.default()
    assert L.fvad_engine_enable_capture_ex(None, C.byref(c)) == EINVAL
    assert L.fvad_engine_poll_clip_s16(None, C.byref(info), None, 0, C.byref(lost)) == EINVAL
    assert L.fvad_engine_clip_rate(None) == 0


def want_s16(x):
    """numpy's statement of the conversion; NaN -> 0."""
    x = np.asarray(x, np.float32)
    y = np.rint(x * np.float32(32768.0))
    y = np.where(np.isnan(y), np.float32(0), y)
    return np.clip(y, -32768, 32767).astype(np.int16)


def test_pcm_f32_to_s16(fvad_mod):
    rng = np.random.default_rng(5)
    x = rng.uniform(-1.5, 1.5, 200000).astype(np.float32)
    got = fvad_mod.pcm_f32_to_s16(x)
    assert got.dtype == np.int16 and np.array_equal(got, want_s16(x))
    assert got.min() == -32768 and got.max() == 32767  # both clamps were reached
    k = np.arange(-300, 300, dtype=np.float32)
    ties = ((k + np.float32(0.5)) / np.float32(32768.0)).astype(np.float32)
    assert np.array_equal(ties * np.float32(32768.0), k + np.float32(0.5))  # the ties are exact
    got = fvad_mod.pcm_f32_to_s16(ties)
    assert np.array_equal(got, want_s16(ties))
    assert np.all(got % 2 == 0)  # every tie went to the even neighbour
    assert list(fvad_mod.pcm_f32_to_s16(np.float32([0.5, 1.5, 2.5, -0.5, -1.5, -2.5]) / np.float32(32768))) == \
        [0, 2, 2, 0, -2, -2]
    edge = np.float32([1.0, -1.0, 0.0, -0.0, np.nan, np.inf, -np.inf])
    assert list(fvad_mod.pcm_f32_to_s16(edge)) == [32767, -32768, 0, 0, 0, 32767, -32768] == list(want_s16(edge))
    assert fvad_mod.pcm_f32_to_s16(np.zeros((3, 5), np.float32)).shape == (3, 5)


def test_clip_range(fvad_mod):
    L = fvad_mod.lib()
    erate = defines()["FVAD_ERATE"]
    rng = np.random.default_rng(6)
    for rate in RATES:
        g = math.gcd(48000, rate)
        l, m = rate // g, 48000 // g
        cases = [(0, 0), (0, 1), (1, 1), (479, 480), (480, 960)]
        for _ in range(2000):
            a, b = sorted(int(v) for v in rng.integers(0, 2 ** 40, 2))
            cases.append((a, b))
        for _ in range(500):
            a = int(rng.integers(0, 10 ** 7))
            cases.append((a, a + int(rng.integers(0, 10 ** 6))))
        for a, b in cases:
            want = (-(-a * l // m), -(-b * l // m))
            assert fvad_mod.clip_range(rate, a, b) == want, (rate, a, b)
            if rate == 48000:
                assert want == (a, b)
        first, end = C.c_uint64(7), C.c_uint64(7)
        assert L.fvad_clip_range(rate, 5, 4, C.byref(first), C.byref(end)) == EINVAL
        assert (first.value, end.value) == (7, 7)
        assert L.fvad_clip_range(rate, 4, 5, None, None) == 0  # both results are optional
    for rate in (0, 22050, 11025, 48001, -16000, 192000):
        first, end = C.c_uint64(7), C.c_uint64(7)
        assert L.fvad_clip_range(rate, 0, 480, C.byref(first), C.byref(end)) == erate, rate
        assert (first.value, end.value) == (7, 7)


def test_rate_core_against_a_direct_model(tmp_path):
    """tests/capture_rate_harness.cpp: cap::to_rate, the due test in both units
    (ceil(to L / M) <= pos L / M iff to <= pos for pos a multiple of 480), the
    cut in clip-rate units and cap::to_s16 against direct models on 200 000
    random cases; a stand-alone program with its own main, under
    -fsanitize=address,undefined (any report fails the run)."""
    exe = tmp_path / "capture_rate"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC,
                           os.path.join(ROOT, "tests", "capture_rate_harness.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 / 200000 mismatches, 0 s16 mismatches" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
