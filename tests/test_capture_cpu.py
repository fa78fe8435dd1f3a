"""Clip capture's host side, no GPU: the four calls are exported and bound,
fvad_clip is laid out as the header states (64 bytes, no padding) in the
binding and in a C compile of the header itself, the flag values agree, the
calls reject a null engine, and the plan's decision code
(csrc/fvad_capture_core.h, which k_cap_plan compiles) agrees with a direct
model on random cases, as a stand-alone program under AddressSanitizer and
UBSan."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "formula-vad_amd", "csrc")
CALLS = ("fvad_engine_enable_capture", "fvad_engine_poll_clip", "fvad_engine_capture_flush",
         "fvad_engine_capture_times")

# name -> (offset, size) as include/fvad.h lays fvad_clip out
LAYOUT = {"stream": (0, 4), "seq": (4, 4), "channel": (8, 4), "flags": (12, 4), "push": (16, 8),
          "sample_from": (24, 8), "sample_to": (32, 8), "first_sample": (40, 8), "n_samples": (48, 8),
          "reserved": (56, 8)}


def test_capture_symbols_exported(fvad_mod):
    L = fvad_mod.lib()
    hdr = open(os.path.join(ROOT, "include", "fvad.h")).read()
    bound = {name for name, _, _ in fvad_mod.SYMBOLS}
    for name in CALLS:
        assert hasattr(L, name), name
        assert name in bound, name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    for m in ("enable_capture", "poll_clips", "capture_flush", "capture_times"):
        assert callable(getattr(fvad_mod.Engine, m)), m


def test_clip_struct_layout(fvad_mod):
    clip = fvad_mod.Clip
    assert C.sizeof(clip) == 64
    assert [n for n, _ in clip._fields_] == list(LAYOUT)
    for name, (off, size) in LAYOUT.items():
        f = getattr(clip, name)
        assert (f.offset, f.size) == (off, size), name
    hdr = open(os.path.join(ROOT, "include", "fvad.h")).read()
    defs = dict((k, int(v)) for k, v in re.findall(r"#define\s+(FVAD_[A-Z0-9_]+)\s+(-?\d+)\b", hdr))
    assert fvad_mod.CLIP_HEAD_SHORT == defs["FVAD_CLIP_HEAD_SHORT"] == 1
    assert fvad_mod.CLIP_TAIL_SHORT == defs["FVAD_CLIP_TAIL_SHORT"] == 2
    assert fvad_mod.CLIP_NO_AUDIO == defs["FVAD_CLIP_NO_AUDIO"] == 4
    core = open(os.path.join(CSRC, "fvad_capture_core.h")).read()
    m = re.search(r"kHeadShort = (\d+), kTailShort = (\d+), kNoAudio = (\d+)", core)
    assert m and [int(v) for v in m.groups()] == [1, 2, 4]


def test_clip_struct_layout_in_c(tmp_path):
    """The header's own struct, through the C compiler the oracle is built with."""
    src = tmp_path / "layout.c"
    checks = ["_Static_assert(sizeof(fvad_clip) == 64, \"size\");"]
    for name, (off, _) in LAYOUT.items():
        checks.append("_Static_assert(offsetof(fvad_clip, %s) == %d, \"%s\");" % (name, off, name))
    src.write_text("#include <stddef.h>\n#include \"fvad.h\"\n" + "\n".join(checks) + "\nint main(void) { return 0; }\n")
    cc = os.environ.get("CC", "gcc")
    r = subprocess.run([cc, "-std=gnu11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_capture_calls_reject_null(fvad_mod):
    L = fvad_mod.lib()
    info, lost = fvad_mod.Clip(), C.c_uint64()
    assert L.fvad_engine_enable_capture(None, 0, 10.0, 0) == -1  # FVAD_EINVAL
    assert L.fvad_engine_poll_clip(None, C.byref(info), None, 0, C.byref(lost)) == -1
    assert L.fvad_engine_capture_flush(None, None, 0) == -1
    assert L.fvad_engine_capture_times(None, None, None) == -1


def test_capture_core_against_a_direct_model(tmp_path):
    """tests/capture_core_harness.cpp: due, cut, queue overflow, ring room and
    placement of csrc/fvad_capture_core.h against a 128-bit model on 200 000
    random cases clustered at the edges; a stand-alone program with its own
    main, under -fsanitize=address,undefined (any report fails the run)."""
    exe = tmp_path / "capture_core"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC,
                           os.path.join(ROOT, "tests", "capture_core_harness.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 / 200000 mismatches" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
