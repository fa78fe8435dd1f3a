"""The speech event feed's host side, no GPU: the fvad_event layout the header
states (48 bytes, no padding) against the binding's ctypes structure and a C
compile of the header itself, the argument checks that need no engine, and
fvad_vadm_state -- the host VADMachine's speech state, which the GPU tests
derive the expected SPEECH_OPEN events from -- against the oracle's machine."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (offset, size) as include/fvad.h lays fvad_event out
LAYOUT = {"kind": (0, 4), "stream": (4, 4), "machine": (8, 4), "seq": (12, 4), "push": (16, 8),
          "sample_from": (24, 8), "sample_to": (32, 8), "debug_rnn_vad": (40, 4),
          "debug_avg_speech_vol_ratio": (44, 4)}


def test_event_struct_layout(fvad_mod):
    ev = fvad_mod.Event
    assert C.sizeof(ev) == 48
    assert [n for n, _ in ev._fields_] == list(LAYOUT)
    for name, (off, size) in LAYOUT.items():
        f = getattr(ev, name)
        assert (f.offset, f.size) == (off, size), name
    hdr = open(os.path.join(ROOT, "include", "fvad.h")).read()
    defs = dict((k, int(v)) for k, v in re.findall(r"#define\s+(FVAD_[A-Z0-9_]+)\s+(-?\d+)\b", hdr))
    assert fvad_mod.EVENT_SPEECH_OPEN == defs["FVAD_EVENT_SPEECH_OPEN"] == 1
    assert fvad_mod.EVENT_SEGMENT == defs["FVAD_EVENT_SEGMENT"] == 2
    assert fvad_mod.DEBUG_EVENTS_CHUNK == defs["FVAD_DEBUG_EVENTS_CHUNK"]


def test_event_struct_layout_in_c(tmp_path):
    """The header's own struct, through the C compiler the oracle is built with."""
    src = tmp_path / "layout.c"
    checks = ["_Static_assert(sizeof(fvad_event) == 48, \"size\");"]
    for name, (off, _) in LAYOUT.items():
        checks.append("_Static_assert(offsetof(fvad_event, %s) == %d, \"%s\");" % (name, off, name))
    src.write_text("#include <stddef.h>\n#include \"fvad.h\"\n" + "\n".join(checks) + "\nint main(void) { return 0; }\n")
    cc = os.environ.get("CC", "gcc")
    r = subprocess.run([cc, "-std=gnu11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_event_calls_reject_null(fvad_mod):
    L = fvad_mod.lib()
    assert L.fvad_engine_enable_events(None, 0) == -1  # FVAD_EINVAL
    buf = (fvad_mod.Event * 4)()
    n, lost = C.c_size_t(7), C.c_uint64()
    assert L.fvad_engine_poll_events(None, buf, 4, C.byref(n), C.byref(lost)) == -1
    assert n.value == 0
    assert L.fvad_engine_poll_events(None, None, 0, None, None) == -1
    assert L.fvad_engine_event_progress(None, None) == -1
    assert L.fvad_vadm_state(None, None, None, None) == -1


@pytest.mark.parametrize("sid", [0, 19, 7])
def test_host_vadm_state_matches_oracle(fvad_mod, oracle_mod, sid):
    """The host machine fed the oracle pipeline's window trace reports, after
    every 0.5 s chunk, the speech state, start and end of the oracle's own
    machine -- and it passes through Open on the way (not a vacuous match)."""
    secs = 14.0
    x, _ = fvad_mod.synth_stream(sid, int(48000 * secs), 2)
    om = oracle_mod.Model(seed=1)
    n = x.shape[1]
    p = oracle_mod.Pipeline(2, om, trace_windows=n // 2048 + 2)
    vm = fvad_mod.VADMachine(fvad_mod.VadmConfig.default(), n_channels=2)
    assert vm.state() == (0, 0, 0)
    fed, seen = 0, set()
    for k in range(0, n, 24000):
        p.push([x[0, k:k + 24000], x[1, k:k + 24000]])
        _, wi = p.trace()
        for w in wi[fed:]:
            vm.run(int(w["index"]), np.array(w["band"][:2], np.float32), float(w["vad"]), float(w["ratio"]))
            seen.add(vm.state()[0])
        fed = len(wi)
        snap = p.vadm_snapshot()
        assert vm.state() == (snap["speech_state"], snap["speech_start"], snap["speech_end"]), (sid, k)
    assert fed == n // 2048
    assert vm.segments() == p.segments()
    assert 2 in seen, seen
