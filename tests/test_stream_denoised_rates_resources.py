"""k_resample_out_ps (csrc/fvad_resample_out.hip) against its k_resample_out
twin, from hipcc's resource remarks as tests/test_stream_rates_resources.py
reads them: every variant has no scratch and no spills, its twin's LDS (the row
map lives in registers), and a VGPR count and a compiler-reported occupancy
that keep the twin's.  The bounds are the twin's own figures of the same
compile."""
import os
import re
import subprocess

import pytest

import test_kernel_resources as tkr
from test_stream_rates_resources import KEYS, waves_by_vgprs


def resources():
    """test_stream_rates_resources.resources over fvad_resample_out.hip"""
    cmd = [tkr.HIPCC] + tkr.FLAGS + ["-c", os.path.join(tkr.PKG, "csrc", "fvad_resample_out.hip"), "-o", os.devnull]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: _ZN4fvad\d+(k_[a-z_]+?)(I[A-Za-z0-9_]+E[a-z]*)?E", line)
        if m:
            cur = m.group(1) + ("<%s>" % m.group(2) if m.group(2) else "")
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|"
                      r"Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur:
            res[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return res


@pytest.mark.skipif(not os.path.exists(tkr.HIPCC), reason="hipcc not available")
def test_k_resample_out_ps_keeps_its_twins_resources():
    got = resources()
    ps = sorted(n for n in got if n.startswith("k_resample_out_ps<"))
    print({n: got[n] for n in got if n.startswith("k_resample_out")})
    assert len(ps) == 6, sorted(got)  # one shape of block and outputs per thread for each of the six rates
    for n in ps:
        twin = "k_resample_out<" + n[len("k_resample_out_ps<"):]
        assert twin in got, (n, sorted(got))
        r, t = got[n], got[twin]
        assert all(k in r and k in t for k in KEYS), (n, r, t)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (n, r)
        assert r["LDS Size"] == t["LDS Size"], (n, r, t)
        assert waves_by_vgprs(r["VGPRs"]) >= waves_by_vgprs(t["VGPRs"]), (n, r, t)
        assert r["Occupancy"] >= t["Occupancy"], (n, r, t)  # (the compiler's own figure: SGPRs and LDS too)
    # the launches beside it: untemplated, no scratch, no LDS
    for k in ("k_resample_out_copy", "k_resample_out_tail_ps"):
        assert k in got, (k, sorted(got))
        r = got[k]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, (k, r)
