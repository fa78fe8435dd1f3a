"""k_resample_ps (csrc/fvad_resample.hip) against its k_resample twin, from
hipcc's resource remarks as tests/test_resample_resources.py reads them: every
variant has no scratch, its twin's LDS plus at most what the row map needs
(nothing: the map lives in registers), and a VGPR count that keeps the twin's
occupancy.  The bounds are the twin's own figures of the same compile."""
import os
import re
import subprocess

import pytest

import test_kernel_resources as tkr

KEYS = ("VGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize", "LDS Size", "Occupancy")
MAP_LDS = 0  # bytes of LDS the row map may add: the list and the offsets are read from global memory


def resources():
    cmd = [tkr.HIPCC] + tkr.FLAGS + ["-c", os.path.join(tkr.PKG, "csrc", "fvad_resample.hip"), "-o", os.devnull]
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


def waves_by_vgprs(v):
    """waves per SIMD that v VGPRs allow on gfx950: 512 registers, granules of 8, 8 waves at most"""
    return min(8, 512 // (8 * ((v + 7) // 8)))


@pytest.mark.skipif(not os.path.exists(tkr.HIPCC), reason="hipcc not available")
def test_k_resample_ps_keeps_its_twins_resources():
    got = resources()
    ps = sorted(n for n in got if n.startswith("k_resample_ps<"))
    print({n: got[n] for n in got if n.startswith("k_resample")})
    assert len(ps) == 6, sorted(got)  # float and 16-bit input, three shapes of block and LDS arrays each
    for n in ps:
        twin = "k_resample<" + n[len("k_resample_ps<"):]
        assert twin in got, (n, sorted(got))
        r, t = got[n], got[twin]
        assert all(k in r and k in t for k in KEYS), (n, r, t)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (n, r)
        assert t["LDS Size"] <= r["LDS Size"] <= t["LDS Size"] + MAP_LDS, (n, r, t)
        assert waves_by_vgprs(r["VGPRs"]) >= waves_by_vgprs(t["VGPRs"]), (n, r, t)
        assert r["Occupancy"] >= t["Occupancy"], (n, r, t)  # (the compiler's own figure: SGPRs and LDS too)
    # the launches beside it: no scratch either
    for k in ("k_resample_copy", "k_resample_tail_ps"):
        mine = [n for n in got if n.startswith(k + "<")]
        assert len(mine) == 2, (k, sorted(got))
        for n in mine:
            assert got[n]["ScratchSize"] == 0 and got[n]["VGPRs Spill"] == 0 and got[n]["LDS Size"] == 0, (n, got[n])
