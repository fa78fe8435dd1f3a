"""The clip capture's kernels (csrc/fvad_capture.hip) compile for gfx950 with
no scratch at all -- no spilled register and no private array (k_cap_plan's
per-stream lists stay in registers) -- and within 64 KB of LDS, read from
hipcc's resource remarks as tests/test_kernel_resources.py does."""
import os
import re
import subprocess

import pytest

import test_kernel_resources as tkr

KERNELS = ("k_hist_append", "k_hist_advance", "k_cap_plan", "k_cap_channel", "k_cap_copy", "k_cap_publish",
           "k_cap_set_pos", "k_cap_drop")


def resources():
    cmd = [tkr.HIPCC] + tkr.FLAGS + ["-c", os.path.join(tkr.PKG, "csrc", "fvad_capture.hip"), "-o", os.devnull]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: _ZN4fvad\d+(k_[a-z_]+?)(I[A-Za-z0-9_]+E[a-z]*)?E", line)
        if m:
            cur = m.group(1) + ("<%s>" % m.group(2) if m.group(2) else "")
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)",
                      line)
        if m and cur:
            res[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return res


@pytest.mark.skipif(not os.path.exists(tkr.HIPCC), reason="hipcc not available")
def test_capture_kernel_resources():
    got = resources()
    print(got)
    for k in KERNELS:
        mine = [n for n in got if n == k or n.startswith(k + "<")]
        assert mine, (k, sorted(got))
        for n in mine:
            r = got[n]
            assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (n, r)
            assert r["LDS Size"] <= 64 * 1024, (n, r)
    assert len([n for n in got if n.startswith("k_hist_append")]) == 2  # the float and the 16-bit input
    assert got["k_cap_channel"]["LDS Size"] > 0 and got["k_cap_plan"]["LDS Size"] > 0
