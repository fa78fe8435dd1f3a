"""The input resampling's kernels (csrc/fvad_resample.hip) compile for gfx950
with no scratch at all -- no spilled register, no private array -- and within
64 KB of LDS, read from hipcc's resource remarks as
tests/test_capture_resources.py does."""
import os
import re
import subprocess

import pytest

import test_kernel_resources as tkr

KERNELS = ("k_resample", "k_resample_tail", "k_resample_clear")


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
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)",
                      line)
        if m and cur:
            res[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return res


@pytest.mark.skipif(not os.path.exists(tkr.HIPCC), reason="hipcc not available")
def test_resample_kernel_resources():
    got = resources()
    print(got)
    for k in KERNELS:
        mine = [n for n in got if n == k or n.startswith(k + "<")]
        assert mine, (k, sorted(got))
        for n in mine:
            r = got[n]
            assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (n, r)
            assert r["LDS Size"] <= 64 * 1024, (n, r)
    # float and 16-bit input, three shapes of block and LDS arrays each; the tail kernel for both inputs
    main = [n for n in got if n.startswith("k_resample<")]
    assert len(main) == 6 and all(got[n]["LDS Size"] > 0 for n in main), sorted(got)
    assert max(got[n]["LDS Size"] for n in main) >= 160 * 48 * 4  # the 44.1 kHz table lies in LDS
    assert len([n for n in got if n.startswith("k_resample_tail<")]) == 2
