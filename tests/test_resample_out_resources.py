"""The output downsampler's kernels (csrc/fvad_resample_out.hip) compile for
gfx950 with no scratch at all -- no spilled register, no private array -- and
within 64 KB of static LDS, read from hipcc's resource remarks as
tests/test_resample_resources.py does."""
import os
import re
import subprocess

import pytest

import test_kernel_resources as tkr

KERNELS = ("k_resample_out", "k_resample_out_tail")


def resources():
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
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)",
                      line)
        if m and cur:
            res[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return res


@pytest.mark.skipif(not os.path.exists(tkr.HIPCC), reason="hipcc not available")
def test_resample_out_kernel_resources():
    got = resources()
    print(got)
    for k in KERNELS:
        mine = [n for n in got if n == k or n.startswith(k + "<")]
        assert mine, (k, sorted(got))
        for n in mine:
            r = got[n]
            assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (n, r)
            assert r["LDS Size"] <= 64 * 1024, (n, r)
    # one shape of block and outputs per thread for each of the six rates; one tail kernel
    main = [n for n in got if n.startswith("k_resample_out<")]
    assert len(main) == 6 and all(got[n]["LDS Size"] > 0 for n in main), sorted(got)
    # the 44.1 kHz table (147 x 96 floats) and its window of 480 + 95 samples lie in LDS
    assert max(got[n]["LDS Size"] for n in main) == 4 * (147 * 96 + 480 + 95)
    assert "k_resample_out_tail" in got and got["k_resample_out_tail"]["LDS Size"] == 0
