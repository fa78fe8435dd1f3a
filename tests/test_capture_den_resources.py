"""The kernels that the denoised / 16-bit clip capture adds or changes
(csrc/fvad_capture.hip: k_den_append in its aligned and its 44.1 kHz
form, k_cap_copy_short, and k_hist_advance, k_cap_plan, k_cap_publish, which
gained arguments) compile for gfx950 with no scratch at all -- no spilled
register, no private array -- read from hipcc's resource remarks as
tests/test_capture_resources.py does."""
import os

import pytest

import test_capture_resources as tcr
import test_kernel_resources as tkr

KERNELS = ("k_den_append", "k_cap_copy_short", "k_hist_advance", "k_cap_plan", "k_cap_publish")


@pytest.mark.skipif(not os.path.exists(tkr.HIPCC), reason="hipcc not available")
def test_capture_den_kernel_resources():
    got = tcr.resources()
    print(got)
    for k in KERNELS:
        mine = [n for n in got if n == k or n.startswith(k + "<")]
        assert mine, (k, sorted(got))
        for n in mine:
            r = got[n]
            assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (n, r)
            assert r["LDS Size"] <= 64 * 1024, (n, r)
    # the float4 form and the form for rows of 441 samples
    assert len([n for n in got if n.startswith("k_den_append<")]) == 2, sorted(got)
    assert got["k_cap_copy_short"]["LDS Size"] == 0
