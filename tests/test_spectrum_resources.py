"""The window-spectrum kernels compile for gfx950 with no scratch at all -- no
spilled register, no private array: the tap twins of the FFT-B kernels
(k_olafb_spec, k_fftbw_spec in csrc/fvad_wave.hip, the kTap instantiations of
k_fftb in csrc/fvad_tail.hip) and k_sweep_bandmin (csrc/fvad_sweep.hip), whose
staged form holds one window's 8 x 1 025 magnitudes in LDS, the 32 800 bytes
DESIGN.md states.  Read from hipcc's resource remarks as
tests/test_resample_resources.py does.  The plain kernels keep their names,
LDS and occupancy (tests/test_kernel_resources.py checks those unchanged)."""
import os
import re
import subprocess

import pytest

import test_kernel_resources as tkr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANDMIN_LDS = 8 * 1025 * 4


def resources(src):
    cmd = [tkr.HIPCC] + tkr.FLAGS + (["-fno-slp-vectorize"] if src in tkr.NO_SLP else []) + \
          ["-c", os.path.join(tkr.PKG, "csrc", src), "-o", os.devnull]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: _ZN4fvad\d+(k_[a-z_]+?)(I[A-Za-z0-9_]+E[a-z]*)?E", line)
        if m:
            cur = m.group(1) + ("<%s>" % m.group(2) if m.group(2) else "")
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|"
                      r"Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur:
            res[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return res


def no_scratch(name, r, sgpr_to_lanes=True):
    """No scratch memory: no spilled vector register, no private array.  (k_olafb and
    k_fftb park scalar registers in lanes of a vector register, which is not scratch;
    their tap forms may too.)"""
    assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
    assert sgpr_to_lanes or r["SGPRs Spill"] == 0, (name, r)


@pytest.mark.skipif(not os.path.exists(tkr.HIPCC), reason="hipcc not available")
def test_tap_twins_of_the_wave_kernels():
    got = resources("fvad_wave.hip")
    print({k: got[k] for k in got if "olafb" in k or "fftbw" in k})
    for plain, tap in (("k_olafb", "k_olafb_spec"), ("k_fftbw", "k_fftbw_spec")):
        assert plain in got and tap in got, sorted(got)
        no_scratch(tap, got[tap])
        # the same LDS and the same residency as the kernel it stands in for
        assert got[tap]["LDS Size"] == got[plain]["LDS Size"], (got[tap], got[plain])
        assert got[tap]["Occupancy"] >= got[plain]["Occupancy"] == 3, (got[tap], got[plain])


@pytest.mark.skipif(not os.path.exists(tkr.HIPCC), reason="hipcc not available")
def test_tap_instantiations_of_k_fftb():
    got = resources("fvad_tail.hip")
    fftb = {n: r for n, r in got.items() if n.startswith("k_fftb<")}
    print(fftb)
    # <NT, kLds, kTap>: 256 / 64 threads in LDS, 256 on device scratch, each without and with the tap
    assert len(fftb) == 6, sorted(fftb)
    taps = [n for n in fftb if n.endswith("Lb1EE>")]
    assert len(taps) == 3, sorted(fftb)
    for n, r in fftb.items():
        no_scratch(n, r)
        assert r["LDS Size"] == 0, (n, r)  # dynamic LDS only, sized by the launch: the tap adds none


@pytest.mark.skipif(not os.path.exists(tkr.HIPCC), reason="hipcc not available")
def test_k_sweep_bandmin():
    got = resources("fvad_sweep.hip")
    mine = {n: r for n, r in got.items() if n.startswith("k_sweep_bandmin")}
    print(mine)
    assert len(mine) == 2, sorted(got)
    for n, r in mine.items():
        no_scratch(n, r, sgpr_to_lanes=False)
    lds = sorted(r["LDS Size"] for r in mine.values())
    assert lds[1] == BANDMIN_LDS and lds[0] <= 4, lds  # staged: one window; unstaged: a placeholder word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "32 800 bytes" in design and "k_sweep_bandmin" in design
    # the other sweep kernels are as they were: no LDS, no scratch
    for n in ("k_sweep_min", "k_vadm_sweep"):
        no_scratch(n, got[n])
