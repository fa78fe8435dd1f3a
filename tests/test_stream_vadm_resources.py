"""The per-stream machine kernels' budgets, from hipcc's resource remarks
(a device-only compile of fvad_vadm.hip for gfx950 with the Makefile's flags,
as test_kernel_resources.py takes them): k_vadm_hbm_ps and k_vadm_par_ps hold
the occupancies the side stream's co-residency plan relies on for k_vadm_hbm
and k_vadm_par (3 and 2 waves per SIMD) without scratch, and k_vadm_par_ps'
LDS is k_vadm_par's plus the four streams' table rows."""
import os
import re

import pytest

import test_kernel_resources as kr

ROW_BYTES = 80  # sizeof(VadmRow), fvad_staged.h (a static_assert there)


@pytest.mark.skipif(not os.path.exists(kr.HIPCC), reason="hipcc not available")
def test_per_stream_machine_kernel_budgets():
    hdr = open(os.path.join(kr.PKG, "csrc", "fvad_staged.h")).read()
    assert re.search(r"static_assert\(sizeof\(VadmRow\) == %d\b" % ROW_BYTES, hdr)
    got = kr.resources("fvad_vadm.hip")
    print({k: got[k] for k in got if k.startswith("k_vadm")})
    for k, occ in (("k_vadm_hbm_ps", 3), ("k_vadm_par_ps", 2), ("k_vadm_hbm", 3), ("k_vadm_par", 2)):
        assert k in got, (k, sorted(got))
        assert got[k]["Occupancy"] >= occ, (k, got[k])
        assert got[k]["VGPRs_spill"] == 0, (k, got[k])
    assert got["k_vadm_hbm_ps"]["LDS"] == 0, got["k_vadm_hbm_ps"]
    assert got["k_vadm_par_ps"]["LDS"] <= got["k_vadm_par"]["LDS"] + 4 * ROW_BYTES, (got["k_vadm_par_ps"], got["k_vadm_par"])
    # k_vadm_retarget, like the other lifecycle kernels: no LDS, no scratch
    ret = kr.resources("fvad_lifecycle.hip")
    assert "k_vadm_retarget" in ret, sorted(ret)
    assert ret["k_vadm_retarget"]["VGPRs_spill"] == 0 and ret["k_vadm_retarget"]["LDS"] == 0, ret["k_vadm_retarget"]
