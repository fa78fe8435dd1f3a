"""The recurrence's feature formulas (csrc/fvad_rnnfeat_core.h, which k_rnn3,
k_rnn3f, k_gru16 and k_fused16 compile) against a direct model of rnnoise's
compute_frame_features, no GPU: a stand-alone program under AddressSanitizer
and UBSan."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "formula-vad_amd", "csrc")


def test_rnnfeat_core_against_a_direct_model(tmp_path):
    """tests/rnnfeat_core_harness.cpp: per active frame the core's 37 items in
    a shuffled order, the row minima, their sum and the mem_id advance, against
    the C algorithm with all 64 distances recomputed from the cepstral memory;
    features, cepstral memory and distance matrix compared by bits after every
    frame of 300 sequences from the all-zero state (inactive frames, repeated
    rows, mixed signs and magnitudes, -0.0f), and gain_smooth against max();
    its own main, -fsanitize=address,undefined (any report fails the run)."""
    exe = tmp_path / "rnnfeat_core"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC,
                           os.path.join(ROOT, "tests", "rnnfeat_core_harness.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert re.search(r"^0 / \d+ mismatches$", out.stdout, re.M), out.stdout
    assert "FAIL" not in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr

