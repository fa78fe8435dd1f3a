"""CPU checks of the f32_fast engine mode (FVAD_MODE_F32_FAST): the fused
multiply-add kernel's register / LDS budget (its exact twin's occupancy, no
spills), that the fusion is really in its code (device-only assembly for
gfx950 with the Makefile's flags: more fused multiply-adds and fewer separate
multiplies and adds than its twin), and the mode's ABI constants."""
import concurrent.futures as cf
import os
import re
import subprocess

import pytest

import test_kernel_resources as tkr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "formula-vad_amd")

# fused kernel -> (exact twin, source, waves per SIMD the twin's plan relies on)
# (fused twins of k_fftAw, k_pspecw, k_synthw and k_olafb were measured and
# did not beat their exact kernels: they and their rows are not in the tree,
# DESIGN.md section 3)
TWINS = {
    "k_rnn3f": ("k_rnn3", "fvad_rnn3.hip", 4),
}
SOURCES = sorted({v[1] for v in TWINS.values()})
# (v_fmac_f32 is v_fma_f32 with the addend in the destination register: the form
# the compiler picks for acc = fmaf(w, v, acc))
FUSED_OPS = ("v_fma_f32", "v_fmac_f32", "v_pk_fma_f32")
SPLIT_OPS = ("v_mul_f32", "v_add_f32", "v_pk_mul_f32", "v_pk_add_f32")

needs_hipcc = pytest.mark.skipif(not os.path.exists(tkr.HIPCC), reason="hipcc not available")


def op_counts(src):
    """{kernel: (fused multiply-adds, separate multiplies / adds)} of a source's device assembly."""
    flags = [f for f in tkr.FLAGS if not f.startswith("-Rpass")]
    cmd = [tkr.HIPCC] + flags + (["-fno-slp-vectorize"] if src in tkr.NO_SLP else []) + \
          ["-S", os.path.join(PKG, "csrc", src), "-o", "-"]
    asm = subprocess.run(cmd, capture_output=True, text=True, timeout=600, check=True).stdout
    res, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"_ZN4fvad\d+(k_\w+?)E\w*:", line)
        if m:
            cur = m.group(1)
            res[cur] = [0, 0]
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        if cur is None or not line.startswith("\t"):
            continue
        op = re.sub(r"_(e32|e64|dpp|sdwa)$", "", line.split()[0]) if line.split() else ""
        if op in FUSED_OPS:
            res[cur][0] += 1
        elif op in SPLIT_OPS:
            res[cur][1] += 1
    return res


@pytest.fixture(scope="module")
def compiled():
    with cf.ThreadPoolExecutor(max_workers=4) as ex:
        r = [ex.submit(tkr.resources, s) for s in SOURCES]
        o = [ex.submit(op_counts, s) for s in SOURCES]
        res, ops = {}, {}
        for f in r:
            res.update(f.result())
        for f in o:
            ops.update(f.result())
    return res, ops


@needs_hipcc
@pytest.mark.parametrize("kernel", sorted(TWINS))
def test_fused_kernel_budget(compiled, kernel):
    res, _ = compiled
    twin, _, occ = TWINS[kernel]
    assert kernel in res, (kernel, sorted(res))
    r = res[kernel]
    print(kernel, r, "twin", res[twin])
    assert r["Occupancy"] >= occ, (kernel, r)
    assert r["VGPRs_spill"] == 0, (kernel, r)
    assert r["LDS"] <= 160 * 1024, (kernel, r)


@needs_hipcc
@pytest.mark.parametrize("kernel", sorted(TWINS))
def test_fusion_is_in_the_code(compiled, kernel):
    """Counts only: the correctly rounded division already puts fused
    multiply-adds into the exact kernels."""
    _, ops = compiled
    twin = TWINS[kernel][0]
    assert kernel in ops and twin in ops, (kernel, sorted(ops))
    (ff, fs), (xf, xs) = ops[kernel], ops[twin]
    print("%s: %d fused, %d separate; %s: %d fused, %d separate" % (kernel, ff, fs, twin, xf, xs))
    assert ff > xf, (kernel, ff, xf)
    assert fs < xs, (kernel, fs, xs)


def test_mode_constant():
    hdr = open(os.path.join(ROOT, "include", "fvad.h")).read()
    m = re.search(r"^#define FVAD_MODE_F32_FAST (\d+)$", hdr, re.M)
    assert m, "include/fvad.h does not define FVAD_MODE_F32_FAST"
    assert int(m.group(1)) == 4
    assert "FVAD_MODE_F32_FAST" in re.search(r"int mode;.*?\*/", hdr, re.S).group(0)
    import fvad
    assert fvad.MODE_F32_FAST == int(m.group(1))
    modes = (fvad.MODE_STAGED, fvad.MODE_FUSED, fvad.MODE_FP16, fvad.MODE_FP16_FUSED, fvad.MODE_F32_FAST)
    assert len(set(modes)) == 5
