"""The GRU kernels on the model domain fvad_model_load_text accepts and the
synthetic model never reaches: int8 weights over the whole [-128, 127] range
and other activation codes than tanh, relu x 3, sigmoid x 2.

Models (parity_util: TEST_MODELS, DOMAIN_MODELS; test_model_domain_cpu.py pins
their bytes and checks the oracle's runs of them), written as rnnoise text
files and loaded by both parsers:

  trained_like   geometric magnitudes clipped at -128 / 127 (mean |w| 23.5)
  uniform_full   uniform over [-128, 127]
  extremes       -128 or 127 only (vad saturates: tansig's x >= 8 branch)
  *-acts         PERMUTED_ACTS (sigmoid, tanh, sigmoid, tanh, tanh, relu)
  *-actsB        PERMUTED_ACTS_B (relu, sigmoid, tanh, sigmoid, relu, tanh)

Streams: synth_stream 0 / 19 / 42, stereo, 2.5 / 6.5 / 3.3 s (ragged, no
multiple of 480 samples, digital silence in 19), pushed in chunks of 37
ticks: three streams leave a partial workgroup in every GRU kernel.

  staged, fused   every output bit-identical to the oracle, on every model
  f32_fast        trained_like at test_gpu_f32_fast.py's bounds (its contract)
  fp16            trained_like: vad |d| <= 2e-2, ratios
                  bit-identical; denoised rel-RMS and band rel at 10x the
                  values measured on an MI355X (test_gpu_fp16.py's margin)
  fp16_fused      trained_like: fp16's outputs bit for bit
  rnnoise shim    extremes, trained_like-acts: the oracle's frames

uniform_full and extremes amplify a rounding error to order one (sensitivity
probe, test_model_domain_cpu.py), so only bit-equality is asked of them.

Measured maxima on an MI355X, trained_like (each test prints its own):

  mode       max |dvad|   denoised rel-RMS   band rel
  f32_fast   2.98e-08     6.08e-07           5.73e-07
  fp16       4.62e-05     4.23e-04           3.23e-04
"""
import numpy as np
import pytest

import parity_util as pu
import test_gpu_f32_fast as f32
from test_gpu_fused16 import KEYS
from test_gpu_parity import assert_stream_equal

pytestmark = pytest.mark.gpu

CHUNK = 37

FP16_VAD_ABS = 2e-2  # SURVEY.md 8(c), the fp16 config's stated bound
# 10x the maxima measured on trained_like (module docstring)
FP16_DEN_RELRMS = 4.3e-3
FP16_BAND_REL = 3.3e-3


@pytest.fixture(scope="module")
def domain(fvad_mod, oracle_mod, tmp_path_factory):
    """The streams, and per case (engine model, oracle model, oracle reference),
    each computed once and left unchanged."""
    tmp = tmp_path_factory.mktemp("models")
    streams = pu.domain_streams(fvad_mod)
    cache = {}

    def get(case):
        if case not in cache:
            path, blob = pu.write_domain_model(fvad_mod, case, tmp)
            m, om = fvad_mod.Model(path=path), oracle_mod.Model(path=path)
            assert np.array_equal(m.blob(), blob) and np.array_equal(om.blob(), blob)
            ref = pu.oracle_run(oracle_mod, om, streams)
            for r in ref:
                r["denoised"].setflags(write=False)
            cache[case] = (m, om, ref)
        return cache[case]

    return streams, get


def engine_outputs(fvad_mod, m, streams, mode):
    eng = fvad_mod.Engine(m, len(streams), 2, max_ticks=CHUNK, want_denoised=True, mode=mode)
    return pu.engine_run(fvad_mod, eng, streams, CHUNK)


@pytest.mark.parametrize("case", list(pu.DOMAIN_MODELS))
@pytest.mark.parametrize("mode", ["staged", "fused"])
def test_bit_exact(fvad_mod, domain, mode, case):
    """vad, ratio, denoised, band, win_ratio, win_vad: bit-identical to the oracle."""
    streams, get = domain
    m, _, ref = get(case)
    got = engine_outputs(fvad_mod, m, streams, mode)
    for r, g in zip(ref, got):
        assert_stream_equal(r, g, 2)


def test_f32_fast_trained_like(fvad_mod, domain):
    """The mode's documented bounds (vad 1e-4, denoised rel-RMS 1e-5, band
    1e-5; ratio, win_ratio, frame and window counts bit-identical), as
    test_gpu_f32_fast.check_stream asserts them."""
    streams, get = domain
    m, _, ref = get("trained_like")
    got = engine_outputs(fvad_mod, m, streams, "f32_fast")
    worst = [f32.check_stream(r, g, 2, i) for r, g, (i, _) in zip(ref, got, pu.DOMAIN_STREAMS)]
    f32.report("trained_like", worst)


def fp16_check_stream(ref, got, tag):
    """One stream of the fp16 mode against the oracle: (max |dvad|, denoised rel-RMS, band rel)."""
    fr, wi = ref["frames"], ref["windows"]
    assert len(fr) == len(got["vad"]), tag
    assert np.array_equal(fr["ratio"], got["ratio"]), tag
    assert len(wi) == int(got["win_flag"].sum()) > 0, tag
    assert np.array_equal(wi["ratio"], got["win_ratio"]), tag
    dv = float(np.abs(fr["vad"] - got["vad"]).max())
    dr, dg = ref["denoised"], got["denoised"]
    rel = float(np.sqrt(np.mean((dr - dg) ** 2)) / max(1e-12, np.sqrt(np.mean(dr ** 2))))
    b_ref, b_got = wi["band"][:, :2], got["band"][:, :, 0]
    brel = float(np.abs(b_ref - b_got).max() / max(1e-12, np.abs(b_ref).max()))
    print("  stream %s: |dvad| %.3g, denoised rel-RMS %.3g, band rel %.3g" % (tag, dv, rel, brel))
    return dv, rel, brel


def test_fp16_fused_equals_fp16_trained_like(fvad_mod, domain):
    """k_fused16 gives k_gru16's outputs bit for bit."""
    streams, get = domain
    m, _, _ = get("trained_like")
    a = engine_outputs(fvad_mod, m, streams, "fp16")
    b = engine_outputs(fvad_mod, m, streams, "fp16_fused")
    for s, (x, y) in enumerate(zip(a, b)):
        for k in KEYS:
            assert np.array_equal(x[k], y[k]), (s, k, pu.first_mismatch(x[k], y[k]))


@pytest.mark.parametrize("case", ["extremes", "trained_like-acts"])
def test_rnnoise_compat_shim(fvad_mod, oracle_mod, domain, case):
    """rnnoise_create/process_frame over the C ABI == the oracle Denoiser, frame by frame."""
    _, get = domain
    m, om, _ = get(case)
    x = fvad_mod.synth_stream(2, 480 * 120, 1)[0][0] * np.float32(32767)
    d = fvad_mod.Denoiser(m)
    o = oracle_mod.Denoiser(om)
    for i in range(120):
        f = x[i * 480:(i + 1) * 480]
        a, va = d.process_s16(f)
        b, vb = o.process(f)
        assert va == vb and np.array_equal(a, b), i


def test_fp16_trained_like(fvad_mod, domain):
    """k_gru16 against the oracle: vad within SURVEY.md 8(c)'s 2e-2, denoised
    and bands within 10x what an MI355X measured (module docstring)."""
    streams, get = domain
    m, _, ref = get("trained_like")
    got = engine_outputs(fvad_mod, m, streams, "fp16")
    worst = [fp16_check_stream(r, g, i) for r, g, (i, _) in zip(ref, got, pu.DOMAIN_STREAMS)]
    dv, rel, brel = (max(w[k] for w in worst) for k in range(3))
    print("fp16 trained_like: max |dvad| %.3g, denoised rel-RMS %.3g, band rel %.3g" % (dv, rel, brel))
    assert dv <= FP16_VAD_ABS, dv
    assert rel <= FP16_DEN_RELRMS, rel
    assert brel <= FP16_BAND_REL, brel
