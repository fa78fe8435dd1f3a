"""The model domain of the GPU tests (test_gpu_model_domain.py), on the CPU:
the deterministic test models of parity_util (int8 weights over the whole
[-128, 127] range, other activation codes than the synthetic model's), both
text-model parsers on them, and the properties of the oracle's runs that make
them a useful reference.  No GPU.

The models (parity_util.TEST_MODELS; one splitmix64 draw per weight):

  trained_like   geometric magnitudes, clipped at both ends   169 x -128, 181 x 127, mean |w| 23.5
  uniform_full   uniform over [-128, 127]                      327 x -128, 337 x 127
  extremes       -128 or 127 only                              43 746 x -128, 43 757 x 127

Oracle runs over the GPU tests' streams (synth_stream 0 / 19 / 42, stereo,
2.5 / 6.5 / 3.3 s), measured here:

  case                 distinct vad values per stream   vad range
  trained_like         250 / 554 / 330                  0 .. 0.482
  uniform_full         250 / 554 / 330                  0 .. 0.436
  extremes             250 / 436 / 330                  0 .. 1.0 (>= 0.999 reached: tansig's x >= 8 branch)
  trained_like-acts    1 / 1 / 1                        0 (relu vad_output, sum never positive)
  seed1-acts           1 / 2 / 1                        0 .. 0.088
  trained_like-actsB   250 / 554 / 330                  -0.469 .. 0
  seed1-actsB          250 / 554 / 330                  0 .. 0.702

Under PERMUTED_ACTS the vad output is pinned at 0 on every synthetic stream
(ids 0..63 tried), so that assignment's reference constrains the vad branch
through the denoised samples (vad_gru feeds denoise_gru) and PERMUTED_ACTS_B
is there to have a vad that moves.

Sensitivity probe (0.01 s16 units added to one sample of frame 10, channel 0):

  stream   model          max |dvad|   denoised rel-RMS
  0        seed 1         1.4e-5       2.8e-4
  0        trained_like   1.5e-5       2.1e-4
  42       seed 1         2.0e-5       5.0e-5
  42       trained_like   3.5e-5       5.5e-5
  0 / 42   uniform_full   1.2e-4 / 5.3e-5   0.44 / 0.99  (chaotic: no tolerance test)
  0 / 42   extremes       1.4e-2 / 1.4e-3   1.8e-4 / 5.6e-5

(on stream 19 the perturbation dies out at the rounding level for both
models, max |dvad| <= 6e-8, a ratio of two roundings: not asserted)
"""
import hashlib

import numpy as np
import pytest

import parity_util as pu

DIGESTS = {
    "trained_like": ("a51528feaf7ebf8f9f79bac1e15849f613c3b0d778c3f3761294f989d5d04fc0", 169, 181),
    "uniform_full": ("861c71123f21e3c754f52e64afbda3690ef371c38dfc6b1004c657bb1611e011", 327, 337),
    "extremes": ("1af93c02f29b55152501dbeb7a8eec222c8e56116e83dec27eb03fe9208c3e28", 43746, 43757),
}

# cases whose vad output the relu of PERMUTED_ACTS pins at 0 (module docstring)
VAD_PINNED = ("trained_like-acts", "seed1-acts")


@pytest.mark.parametrize("name", sorted(pu.TEST_MODELS))
def test_blob_digests(name):
    b = pu.model_blob(name)
    digest, n_min, n_max = DIGESTS[name]
    assert b.dtype == np.int8 and len(b) == pu.N_WEIGHTS == 87503
    assert hashlib.sha256(b.tobytes()).hexdigest() == digest
    assert (int((b == -128).sum()), int((b == 127).sum())) == (n_min, n_max)
    if name == "trained_like":
        assert abs(float(np.abs(b.astype(np.int32)).mean()) - 23.5) < 0.05


def test_permutations_change_every_layer():
    """The three assignments give every layer each of the three codes once."""
    default = [act for _, _, act, _ in pu.LAYERS]
    for k in range(6):
        assert sorted((default[k], pu.PERMUTED_ACTS[k], pu.PERMUTED_ACTS_B[k])) == [0, 1, 2], k


@pytest.mark.parametrize("case", sorted(pu.DOMAIN_MODELS))
def test_loader_parity(fvad_mod, oracle_mod, tmp_path, case):
    """Both text parsers return the generated weights, -128 and 127 included."""
    path, blob = pu.write_domain_model(fvad_mod, case, tmp_path)
    a = fvad_mod.Model(path=path).blob()
    b = oracle_mod.Model(path=path).blob()
    assert a.dtype == b.dtype == np.int8
    assert np.array_equal(a, blob), pu.first_mismatch(a, blob)
    assert np.array_equal(b, blob), pu.first_mismatch(b, blob)


@pytest.fixture(scope="module")
def refs(fvad_mod, oracle_mod, tmp_path_factory):
    """The oracle's run of every case over the GPU tests' streams, computed once."""
    tmp = tmp_path_factory.mktemp("models")
    streams = pu.domain_streams(fvad_mod)
    out = {"seed1": pu.oracle_run(oracle_mod, oracle_mod.Model(seed=1), streams)}
    for case in pu.DOMAIN_MODELS:
        path, _ = pu.write_domain_model(fvad_mod, case, tmp)
        out[case] = pu.oracle_run(oracle_mod, oracle_mod.Model(path=path), streams)
    return out


@pytest.mark.parametrize("case", sorted(pu.DOMAIN_MODELS))
def test_oracle_preconditions(refs, case):
    """The reference runs are finite and move: a comparison with them can fail."""
    ref = refs[case]
    vads = []
    for (sid, _), r in zip(pu.DOMAIN_STREAMS, ref):
        fr, wi = r["frames"], r["windows"]
        assert len(fr) > 0 and len(wi) > 0
        for name, x in (("vad", fr["vad"]), ("ratio", fr["ratio"]), ("denoised", r["denoised"]),
                        ("band", wi["band"]), ("win_ratio", wi["ratio"]), ("win_vad", wi["vad"])):
            assert np.isfinite(x).all(), (sid, name)
        assert float(np.abs(r["denoised"]).max()) > 1e-3, sid
        vads.append(fr["vad"])
    distinct = len(np.unique(np.concatenate(vads)))
    print("%s: %d distinct vad values, range %.6g .. %.6g" %
          (case, distinct, min(v.min() for v in vads), max(v.max() for v in vads)))
    if case not in VAD_PINNED:
        assert distinct >= 50
    if case == "extremes":  # the saturation branch of tansig / sigmoid is reached
        assert max(float(v.max()) for v in vads) >= 0.999
    # other activation codes give another reference than the same weights' default codes
    weights, acts = pu.DOMAIN_MODELS[case]
    if acts is not None:
        for r, r0 in zip(ref, refs[weights]):
            assert not np.array_equal(r["denoised"], r0["denoised"])


@pytest.mark.parametrize("case", ["extremes", "trained_like-acts"])
def test_oracle_preconditions_compat_frames(fvad_mod, oracle_mod, tmp_path, case):
    """The compat shim test's 120 frames of stream 2 (s16 scale): finite, non-trivial output."""
    path, _ = pu.write_domain_model(fvad_mod, case, tmp_path)
    x = fvad_mod.synth_stream(2, 480 * 120, 1)[0][0] * np.float32(32767)
    d = oracle_mod.Denoiser(oracle_mod.Model(path=path))
    res = [d.process(x[i * 480:(i + 1) * 480]) for i in range(120)]
    out = np.concatenate([r[0] for r in res])
    assert np.isfinite(out).all() and np.isfinite([r[1] for r in res]).all()
    assert float(np.abs(out).max()) > 1.0  # s16 units


@pytest.mark.parametrize("sid,secs", [(0, 2.5), (42, 3.3)])
def test_sensitivity_trained_like_is_tame(fvad_mod, oracle_mod, tmp_path, sid, secs):
    """trained_like carries a rounding-sized input error no further than 4x
    what the synthetic model does, so the tolerance modes' bounds mean on it
    what they mean on seed 1 (uniform_full and extremes are chaotic as
    recurrent nets and stay with the bit-exact modes)."""
    x = fvad_mod.synth_stream(sid, int(48000 * secs), 1)[0][0] * np.float32(32767)
    path, _ = pu.write_domain_model(fvad_mod, "trained_like", tmp_path)
    dv0, rel0 = pu.sensitivity_probe(oracle_mod, oracle_mod.Model(seed=1), x)
    dv1, rel1 = pu.sensitivity_probe(oracle_mod, oracle_mod.Model(path=path), x)
    print("stream %d: seed 1 max |dvad| %.3g, rel-RMS %.3g; trained_like %.3g, %.3g" % (sid, dv0, rel0, dv1, rel1))
    assert dv0 > 0 and rel0 > 0  # the probe reaches the outputs
    assert dv1 <= 4 * dv0
    assert rel1 <= 4 * rel0
