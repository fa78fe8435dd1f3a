"""The band-energy chains of the wave-per-frame kernels (k_fftAw, k_pspecw,
k_synthw).  k_fftAw takes a batch's valid frames in pairs and runs the two
frames' chains side by side as one straight line per lane with the LDS loads
ahead of the adds (band_chain_ahead); k_pspecw, k_synthw and k_fused16 run
band_chain's loops.  Every add stays on its lane in the oracle's order, so the
staged mode must still equal the CPU oracle bit for bit.

The shapes are the smallest at which the pairing can go wrong: V = max_ticks x
channels is no multiple of the 8-frame batch, so batches straddle streams;
ragged ticks_valid leaves invalid slots at even and at odd batch positions and
odd counts of valid frames (a leftover single frame); one stream of digital
silence lies between active ones, so a silent frame sits inside a pair; and
every case is two pushes, so state carries from one to the next.

The modes f32_fast and fp16 run the same three kernels but another GRU stack,
which by design meets the oracle within their stated bounds and not bit for
bit: they are held to those bounds (test_gpu_f32_fast.py / test_gpu_fp16.py:
the outputs computed before the GRU -- counts, volume ratios, window ratios --
bit-identical, vad, denoised PCM and band sums within the mode's tolerance).
fp16_fused runs the chains inside k_fused16 and must equal fp16 bit for bit.
"""
import functools

import numpy as np
import pytest

import parity_util as pu
from test_gpu_f32_fast import check_stream as check_f32_fast
from test_gpu_fp16 import check_stream as check_fp16

pytestmark = pytest.mark.gpu

KEYS = ("vad", "ratio", "win_flag", "win_ratio", "win_vad", "band", "denoised")

# name -> (channels, max_ticks, synth_stream ids (None: digital silence), ticks_valid of each push)
CASES = {
    # V = 3: batches of 8 straddle streams; the second push leaves 7 and 5 valid frames per batch
    "5x1x3": (1, 3, (0, 1, None, 42, 5), ((3, 3, 3, 3, 3), (3, 2, 3, 1, 3))),
    # V = 10, every slot valid: 30 frames = 3 full batches + 6
    "3x2x5": (2, 5, (0, None, 42), ((5, 5, 5), (5, 5, 5))),
    # V = 10, ragged: an empty stream, batches with 0, 2, 4, 6 and 8 valid frames
    "6x2-ragged": (2, 5, (0, 1, 3, 42, None, 5), ((0, 1, 5, 2, 5, 3), (3, 5, 0, 5, 2, 1))),
    # V = 9, ragged: streams start at odd frame indices, valid runs of 3, 6 and 9 frames
    "5x3-ragged": (3, 3, (0, 1, None, 42, 5), ((3, 2, 3, 1, 3), (1, 3, 0, 3, 2))),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's streams (cut to the ticks its pushes consume) and their oracle results, computed once."""
    import fvad
    import oracle
    oracle.build()
    ch, _, ids, pushes = CASES[name]
    total = [sum(p[s] for p in pushes) for s in range(len(ids))]
    streams = []
    for sid, n in zip(ids, total):
        x = np.zeros((ch, n * pu.FRAME), np.float32) if sid is None else fvad.synth_stream(sid, n * pu.FRAME, ch)[0]
        x.setflags(write=False)
        streams.append(x)
    ref = pu.oracle_run(oracle, oracle.Model(seed=1), streams)
    for r in ref:
        for v in (r["frames"], r["windows"], r["denoised"]):
            v.setflags(write=False)
    return streams, ref


def _run(fvad_mod, model, name, mode):
    """The case's pushes through an engine of the given mode: per stream, the outputs of its valid ticks in order."""
    ch, T, ids, pushes = CASES[name]
    streams, _ = _case(name)
    B = len(ids)
    eng = fvad_mod.Engine(model, B, ch, max_ticks=T, want_denoised=True, mode=mode)
    W = getattr(eng, "wpt", 1)
    pos = [0] * B
    per = [{k: [] for k in KEYS} for _ in range(B)]
    for valid in pushes:
        pcm = np.zeros((T, B, ch, pu.FRAME), np.float32)
        for s, v in enumerate(valid):
            seg = streams[s][:, pos[s] * pu.FRAME:(pos[s] + v) * pu.FRAME].reshape(ch, v, pu.FRAME)
            pcm[:v, s] = seg.transpose(1, 0, 2)
            pos[s] += v
        o = eng.push(pcm, ticks_valid=np.array(valid, np.int32), denoised=True)
        for s, v in enumerate(valid):
            cnt = o["win_flag"][:v, s]
            per[s]["vad"].append(o["vad"][:v, s])
            per[s]["ratio"].append(o["ratio"][:v, s])
            per[s]["win_flag"].append(cnt)
            for k in ("win_ratio", "win_vad", "band"):
                per[s][k].append(pu.tick_windows(o[k][:v, s], cnt, W))
            per[s]["denoised"].append(o["denoised"][:v, s])
    out = []
    for r in per:
        g = {k: np.concatenate(v) for k, v in r.items()}
        g["denoised"] = g["denoised"].transpose(1, 0, 2).reshape(ch, -1)  # [T][Ch][480] -> [Ch][samples]
        out.append(g)
    return out


@pytest.fixture(scope="module")
def model(fvad_mod):
    return fvad_mod.Model(seed=1)


@pytest.mark.parametrize("name", list(CASES))
def test_staged_equals_oracle(fvad_mod, oracle_mod, model, name):
    """Every output the parity tests compare, bit for bit."""
    ch = CASES[name][0]
    _, ref = _case(name)
    got = _run(fvad_mod, model, name, "staged")
    n_win = 0
    for s, (r, g) in enumerate(zip(ref, got)):
        fr, wi = r["frames"], r["windows"]
        assert len(fr) == len(g["vad"]), (name, s)
        assert len(wi) == int(g["win_flag"].sum()), (name, s)
        n_win += len(wi)
        for k, a, b in (("vad", fr["vad"], g["vad"]), ("ratio", fr["ratio"], g["ratio"]),
                        ("win_ratio", wi["ratio"], g["win_ratio"]), ("win_vad", wi["vad"], g["win_vad"]),
                        ("band", wi["band"][:, :ch], g["band"][:, :, 0]), ("denoised", r["denoised"], g["denoised"])):
            assert np.array_equal(a, b), (name, s, k, pu.first_mismatch(a, b))
    assert n_win > 0, name  # the pushes complete FFT B windows, so the band sums are compared


@pytest.mark.parametrize("mode,check", [("f32_fast", check_f32_fast), ("fp16", check_fp16)])
@pytest.mark.parametrize("name", list(CASES))
def test_tolerance_modes_vs_oracle(fvad_mod, oracle_mod, model, name, mode, check):
    """The same cases in the modes that share the three kernels, at each mode's own bounds."""
    ch = CASES[name][0]
    _, ref = _case(name)
    got = _run(fvad_mod, model, name, mode)
    for s, (r, g) in enumerate(zip(ref, got)):
        check(r, g, ch, (name, mode, s))


def test_fp16_fused_equals_fp16_ragged(fvad_mod, model):
    """k_fused16 runs the Ep / Exp chains through the same pspec_features: bit for bit the fp16 mode's."""
    a = _run(fvad_mod, model, "6x2-ragged", "fp16")
    b = _run(fvad_mod, model, "6x2-ragged", "fp16_fused")
    for s, (x, y) in enumerate(zip(a, b)):
        for k in KEYS:
            assert np.array_equal(x[k], y[k]), (s, k)
