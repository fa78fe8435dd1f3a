"""The output downsampler on the host alone (no GPU): fvad_resample_out_info,
fvad_resample_out_taps and fvad_resample_out_host (csrc/fvad_resample.cpp),
the mirror the GPU tests hold k_resample_out to.  As in
tests/test_resample_cpu.py the oracle is an independent f64 computation in
numpy: the tap design from include/fvad.h's formulas (section 2d), and a direct
convolution with the returned f32 taps.  The bounds are that file's."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ERATE = -1, -6
FRAME = 480
# rate: (L, M, K, frame_out, tail, delay in 48 kHz samples)
TABLE = {8000: (1, 6, 288, 80, 287, 143.5), 16000: (1, 3, 144, 160, 143, 71.5), 24000: (1, 2, 96, 240, 95, 47.5),
         32000: (2, 3, 96, 320, 95, 47.75), 44100: (147, 160, 96, 441, 95, 14111 / 294),
         96000: (2, 1, 48, 960, 47, 23.75)}
RATES = sorted(TABLE)


def design(rate):
    """The prototype in f64 from the formulas: (proto [N] summing to L, f_stop, df, Fp, (L, M, K))."""
    g = math.gcd(48000, rate)
    L, M = rate // g, 48000 // g
    K = 48 * max(1, -(-M // L))
    N, Fp, A = L * K, float(48000 * L), 80.0
    beta = 0.1102 * (A - 8.7)
    df = (A - 8.0) / (2.285 * (N - 1)) * Fp / (2.0 * np.pi)
    f_stop = min(rate, 48000) / 2.0
    fc = f_stop - df / 2.0
    j = np.arange(N, dtype=np.float64)
    proto = np.sinc(2.0 * fc / Fp * (j - (N - 1) / 2.0)) * \
        np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (2.0 * j / (N - 1) - 1.0) ** 2))) / np.i0(beta)
    proto *= L / proto.sum()
    return proto, f_stop, df, Fp, (L, M, K)


def convolve64(rate, taps, y):
    """out[n] over whole 48 kHz ticks of y in f64 with the f32 taps, zeros before y[0]."""
    L, M, K = TABLE[rate][:3]
    n_out = y.size * L // M
    n = np.arange(n_out)
    i, p = (n * M) // L, (n * M) % L
    yp = np.concatenate([np.zeros(K - 1), y.astype(np.float64)])
    k = np.arange(K)
    return (taps.astype(np.float64)[p] * yp[(K - 1) + i[:, None] - k[None, :]]).sum(axis=1)


def test_info_table_and_rate_list(fvad_mod):
    for rate, (L, M, K, n_out, tail, delay) in TABLE.items():
        d = fvad_mod.resample_out_info(rate)
        assert (d["rate"], d["L"], d["M"], d["taps_per_phase"], d["frame_out"]) == (rate, L, M, K, n_out)
        assert d["taps_per_phase"] - 1 == tail <= FRAME
        assert FRAME * L == n_out * M  # every tick starts at phase 0
        assert d["delay"] == pytest.approx(delay, abs=1e-12) and d["delay"] == (L * K - 1) / (2 * L)
        assert L * K * 4 <= 56448
    for rate in (0, 7999, 11025, 12000, 22050, 48000, 48001, 192000):
        for call in (fvad_mod.resample_out_info, fvad_mod.resample_out_taps,
                     lambda r: fvad_mod.lib().fvad_resample_out_host(r, None, 0, None, None)):
            try:
                rc = call(rate)
            except fvad_mod.FvadError as err:
                rc = err.code
            assert rc == ERATE, rate


def test_engine_create_checks_the_rate_before_the_device(fvad_mod):
    model = fvad_mod.Model(seed=1)
    with pytest.raises(fvad_mod.FvadError) as ei:
        fvad_mod.Engine(model, 2, want_denoised=True, denoised_rate=22050)
    assert ei.value.code == ERATE
    # a listed rate needs the denoised rows: want_denoised and the denoiser
    for kw in (dict(), dict(want_denoised=True, use_denoiser=False)):
        with pytest.raises(fvad_mod.FvadError) as ei:
            fvad_mod.Engine(model, 2, denoised_rate=16000, **kw)
        assert ei.value.code == EINVAL, kw


@pytest.mark.parametrize("rate", RATES)
def test_taps_match_the_formulas(fvad_mod, rate):
    taps = fvad_mod.resample_out_taps(rate)
    proto, _, _, _, (L, M, K) = design(rate)
    assert (L, M, K) == TABLE[rate][:3]
    assert taps.shape == (L, K) and taps.dtype == np.float32
    want = proto.reshape(K, L).T  # taps[p][k] = proto[k L + p]
    err = np.abs(taps.astype(np.float64) - want).max()
    print(rate, "max |tap - f64 design|", err)
    assert np.abs(taps).max() < 1.0
    assert err <= 2.0 ** -22


@pytest.mark.parametrize("rate", RATES)
def test_frequency_response(fvad_mod, rate):
    taps = fvad_mod.resample_out_taps(rate)
    _, f_stop, df, Fp, (L, M, K) = design(rate)
    proto = taps.astype(np.float64).T.reshape(-1)  # proto[k L + p]
    n_fft = 1 << 20
    H = np.abs(np.fft.rfft(proto, n_fft)) / L
    f = np.arange(H.size) * Fp / n_fft
    with np.errstate(divide="ignore"):
        db = 20.0 * np.log10(H)
    ripple = np.abs(db[f <= f_stop - df]).max()
    stop = db[f >= f_stop].max()
    print(rate, "ripple dB", ripple, "stopband dB", stop)
    assert ripple <= 0.002
    assert stop <= -78.0


@pytest.mark.parametrize("rate", RATES)
def test_host_against_f64_convolution(fvad_mod, rate):
    L, M, K, n_out = TABLE[rate][:4]
    taps = fvad_mod.resample_out_taps(rate)
    y = np.random.default_rng(rate).uniform(-1.0, 1.0, 20 * FRAME).astype(np.float32)
    got = fvad_mod.resample_out_host(rate, y)
    want = convolve64(rate, taps, y)
    assert got.shape == (20 * n_out,) == want.shape
    bound = (K + 1) * 2.0 ** -24 * np.abs(taps.astype(np.float64)).sum(axis=1).max() * np.abs(y).max()
    err = np.abs(got.astype(np.float64) - want).max()
    print(rate, "max |host - f64|", err, "bound", bound)
    assert err <= bound


@pytest.mark.parametrize("rate", RATES)
def test_streaming_equals_one_call(fvad_mod, rate):
    L, M, K, n_out = TABLE[rate][:4]
    n_ticks = 36
    y = np.random.default_rng(7 + rate).uniform(-1.0, 1.0, n_ticks * FRAME).astype(np.float32)
    whole = fvad_mod.resample_out_host(rate, y)
    tail = np.zeros(K - 1, np.float32)
    parts, t = [], 0
    for n in (1, 2, 3, 4, 5, 6, 7, 8):  # 36 ticks
        parts.append(fvad_mod.resample_out_host(rate, y[t * FRAME:(t + n) * FRAME], tail))
        t += n
    assert t == n_ticks
    assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))
    assert np.array_equal(tail, y[-(K - 1):])
    # no tail: zeros for history, and nothing kept
    first = fvad_mod.resample_out_host(rate, y[:FRAME])
    assert np.array_equal(first.view(np.uint32), whole[:n_out].view(np.uint32))
    later = fvad_mod.resample_out_host(rate, y[FRAME:2 * FRAME])
    z = np.zeros(K - 1, np.float32)
    assert np.array_equal(later.view(np.uint32),
                          fvad_mod.resample_out_host(rate, y[FRAME:2 * FRAME], z).view(np.uint32))


@pytest.mark.parametrize("rate", RATES)
def test_sines_come_out_delayed(fvad_mod, rate):
    L, M, K, n_out, _, delay = TABLE[rate]
    _, f_stop, df, _, _ = design(rate)
    for freq in (1000.0, 0.9 * (f_stop - df)):
        t = np.arange(30 * FRAME, dtype=np.float64)
        y = np.sin(2.0 * np.pi * freq * t / 48000.0).astype(np.float32)
        out = fvad_mod.resample_out_host(rate, y).astype(np.float64)
        # output n stands at the 48 kHz position n M / L, the signal delayed by `delay` samples of 48 kHz
        n = np.arange(out.size, dtype=np.float64)
        want = np.sin(2.0 * np.pi * freq * (n * M / L - delay) / 48000.0)
        n0 = int(math.ceil((2 * delay + 1) * L / M))
        err = np.abs(out - want)[n0:].max()
        print(rate, freq, "max |out - delayed sine|", err)
        assert err <= 2.5e-4


def test_engine_config_size_in_c(fvad_mod, tmp_path):
    """The header's own structs, through the C compiler the oracle is built with."""
    size = ctypes.sizeof(fvad_mod.EngineConfig)
    assert fvad_mod.EngineConfig.denoised_rate.offset == size - 8
    assert fvad_mod.EngineConfig.input_rate.offset == size - 4
    assert ctypes.sizeof(fvad_mod.ResampleDesc) == 32  # fvad_resample_desc keeps its size
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include \"fvad.h\"\n"
                   "_Static_assert(sizeof(fvad_engine_config) == %d, \"size\");\n"
                   "_Static_assert(offsetof(fvad_engine_config, denoised_rate) == %d, \"denoised_rate\");\n"
                   "_Static_assert(offsetof(fvad_engine_config, input_rate) == %d, \"input_rate\");\n"
                   "_Static_assert(sizeof(fvad_resample_desc) == 32, \"desc\");\n"
                   "_Static_assert(sizeof(fvad_resample_out_desc) == %d, \"out desc\");\n"
                   "_Static_assert(offsetof(fvad_resample_out_desc, frame_out) == %d, \"frame_out\");\n"
                   "_Static_assert(offsetof(fvad_resample_out_desc, delay) == %d, \"delay\");\n"
                   "int main(void) { return 0; }\n"
                   % (size, size - 8, size - 4, ctypes.sizeof(fvad_mod.ResampleOutDesc),
                      fvad_mod.ResampleOutDesc.frame_out.offset, fvad_mod.ResampleOutDesc.delay.offset))
    cc = os.environ.get("CC", "gcc")
    r = subprocess.run([cc, "-std=gnu11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
