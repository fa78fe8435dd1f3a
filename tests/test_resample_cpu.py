"""Input resampling on the host alone (no GPU): fvad_resample_info,
fvad_resample_taps and fvad_resample_host (csrc/fvad_resample.cpp), the mirror
the GPU tests hold k_resample to.  The oracle for the mirror is an independent
f64 computation in numpy: the tap design from include/fvad.h's formulas, and a
direct convolution with the returned f32 taps."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERATE, EDEVICE = -6, -2
# rate: (L, M, K, frame_in, tail, delay in 48 kHz samples)
TABLE = {8000: (6, 1, 48, 80, 47, 143.5), 16000: (3, 1, 48, 160, 47, 71.5), 24000: (2, 1, 48, 240, 47, 47.5),
         32000: (3, 2, 48, 320, 47, 35.75), 44100: (160, 147, 48, 441, 47, (160 * 48 - 1) / (2 * 147)),
         96000: (1, 2, 96, 960, 95, 23.75)}
RATES = sorted(TABLE)


def design(rate):
    """The prototype in f64 from the formulas: (proto [N] summing to L, f_stop, df, Fp)."""
    g = math.gcd(48000, rate)
    L, M = 48000 // g, rate // g
    K = 48 * max(1, -(-M // L))
    N, Fp, A = L * K, float(L * rate), 80.0
    beta = 0.1102 * (A - 8.7)
    df = (A - 8.0) / (2.285 * (N - 1)) * Fp / (2.0 * np.pi)
    f_stop = min(rate, 48000) / 2.0
    fc = f_stop - df / 2.0
    j = np.arange(N, dtype=np.float64)
    proto = np.sinc(2.0 * fc / Fp * (j - (N - 1) / 2.0)) * \
        np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (2.0 * j / (N - 1) - 1.0) ** 2))) / np.i0(beta)
    proto *= L / proto.sum()
    return proto, f_stop, df, Fp, (L, M, K)


def convolve64(rate, taps, x):
    """y[n] over whole ticks of x in f64 with the f32 taps, zeros before x[0]."""
    L, M, K = TABLE[rate][:3]
    n_out = x.size * L // M
    n = np.arange(n_out)
    i, p = (n * M) // L, (n * M) % L
    xp = np.concatenate([np.zeros(K - 1), x.astype(np.float64)])
    k = np.arange(K)
    return (taps.astype(np.float64)[p] * xp[(K - 1) + i[:, None] - k[None, :]]).sum(axis=1)


def test_info_table_and_rate_list(fvad_mod):
    for rate, (L, M, K, n_in, tail, delay) in TABLE.items():
        d = fvad_mod.resample_info(rate)
        assert (d["input_rate"], d["L"], d["M"], d["taps_per_phase"], d["frame_in"]) == (rate, L, M, K, n_in)
        assert d["taps_per_phase"] - 1 == tail <= n_in
        assert d["delay"] == pytest.approx(delay, abs=1e-12) and d["delay"] == (L * K - 1) / (2 * M)
    for rate in (0, 7999, 11025, 12000, 22050, 48000, 48001, 192000):
        with pytest.raises(fvad_mod.FvadError) as ei:
            fvad_mod.resample_info(rate)
        assert ei.value.code == ERATE, rate


def test_engine_create_checks_the_rate_before_the_device(fvad_mod):
    from conftest import gpu_available
    model = fvad_mod.Model(seed=1)
    with pytest.raises(fvad_mod.FvadError) as ei:
        fvad_mod.Engine(model, 2, input_rate=22050)
    assert ei.value.code == ERATE
    if not gpu_available():
        with pytest.raises(fvad_mod.FvadError) as ei:
            fvad_mod.Engine(model, 2, input_rate=16000)
        assert ei.value.code == EDEVICE


@pytest.mark.parametrize("rate", RATES)
def test_taps_match_the_formulas(fvad_mod, rate):
    taps = fvad_mod.resample_taps(rate)
    proto, _, _, _, (L, M, K) = design(rate)
    assert taps.shape == (L, K) and taps.dtype == np.float32
    want = proto.reshape(K, L).T  # taps[p][k] = proto[k L + p]
    err = np.abs(taps.astype(np.float64) - want).max()
    print(rate, "max |tap - f64 design|", err)
    assert np.abs(taps).max() < 1.0
    assert err <= 2.0 ** -22


@pytest.mark.parametrize("rate", RATES)
def test_frequency_response(fvad_mod, rate):
    taps = fvad_mod.resample_taps(rate)
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
    L, M, K, n_in = TABLE[rate][:4]
    taps = fvad_mod.resample_taps(rate)
    x = np.random.default_rng(rate).uniform(-1.0, 1.0, 20 * n_in).astype(np.float32)
    got = fvad_mod.resample_host(rate, x)
    want = convolve64(rate, taps, x)
    assert got.shape == (20 * 480,) == want.shape
    bound = (K + 1) * 2.0 ** -24 * np.abs(taps.astype(np.float64)).sum(axis=1).max() * np.abs(x).max()
    err = np.abs(got.astype(np.float64) - want).max()
    print(rate, "max |host - f64|", err, "bound", bound)
    assert err <= bound


@pytest.mark.parametrize("rate", RATES)
def test_streaming_equals_one_call(fvad_mod, rate):
    L, M, K, n_in = TABLE[rate][:4]
    x = np.random.default_rng(7 + rate).uniform(-1.0, 1.0, 30 * n_in).astype(np.float32)
    whole = fvad_mod.resample_host(rate, x)
    tail = np.zeros(K - 1, np.float32)
    parts, t = [], 0
    for n in (1, 2, 3, 4, 5, 6, 7, 2):  # 30 ticks
        parts.append(fvad_mod.resample_host(rate, x[t * n_in:(t + n) * n_in], tail))
        t += n
    assert t == 30
    assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))
    assert np.array_equal(tail, x[-(K - 1):])
    # no tail: zeros for history, and nothing kept
    first = fvad_mod.resample_host(rate, x[:n_in])
    assert np.array_equal(first.view(np.uint32), whole[:480].view(np.uint32))
    later = fvad_mod.resample_host(rate, x[n_in:2 * n_in])
    z = np.zeros(K - 1, np.float32)
    assert np.array_equal(later.view(np.uint32), fvad_mod.resample_host(rate, x[n_in:2 * n_in], z).view(np.uint32))


@pytest.mark.parametrize("rate", RATES)
def test_sines_come_out_delayed(fvad_mod, rate):
    L, M, K, n_in, _, delay = TABLE[rate]
    _, f_stop, df, _, _ = design(rate)
    for freq in (1000.0, 0.9 * (f_stop - df)):
        t = np.arange(30 * n_in, dtype=np.float64)
        x = np.sin(2.0 * np.pi * freq * t / rate).astype(np.float32)
        y = fvad_mod.resample_host(rate, x).astype(np.float64)
        n = np.arange(y.size, dtype=np.float64)
        want = np.sin(2.0 * np.pi * freq * (n - delay) / 48000.0)
        n0 = int(math.ceil(2 * delay + 1))
        err = np.abs(y - want)[n0:].max()
        print(rate, freq, "max |y - delayed sine|", err)
        assert err <= 2.5e-4


def test_engine_config_size_in_c(fvad_mod, tmp_path):
    """The header's own struct, through the C compiler the oracle is built with."""
    size = ctypes.sizeof(fvad_mod.EngineConfig)
    assert fvad_mod.EngineConfig.input_rate.offset == size - 4
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include \"fvad.h\"\n"
                   "_Static_assert(sizeof(fvad_engine_config) == %d, \"size\");\n"
                   "_Static_assert(offsetof(fvad_engine_config, input_rate) == %d, \"input_rate\");\n"
                   "_Static_assert(sizeof(fvad_resample_desc) == %d, \"desc\");\n"
                   "int main(void) { return 0; }\n" % (size, size - 4, ctypes.sizeof(fvad_mod.ResampleDesc)))
    cc = os.environ.get("CC", "gcc")
    r = subprocess.run([cc, "-std=gnu11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
