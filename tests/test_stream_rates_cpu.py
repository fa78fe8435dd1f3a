"""Per-stream input rates (FVAD_INPUT_RATE_PER_STREAM), the host's part: the
packed layout fvad_input_layout against a direct computation, the config
struct's new field through the C compiler, and Engine.pack_input against the
layout.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (8000, 16000, 24000, 32000, 44100, 48000, 96000)
ERATE = -6


def direct(rates, C):
    off = [0]
    for r in rates:
        off.append(off[-1] + C * (r // 100))
    return np.array(off, np.int64)


@pytest.mark.parametrize("C", [1, 8])
def test_layout_all_rates(fvad_mod, C):
    rates = list(RATES) + [44100, 8000, 96000]
    off = fvad_mod.input_layout(rates, C)
    assert off.dtype == np.int64 and np.array_equal(off, direct(rates, C))
    assert off[0] == 0 and off[-1] == C * sum(r // 100 for r in rates)


@pytest.mark.parametrize("rate", RATES)
def test_layout_single_stream(fvad_mod, rate):
    assert np.array_equal(fvad_mod.input_layout([rate], 2), [0, 2 * rate // 100])


def test_layout_past_2_31(fvad_mod):
    """offsets are 64-bit: 400000 streams of 8 channels at 96 kHz are 3e9 samples a tick"""
    n = 400000
    rates = np.full(n, 96000, np.int32)
    rates[::7] = 44100
    off = fvad_mod.input_layout(rates, 8)
    assert off[-1] > 2 ** 31 and np.array_equal(off, direct(rates.tolist(), 8))


@pytest.mark.parametrize("bad", [0, 48001, 11025, -1, 192000])
def test_layout_refuses_unlisted_rate(fvad_mod, bad):
    with pytest.raises(fvad_mod.FvadError) as ei:
        fvad_mod.input_layout([16000, bad, 8000], 2)
    assert ei.value.code == ERATE


def test_engine_config_layout_in_c(fvad_mod, tmp_path):
    """input_rate_max stands in front of denoised_rate and input_rate, which stay
    the last two fields: the header's struct through the C compiler."""
    E = fvad_mod.EngineConfig
    size = ctypes.sizeof(E)
    assert E.input_rate_max.offset == size - 12
    assert E.denoised_rate.offset == size - 8
    assert E.input_rate.offset == size - 4
    assert fvad_mod.INPUT_RATE_PER_STREAM == -1
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include \"fvad.h\"\n"
                   "_Static_assert(sizeof(fvad_engine_config) == %d, \"size\");\n"
                   "_Static_assert(offsetof(fvad_engine_config, input_rate_max) == %d, \"input_rate_max\");\n"
                   "_Static_assert(offsetof(fvad_engine_config, denoised_rate) == %d, \"denoised_rate\");\n"
                   "_Static_assert(offsetof(fvad_engine_config, input_rate) == %d, \"input_rate\");\n"
                   "_Static_assert(FVAD_INPUT_RATE_PER_STREAM == -1, \"marker\");\n"
                   "int main(void) { return 0; }\n" % (size, size - 12, size - 8, size - 4))
    cc = os.environ.get("CC", "gcc")
    r = subprocess.run([cc, "-std=gnu11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the default leaves the field at 0
    cfg = E()
    cfg.input_rate_max = 7
    fvad_mod.lib().fvad_engine_config_default(ctypes.byref(cfg), 3, 2)
    assert cfg.input_rate_max == 0 and cfg.input_rate == 0 and cfg.denoised_rate == 0


class _Packer:
    """Engine.pack_input needs only the layout: an engine's B, C and input_layout()."""

    def __init__(self, fvad, rates, C):
        self.B, self.C = len(rates), C
        self._off = fvad.input_layout(rates, C)
        self.pack_input = fvad.Engine.pack_input.__get__(self)

    def input_layout(self):
        return self._off


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_pack_input_round_trip(fvad_mod, dtype):
    rates, C, T = [8000, 44100, 8000, 48000, 96000], 2, 3
    rng = np.random.default_rng(3)
    rows = [rng.integers(-30000, 30000, (T, C, r // 100)).astype(dtype) for r in rates]
    p = _Packer(fvad_mod, rates, C)
    packed = p.pack_input(rows)
    off = p.input_layout()
    assert packed.dtype == dtype and packed.shape == (T * off[-1],)
    ticks = packed.reshape(T, off[-1])
    for s, r in enumerate(rates):
        got = ticks[:, off[s]:off[s + 1]].reshape(T, C, r // 100)
        assert np.array_equal(got, rows[s])
        for t in range(T):
            for c in range(C):  # the kernel's address: tick * tick_len + offsets[s] + c * n_in
                a = t * off[-1] + off[s] + c * (r // 100)
                assert np.array_equal(packed[a:a + r // 100], rows[s][t, c])
    with pytest.raises(ValueError):
        p.pack_input(rows[:-1])
    with pytest.raises(ValueError):
        p.pack_input(rows[:1] + [rows[0]] + rows[2:])
