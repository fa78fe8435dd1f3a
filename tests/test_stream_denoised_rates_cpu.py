"""Per-stream denoised rates (FVAD_DENOISED_RATE_PER_STREAM), the host's part:
the packed layout fvad_denoised_layout against a direct computation, the config
struct's new field through the C compiler, and Engine.unpack_denoised against a
hand-packed array.  No GPU."""
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
    off = fvad_mod.denoised_layout(rates, C)
    assert off.dtype == np.int64 and np.array_equal(off, direct(rates, C))
    assert off[0] == 0 and off[-1] == C * sum(r // 100 for r in rates)
    assert np.array_equal(off, fvad_mod.input_layout(rates, C))  # one arithmetic for both sides


def test_layout_past_2_31(fvad_mod):
    """offsets are 64-bit: 400000 streams of 8 channels at 96 kHz are 3e9 samples a tick"""
    rates = np.full(400000, 96000, np.int32)
    rates[::7] = 44100
    off = fvad_mod.denoised_layout(rates, 8)
    assert off[-1] > 2 ** 31 and np.array_equal(off, direct(rates.tolist(), 8))


@pytest.mark.parametrize("bad", [0, 48001, 11025, -1, 192000])
def test_layout_refuses_unlisted_rate(fvad_mod, bad):
    with pytest.raises(fvad_mod.FvadError) as ei:
        fvad_mod.denoised_layout([16000, bad, 8000], 2)
    assert ei.value.code == ERATE


def test_engine_config_layout_in_c(fvad_mod, tmp_path):
    """denoised_rate_max stands in front of input_rate_max, denoised_rate and
    input_rate, which stay where they were: the header's struct through the C
    compiler."""
    E = fvad_mod.EngineConfig
    size = ctypes.sizeof(E)
    assert E.denoised_rate_max.offset == size - 16
    assert E.input_rate_max.offset == size - 12
    assert E.denoised_rate.offset == size - 8
    assert E.input_rate.offset == size - 4
    assert fvad_mod.DENOISED_RATE_PER_STREAM == -1
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include \"fvad.h\"\n"
                   "_Static_assert(sizeof(fvad_engine_config) == %d, \"size\");\n"
                   "_Static_assert(offsetof(fvad_engine_config, denoised_rate_max) == %d, \"denoised_rate_max\");\n"
                   "_Static_assert(offsetof(fvad_engine_config, input_rate_max) == %d, \"input_rate_max\");\n"
                   "_Static_assert(offsetof(fvad_engine_config, denoised_rate) == %d, \"denoised_rate\");\n"
                   "_Static_assert(offsetof(fvad_engine_config, input_rate) == %d, \"input_rate\");\n"
                   "_Static_assert(FVAD_DENOISED_RATE_PER_STREAM == -1, \"marker\");\n"
                   "int main(void) { return 0; }\n" % (size, size - 16, size - 12, size - 8, size - 4))
    cc = os.environ.get("CC", "gcc")
    r = subprocess.run([cc, "-std=gnu11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the default leaves the field at 0
    cfg = E()
    cfg.denoised_rate_max = 7
    fvad_mod.lib().fvad_engine_config_default(ctypes.byref(cfg), 3, 2)
    assert cfg.denoised_rate_max == 0 and cfg.input_rate_max == 0 and cfg.input_rate == 0 and cfg.denoised_rate == 0


class _Unpacker:
    """Engine.unpack_denoised needs only the layout: an engine's C and denoised_layout()."""

    def __init__(self, fvad, rates, C):
        self.B, self.C = len(rates), C
        self._off = fvad.denoised_layout(rates, C)
        self.unpack_denoised = fvad.Engine.unpack_denoised.__get__(self)

    def denoised_layout(self):
        return self._off


def test_unpack_denoised_inverts_a_hand_packed_array(fvad_mod):
    rates, C, T = [8000, 44100, 8000, 48000, 96000], 2, 3
    rng = np.random.default_rng(3)
    rows = [rng.standard_normal((T, C, r // 100)).astype(np.float32) for r in rates]
    off = direct(rates, C)
    packed = np.zeros(T * off[-1], np.float32)
    for s, r in enumerate(rates):
        for t in range(T):
            for c in range(C):  # the kernel's address: tick * tick_len + offsets[s] + c * n_out
                a = t * off[-1] + off[s] + c * (r // 100)
                packed[a:a + r // 100] = rows[s][t, c]
    u = _Unpacker(fvad_mod, rates, C)
    for layout in (None, off):
        got = u.unpack_denoised(packed, T, layout)
        assert len(got) == len(rates)
        for s in range(len(rates)):
            assert got[s].shape == rows[s].shape and np.array_equal(got[s], rows[s])
    # a slot longer than the push (collect's max_ticks buffer): only n_ticks ticks are read
    got = u.unpack_denoised(np.concatenate([packed, np.full(17, 9.0, np.float32)]), T)
    assert all(np.array_equal(g, r) for g, r in zip(got, rows))
    # another layout than the engine's current one
    got = u.unpack_denoised(packed[: T * 2 * 80 * 2], T, direct([8000, 8000], C))
    assert [g.shape for g in got] == [(T, C, 80)] * 2
