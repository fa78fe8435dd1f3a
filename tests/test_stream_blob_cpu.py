"""Stream blobs on the host alone (no GPU): fvad_stream_blob_info parses and
validates a header assembled here from the layout include/fvad.h documents,
the header's constants equal the binding's, and the lifecycle kernels
(fvad_lifecycle.hip) compile for gfx950 without scratch spills or LDS."""
import os
import re
import struct

import numpy as np
import pytest

from test_kernel_resources import HIPCC, resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the documented layout: offset -> field, little endian, 128 bytes
FIELDS = [("magic", "I"), ("version", "I"), ("header_bytes", "I"), ("count", "I"), ("stream_bytes", "Q"),
          ("mode", "I"), ("n_channels", "I"), ("fft_size", "I"), ("use_denoiser", "I"), ("n_bands", "I"),
          ("n_machines", "I"), ("seg_capacity", "I"), ("state_words", "I"), ("config_hash", "Q"),
          ("model_hash", "Q"), ("sample_rate", "I")]
FMT = "<" + "".join(f for _, f in FIELDS) + "52x"


def header(**over):
    v = dict(magic=0x42535646, version=1, header_bytes=128, count=3, stream_bytes=4096, mode=4, n_channels=2,
             fft_size=2048, use_denoiser=1, n_bands=2, n_machines=2, seg_capacity=8, state_words=2880,
             config_hash=0x0123456789abcdef, model_hash=0xfedcba9876543210, sample_rate=48000)
    v.update(over)
    return v, struct.pack(FMT, *[v[n] for n, _ in FIELDS])


def blob_of(hdr_bytes, body):
    return np.frombuffer(hdr_bytes + bytes(body), np.uint8)


def test_layout_is_128_bytes_with_the_documented_offsets():
    assert struct.calcsize(FMT) == 128
    off = {}
    for i, (n, _) in enumerate(FIELDS):
        off[n] = struct.calcsize("<" + "".join(f for _, f in FIELDS[:i]))
    assert (off["stream_bytes"], off["mode"], off["state_words"], off["config_hash"], off["model_hash"],
            off["sample_rate"]) == (16, 24, 52, 56, 64, 72)
    hdr = open(os.path.join(ROOT, "include", "fvad.h")).read()
    for n, _ in FIELDS:  # the header documents each field at that offset
        assert re.search(r"\b%s;\s*/\*\s*%d\b" % (n, off[n]), hdr), (n, off[n])


def test_blob_info_returns_the_fields(fvad_mod):
    v, h = header()
    info = fvad_mod.stream_blob_info(blob_of(h, 3 * 4096))
    assert info == v
    # trailing bytes past the records are allowed, a count of zero too
    assert fvad_mod.stream_blob_info(blob_of(h, 3 * 4096 + 5))["count"] == 3
    assert fvad_mod.stream_blob_info(blob_of(header(count=0)[1], 0))["count"] == 0


@pytest.mark.parametrize("case", ["short", "magic", "version", "overrun", "overrun_by_one", "header_bytes",
                                  "huge_product"])
def test_blob_info_rejects(fvad_mod, case):
    _, h = header()
    blob = {
        "short": np.frombuffer(h[:127], np.uint8),
        "magic": blob_of(header(magic=0x42535647)[1], 3 * 4096),
        "version": blob_of(header(version=2)[1], 3 * 4096),
        "overrun": blob_of(h, 2 * 4096),
        "overrun_by_one": blob_of(h, 3 * 4096 - 1),
        "header_bytes": blob_of(header(header_bytes=64)[1], 3 * 4096),
        # stream_bytes * count wraps 2^64: must not pass as a small product
        "huge_product": blob_of(header(stream_bytes=2 ** 62, count=4)[1], 4096),
    }[case]
    with pytest.raises(fvad_mod.FvadError) as ei:
        fvad_mod.stream_blob_info(blob)
    assert ei.value.code == fvad_mod.EFORMAT


def test_header_constants_match_binding(fvad_mod):
    hdr = open(os.path.join(ROOT, "include", "fvad.h")).read()
    defs = dict(re.findall(r"#define\s+(FVAD_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|-?\d+)", hdr))
    val = lambda k: int(defs[k].rstrip("u"), 0)
    assert fvad_mod.STREAM_BLOB_MAGIC == val("FVAD_STREAM_BLOB_MAGIC") == struct.unpack("<I", b"FVSB")[0]
    assert fvad_mod.STREAM_BLOB_VERSION == val("FVAD_STREAM_BLOB_VERSION")
    assert fvad_mod.STREAM_BLOB_HEADER_BYTES == val("FVAD_STREAM_BLOB_HEADER_BYTES") == 128
    assert fvad_mod.DEBUG_RESET_TIMES == val("FVAD_DEBUG_RESET_TIMES")
    errs = dict((k, int(v)) for k, v in re.findall(r"#define\s+(FVAD_E[A-Z]+)\s+\((-\d+)\)", hdr))
    assert (fvad_mod.EINVAL, fvad_mod.EFORMAT) == (errs["FVAD_EINVAL"], errs["FVAD_EFORMAT"])
    import ctypes
    assert ctypes.sizeof(fvad_mod.StreamBlobHeader) == 128
    for n, _ in FIELDS:
        assert hasattr(fvad_mod.StreamBlobHeader, n)
    assert fvad_mod.StreamBlobHeader.stream_bytes.offset == 16 and fvad_mod.StreamBlobHeader.sample_rate.offset == 72


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_lifecycle_kernels_use_no_lds_and_spill_nothing():
    got = resources("fvad_lifecycle.hip")
    for k in ("k_stream_clear", "k_stream_vclear", "k_stream_gather", "k_stream_scatter"):
        assert k in got, (k, sorted(got))
        assert got[k]["VGPRs_spill"] == 0 and got[k]["LDS"] == 0, (k, got[k])
    print({k: got[k] for k in sorted(got)})
