"""CPU: block-compressed (BC1-BC7) .gtx files through the reader and writer, and the parts of the texture-decode ABI that need no
device: the format tables, and gr_texture_decode's refusals against the device-less HIP stand-in of tests/hip_stub."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from granite_amd import app as gapp
from granite_amd import capi, gtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hip_stub", "libhip_stub.so")


def _levels(rng, fmt, w, h, levels, layers):
    out = []
    for l in range(levels):
        bx, by = (max(w >> l, 1) + 3) // 4, (max(h >> l, 1) + 3) // 4
        out.append(rng.integers(0, 256, (layers, by, bx, gtx.block_bytes(fmt)), dtype=np.uint8))
    return out


def test_bc_gtx_round_trip_and_hand_computed_layout(tmp_path):
    rng = np.random.default_rng(3)
    # BC3, 20 x 12, three levels (20x12, 10x6, 5x3 -> 5x3, 3x2, 2x1 blocks of 16 bytes), two layers
    levels = _levels(rng, capi.FORMAT_BC3_UNORM_BLOCK, 20, 12, 3, 2)
    path = str(tmp_path / "bc3.gtx")
    gtx.write(path, capi.FORMAT_BC3_UNORM_BLOCK, levels, flags=0x1234 << 16, layers=2, size=(20, 12))
    f = gtx.read(path)
    assert (f.info.format, f.info.width, f.info.height, f.info.layers, f.info.levels, f.info.flags) == (137, 20, 12, 2, 3, 0x1234 << 16)
    assert [f.level_offset(l) for l in range(3)] == [0, 480, 672] and f.info.payload_size == 736
    assert os.path.getsize(path) == 64 + 736
    for l in range(3):
        assert f.level(l).shape == levels[l].shape and np.array_equal(f.level(l), levels[l])
    # BC1 (8-byte blocks), one layer: level 0 is 120 bytes, so level 1 starts at the next multiple of 16
    levels = _levels(rng, capi.FORMAT_BC1_RGB_SRGB_BLOCK, 20, 12, 3, 1)
    path = str(tmp_path / "bc1.gtx")
    gtx.write(path, capi.FORMAT_BC1_RGB_SRGB_BLOCK, [a[0] for a in levels], size=(20, 12))
    f = gtx.read(path)
    assert [f.level_offset(l) for l in range(3)] == [0, 128, 176] and f.info.payload_size == 192
    assert np.array_equal(f.level(2), levels[2]) and f.level(2).shape == (1, 1, 2, 8)


def test_truncated_bc_payload_is_refused(tmp_path):
    rng = np.random.default_rng(4)
    path = str(tmp_path / "bc7.gtx")
    gtx.write(path, capi.FORMAT_BC7_UNORM_BLOCK, [a[0] for a in _levels(rng, capi.FORMAT_BC7_UNORM_BLOCK, 13, 7, 1, 1)], size=(13, 7))
    raw = open(path, "rb").read()
    assert len(raw) == 64 + 4 * 2 * 16
    short = str(tmp_path / "short.gtx")
    open(short, "wb").write(raw[:-16])
    with pytest.raises(gtx.GtxError, match="truncated"):
        gtx.read(short)
    # a header that declares the texel-sized payload of an uncompressed image of the same extent
    wrong = bytearray(raw)
    wrong[48:56] = (13 * 7 * 16).to_bytes(8, "little")
    open(short, "wb").write(bytes(wrong) + bytes(13 * 7 * 16))
    with pytest.raises(gtx.GtxError, match="payload size"):
        gtx.read(short)


@pytest.mark.parametrize("fmt", [140, 142, 147])
def test_snorm_and_etc2_stay_refused(tmp_path, fmt):
    path = str(tmp_path / "x.gtx")
    gtx.write(path, capi.FORMAT_BC5_UNORM_BLOCK, [np.zeros((1, 1, 16), np.uint8)], size=(4, 4))
    raw = bytearray(open(path, "rb").read())
    raw[20:24] = fmt.to_bytes(4, "little")
    open(path, "wb").write(raw)
    with pytest.raises(gtx.GtxError, match="format"):
        gtx.probe(path)


def test_decoded_format_and_block_bytes_of_every_enumerant():
    lib = capi.load_library()
    rgba, srgb = capi.FORMAT_R8G8B8A8_UNORM, capi.FORMAT_R8G8B8A8_SRGB
    want = {131: (rgba, 8), 132: (srgb, 8), 133: (rgba, 8), 134: (srgb, 8), 135: (rgba, 16), 136: (srgb, 16), 137: (rgba, 16), 138: (srgb, 16),
            139: (capi.FORMAT_R8_UNORM, 8), 141: (capi.FORMAT_R8G8_UNORM, 16), 143: (capi.FORMAT_R16G16B16A16_SFLOAT, 16),
            144: (capi.FORMAT_R16G16B16A16_SFLOAT, 16), 145: (rgba, 16), 146: (srgb, 16)}
    assert sorted(want) == sorted(capi.BLOCK_FORMATS)
    for fmt in range(0, 200):
        decoded, nbytes = want.get(fmt, (capi.FORMAT_UNDEFINED if hasattr(capi, "FORMAT_UNDEFINED") else 0, 0))
        assert lib.gr_texture_decoded_format(fmt) == decoded, fmt
        assert lib.gr_texture_block_bytes(fmt) == nbytes, fmt
        if nbytes:
            assert gtx.block_bytes(fmt) == nbytes


def test_decode_symbols_are_bound():
    lib = gapp.load_library()
    assert "gra_gtx_decode" in gapp.EXPORTED_SYMBOLS and hasattr(lib, "gra_gtx_decode")
    for name in ("gr_texture_decode", "gr_texture_decoded_format", "gr_texture_block_bytes"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(capi.load_library(), name)


WORKER = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
from granite_amd import capi
stub = C.CDLL(%(stub)r); stub.hip_stub_count.restype = C.c_uint64; stub.hip_stub_count.argtypes = [C.c_char_p]
gr = capi.Context(0)
blocks, texels = capi.DeviceBuffer(gr, 4096), capi.DeviceBuffer(gr, 65536)
def call(fmt, pitch, w, h, out_pitch, out_fmt, blocks_ptr=blocks.ptr, out_ptr=texels.ptr):
    before = stub.hip_stub_count(b"launches")
    code = gr.lib.gr_texture_decode(gr.handle, None, fmt, blocks_ptr, pitch, C.byref(capi.Image(out_ptr, w, h, out_pitch, out_fmt)))
    return [code, gr.lib.gr_last_error(gr.handle).decode() if code < 0 else "", stub.hip_stub_count(b"launches") - before]
rgba, rg = capi.FORMAT_R8G8B8A8_UNORM, capi.FORMAT_R8G8_UNORM
out = {
    "ok": call(145, 64, 13, 7, 52, rgba),
    "wrong_out_format": call(145, 64, 13, 7, 52, capi.FORMAT_R8G8B8A8_SRGB),
    "bc5_into_rgba": call(141, 64, 13, 7, 52, rgba),
    "out_pitch_small": call(145, 64, 13, 7, 51, rgba),
    "block_pitch_small": call(145, 63, 13, 7, 52, rgba),
    "unknown": call(147, 64, 13, 7, 52, rgba),
    "snorm": call(140, 64, 13, 7, 13, capi.FORMAT_R8_UNORM),
    "uncompressed": call(rgba, 64, 13, 7, 52, rgba),
    "null_blocks": call(145, 64, 13, 7, 52, rgba, blocks_ptr=None),
    "empty": call(145, 0, 0, 7, 0, rgba),
    "too_large": call(139, 1 << 20, 65537, 4, 1 << 17, capi.FORMAT_R8_UNORM),
}
print(json.dumps(out))
'''


def test_texture_decode_refusals_need_no_device():
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(os.path.join(os.path.dirname(STUB), "hip_stub.cpp")):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(STUB)])
    r = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT, "stub": STUB}], env=dict(os.environ, LD_PRELOAD=STUB),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"] == [0, "", 1]
    assert out["empty"] == [0, "", 0]  # GR_OK without a launch
    INVALID, UNSUPPORTED = -1, -3
    for key, code, text in (("wrong_out_format", UNSUPPORTED, "decoded format"), ("bc5_into_rgba", UNSUPPORTED, "decoded format"),
                            ("out_pitch_small", INVALID, "output pitch"), ("block_pitch_small", INVALID, "block row pitch"),
                            ("unknown", UNSUPPORTED, "not a block format"), ("snorm", UNSUPPORTED, "not a block format"),
                            ("uncompressed", UNSUPPORTED, "not a block format"), ("null_blocks", INVALID, "blocks"),
                            ("too_large", INVALID, "larger than")):
        got = out[key]
        assert got[0] == code and text in got[1] and got[2] == 0, (key, got)
