"""CPU: the parts of the ASTC texture-decode ABI that need no device, against the device-less HIP stand-in of tests/hip_stub: a valid call
costs one launch, an empty one none, everything gr_texture_decode refuses is refused before a launch, and the host-only queries answer for
the 28 ASTC LDR formats, for BC1-BC7 and for formats that are neither."""
import ctypes as C
import json
import os
import subprocess
import sys

from granite_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hip_stub", "libhip_stub.so")
ASTC_4x4_SFLOAT = 1000066000  # VK_FORMAT_ASTC_4x4_SFLOAT_BLOCK: the HDR profile, not handled


def test_block_queries_answer_for_astc_bc_and_neither():
    lib = capi.load_library()
    for name in ("gr_texture_block_dim", "gr_texture_block_info"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert sorted(capi.ASTC_FORMATS) == list(range(157, 185))
    assert capi.FORMAT_ASTC_4x4_UNORM_BLOCK == 157 and capi.FORMAT_ASTC_6x5_SRGB_BLOCK == 164 and capi.FORMAT_ASTC_12x12_SRGB_BLOCK == 184
    w, h, nbytes, decoded = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    footprints = ((4, 4), (5, 4), (5, 5), (6, 5), (6, 6), (8, 5), (8, 6), (8, 8), (10, 5), (10, 6), (10, 8), (10, 10), (12, 10), (12, 12))
    for fmt in list(range(0, 256)) + [ASTC_4x4_SFLOAT, ASTC_4x4_SFLOAT + 13]:
        w.value = h.value = nbytes.value = decoded.value = 77
        dim, info = lib.gr_texture_block_dim(fmt, C.byref(w), C.byref(h)), lib.gr_texture_block_info(fmt, C.byref(nbytes), C.byref(decoded))
        if 157 <= fmt <= 184:
            assert (dim, info) == (0, 0) and (w.value, h.value) == footprints[(fmt - 157) // 2] == capi.ASTC_FORMATS[fmt], fmt
            assert nbytes.value == 16 and decoded.value == (capi.FORMAT_R8G8B8A8_SRGB if (fmt - 157) & 1 else capi.FORMAT_R8G8B8A8_UNORM), fmt
            assert capi.Context.texture_block_info(fmt) == (w.value, h.value, 16, decoded.value)
        elif fmt in capi.BLOCK_FORMATS:
            assert (dim, info) == (0, 0) and (w.value, h.value) == (4, 4), fmt
            assert nbytes.value == lib.gr_texture_block_bytes(fmt) and decoded.value == lib.gr_texture_decoded_format(fmt), fmt
        else:  # uncompressed formats, the SNORM forms, ETC2 / EAC, ASTC SFLOAT, numbers that name nothing
            assert dim == -3 and info == -3 and (w.value, h.value) == (77, 77), fmt
    assert lib.gr_texture_block_dim(157, None, C.byref(h)) == -1 and lib.gr_texture_block_info(157, C.byref(nbytes), None) == -1


WORKER = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
from granite_amd import capi
stub = C.CDLL(%(stub)r); stub.hip_stub_count.restype = C.c_uint64; stub.hip_stub_count.argtypes = [C.c_char_p]
gr = capi.Context(0)
blocks, texels = capi.DeviceBuffer(gr, 4096), capi.DeviceBuffer(gr, 1 << 20)
def call(fmt, pitch, w, h, out_pitch, out_fmt, blocks_ptr=blocks.ptr, out_ptr=texels.ptr):
    before = stub.hip_stub_count(b"launches")
    code = gr.lib.gr_texture_decode(gr.handle, None, fmt, blocks_ptr, pitch, C.byref(capi.Image(out_ptr, w, h, out_pitch, out_fmt)))
    return [code, gr.lib.gr_last_error(gr.handle).decode() if code < 0 else "", stub.hip_stub_count(b"launches") - before]
rgba, srgb = capi.FORMAT_R8G8B8A8_UNORM, capi.FORMAT_R8G8B8A8_SRGB
out = {
    "ok_4x4": call(157, 64, 13, 7, 52, rgba),           # 4 x 2 blocks
    "ok_6x5_srgb": call(164, 48, 13, 7, 52, srgb),      # 3 x 2 blocks
    "ok_12x12_padded": call(183, 72, 25, 13, 128, rgba),  # 3 x 2 blocks, both pitches padded
    "ok_offset_by_one": call(157, 65, 13, 7, 53, rgba, blocks_ptr=blocks.ptr + 1, out_ptr=texels.ptr + 1),
    "srgb_into_unorm": call(158, 64, 13, 7, 52, rgba),
    "unorm_into_srgb": call(183, 48, 13, 7, 52, srgb),
    "into_rg8": call(157, 64, 13, 7, 26, capi.FORMAT_R8G8_UNORM),
    "block_pitch_small": call(163, 47, 13, 7, 52, rgba),  # three 6 x 5 blocks are 48 bytes
    "block_pitch_small_12x12": call(183, 47, 25, 13, 100, rgba),
    "out_pitch_small": call(157, 64, 13, 7, 51, rgba),
    "null_blocks": call(157, 64, 13, 7, 52, rgba, blocks_ptr=None),
    "null_out": call(157, 64, 13, 7, 52, rgba, out_ptr=None),
    "empty_width": call(157, 0, 0, 7, 0, rgba),
    "empty_height": call(183, 48, 13, 0, 52, rgba),
    "too_wide": call(183, 1 << 20, 65537, 4, 1 << 19, rgba),
    "too_high": call(157, 64, 4, 65537, 16, rgba),
    "sfloat": call(%(sfloat)d, 64, 13, 7, 52, rgba),
    "sfloat_into_fp16": call(%(sfloat)d, 64, 13, 7, 104, capi.FORMAT_R16G16B16A16_SFLOAT),
    "after_the_last": call(185, 64, 13, 7, 52, rgba),
    "etc2": call(147, 64, 13, 7, 52, rgba),
}
print(json.dumps(out))
'''


def test_astc_decode_launches_and_refusals_need_no_device():
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(os.path.join(os.path.dirname(STUB), "hip_stub.cpp")):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(STUB)])
    r = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT, "stub": STUB, "sfloat": ASTC_4x4_SFLOAT}], env=dict(os.environ, LD_PRELOAD=STUB),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ("ok_4x4", "ok_6x5_srgb", "ok_12x12_padded", "ok_offset_by_one"):
        assert out[key] == [0, "", 1], (key, out[key])  # exactly one launch
    for key in ("empty_width", "empty_height"):
        assert out[key] == [0, "", 0], (key, out[key])  # GR_OK without a launch
    INVALID, UNSUPPORTED = -1, -3
    for key, code, text in (("srgb_into_unorm", UNSUPPORTED, "decoded format"), ("unorm_into_srgb", UNSUPPORTED, "decoded format"),
                            ("into_rg8", UNSUPPORTED, "decoded format"), ("block_pitch_small", INVALID, "block row pitch"),
                            ("block_pitch_small_12x12", INVALID, "block row pitch"), ("out_pitch_small", INVALID, "output pitch"),
                            ("null_blocks", INVALID, "blocks"), ("null_out", INVALID, "out"), ("too_wide", INVALID, "larger than"),
                            ("too_high", INVALID, "larger than"), ("sfloat", UNSUPPORTED, "not a block format"),
                            ("sfloat_into_fp16", UNSUPPORTED, "not a block format"), ("after_the_last", UNSUPPORTED, "not a block format"),
                            ("etc2", UNSUPPORTED, "not a block format")):
        got = out[key]
        assert got[0] == code and text in got[1] and got[2] == 0, (key, got)
