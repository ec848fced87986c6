"""Device-side copies of a tests/sky_cases.py case and the two sky launches on them (tests/test_gpu_sky.py, tools/sky_time.py)."""
import ctypes as C

import numpy as np

from granite_amd import capi

GUARD = 0xA5
TAIL_BYTES = 256


def ufloat_codes(values, mant_bits):
    """fp32 -> the code of the unsigned float with `mant_bits` mantissa bits and a half's exponent (csrc/packed_float.hpp: float_to_ufloat):
    nearest, ties to even, the closest finite value above the range, 0 for negatives.  Codes of non-negative values are monotonic."""
    v = np.ascontiguousarray(values, np.float32)
    a = v.view(np.uint32) & np.uint32(0x7fffffff)
    shift = 23 - mant_bits
    normal = ((a.astype(np.uint64) + ((1 << (shift - 1)) - 1) + ((a >> shift) & 1)) >> shift).astype(np.int64) - (112 << mant_bits)
    small = np.rint(np.where(a < 0x38800000, np.abs(v), 0).astype(np.float64) * float(1 << (14 + mant_bits))).astype(np.int64)
    q = np.where(a < 0x38800000, small, normal)
    q = np.minimum(q, (31 << mant_bits) - 1)
    assert np.isfinite(v).all()
    return np.where(np.signbit(v), 0, q).astype(np.int64)


def unpack_codes(words):
    words = np.asarray(words, np.uint32)
    return np.stack([words & 0x7ff, (words >> 11) & 0x7ff, words >> 22], -1).astype(np.int64)


class PaddedImage:
    """An image whose rows are `pad` bytes further apart than they need to be, with guard bytes in every gap and behind the last row."""

    def __init__(self, gr, width, height, fmt, pad):
        self.width, self.height, self.format = width, height, fmt
        self.row = width * capi.FORMAT_BPP[fmt]
        self.pitch = self.row + pad
        self.buffer = capi.DeviceBuffer(gr, self.pitch * height + TAIL_BYTES)
        self.desc = capi.Image(self.buffer.ptr, width, height, self.pitch, fmt)

    def upload(self, array):
        raw = np.full(self.buffer.nbytes, GUARD, np.uint8)
        rows = raw[:self.pitch * self.height].reshape(self.height, self.pitch)
        rows[:, :self.row] = np.ascontiguousarray(array).view(np.uint8).reshape(self.height, self.row)
        self.buffer.upload(raw)
        return self

    def download(self):
        """-> (texel bytes (height, row), guard bytes)"""
        raw = self.buffer.download(np.uint8)
        rows = raw[:self.pitch * self.height].reshape(self.height, self.pitch)
        return rows[:, :self.row].copy(), np.concatenate([rows[:, self.row:].reshape(-1), raw[self.pitch * self.height:]])


def emissive_input(rng, width, height, fmt):
    """What the caller uploaded as emissive: finite fp16 colours with an alpha of their own, or packed words."""
    if fmt == capi.FORMAT_R16G16B16A16_SFLOAT:
        return rng.uniform(0.0, 4.0, (height, width, 4)).astype(np.float16).view(np.uint16)
    return rng.integers(0, 1 << 32, (height, width), dtype=np.uint64).astype(np.uint32)


def sky_args(emissive, depth, case, cube=None):
    a = capi.SkyArgs()
    a.emissive, a.depth = emissive.desc, depth.desc
    a.inv_local_view_projection[:] = [float(v) for v in case["inv"]]
    a.color[:] = [float(v) for v in case["color"]]
    a.camera_height = float(case["camera_height"])
    a.sun_direction[:] = [float(v) for v in case["sun_direction"]]
    if cube is not None:
        a.cube = capi.Cube(cube.ptr, case["cube_size"], case["cube_levels"])
    return a


def apply(gr, case, fmt, uploaded, pad=(0, 0), depth_values=None):
    """gr_sky_apply on fresh copies -> (emissive texel bytes (height, row bytes), guard bytes of both images, the depth bytes afterwards)"""
    w, h = case["width"], case["height"]
    emissive = PaddedImage(gr, w, h, fmt, pad[0]).upload(uploaded)
    depth = PaddedImage(gr, w, h, capi.FORMAT_D32_SFLOAT, pad[1]).upload(np.ascontiguousarray(case["depth"] if depth_values is None else depth_values, np.float32))
    cube = capi.DeviceBuffer(gr, case["cube"].nbytes).upload(case["cube"]) if "cube" in case else None
    args = sky_args(emissive, depth, case, cube)
    gr.check(gr.lib.gr_sky_apply(gr.handle, None, C.byref(args)))
    gr.sync()
    texels, guard = emissive.download()
    depth_after, depth_guard = depth.download()
    return texels, np.concatenate([guard, depth_guard]), depth_after
