"""GTX ("GRANITE TEXFMT1") files through the host library's C ABI (gra_gtx_*): the container Granite keeps textures and
image dumps in (vulkan/texture/memory_mapped_texture.cpp:29-44; payload layout vulkan/texture/texture_format.cpp:349-387)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List

import numpy as np

from . import app as gapp
from . import capi

HEADER_SIZE = 64


class GtxInfo(C.Structure):
    _fields_ = [("type", C.c_uint32), ("format", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("depth", C.c_uint32), ("layers", C.c_uint32), ("levels", C.c_uint32), ("flags", C.c_uint32),
                ("payload_size", C.c_uint64)]


class GtxError(RuntimeError):
    pass


@dataclass
class GtxFile:
    info: GtxInfo
    payload: np.ndarray  # uint8

    def level_offset(self, level: int) -> int:
        return level_offset(self.info, level)

    def level(self, level: int = 0) -> np.ndarray:
        """Raw bytes of one mip level (all layers), shaped (layers, height, width, bytes per texel); for a block-compressed format
        the raw blocks, shaped (layers, rows of blocks, blocks per row, bytes per block)."""
        bx, by, bpp = level_blocks(self.info, level)
        o = self.level_offset(level)
        return self.payload[o:o + self.info.layers * bx * by * bpp].reshape(self.info.layers, by, bx, bpp)


def block_bytes(fmt: int) -> int:
    """Bytes per texel, or per block of a BC or ASTC format."""
    if fmt in capi.ASTC_FORMATS:
        return 16
    return capi.load_library().gr_texture_block_bytes(fmt) or capi.FORMAT_BPP[fmt]


def block_dim(fmt: int):
    """(width, height) of a block in texels: 4 x 4 for BC, the footprint for ASTC, 1 x 1 otherwise."""
    return capi.ASTC_FORMATS.get(fmt, (4, 4) if fmt in capi.BLOCK_FORMATS else (1, 1))


def level_blocks(info: GtxInfo, level: int):
    """(blocks per row, rows of blocks, bytes per block) of a level; a block is one texel unless the format is block-compressed."""
    bw, bh = block_dim(info.format)
    w, h = max(info.width >> level, 1), max(info.height >> level, 1)
    return (w + bw - 1) // bw, (h + bh - 1) // bh, block_bytes(info.format)


def level_size(info: GtxInfo, level: int) -> int:
    bx, by, bpp = level_blocks(info, level)
    return bx * by * max(info.depth >> level, 1) * info.layers * bpp


def level_offset(info: GtxInfo, level: int) -> int:
    offset = 0
    for l in range(level + 1):
        offset = (offset + 15) & ~15
        if l == level:
            return offset
        offset += level_size(info, l)
    return offset


def payload_size(info: GtxInfo) -> int:
    last = info.levels - 1
    return level_offset(info, last) + level_size(info, last)


def _lib():
    lib = gapp.load_library()
    return lib


def probe(path: str) -> GtxInfo:
    info = GtxInfo()
    err = C.create_string_buffer(512)
    if _lib().gra_gtx_probe(path.encode(), C.byref(info), err, len(err)) < 0:
        raise GtxError(err.value.decode())
    return info


def read(path: str) -> GtxFile:
    info = probe(path)
    payload = np.empty(info.payload_size, np.uint8)
    err = C.create_string_buffer(512)
    if _lib().gra_gtx_read(path.encode(), payload.ctypes.data, payload.nbytes, err, len(err)) < 0:
        raise GtxError(err.value.decode())
    return GtxFile(info, payload)


def write(path: str, fmt: int, levels: List[np.ndarray], flags: int = 0, layers: int = 1, size=None):
    """levels[l]: array whose bytes are level l (all layers), level 0 first; shape[-3:-1] or [0:2] of level 0 gives h, w.
    A block-compressed format takes raw blocks and needs size = (width, height) in texels."""
    first = np.ascontiguousarray(levels[0])
    if (fmt in capi.BLOCK_FORMATS or fmt in capi.ASTC_FORMATS) and size is None:
        raise GtxError("a block-compressed format needs size=(width, height)")
    h, w = (size[1], size[0]) if size is not None else (first.shape[1], first.shape[2]) if layers > 1 else (first.shape[0], first.shape[1])
    info = GtxInfo(1, fmt, w, h, 1, layers, len(levels), flags, 0)
    info.payload_size = payload_size(info)
    payload = np.zeros(info.payload_size, np.uint8)
    for l, a in enumerate(levels):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        want = level_size(info, l)
        if raw.size != want:
            raise GtxError(f"level {l}: {raw.size} bytes, layout wants {want}")
        o = level_offset(info, l)
        payload[o:o + raw.size] = raw
    err = C.create_string_buffer(512)
    if _lib().gra_gtx_write(path.encode(), C.byref(info), payload.ctypes.data, err, len(err)) < 0:
        raise GtxError(err.value.decode())


def encode_layout(info: GtxInfo, fmt: int, mipgen: bool = False):
    """(GtxInfo, [level offsets]) of what Application.encode_gtx writes for an image described by `info` (gra_gtx_encode_layout; no device)."""
    out = GtxInfo()
    offsets = (C.c_uint64 * 32)()
    err = C.create_string_buffer(512)
    if _lib().gra_gtx_encode_layout(C.byref(info), int(fmt), int(bool(mipgen)), C.byref(out), offsets, len(offsets), err, len(err)) < 0:
        raise GtxError(err.value.decode())
    return out, [int(o) for o in offsets[:out.levels]]
