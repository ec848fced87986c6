"""CPU: ASTC .gtx files through the writer and both readers: footprints other than 4 x 4 in the level layout (blocks per level,
16-byte aligned level offsets, the mip tail where every level is one block), the C++ reader (gra_gtx_probe / gra_gtx_read, which check
the payload size against Granite::GtxImage's own layout) and granite_amd/gtx.py agreeing on it."""
import os

import numpy as np
import pytest

from granite_amd import capi, gtx


def _chain(w, h):
    sizes = [(w, h)]
    while sizes[-1] != (1, 1):
        sizes.append((max(sizes[-1][0] >> 1, 1), max(sizes[-1][1] >> 1, 1)))
    return sizes


@pytest.mark.parametrize("fmt,size,blocks,offsets,total", [
    # 6 x 5, 20 x 12 with its full chain 20x12, 10x6, 5x3, 2x1, 1x1 -> 4x3, 2x2, 1x1, 1x1, 1x1 blocks, two layers, 16 bytes a block
    (capi.FORMAT_ASTC_6x5_UNORM_BLOCK, (20, 12), [(4, 3), (2, 2), (1, 1), (1, 1), (1, 1)], [0, 384, 512, 544, 576], 608),
    # 12 x 12, 30 x 25: 30x25, 15x12, 7x6, 3x3, 1x1 -> 3x3, 2x1, 1x1, 1x1, 1x1 blocks
    (capi.FORMAT_ASTC_12x12_SRGB_BLOCK, (30, 25), [(3, 3), (2, 1), (1, 1), (1, 1), (1, 1)], [0, 288, 352, 384, 416], 448),
])
def test_astc_gtx_round_trip_and_hand_computed_layout(tmp_path, fmt, size, blocks, offsets, total):
    rng = np.random.default_rng(fmt)
    sizes = _chain(*size)
    assert len(sizes) == len(blocks)
    bw, bh = gtx.block_dim(fmt)
    assert (bw, bh) == capi.ASTC_FORMATS[fmt] and gtx.block_bytes(fmt) == 16
    levels = [rng.integers(0, 256, (2, by, bx, 16), dtype=np.uint8) for bx, by in blocks]
    path = str(tmp_path / "astc.gtx")
    flags = 0x0688 << 16
    gtx.write(path, fmt, levels, flags=flags, layers=2, size=size)
    assert os.path.getsize(path) == 64 + total
    info = gtx.probe(path)  # the C++ reader's view of the header; it refuses a payload size that is not its own layout's
    assert (info.type, info.format, info.width, info.height, info.depth, info.layers, info.levels, info.flags, info.payload_size) == \
        (1, fmt, size[0], size[1], 1, 2, len(levels), flags, total)
    f = gtx.read(path)
    assert [f.level_offset(l) for l in range(len(levels))] == offsets and gtx.payload_size(f.info) == total
    for l, (bx, by) in enumerate(blocks):
        w, h = sizes[l]
        assert gtx.level_blocks(f.info, l) == ((w + bw - 1) // bw, (h + bh - 1) // bh, 16) == (bx, by, 16)
        assert f.level(l).shape == (2, by, bx, 16) and np.array_equal(f.level(l), levels[l]), l
    # one byte short of the layout, and the texel-sized payload of an uncompressed image: refused by the C++ reader
    raw = open(path, "rb").read()
    short = str(tmp_path / "short.gtx")
    open(short, "wb").write(raw[:-1])
    with pytest.raises(gtx.GtxError, match="truncated"):
        gtx.read(short)
    wrong = bytearray(raw)
    wrong[48:56] = (total + 16).to_bytes(8, "little")
    open(short, "wb").write(bytes(wrong) + bytes(16))
    with pytest.raises(gtx.GtxError, match="payload size"):
        gtx.read(short)


def test_a_block_compressed_write_needs_its_size(tmp_path):
    with pytest.raises(gtx.GtxError, match="size"):
        gtx.write(str(tmp_path / "x.gtx"), capi.FORMAT_ASTC_8x8_UNORM_BLOCK, [np.zeros((1, 1, 16), np.uint8)])


@pytest.mark.parametrize("fmt", [185, 1000066000])
def test_formats_next_to_astc_ldr_stay_refused(tmp_path, fmt):
    path = str(tmp_path / "x.gtx")
    gtx.write(path, capi.FORMAT_ASTC_4x4_UNORM_BLOCK, [np.zeros((1, 1, 16), np.uint8)], size=(4, 4))
    raw = bytearray(open(path, "rb").read())
    raw[20:24] = fmt.to_bytes(4, "little")
    open(path, "wb").write(raw)
    with pytest.raises(gtx.GtxError, match="format"):
        gtx.probe(path)
