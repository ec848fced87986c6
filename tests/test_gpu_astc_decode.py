"""GPU: gr_texture_decode of the ASTC LDR formats against the reference's decode shader executed on the CPU
(tests/golden/astc_decode_shader_v1.npz), byte for byte on every case: the decode is integer.  Sizes the golden does not hold are checked
against tests/astc_ref.py, itself held to the golden by tests/test_astc_ref_cpu.py.  Guard bytes around and between the rows must survive
every footprint, tail size, pitch and pointer alignment."""
import numpy as np
import pytest

import astc_cases
import astc_ref
from granite_amd import capi

pytestmark = pytest.mark.gpu
CASES = astc_cases.golden()
GUARD = 0xA5


@pytest.fixture(scope="module")
def gr():
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def decode(gr, fmt, blocks, w, h, out_pad=0, out_offset=0, block_offset=0, block_pad=0):
    """Decoded texels (h, w, 4) after checking that nothing but them was written."""
    bw, bh, nb, out_fmt = gr.texture_block_info(fmt)
    assert nb == 16 and out_fmt == (capi.FORMAT_R8G8B8A8_SRGB if (fmt - 157) & 1 else capi.FORMAT_R8G8B8A8_UNORM)
    bx, by = (w + bw - 1) // bw, (h + bh - 1) // bh
    block_pitch = bx * 16 + block_pad
    src = np.full(block_offset + by * block_pitch + 32, 0x5A, np.uint8)
    rows = src[block_offset:block_offset + by * block_pitch].reshape(by, block_pitch)
    rows[:, :bx * 16] = np.ascontiguousarray(blocks, np.uint8).reshape(by, bx * 16)
    pitch = w * 4 + out_pad
    total = 64 + out_offset + h * pitch + 64
    dsrc, dout = capi.DeviceBuffer(gr, src.size).upload(src), capi.DeviceBuffer(gr, total).upload(np.full(total, GUARD, np.uint8))
    gr.texture_decode(fmt, dsrc.ptr + block_offset, block_pitch, capi.Image(dout.ptr + 64 + out_offset, w, h, pitch, out_fmt))
    gr.sync()
    raw = dout.download()
    body = raw[64 + out_offset:64 + out_offset + h * pitch].reshape(h, pitch)
    assert (raw[:64 + out_offset] == GUARD).all() and (raw[64 + out_offset + h * pitch:] == GUARD).all(), "bytes outside the image were written"
    assert (body[:, w * 4:] == GUARD).all(), "pitch padding was written"
    dsrc.free()
    dout.free()
    return np.ascontiguousarray(body[:, :w * 4]).reshape(h, w, 4)


@pytest.mark.parametrize("footprint", astc_ref.FOOTPRINTS, ids=lambda f: f"{f[0]}x{f[1]}")
def test_every_golden_case_matches_the_executed_shader(gr, footprint):
    names = [n for n, c in CASES.items() if astc_ref.format_footprint(c[0]) == footprint]
    assert len(names) >= 6
    for name in names:
        fmt, w, h, blocks, out = CASES[name]
        got = decode(gr, fmt, blocks, w, h)
        assert np.array_equal(got, out), (name, int((got != out).any(-1).sum()))


@pytest.mark.parametrize("footprint", astc_ref.FOOTPRINTS, ids=lambda f: f"{f[0]}x{f[1]}")
def test_srgb_formats_give_the_unorm_bytes(gr, footprint):
    bw, bh = footprint
    fmt, w, h, blocks, out = CASES[f"f{bw}x{bh}_tail_{2 * bw + 1}x{bh + 2}"]
    assert fmt == astc_cases.astc_format(bw, bh) and gr.texture_block_info(fmt + 1)[3] == capi.FORMAT_R8G8B8A8_SRGB
    assert np.array_equal(decode(gr, fmt + 1, blocks, w, h), out)


@pytest.mark.parametrize("footprint", [(4, 4), (5, 5), (8, 6), (10, 10), (12, 12)], ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("layout", ["tight", "pitch+12", "offset4", "offset1", "block_pitch"])
def test_guard_bytes_and_odd_layouts(gr, footprint, layout):
    bw, bh = footprint
    kw = {"tight": {}, "pitch+12": {"out_pad": 12}, "offset4": {"out_offset": 4, "block_offset": 4}, "offset1": {"out_offset": 1, "block_offset": 1},
          "block_pitch": {"block_pad": 40}}[layout]
    for w, h in astc_cases.tail_sizes(bw, bh):
        fmt, _, _, blocks, out = CASES[f"f{bw}x{bh}_tail_{w}x{h}"]
        assert np.array_equal(decode(gr, fmt, blocks, w, h, **kw), out), (footprint, layout, w, h)


@pytest.mark.parametrize("footprint,w,h", [((4, 4), 1030, 9), ((8, 8), 1030, 17), ((12, 10), 1550, 21)])
def test_sizes_of_more_than_one_wave_per_row(gr, footprint, w, h):
    bw, bh = footprint
    bx, by = (w + bw - 1) // bw, (h + bh - 1) // bh
    assert bx > 64  # a wave takes 64 blocks of a row
    rng = np.random.default_rng(w)
    blocks = astc_cases.valid_blocks(rng, bw, bh, bx * by)
    blocks[rng.integers(0, bx * by, 24)] = rng.integers(0, 256, (24, 16), dtype=np.uint8)  # and some that are most likely illegal
    ref = astc_ref.decode(footprint, blocks, w, h)
    assert astc_cases.blocks_with_error(ref, bw, bh).mean() < 0.25
    fmt = astc_cases.astc_format(bw, bh)
    assert np.array_equal(decode(gr, fmt, blocks, w, h), ref)
    assert np.array_equal(decode(gr, fmt, blocks, w, h, out_pad=12), ref)
