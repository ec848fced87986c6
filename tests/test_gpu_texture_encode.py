"""GPU: gr_texture_encode and gr_texture_generate_mipmap against the reference's own compressor and mip filter run on the CPU
(tests/golden/texture_encode_v1.npz): every encode case and every mip case byte for byte, no tolerance anywhere.  One case of each again
from an odd byte offset, from a padded pitch, and into a buffer of guard bytes with a wider pitch, of which every byte outside the written
blocks or texels must survive.  Then Application.encode_gtx: a 13 x 6 RG8 file to BC5 with a mip chain, decoded back by decode_gtx, and
taken as the pbr attachment."""
import numpy as np
import pytest

import texture_encode_cases as tc
from granite_amd import app as gapp
from granite_amd import capi, gtx

pytestmark = pytest.mark.gpu
GOLDEN = tc.load_golden()
ENCODE = [(name, fmt) for name, case in tc.ENCODE_CASES.items() for fmt in case[3]]
GUARD = 0xA5


@pytest.fixture(scope="module")
def gr():
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def upload_image(gr, image, fmt, offset=0, pad=0):
    """(buffer, Image) of an (h, w, c) uint8 image `offset` bytes into a buffer, rows `pad` bytes apart beyond their own."""
    h, w, c = image.shape
    pitch = w * c + pad
    raw = np.full(offset + h * pitch + 16, 0x5A, np.uint8)
    rows = raw[offset:offset + h * pitch].reshape(h, pitch)
    rows[:, :w * c] = image.reshape(h, w * c)
    buf = capi.DeviceBuffer(gr, raw.size).upload(raw)
    return buf, capi.Image(buf.ptr + offset, w, h, pitch, fmt)


def guarded_rows(gr, rows, row_bytes, pad, run):
    """`rows` x `row_bytes` written by run(pointer, pitch) inside a buffer of guard bytes; everything else must still be the guard."""
    pitch = row_bytes + pad
    total = 64 + rows * pitch + 64
    out = capi.DeviceBuffer(gr, total).upload(np.full(total, GUARD, np.uint8))
    run(out.ptr + 64, pitch)
    gr.sync()
    raw = out.download()
    out.free()
    body = raw[64:64 + rows * pitch].reshape(rows, pitch)
    assert (raw[:64] == GUARD).all() and (raw[64 + rows * pitch:] == GUARD).all(), "bytes outside the output were written"
    assert (body[:, row_bytes:] == GUARD).all(), "bytes between the rows were written"
    return np.ascontiguousarray(body[:, :row_bytes])


def encode(gr, image, in_fmt, fmt, offset=0, pad=0, block_pad=0):
    h, w, _ = image.shape
    by, bx = (h + 3) // 4, (w + 3) // 4
    src, desc = upload_image(gr, image, in_fmt, offset, pad)
    got = guarded_rows(gr, by, bx * tc.BLOCK_BYTES[fmt], block_pad, lambda ptr, pitch: gr.texture_encode(fmt, desc, ptr, pitch))
    src.free()
    return got.reshape(by, bx, tc.BLOCK_BYTES[fmt])


def mip_level(gr, above, fmt, offset=0, pad=0, out_pad=0):
    """The next level of one (h, w, c) layer."""
    h, w, c = above.shape
    dh, dw = tc.level_extent(h, 1), tc.level_extent(w, 1)
    src, desc = upload_image(gr, above, fmt, offset, pad)
    got = guarded_rows(gr, dh, dw * c, out_pad,
                       lambda ptr, pitch: gr.texture_generate_mipmap(desc, capi.Image(ptr, dw, dh, pitch, fmt)))
    src.free()
    return got.reshape(dh, dw, c)


@pytest.mark.parametrize("name,fmt", ENCODE)
def test_every_encode_case_matches_the_reference(gr, name, fmt):
    got = encode(gr, GOLDEN[f"enc/{name}/input"], tc.ENCODE_CASES[name][2], fmt)
    want = GOLDEN[f"enc/{name}/{fmt}/blocks"]
    assert np.array_equal(got, want), (name, int((got != want).any(axis=2).sum()), "blocks differ")


@pytest.mark.parametrize("name", tc.MIP_CASES)
def test_every_mip_case_matches_the_reference(gr, name):
    fmt, w, h, layers, levels = tc.MIP_CASES[name]
    payload = GOLDEN[f"mip/{name}/payload"]
    assert np.array_equal(tc.chain_level(payload, fmt, w, h, layers, levels, 0), GOLDEN[f"mip/{name}/level0"])
    for level in range(1, levels):
        above, below = (tc.chain_level(payload, fmt, w, h, layers, levels, l) for l in (level - 1, level))
        for layer in range(layers):
            assert np.array_equal(mip_level(gr, above[layer], fmt), below[layer]), (name, level, layer)


@pytest.mark.parametrize("layout", ["offset1", "pitch+7", "block_pitch+2"])
def test_encode_from_and_into_odd_layouts(gr, layout):
    kw = {"offset1": {"offset": 1}, "pitch+7": {"pad": 7}, "block_pitch+2": {"block_pad": 2 * 16}}[layout]
    got = encode(gr, GOLDEN["enc/edge_rg8/input"], tc.RG8, tc.BC5, **kw)
    assert np.array_equal(got, GOLDEN[f"enc/edge_rg8/{tc.BC5}/blocks"])


@pytest.mark.parametrize("layout", ["offset1", "pitch+7", "out_pitch+5"])
def test_mip_from_and_into_odd_layouts(gr, layout):
    kw = {"offset1": {"offset": 1}, "pitch+7": {"pad": 7}, "out_pitch+5": {"out_pad": 5}}[layout]
    fmt, w, h, layers, levels = tc.MIP_CASES["rgba8_7x13"]
    payload = GOLDEN["mip/rgba8_7x13/payload"]
    above, below = (tc.chain_level(payload, fmt, w, h, layers, levels, l)[0] for l in (0, 1))
    assert np.array_equal(mip_level(gr, above, fmt, **kw), below)


def test_encode_gtx_with_mips_decodes_back_and_is_taken_as_pbr(tmp_path):
    w, h, _, _ = tc.ENCODE_CASES["edge_rg8"]
    src, packed, back = (str(tmp_path / n) for n in ("rg8.gtx", "bc5.gtx", "back.gtx"))
    flags = 0x0688 << 16 | 2  # a swizzle, and the mipgen-on-load bit that generate_mipmaps clears
    gtx.write(src, tc.RG8, [GOLDEN["enc/edge_rg8/input"]], flags=flags)
    a = gapp.Application(w, h, dynamic_exposure=False)
    a.encode_gtx(src, packed, "bc5_unorm", mipgen=True)
    f = gtx.read(packed)
    i = f.info
    assert (i.type, i.format, i.width, i.height, i.depth, i.layers, i.levels, i.flags) == (1, tc.BC5, w, h, 1, 1, tc.GTX_LEVELS, 0x0688 << 16)
    for level in range(tc.GTX_LEVELS):
        assert np.array_equal(f.level(level)[0], GOLDEN[f"gtx/{level}/blocks"]), level
    a.decode_gtx(packed, back)
    f = gtx.read(back)
    i = f.info
    assert (i.type, i.format, i.width, i.height, i.depth, i.layers, i.levels, i.flags) == (1, tc.RG8, w, h, 1, 1, tc.GTX_LEVELS, 0x0688 << 16)
    for level in range(tc.GTX_LEVELS):
        lw, lh = tc.level_extent(w, level), tc.level_extent(h, level)
        assert np.array_equal(f.level(level)[0], GOLDEN[f"gtx/{level}/decoded"][:lh, :lw]), level
    # the chain alone, as a copy to the input's own format
    chain = str(tmp_path / "chain.gtx")
    a.encode_gtx(src, chain, "rg8_unorm", mipgen=True)
    assert np.array_equal(gtx.read(chain).payload, GOLDEN["gtx/chain"])
    a.upload_gbuffer_gtx(pbr=packed)
    with pytest.raises(capi.GraniteHipError, match="cannot be compressed"):
        a.encode_gtx(back, str(tmp_path / "no.gtx"), 145)  # BC7 is not encoded here
    a.close()
