"""GPU: gr_texture_decode against the reference's decode shaders executed on the CPU (tests/golden/bc_decode_shader_v1.npz) on every
forced branch: BC7 and BC6H byte-identical; BC1-BC5 identical outside tests/bc_ref.py's tie mask and within one code inside it.  Sizes the
golden does not hold are checked against bc_ref.py, itself held to the golden by tests/test_bc_ref_cpu.py.  Guard bytes around and
between the rows must survive every shape, pitch and pointer alignment."""
import numpy as np
import pytest

import bc_cases
import bc_ref
from granite_amd import capi

pytestmark = pytest.mark.gpu
CASES = bc_cases.golden()
TEXEL_BYTES = {capi.FORMAT_R8_UNORM: 1, capi.FORMAT_R8G8_UNORM: 2, capi.FORMAT_R8G8B8A8_UNORM: 4, capi.FORMAT_R8G8B8A8_SRGB: 4, capi.FORMAT_R16G16B16A16_SFLOAT: 8}
GUARD = 0xA5


@pytest.fixture(scope="module")
def gr():
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def decode(gr, fmt, blocks, w, h, out_pad=0, out_offset=0, block_offset=0, block_pad=0):
    """Decoded bytes (h, w * texel bytes) after checking that nothing but them was written."""
    out_fmt = gr.lib.gr_texture_decoded_format(fmt)
    tb, nb = TEXEL_BYTES[out_fmt], bc_ref.BLOCK_BYTES[fmt]
    bw, bh = (w + 3) // 4, (h + 3) // 4
    block_pitch = bw * nb + block_pad
    src = np.full(block_offset + bh * block_pitch + 32, 0x5A, np.uint8)
    rows = src[block_offset:block_offset + bh * block_pitch].reshape(bh, block_pitch)
    rows[:, :bw * nb] = np.ascontiguousarray(blocks, np.uint8).reshape(bh, bw * nb)
    pitch = w * tb + out_pad
    total = 64 + out_offset + h * pitch + 64
    dsrc, dout = capi.DeviceBuffer(gr, src.size).upload(src), capi.DeviceBuffer(gr, total).upload(np.full(total, GUARD, np.uint8))
    gr.texture_decode(fmt, dsrc.ptr + block_offset, block_pitch, capi.Image(dout.ptr + 64 + out_offset, w, h, pitch, out_fmt))
    gr.sync()
    raw = dout.download()
    body = raw[64 + out_offset:64 + out_offset + h * pitch].reshape(h, pitch)
    assert (raw[:64 + out_offset] == GUARD).all() and (raw[64 + out_offset + h * pitch:] == GUARD).all(), "bytes outside the image were written"
    assert (body[:, w * tb:] == GUARD).all(), "pitch padding was written"
    dsrc.free()
    dout.free()
    return np.ascontiguousarray(body[:, :w * tb])


def check(got, ref, ties, what):
    got = got.view(ref.dtype).reshape(ref.shape)
    diff = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    assert not diff[~ties].any(), (what, int((diff[~ties] > 0).sum()))
    assert diff.max(initial=0) <= 1, what


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_golden_case_matches_the_executed_shaders(gr, name):
    fmt, w, h, blocks, out = CASES[name]
    _, ties = bc_cases.reference(name)
    if fmt in (bc_ref.BC6H_UFLOAT, bc_ref.BC6H_SFLOAT, bc_ref.BC7_UNORM):
        assert not ties.any()
    check(decode(gr, fmt, blocks, w, h), out, ties, name)


@pytest.mark.parametrize("unorm,srgb,name", [(131, 132, "bc1_rgb_random"), (133, 134, "bc1_rgba_random"), (135, 136, "bc2_random"),
                                             (137, 138, "bc3_random"), (145, 146, "bc7_modes")])
def test_srgb_formats_give_the_unorm_bytes(gr, unorm, srgb, name):
    _, w, h, blocks, _ = CASES[name]
    assert gr.lib.gr_texture_decoded_format(srgb) == capi.FORMAT_R8G8B8A8_SRGB
    assert np.array_equal(decode(gr, unorm, blocks, w, h), decode(gr, srgb, blocks, w, h))


@pytest.mark.parametrize("fmt", [bc_ref.BC1_RGBA_UNORM, bc_ref.BC3_UNORM, bc_ref.BC4_UNORM, bc_ref.BC5_UNORM, bc_ref.BC6H_SFLOAT, bc_ref.BC7_UNORM])
@pytest.mark.parametrize("layout", ["tight", "pitch+12", "offset4", "offset1", "block_pitch"])
def test_guard_bytes_and_odd_layouts(gr, fmt, layout):
    rng = np.random.default_rng(fmt)
    kw = {"tight": {}, "pitch+12": {"out_pad": 12}, "offset4": {"out_offset": 4, "block_offset": 4}, "offset1": {"out_offset": 1, "block_offset": 1},
          "block_pitch": {"block_pad": 40}}[layout]
    for w, h in bc_cases.TAIL_SIZES:
        bw, bh = (w + 3) // 4, (h + 3) // 4
        blocks = rng.integers(0, 256, (bh, bw, bc_ref.BLOCK_BYTES[fmt]), dtype=np.uint8)
        ref, ties = bc_ref.decode(fmt, blocks, w, h)
        check(decode(gr, fmt, blocks, w, h, **kw), ref, ties, (fmt, layout, w, h))


@pytest.mark.parametrize("fmt,w,h", [(bc_ref.BC7_UNORM, 67, 35), (bc_ref.BC1_RGBA_UNORM, 130, 66), (bc_ref.BC6H_UFLOAT, 260, 9)])
def test_sizes_of_more_than_one_wave_per_row(gr, fmt, w, h):
    rng = np.random.default_rng(w)
    blocks = rng.integers(0, 256, ((h + 3) // 4, (w + 3) // 4, bc_ref.BLOCK_BYTES[fmt]), dtype=np.uint8)
    ref, ties = bc_ref.decode(fmt, blocks, w, h)
    check(decode(gr, fmt, blocks, w, h), ref, ties, (fmt, w, h))
    check(decode(gr, fmt, blocks, w, h, out_pad=12), ref, ties, (fmt, w, h, "padded"))
