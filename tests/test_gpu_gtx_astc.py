"""GPU: Application.decode_gtx (gra_gtx_decode) of an ASTC .gtx with a full mip chain and two layers, level by level and layer by layer
against tests/astc_ref.py; header fields and flags preserved."""
import numpy as np
import pytest

import astc_cases
import astc_ref
from granite_amd import app as gapp
from granite_amd import capi, gtx

pytestmark = pytest.mark.gpu


def test_decode_gtx_astc_6x5_mips_and_layers(tmp_path):
    rng = np.random.default_rng(65)
    bw, bh = 6, 5
    sizes = [(20, 12), (10, 6), (5, 3), (2, 1), (1, 1)]
    counts = [((w + bw - 1) // bw, (h + bh - 1) // bh) for w, h in sizes]
    levels = [astc_cases.valid_blocks(rng, bw, bh, 2 * bx * by).reshape(2, by, bx, 16) for bx, by in counts]
    src, dst = str(tmp_path / "astc.gtx"), str(tmp_path / "rgba.gtx")
    flags = 0x0688 << 16 | 1
    gtx.write(src, capi.FORMAT_ASTC_6x5_SRGB_BLOCK, levels, flags=flags, layers=2, size=sizes[0])
    a = gapp.Application(64, 64, lighting=False)
    a.decode_gtx(src, dst)
    a.close()
    f = gtx.read(dst)
    i = f.info
    assert (i.type, i.format, i.width, i.height, i.depth, i.layers, i.levels, i.flags) == (1, capi.FORMAT_R8G8B8A8_SRGB, 20, 12, 1, 2, 5, flags)
    for l, (w, h) in enumerate(sizes):
        got = f.level(l)
        assert got.shape == (2, h, w, 4)
        for layer in range(2):
            assert np.array_equal(got[layer], astc_ref.decode((bw, bh), levels[l][layer], w, h)), (l, layer)


def test_upload_gbuffer_gtx_takes_an_astc_albedo(tmp_path):
    """An ASTC 10 x 6 SRGB albedo whose footprint does not divide the frame, decoded into the attachment on the device, renders the same bytes
    as the same scene uploaded from the file decoded beforehand (astc_ref).  An ASTC file is refused where RGBA8 is not the attachment's format."""
    from granite_amd import synth
    w, h = 64, 32
    cam = synth.Camera(w, h)
    gbuf = synth.make_gbuffer(cam)
    descs = synth.make_lights(cam, 64)
    rng = np.random.default_rng(88)
    bx, by = (w + 9) // 10, (h + 5) // 6
    albedo_blocks = astc_cases.valid_blocks(rng, 10, 6, bx * by).reshape(by, bx, 16)
    albedo = astc_ref.decode((10, 6), albedo_blocks, w, h)
    formats = {"emissive": capi.FORMAT_R16G16B16A16_SFLOAT, "normal": capi.FORMAT_A2B10G10R10_UNORM_PACK32, "depth": capi.FORMAT_D32_SFLOAT,
               "pbr": capi.FORMAT_R8G8_UNORM}
    plain, packed = {}, {}
    for k, fmt in formats.items():
        plain[k] = packed[k] = str(tmp_path / f"{k}.gtx")
        gtx.write(plain[k], fmt, [np.ascontiguousarray(gbuf[k]).view(np.uint8).reshape(h, w, -1)])
    plain["albedo"], packed["albedo"] = str(tmp_path / "albedo.gtx"), str(tmp_path / "albedo_astc.gtx")
    gtx.write(plain["albedo"], capi.FORMAT_R8G8B8A8_SRGB, [albedo])
    gtx.write(packed["albedo"], capi.FORMAT_ASTC_10x6_SRGB_BLOCK, [albedo_blocks], size=(w, h))
    frames = []
    for paths in (plain, packed):
        a = gapp.Application(w, h, dynamic_exposure=False)  # a 64 x 32 frame leaves the luminance pass no texels
        a.set_render_parameters(cam.render_params())
        a.set_lights(descs)
        a.upload_gbuffer_gtx(**paths)
        a.render_frames(3)
        frames.append(a.read_backbuffer().copy())
        if paths is packed:
            with pytest.raises(capi.GraniteHipError, match="wrong format"):
                a.upload_gbuffer_gtx(pbr=packed["albedo"])
        a.close()
    assert frames[0].any()
    np.testing.assert_array_equal(frames[1], frames[0])
