"""GPU: Application.decode_gtx -- a block-compressed .gtx with mip levels and layers decoded on the device, level by level and layer by
layer, against tests/bc_ref.py; header fields and flags preserved; what is not block-compressed is refused."""
import numpy as np
import pytest

import bc_ref
from granite_amd import app as gapp
from granite_amd import capi, gtx

pytestmark = pytest.mark.gpu


def test_decode_gtx_bc3_mips_and_layers(tmp_path):
    rng = np.random.default_rng(11)
    sizes = [(32, 16), (16, 8), (8, 4), (4, 2)]
    levels = [rng.integers(0, 256, (2, (h + 3) // 4, (w + 3) // 4, 16), dtype=np.uint8) for w, h in sizes]
    src, dst = str(tmp_path / "bc3.gtx"), str(tmp_path / "rgba.gtx")
    flags = 0x0688 << 16 | 1
    gtx.write(src, capi.FORMAT_BC3_SRGB_BLOCK, levels, flags=flags, layers=2, size=sizes[0])
    a = gapp.Application(64, 64, lighting=False)
    a.decode_gtx(src, dst)
    f = gtx.read(dst)
    i = f.info
    assert (i.type, i.format, i.width, i.height, i.depth, i.layers, i.levels, i.flags) == (1, capi.FORMAT_R8G8B8A8_SRGB, 32, 16, 1, 2, 4, flags)
    for l, (w, h) in enumerate(sizes):
        got = f.level(l)
        assert got.shape == (2, h, w, 4)
        for layer in range(2):
            ref, ties = bc_ref.decode(bc_ref.BC3_SRGB, levels[l][layer], w, h)
            assert not ties.any() and np.array_equal(got[layer], ref), (l, layer)
    # an uncompressed file is not a compressed format
    with pytest.raises(capi.GraniteHipError, match="Not a compressed format"):
        a.decode_gtx(dst, str(tmp_path / "again.gtx"))
    a.close()


def test_decode_gtx_bc6h_and_bc4(tmp_path):
    rng = np.random.default_rng(12)
    a = gapp.Application(64, 64, lighting=False)
    for fmt, nbytes, decoded in ((capi.FORMAT_BC6H_UFLOAT_BLOCK, 16, capi.FORMAT_R16G16B16A16_SFLOAT), (capi.FORMAT_BC4_UNORM_BLOCK, 8, capi.FORMAT_R8_UNORM)):
        blocks = rng.integers(0, 256, (2, 4, nbytes), dtype=np.uint8)  # 13 x 7
        src, dst = str(tmp_path / "in.gtx"), str(tmp_path / "out.gtx")
        gtx.write(src, fmt, [blocks], size=(13, 7))
        a.decode_gtx(src, dst)
        f = gtx.read(dst)
        assert f.info.format == decoded
        ref, _ = bc_ref.decode(fmt, blocks, 13, 7)
        assert np.array_equal(f.level(0)[0].reshape(-1).view(ref.dtype).reshape(ref.shape), ref)
    a.close()


def test_upload_gbuffer_gtx_takes_bc7_albedo_and_bc5_pbr(tmp_path):
    """A BC7_SRGB albedo and a BC5 pbr, decoded into the attachments on the device, render the same bytes as the same scene uploaded from
    the files decoded beforehand (bc_ref; BC7 and BC5 have no tie samples).  A BC4 albedo is refused."""
    from granite_amd import synth
    w, h = 64, 32
    cam = synth.Camera(w, h)
    gbuf = synth.make_gbuffer(cam)
    descs = synth.make_lights(cam, 64)
    rng = np.random.default_rng(21)
    albedo_blocks = rng.integers(0, 256, (h // 4, w // 4, 16), dtype=np.uint8)
    albedo_blocks[..., 0] |= 0x40  # every block a defined BC7 mode
    pbr_blocks = rng.integers(0, 256, (h // 4, w // 4, 16), dtype=np.uint8)
    albedo, ties_a = bc_ref.decode(bc_ref.BC7_SRGB, albedo_blocks, w, h)
    pbr, ties_p = bc_ref.decode(bc_ref.BC5_UNORM, pbr_blocks, w, h)
    assert not ties_a.any() and not ties_p.any()
    formats = {"emissive": capi.FORMAT_R16G16B16A16_SFLOAT, "normal": capi.FORMAT_A2B10G10R10_UNORM_PACK32, "depth": capi.FORMAT_D32_SFLOAT}
    plain, packed = {}, {}
    for k, fmt in formats.items():
        plain[k] = packed[k] = str(tmp_path / f"{k}.gtx")
        gtx.write(plain[k], fmt, [np.ascontiguousarray(gbuf[k]).view(np.uint8).reshape(h, w, -1)])
    plain["albedo"], plain["pbr"] = str(tmp_path / "albedo.gtx"), str(tmp_path / "pbr.gtx")
    gtx.write(plain["albedo"], capi.FORMAT_R8G8B8A8_SRGB, [albedo])
    gtx.write(plain["pbr"], capi.FORMAT_R8G8_UNORM, [pbr])
    packed["albedo"], packed["pbr"] = str(tmp_path / "albedo_bc7.gtx"), str(tmp_path / "pbr_bc5.gtx")
    gtx.write(packed["albedo"], capi.FORMAT_BC7_SRGB_BLOCK, [albedo_blocks], size=(w, h))
    gtx.write(packed["pbr"], capi.FORMAT_BC5_UNORM_BLOCK, [pbr_blocks], size=(w, h))

    frames = []
    for paths in (plain, packed):
        a = gapp.Application(w, h, dynamic_exposure=False)  # a 64 x 32 frame leaves the luminance pass no texels
        a.set_render_parameters(cam.render_params())
        a.set_lights(descs)
        a.upload_gbuffer_gtx(**paths)
        a.render_frames(3)
        frames.append(a.read_backbuffer().copy())
        if paths is packed:
            bc4 = str(tmp_path / "albedo_bc4.gtx")
            gtx.write(bc4, capi.FORMAT_BC4_UNORM_BLOCK, [rng.integers(0, 256, (h // 4, w // 4, 8), dtype=np.uint8)], size=(w, h))
            with pytest.raises(capi.GraniteHipError, match="wrong format"):
                a.upload_gbuffer_gtx(albedo=bc4)
            with pytest.raises(capi.GraniteHipError, match="wrong format"):
                a.upload_gbuffer_gtx(pbr=packed["albedo"])
        a.close()
    assert frames[0].any()
    np.testing.assert_array_equal(frames[1], frames[0])
