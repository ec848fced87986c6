"""GPU: directional shadows in the application -- gapp.Application at 96 x 64 on the synthetic G-buffer, Application.set_directional_shadows.

Without positional lights the lit target "HDR-main" of a shadowed frame equals, byte for byte, gr_directional_light run stand-alone on the
uploaded G-buffer with the application's render parameters (the launch tests/test_gpu_shadows.py holds to the executed shaders): cascaded
PCF on a D16 map, the wide kernel on a D32 map, and VSM on a depth map, where the application runs the VSM chain on upload and the
stand-alone side runs gr_vsm_moments and gr_vsm_blur itself.  With lights, a shadow map whose term is 1 everywhere gives the frame of an
application that never had shadows, under the lighting bound (the two paths round alike but are different kernels); a map with occluders
gives another frame.  set_directional_shadows(None) afterwards gives the lit target, byte for byte, of an application that never had shadows
(what follows the lighting pass carries exposure history from the frames before and is not compared)."""
import numpy as np
import pytest

import shadow_cases as sc
import shadow_device as dev
from granite_amd import app as gapp, capi, synth
from util import assert_rgba16f_close

pytestmark = pytest.mark.gpu
W, H = 96, 64
LOG_BIAS = float(np.float32(1.0 - np.log2(10.0)))


@pytest.fixture(scope="module")
def scene():
    cam = synth.Camera(W, H)
    return cam, synth.make_gbuffer(cam)


def make_app(scene, lights=0, **kw):
    cam, gbuf = scene
    a = gapp.Application(W, H, **kw)
    a.set_camera(synth._cm(cam.P), synth._cm(cam.V))
    a.set_lights(synth.make_lights(cam, lights) if lights else np.zeros(0, synth.LIGHT_DESC_DTYPE))
    a.upload_gbuffer(gbuf)
    return a


def transforms():
    """world -> (u, v, z): the light looks down the y axis; cascade i covers 12 * 2^i units around the origin"""
    out = np.zeros((4, 4, 4), np.float32)
    for i in range(4):
        r = 12.0 * 2.0 ** i
        out[i] = np.float32([[0.5 / r, 0, 0, 0.5], [0, 0, 0.5 / r, 0.5], [0, 1.0 / 128.0, 0, 0.5], [0, 0, 0, 1]])
    return np.ascontiguousarray(out.transpose(0, 2, 1)).reshape(4, 16)  # column-major


def depth_maps(layers, height, width, d16):
    rng = np.random.default_rng(11)
    blocks = rng.choice([0.35, 0.5, 0.5, 0.62], (layers, (height + 3) // 4, (width + 3) // 4))
    field = np.repeat(np.repeat(blocks, 4, 1), 4, 2)[:, :height, :width] + rng.normal(0.0, 0.01, (layers, height, width))
    return np.rint(np.clip(field, 0, 1) * 65535.0).astype(np.uint16) if d16 else field.astype(np.float32)


def standalone(gr, scene, rp, maps, mode):
    """gr_directional_light on fresh copies of what was uploaded, with the application's parameters -> the lit target's halves"""
    _, gbuf = scene
    case = dict(width=W, height=H, albedo=gbuf["albedo"], normal=gbuf["normal"], pbr=gbuf["pbr"], depth=gbuf["depth"], emissive=gbuf["emissive"],
                inv_view_projection=rp[80:96], color=synth.DIRECTIONAL_COLOR, direction=synth.DIRECTIONAL_DIRECTION, camera_pos=rp[96:99],
                camera_front=rp[99:102], cascade_log_bias=LOG_BIAS, fallback=True, mode=mode, maps=maps, transforms=transforms())
    args, imgs = dev.directional_args(case, dev.tight(gr), in_place=False)
    gr.directional_light(args)
    gr.sync()
    return dev.download_rgba16f(imgs["hdr"])


def moments_chain(gr, depth):
    """gr_vsm_moments, the down blur and the up blur on every layer -> (layers, h, w, 2)"""
    out = []
    for layer in depth:
        h, w = layer.shape
        src = capi.DeviceImage(gr, w, h, capi.FORMAT_D16_UNORM if layer.dtype == np.uint16 else capi.FORMAT_D32_SFLOAT).upload(layer)
        raw = capi.DeviceImage(gr, w, h, capi.FORMAT_R32G32_SFLOAT)
        half = capi.DeviceImage(gr, sc.half_size(w), sc.half_size(h), capi.FORMAT_R32G32_SFLOAT)
        blurred = capi.DeviceImage(gr, w, h, capi.FORMAT_R32G32_SFLOAT)
        gr.vsm_moments(src, raw)
        gr.vsm_blur(raw, half, False)
        gr.vsm_blur(half, blurred, True)
        gr.sync()
        out.append(dev.download_moments(blurred))
    return np.stack(out)


def hdr(a):
    return np.ascontiguousarray(a.read("HDR-main")).view(np.uint16).reshape(H, W, 4)


def test_a_shadowed_frame_is_the_standalone_launch(gr, scene):
    never = make_app(scene)
    never.render_frames(2)
    unshadowed = hdr(never)
    never.close()
    # cascaded PCF on a D16 map, the wide kernel on one D32 layer, VSM from a D16 map through the chain
    for mode, layers, d16 in ((capi.SHADOW_PCF, 4, True), (capi.SHADOW_PCF_WIDE, 1, False), (capi.SHADOW_VSM, 4, True)):
        maps = depth_maps(layers, 33, 17 if mode == capi.SHADOW_VSM else 32, d16)
        a = make_app(scene)
        a.set_directional_shadows(maps, mode, transforms(), LOG_BIAS)
        a.render_frames(2)
        got = hdr(a)
        want = standalone(gr, scene, a.get_render_parameters(), moments_chain(gr, maps) if mode == capi.SHADOW_VSM else maps, mode)
        assert np.array_equal(got, want), mode
        assert not np.array_equal(got, unshadowed), "the shadows reach the lit target"
        a.set_directional_shadows(None)
        a.render_frames(2)
        assert np.array_equal(hdr(a), unshadowed), "shadows off: the lit target of an application that never had them"
        a.close()


def test_with_lights_a_term_of_one_is_the_unshadowed_frame(scene):
    lit = np.tile(np.float32([2.0, 4.0]), (1, 4, 4, 1))  # moments.x above every depth: vsm() is exactly 1
    a, never = make_app(scene, 40), make_app(scene, 40)
    a.set_directional_shadows(lit, capi.SHADOW_VSM, transforms(), LOG_BIAS)
    for each in (a, never):
        each.render_frames(2)
    unshadowed = hdr(never)
    assert_rgba16f_close(hdr(a), unshadowed, ulps=2.0, abs_tol=1e-4, what="directional + clustered against the fused kernel")
    a.set_directional_shadows(depth_maps(4, 24, 32, True), capi.SHADOW_PCF, transforms(), LOG_BIAS)
    a.render_frames(2)
    darker = hdr(a).view(np.float16).astype(np.float32)[..., :3]
    assert (darker <= unshadowed.view(np.float16).astype(np.float32)[..., :3] + 1e-2).all() and not np.array_equal(hdr(a), unshadowed), "occluders only take light away"
    a.set_directional_shadows(None)
    a.render_frames(2)
    assert np.array_equal(hdr(a), unshadowed)
    a.close()
    never.close()
