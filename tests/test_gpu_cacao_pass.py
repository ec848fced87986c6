"""GPU: ambient_occlusion = AMBIENT_OCCLUSION_CACAO through the application -- setup_ffx_cacao in the "ssao-main" pass of the deferred
graph.  The pass equals the gr_cacao_* entry points called one by one on the same inputs, byte for byte, on two consecutive frames,
whatever a tolerance would allow; it stays within tests/cacao_chain.py's whole-pass bound of tests/cacao_ref.py's chain; the lit HDR-main is
the oracle's lighting with the computed image as its ambient occlusion; an upload into the computed pass is refused; and
ambient_occlusion = 1 is what it was."""
import numpy as np
import pytest

import cacao_cases as cc
import cacao_chain as chain
import cacao_ref as cr
from granite_amd import app as gapp, capi, synth
from oracle import oracle as orc
from util import assert_rgba16f_close

pytestmark = pytest.mark.gpu

PASS_CASES = tuple(c for c in cc.CASES if c in ((130, 98, "survey", "reference", "synthetic"), (61, 45, "oblique", "reference", "box")))


def oracle_lighting(cam, gbuf, descs, ao):
    rp = cam.render_params()
    n, lights, model, tmask, _ = orc.pack_lights(descs, rp[99:102])
    prm = orc.cluster_params(rp, *synth.CLUSTER_RESOLUTION, n)
    cb = orc.cluster_build(rp, prm, lights, model, tmask, n, synth.CLUSTER_RESOLUTION[2])
    return orc.lighting(gbuf, rp, prm, lights, tmask, cb["bitmask"], cb["range"], synth.DIRECTIONAL_COLOR, synth.DIRECTIONAL_DIRECTION,
                        ambient_occlusion=ao)


def make_app(cam, gbuf, descs, **kw):
    a = gapp.Application(cam.width, cam.height, **kw)
    a.set_render_parameters(cam.render_params())
    a.set_lights(descs)
    a.upload_gbuffer(gbuf)
    return a


@pytest.mark.parametrize("case", PASS_CASES, ids=cc.case_id)
def test_pass_is_the_chain_and_lights_the_frame(case):
    assert len(PASS_CASES) == 2
    w, h, cam_name, variant, _ = case
    cam = cc.camera(cam_name, w, h)
    depth, normal = cc.case_inputs(case)
    gbuf = dict(synth.make_gbuffer(cam), depth=depth, normal=normal)
    descs = synth.make_lights(cam, 60)
    a = make_app(cam, gbuf, descs, ambient_occlusion=gapp.AMBIENT_OCCLUSION_CACAO)
    graph = a.graph()
    order = [p["name"] for p in graph["passes"]]
    assert order.index("gbuffer-main") < order.index("ssao-main") < order.index("lighting-main")
    frames = []
    for _ in range(2):
        a.render_frames(1)
        frames.append(a.read("ssao-output-main").reshape(h, w).copy())
    hdr = a.read("HDR-main").copy()
    with pytest.raises(capi.GraniteHipError, match="computes its ambient occlusion"):
        a.upload_ambient_occlusion(np.zeros((h, w), np.uint8))
    a.close()

    # the entry points one by one: the constants of the library for the camera the application was given
    gr = capi.Context(0)
    proj, view = cc.matrices(cam)
    constants = capi.cacao_constants(w, h, proj, view, ctx=gr)
    d = capi.DeviceImage(gr, w, h, capi.FORMAT_D32_SFLOAT).upload(depth)
    n = capi.DeviceImage(gr, w, h, capi.FORMAT_A2B10G10R10_UNORM_PACK32).upload(normal)
    out = capi.DeviceImage(gr, w, h, capi.FORMAT_R8_UNORM)
    workspace = gr.cacao_workspace(w, h)
    for frame in frames:
        gr.cacao(d, n, out, workspace, constants)
        gr.sync()
        np.testing.assert_array_equal(frame, out.download())
    gr.close()

    want = chain.reference(case, cr.QUALITY_HIGHEST)["output"]
    distance = chain.codes(frames[0], want)
    largest, mean = chain.whole_pass_bound(case, cr.QUALITY_HIGHEST)
    print(f"{cc.case_id(case)}: pass against the reference chain largest {int(distance.max())} code(s), mean {float(distance.mean()):.5f}")
    assert distance.max() <= largest and distance.mean() <= mean, (int(distance.max()), float(distance.mean()), largest, mean)
    assert frames[0].min() < 255, "no occlusion anywhere"

    assert_rgba16f_close(hdr, oracle_lighting(cam, gbuf, descs, frames[0]), ulps=2.0, abs_tol=1e-4, what="HDR-main with computed ambient occlusion")


def test_uploaded_ambient_occlusion_is_unchanged():
    """ambient_occlusion = True and = 1 are one configuration: white until an image is uploaded, then that image"""
    cam = synth.Camera(130, 98)
    gbuf, descs = synth.make_gbuffer(cam), synth.make_lights(cam, 60)
    reads = []
    ao = np.random.default_rng(4).integers(0, 256, (cam.height, cam.width), dtype=np.uint8)
    for value in (True, gapp.AMBIENT_OCCLUSION_UPLOAD):
        a = make_app(cam, gbuf, descs, ambient_occlusion=value)
        a.render_frames(2)
        white = a.read("ssao-output-main").copy()
        assert (white == 255).all()
        a.upload_ambient_occlusion(ao)
        a.render_frames(2)
        reads.append((a.read("ssao-output-main").reshape(cam.height, cam.width).copy(), a.read("HDR-main").copy()))
        a.close()
    np.testing.assert_array_equal(reads[0][0], ao)
    np.testing.assert_array_equal(reads[0][0], reads[1][0])
    np.testing.assert_array_equal(reads[0][1], reads[1][1])
