"""GPU: the sky in the application -- gapp.Application with sky = 1 (atmosphere) and 2 (cube) on the synthetic G-buffer.

With a camera that moves (and climbs) over two frames, "emissive-main" after each frame equals, byte for byte, gr_sky_apply run stand-alone
on the uploaded emissive and depth with that frame's parameters (gra_get_sky_state: inv_local_view_projection and the Skybox's push values),
in both emissive formats: the pass refills emissive from its source every frame and applies the sky once.  With sky = 0 the emissive and
the backbuffer are those of an application whose config never names the field.  With decals and sky both on, both are applied.  sky = 2
without a cube fails the frame with a message that says so; the .gtx form gives the frame of the in-memory form."""
import numpy as np
import pytest

import sky_cases as sc
from granite_amd import app as gapp, capi, gtx, synth

pytestmark = pytest.mark.gpu
W, H = 200, 120
GOLDEN = sc.load_golden()
CUBE = dict(cube=GOLDEN["cube16_crossing/40x24/cube"], size=16, levels=5, color=(0.5, 1.0, 1.5))


@pytest.fixture(scope="module")
def scene():
    cam = synth.Camera(W, H)
    gbuf = synth.make_gbuffer(cam)
    far = gbuf["depth"] == 0
    assert far.any() and not far.all()
    return cam, gbuf


def make_app(scene, rt_fp16=True, **kw):
    cam, gbuf = scene
    a = gapp.Application(W, H, rt_fp16=rt_fp16, **kw)
    a.set_camera(synth._cm(cam.P), synth._cm(cam.V))
    a.set_lights(synth.make_lights(cam, 40))
    a.upload_gbuffer(dict(gbuf, emissive=gbuf["emissive"] if rt_fp16 else synth.pack_b10g11r11(gbuf["emissive"])))
    return a


def standalone(gr, scene, rt_fp16, state, cube=None):
    """gr_sky_apply on fresh copies of what was uploaded, with the application's parameters of that frame -> emissive bytes"""
    _, gbuf = scene
    fmt = capi.FORMAT_R16G16B16A16_SFLOAT if rt_fp16 else capi.FORMAT_B10G11R11_UFLOAT_PACK32
    emissive = capi.DeviceImage(gr, W, H, fmt).upload(gbuf["emissive"] if rt_fp16 else synth.pack_b10g11r11(gbuf["emissive"]))
    depth = capi.DeviceImage(gr, W, H, capi.FORMAT_D32_SFLOAT).upload(gbuf["depth"])
    chain = capi.DeviceBuffer(gr, cube["cube"].nbytes).upload(cube["cube"]) if cube else None
    gr.sky_apply(emissive, depth, state["inv_local_view_projection"], state["color"], state["camera_height"], state["direction"], chain,
                 cube["size"] if cube else 0, cube["levels"] if cube else 0)
    gr.sync()
    return np.ascontiguousarray(emissive.download()).view(np.uint8).reshape(-1)


def frame_bytes(a, name="emissive-main"):
    return np.ascontiguousarray(a.read(name)).view(np.uint8).reshape(-1)


@pytest.mark.parametrize("rt_fp16", [True, False], ids=["rgba16f", "b10g11r11"])
def test_the_atmosphere_over_two_frames_of_a_moving_camera(gr, scene, rt_fp16):
    a = make_app(scene, rt_fp16, sky=gapp.SKY_ATMOSPHERE)
    a.set_directional(sc.sun(25.0, 30.0), (30.0, 28.0, 26.0))
    a.set_camera_motion((0.25, 400.0, -0.5))
    uploaded = standalone_input(scene, rt_fp16)
    heights = []
    for frame in range(2):
        a.render_frames(1)
        state = a.get_sky_state()
        heights.append(state["camera_height"])
        assert np.array_equal(state["color"], np.float32([30.0, 28.0, 26.0])) and np.allclose(state["direction"], sc.sun(25.0, 30.0), atol=1e-6)
        got = frame_bytes(a)
        assert np.array_equal(got, standalone(gr, scene, rt_fp16, state)), f"frame {frame}"
        assert not np.array_equal(got, uploaded), "the far pixels were written"
    assert heights[1] - heights[0] == pytest.approx(400.0, abs=1e-2), "the second frame is drawn from the camera's new height"
    a.close()


def standalone_input(scene, rt_fp16):
    _, gbuf = scene
    return np.ascontiguousarray(gbuf["emissive"] if rt_fp16 else synth.pack_b10g11r11(gbuf["emissive"])).view(np.uint8).reshape(-1)


@pytest.mark.parametrize("rt_fp16", [True, False], ids=["rgba16f", "b10g11r11"])
def test_the_cube_over_two_frames(gr, scene, rt_fp16):
    a = make_app(scene, rt_fp16, sky=gapp.SKY_CUBE)
    a.set_sky_cube(CUBE["cube"], CUBE["size"], CUBE["levels"], CUBE["color"])
    a.set_camera_motion((0.25, 3.0, -0.5))
    for frame in range(2):
        a.render_frames(1)
        state = a.get_sky_state()
        assert np.array_equal(state["color"], np.float32(CUBE["color"])) and state["camera_height"] == 0.0 and not state["direction"].any()
        assert np.array_equal(frame_bytes(a), standalone(gr, scene, rt_fp16, state, CUBE)), f"frame {frame}"
    a.close()


def test_the_cube_mode_without_a_cube_fails_the_frame(scene):
    a = make_app(scene, sky=gapp.SKY_CUBE)
    with pytest.raises(capi.GraniteHipError, match="no cube is set"):
        a.render_frames(1)
    a.close()


def test_the_gtx_form_gives_the_frame_of_the_in_memory_form(scene, tmp_path):
    levels, at = [], 0
    for l in range(CUBE["levels"]):
        n = max(CUBE["size"] >> l, 1)
        levels.append(CUBE["cube"][at:at + 6 * n * n * 4].reshape(6, n, n, 4))
        at += 6 * n * n * 4
    path = str(tmp_path / "cube.gtx")
    gtx.write(path, capi.FORMAT_R16G16B16A16_SFLOAT, levels, layers=6)
    frames = []
    for source in (path, None):
        a = make_app(scene, sky=gapp.SKY_CUBE)
        if source:
            a.set_sky_cube(source, color=CUBE["color"])
        else:
            a.set_sky_cube(CUBE["cube"], CUBE["size"], CUBE["levels"], CUBE["color"])
        a.render_frames(1)
        frames.append(frame_bytes(a))
        a.close()
    assert np.array_equal(frames[0], frames[1])


def test_off_is_the_application_without_the_field(scene):
    off, never = make_app(scene, sky=gapp.SKY_OFF), make_app(scene)
    for a in (off, never):
        a.render_frames(2)
    assert np.array_equal(frame_bytes(off), frame_bytes(never)) and np.array_equal(frame_bytes(off), standalone_input(scene, True))
    assert np.array_equal(off.read_backbuffer(), never.read_backbuffer())
    on = make_app(scene, sky=gapp.SKY_ATMOSPHERE)
    on.render_frames(2)
    assert not np.array_equal(on.read_backbuffer(), off.read_backbuffer()), "the sky reaches the backbuffer"
    for a in (off, never, on):
        a.close()


def test_decals_and_sky_are_both_applied(gr, scene):
    cam, gbuf = scene
    textures = [synth.make_decal_texture(16, 4, 5, True), synth.make_decal_texture(8, 8, 1, False)]
    a = make_app(scene, sky=gapp.SKY_ATMOSPHERE, volumetric_decals=True)
    for i, t in enumerate(textures):
        a.set_decal_texture(i, t)
    a.set_decals(synth.make_decals(cam, 16, len(textures), size=(1.5, 3.0)))
    a.render_frames(2)
    albedo = a.read("albedo-main").reshape(H, W, 4).copy().view(np.uint32)[..., 0]
    assert not np.array_equal(albedo, gbuf["albedo"]), "the decals changed the base colour"
    far = gbuf["depth"] == 0
    assert np.array_equal(albedo[far], np.asarray(gbuf["albedo"], np.uint32)[far])
    assert np.array_equal(frame_bytes(a), standalone(gr, scene, True, a.get_sky_state()))
    a.close()
