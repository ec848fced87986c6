"""GPU: volumetric decals in the application -- gapp.Application with volumetric_decals = 1, synth decals, textures and lights.

One frame: "cluster-bitmask-decal" and "cluster-range-decal" equal tests/decal_ref.py word for word (the restatement equals the executed
shaders: tests/test_decal_ref_cpu.py); "albedo" is held to decal_ref.apply by the rules of tests/test_gpu_decals.py -- bytes untouched
outside decals, on the far plane and in alpha, within 1 code value inside, pixels within the margin of a decal's faces left out, at most
0.5 % of the covered ones.  The lit "HDR" target is held, at every pixel, to oracle.lighting fed the reference's decaled albedo at the
tolerance tests/test_gpu_app.py uses for lighting.
Three frames give the albedo of one frame (decals do not accumulate), and with no decals set the frame equals a volumetric_decals = 0
frame byte for byte."""
import numpy as np
import pytest

import decal_cases as dc
import decal_ref as ref
from granite_amd import app as gapp, synth
from oracle import oracle as orc
from util import assert_rgba16f_close

pytestmark = pytest.mark.gpu
W, H, RES = 256, 144, (32, 16, 64)
LEFT_OUT_CAP = 0.005


@pytest.fixture(scope="module")
def scene():
    cam = synth.Camera(W, H)
    textures = [synth.make_decal_texture(16, 4, 5, True), synth.make_decal_texture(8, 8, 1, False), synth.make_decal_texture(32, 32, 6, True)]
    return cam, synth.make_gbuffer(cam), synth.make_lights(cam, 60), synth.make_decals(cam, 16, len(textures), size=(1.5, 3.0)), textures


def make_app(scene, decals=True, **kw):
    cam, gbuf, lights, descs, textures = scene
    a = gapp.Application(W, H, cluster_res=RES, **kw)
    a.set_render_parameters(cam.render_params())
    a.set_lights(lights)
    a.upload_gbuffer(gbuf)
    if decals:
        for i, t in enumerate(textures):
            a.set_decal_texture(i, t)
        a.set_decals(descs)
    return a


def reference_case(scene, prm):
    cam, gbuf, _, descs, textures = scene
    rp = cam.render_params()
    order = ref.host_sort_order(descs["transform"], rp[99:102])
    rows = descs["transform"][order]
    extent = ref.z_slice_extent(rp[103], RES[2])
    intervals = np.array([ref.compute_uint_range(*ref.decal_z_range(r, rp[96:99], rp[99:102]), extent, RES[2]) for r in rows], np.uint32)
    mvps = np.stack([ref.host_mvp(rp[32:48], r) for r in rows])
    case = {"width": W, "height": H, "prm": prm, "mvps": mvps, "intervals": intervals, "decal_rows": np.stack([ref.host_world_to_texture(r) for r in rows]),
            "albedo": gbuf["albedo"], "depth": gbuf["depth"], "inv_view_projection": rp[80:96], "textures": [textures[int(i)] for i in descs["texture"][order]]}
    case["bitmask_decal"], case["range_decal"] = ref.binning(prm, mvps), ref.z_ranges(intervals, RES[2])
    return case


def test_one_frame_against_the_reference(scene):
    cam, gbuf, lights, descs, _ = scene
    a = make_app(scene, volumetric_decals=True)
    a.render_frames(1)
    prm = np.frombuffer(a.cluster_state()["params"].tobytes(), dc.PRM_DTYPE)[0]
    assert (int(prm["num_decals"]), int(prm["num_decals_32"]), int(prm["decals_texture_offset"])) == (len(descs), 1, 0)
    case = reference_case(scene, prm)
    words = RES[0] * RES[1] * int(prm["num_decals_32"])
    assert np.array_equal(a.read("cluster-bitmask-decal").view(np.uint32)[:words], case["bitmask_decal"])
    assert np.array_equal(a.read("cluster-range-decal").view(np.uint32).reshape(-1, 2), case["range_decal"])

    mine = ref.apply(case)
    margin = 64.0 * mine["uvw_error"]
    left_out, touched = mine["edge_distance"] < margin, mine["touched"]
    covered = int(touched.sum())
    print(f"margin {margin:.3g}, {int(left_out.sum())} of {covered} covered pixels left out")
    assert covered > 1000 and int(left_out.sum()) <= LEFT_OUT_CAP * covered
    albedo = gbuf["albedo"]
    got = a.read("albedo-main").reshape(H, W, 4).copy().view(np.uint32)[..., 0]
    want = mine["bytes"]
    assert np.array_equal(got >> 24, albedo >> 24), "an alpha byte changed"
    far = gbuf["depth"] == 0
    assert far.any() and np.array_equal(got[far], albedo[far]), "a far-plane pixel was written"
    outside = ~touched & ~left_out
    assert np.array_equal(got[outside], albedo[outside]), "a pixel outside every decal changed"
    inside = touched & ~left_out
    channels = lambda x: np.stack([(x >> s) & 255 for s in (0, 8, 16)], -1).astype(np.int64)
    error = np.abs(channels(got[inside]) - channels(want[inside]))
    print(f"largest difference inside decals {int(error.max())} code values, {int((error > 0).sum())} of {error.size} channel values differ")
    assert error.max() <= 1

    rp = cam.render_params()
    n, packed, model, tmask, _ = orc.pack_lights(lights, rp[99:102])
    light_prm = orc.cluster_params(rp, *RES, n)
    cb = orc.cluster_build(rp, light_prm, packed, model, tmask, n, RES[2])
    lit = lambda alb: orc.lighting(dict(gbuf, albedo=np.ascontiguousarray(alb, np.uint32)), rp, light_prm, packed, tmask, cb["bitmask"], cb["range"],
                                   synth.DIRECTIONAL_COLOR, synth.DIRECTIONAL_DIRECTION)
    hdr = a.read("HDR-main")
    assert_rgba16f_close(hdr, lit(want), ulps=2.0, what="HDR-main against lighting of the reference's decaled albedo")
    assert not np.array_equal(hdr, a_without_decals_hdr(scene)), "the decals reach the lit target"
    a.close()


def a_without_decals_hdr(scene):
    a = make_app(scene, decals=False)
    a.render_frames(1)
    hdr = a.read("HDR-main")
    a.close()
    return hdr


def test_decals_do_not_accumulate(scene):
    one, three = make_app(scene, volumetric_decals=True), make_app(scene, volumetric_decals=True)
    one.render_frames(1)
    three.render_frames(3)
    assert np.array_equal(one.read("albedo-main"), three.read("albedo-main"))
    assert not np.array_equal(one.read("albedo-main").reshape(H, W, 4).view(np.uint32)[..., 0], scene[1]["albedo"])
    assert_rgba16f_close(one.read("HDR-main"), three.read("HDR-main"), ulps=0.0, abs_tol=0.0, what="HDR-main after three frames")
    one.close()
    three.close()


def test_no_decals_is_the_frame_without_the_feature(scene):
    on, off = make_app(scene, decals=False, volumetric_decals=True), make_app(scene, decals=False, volumetric_decals=False)
    for a in (on, off):
        a.render_frames(2)
    for name in ("albedo-main", "HDR-main"):
        assert np.array_equal(on.read(name), off.read(name)), name
    assert np.array_equal(on.read_backbuffer(), off.read_backbuffer())
    assert np.all(on.read("cluster-range-decal").view(np.uint32).reshape(-1, 2) == np.uint32(ref.EMPTY_RANGE)), "the decal ranges read empty"
    on.close()
    off.close()
