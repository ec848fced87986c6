"""GPU: the `ocean-update-lods` pass through gra_ocean_update (Granite::Ocean, granite_amd/ocean.py), directly and inside a RenderGraph,
moving and fixed-position, with the configurations, cameras and planes of golden cases.  ocean-lods is held to the golden as
tests/test_gpu_ocean_lod.py holds gr_ocean_update_lod; counters and patches equal tests/ocean_lod_ref.py applied to the LOD image the
device itself produced, which makes that comparison exact however log2 rounded; the instance counts add up to the number of boxes the
reference keeps; every patch's bucket is at most each of its four edge LODs; the meshes and the draw info read back are the host's.  An
ocean without lod_update has no resources 9 .. 11, and its nine resources are byte-identical to those of an ocean with it."""
import numpy as np
import pytest

import ocean_lod_ref as olr
from granite_amd import app as gapp
from granite_amd import capi
from granite_amd.ocean import LOD_RESOURCES, RESOURCES, Ocean
from ocean_lod_cases import GOLDEN, assert_lods, spec

pytestmark = pytest.mark.gpu
PASS_CASES = ["lod_g16_origin_perspective_moving", "lod_g16_origin_perspective_fixed", "lod_g16_negative_all_moving", "lod_g4_negative_perspective_moving",
              "lod_g8_origin_perspective_fixed", "lod_g16_far_all_moving"]


@pytest.fixture(scope="module")
def application():
    a = gapp.Application(64, 64, lighting=False)
    yield a
    a.close()


def make(application, name, **extra):
    gc, gr, fixed, _ = spec(name)
    cfg = GOLDEN[name + "/config"]
    ocean = Ocean(application, lod_update=1, fft_resolution=128, displacement_downsample=1, grid_count=gc, grid_resolution=gr,
                  ocean_size=(float(cfg[0]), float(cfg[1])), lod_bias=float(cfg[2]), fixed_position=fixed, center_position=cfg[6:9], **extra)
    ocean.set_camera(cfg[3:6], GOLDEN[name + "/frustum"])
    return ocean


@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("name", PASS_CASES)
def test_pass(application, name, route):
    gc, gr, fixed, wrap = spec(name)
    cfg = GOLDEN[name + "/config"]
    ocean = make(application, name, through_render_graph=route)
    try:
        for frame in range(2):  # a second frame of the same graph: the counters start from zero again
            ocean.update(1.5 + frame)
            info = ocean.describe("ocean-lods")
            assert (info.exists, info.is_image, info.width, info.height, info.format, info.levels) == (1, 1, gc, gc, capi.FORMAT_R16_SFLOAT, 1)
            assert ocean.describe("ocean-lod-counter").size_bytes == 8 * 32 and ocean.describe("ocean-lod-data").size_bytes == gc * gc * 8 * 32
            lods = ocean.read("ocean-lods")
            print(f"{name} route {route}: {assert_lods(name, lods, 'pass')} texels differ from the golden")
            draws = ocean.read("ocean-lod-counter").reshape(8, 8)
            data = ocean.read("ocean-lod-data")
            meshes = olr.lod_meshes(gr)
            init = olr.init_counters([len(i) for _, i in meshes] + [0] * (16 - len(meshes)))
            want_draws, want_patches = olr.cull_blocks(lods, GOLDEN[name + "/cull_push"], GOLDEN[name + "/frustum"], wrap, init)
            assert np.array_equal(draws, want_draws)
            got = olr.buckets_of(data, draws, gc * gc)
            for l in range(8):
                assert np.array_equal(got[l].view(np.uint32), olr.sorted_bucket(want_patches[l]).view(np.uint32)), l
                assert np.all(got[l][:, 4:8] >= l)
            assert int(draws[:, 1].sum()) == int(GOLDEN[name + "/draws"][:, 1].sum())
        # what a rasteriser binds beside the buffers
        info = ocean.draw_info()
        pushes = olr.pass_pushes(gc, gr, cfg[0:2], cfg[2], cfg[3:6], bool(fixed), cfg[6:9])
        want = olr.draw_data(128, gc, gr, cfg[0:2], 7.3, pushes["world_offset"], pushes["coord_offset"])
        assert np.array_equal(np.array(info.data[:], np.float32).view(np.uint32), want.view(np.uint32))
        assert (info.lods, info.lod_stride, info.index_type) == (len(meshes), gc * gc * 32, 0)
        for level, (rv, ri) in enumerate(meshes):
            assert ocean.mesh_info(level).on_device == 1
            v, i = ocean.mesh(level)
            assert np.array_equal(v, rv) and np.array_equal(i, ri), level
        assert not ocean.mesh_info(len(meshes)).exists
        positions, indices = olr.border_mesh(gc, gr, True, bool(fixed))
        assert info.border_count == len(indices)
        if fixed:
            assert not ocean.mesh_info("border").exists
        else:
            v, i = ocean.mesh("border")
            assert np.array_equal(v, positions) and np.array_equal(i, indices)
    finally:
        ocean.close()


def test_a_camera_moves_the_grid(application):
    name = "lod_g16_origin_all_moving"
    ocean = make(application, name)
    try:
        ocean.update(0.0)
        first = ocean.read("ocean-lod-data").copy()
        cfg = GOLDEN[name + "/config"]
        ocean.set_camera(cfg[3:6] + np.array([160.0, 0.0, -320.0], np.float32), GOLDEN[name + "/frustum"])
        ocean.update(0.0)
        draws = ocean.read("ocean-lod-counter").reshape(8, 8)
        moved = olr.buckets_of(ocean.read("ocean-lod-data"), draws, 256)
        offsets = np.concatenate(moved)[:, 0:2]
        # ten blocks along x, twenty back along z, 128 vertices a block
        want = np.concatenate(olr.buckets_of(first, GOLDEN[name + "/draws"], 256))[:, 0:2] + np.array([10 * 128, -20 * 128], np.float32)
        assert sorted(map(tuple, offsets)) == sorted(map(tuple, want))
        with pytest.raises(capi.GraniteHipError):
            ocean.set_camera((float("nan"), 0.0, 0.0), GOLDEN[name + "/frustum"])
        with pytest.raises(capi.GraniteHipError):
            ocean.set_camera((3.0e9, 0.0, 0.0), GOLDEN[name + "/frustum"])
    finally:
        ocean.close()


@pytest.mark.parametrize("route", [0, 1])
def test_without_lod_update_nothing_changes(application, route):
    config = dict(fft_resolution=128, displacement_downsample=1, grid_count=4, grid_resolution=32, ocean_size=(128.0, 128.0), through_render_graph=route)
    plain, with_lods = Ocean(application, **config), Ocean(application, lod_update=1, **config)
    try:
        plain.update(300.0)
        with_lods.update(300.0)
        for name in LOD_RESOURCES:
            assert not plain.describe(name).exists and with_lods.describe(name).exists
            with pytest.raises(capi.GraniteHipError):
                plain.read(name)
        for name in RESOURCES:
            a, b = plain.describe(name), with_lods.describe(name)
            assert (a.exists, a.is_image, a.width, a.height, a.format, a.levels, a.size_bytes) == (b.exists, b.is_image, b.width, b.height, b.format, b.levels, b.size_bytes)
            if name == "ocean-spd-counter":  # never written: the downsampler here has no ticket
                continue
            for level in range(a.levels if a.is_image else 1):
                assert np.array_equal(plain.read(name, level), with_lods.read(name, level)), (name, level)
        assert plain.mesh_info(0).exists and not plain.mesh_info(0).on_device
        assert np.array_equal(plain.mesh(0)[0], with_lods.mesh(0)[0]) and np.array_equal(plain.mesh("border")[1], with_lods.mesh("border")[1])
    finally:
        plain.close()
        with_lods.close()


@pytest.mark.parametrize("bad", [dict(heightmap=0), dict(grid_count=3), dict(grid_count=256), dict(grid_resolution=48), dict(grid_resolution=256)])
def test_refusals(application, bad):
    config = dict(fft_resolution=128, displacement_downsample=1, grid_count=4, grid_resolution=32, ocean_size=(128.0, 128.0))
    with pytest.raises(capi.GraniteHipError):
        Ocean(application, lod_update=1, **{**config, **bad})
    Ocean(application, **{**config, **bad}).close()  # without the LOD update the same configuration is today's ocean
