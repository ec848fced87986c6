"""GPU: the whole `ocean-update-fft` pass through gra_ocean_* (Granite::Ocean, granite_amd/ocean.py) at fft_resolution 128, displacement
64, grid 4 x 32, ocean_size 128.  Every resource and level read back equals, byte for byte, the same chain called entry point by entry
point on the same distributions (tests/ocean_chain.py); with force_mipmap_shader every level of every chain is ocean_ref's level-by-level
result; without a heightmap the height / displacement resource does not exist and the rest is unchanged; the route through a RenderGraph
gives the bytes of the direct one."""
import math

import numpy as np
import pytest

import ocean_chain
import ocean_ref as ocr
from granite_amd import app as gapp
from granite_amd import capi
from granite_amd.ocean import RESOURCES, Ocean

pytestmark = pytest.mark.gpu
CONFIG = dict(fft_resolution=128, displacement_downsample=1, grid_count=4, grid_resolution=32, ocean_size=(128.0, 128.0))
N, M, VERTEX_LEVELS, FULL = 128, 64, 5, 8
# resource name -> key of ocean_chain.run_update's result
BUFFERS = {"ocean-height-fft-input": "height-fft-input", "ocean-normal-fft-input": "normal-fft-input",
           "ocean-displacement-fft-input": "displacement-fft-input"}
IMAGES = {"ocean-height-fft-output": "height-fft-output", "ocean-displacement-fft-output": "displacement-fft-output"}
CHAINS = {"ocean-normal-fft-output": ("normal", FULL), "ocean-gradient-jacobian-output": ("gradient-jacobian", FULL),
          "ocean-height-displacement-output": ("height-displacement", VERTEX_LEVELS)}


@pytest.fixture(scope="module")
def application():
    a = gapp.Application(64, 64, lighting=False)
    yield a
    a.close()


@pytest.fixture(scope="module")
def gr():
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def read_all(ocean, heightmap=True):
    got = {}
    for name in RESOURCES:
        info = ocean.describe(name)
        if name == "ocean-height-displacement-output" and not heightmap:
            assert not info.exists
            with pytest.raises(capi.GraniteHipError):
                ocean.read(name)
            continue
        assert info.exists, name
        got[name] = [ocean.read(name, level) for level in range(info.levels)] if info.is_image else ocean.read(name)
    return got


def by_entry_points(gr, ocean, t, spd, heightmap=True):
    time = np.float32(math.fmod(t, 256.0))
    return ocean_chain.run_update(gr, ocean.distribution("height"), ocean.distribution("displacement"), ocean.distribution("normal"), time,
                                  world=128.0, delta=1.0, vertex_levels=VERTEX_LEVELS, spd=spd, heightmap=heightmap)


def assert_same(got, want, heightmap=True):
    for name, key in BUFFERS.items():
        assert np.array_equal(got[name].reshape(want[key].shape), want[key]), name
    for name, key in IMAGES.items():
        assert len(got[name]) == 1 and np.array_equal(got[name][0], want[key]), name
    for name, (key, levels) in CHAINS.items():
        if name == "ocean-height-displacement-output" and not heightmap:
            assert name not in got
            continue
        assert len(got[name]) == levels == len(want[key]), name
        for level, (a, b) in enumerate(zip(got[name], want[key])):
            assert np.array_equal(a, b), (name, level)


@pytest.fixture(scope="module")
def direct(application):
    ocean = Ocean(application, **CONFIG)
    yield ocean
    ocean.close()


def test_sizes_and_formats(direct):
    direct.update(0.0)
    expect = {"ocean-height-fft-input": 4 * N * N, "ocean-normal-fft-input": 4 * N * N, "ocean-displacement-fft-input": 4 * M * M}
    for name, size in expect.items():
        info = direct.describe(name)
        assert info.exists and not info.is_image and info.size_bytes == size
    assert direct.describe("ocean-spd-counter").exists
    for name, (size, fmt, levels) in {"ocean-height-fft-output": (N, capi.FORMAT_R16_SFLOAT, 1), "ocean-displacement-fft-output": (M, capi.FORMAT_R16G16_SFLOAT, 1),
                                      "ocean-normal-fft-output": (N, capi.FORMAT_R16G16_SFLOAT, FULL),
                                      "ocean-gradient-jacobian-output": (N, capi.FORMAT_R16G16B16A16_SFLOAT, FULL),
                                      "ocean-height-displacement-output": (N, capi.FORMAT_R16G16B16A16_SFLOAT, VERTEX_LEVELS)}.items():
        info = direct.describe(name)
        assert (info.is_image, info.width, info.height, info.format, info.levels) == (1, size, size, fmt, levels), name


@pytest.mark.parametrize("t", [0.0, 300.0])  # the second wraps to 44
def test_pass_equals_the_chain_entry_point_by_entry_point(gr, direct, t):
    direct.update(t)
    got = read_all(direct)
    assert_same(got, by_entry_points(gr, direct, t, spd=True))
    direct.update(t)
    again = read_all(direct)
    for name in got:
        for a, b in zip(got[name] if isinstance(got[name], list) else [got[name]], again[name] if isinstance(again[name], list) else [again[name]]):
            assert np.array_equal(a, b), name


def test_time_wraps_at_256(direct):
    direct.update(300.0)
    a = direct.read("ocean-height-fft-input")
    direct.update(44.0)
    assert np.array_equal(a, direct.read("ocean-height-fft-input"))
    direct.update(45.0)
    assert not np.array_equal(a, direct.read("ocean-height-fft-input"))


def test_force_mipmap_shader(gr, application):
    ocean = Ocean(application, force_mipmap_shader=1, **CONFIG)
    try:
        ocean.update(300.0)
        got = read_all(ocean)
        assert_same(got, by_entry_points(gr, ocean, 300.0, spd=False))
        for name, mod in (("ocean-normal-fft-output", ocean_chain.ONE), ("ocean-gradient-jacobian-output", ocean_chain.ONE),
                          ("ocean-height-displacement-output", ocean_chain.ZERO_FIRST)):
            want = ocr.mip_chain(got[name][0], len(got[name]), mod)
            for level, (a, b) in enumerate(zip(got[name], want)):
                assert np.array_equal(a, b), (name, level)
        last = got["ocean-height-displacement-output"]
        assert not np.any(last[-1][..., 0] & 0x7fff) and np.any(last[-2][..., 0] & 0x7fff)
    finally:
        ocean.close()


def test_without_heightmap(gr, application, direct):
    ocean = Ocean(application, heightmap=0, **CONFIG)
    try:
        ocean.update(300.0)
        got = read_all(ocean, heightmap=False)
        assert_same(got, by_entry_points(gr, ocean, 300.0, spd=True, heightmap=False), heightmap=False)
        direct.update(300.0)
        full = read_all(direct)
        for name in got:
            if name == "ocean-spd-counter":  # never written: the downsampler here has no ticket
                continue
            for a, b in zip(got[name] if isinstance(got[name], list) else [got[name]], full[name] if isinstance(full[name], list) else [full[name]]):
                assert np.array_equal(a, b), name
    finally:
        ocean.close()


def test_through_the_render_graph(application, direct):
    ocean = Ocean(application, through_render_graph=1, **CONFIG)
    try:
        for t in (300.0, 1.5):  # a second frame of the same graph
            ocean.update(t)
            direct.update(t)
            got, want = read_all(ocean), read_all(direct)
            for name in want:
                if name == "ocean-spd-counter":
                    continue
                for a, b in zip(got[name] if isinstance(got[name], list) else [got[name]], want[name] if isinstance(want[name], list) else [want[name]]):
                    assert np.array_equal(a, b), (name, t)
    finally:
        ocean.close()


def test_distributions_are_the_hosts(direct):
    height, disp, normal = direct.distribution("height"), direct.distribution("displacement"), direct.distribution("normal")
    assert height.shape == (N, N, 2) and disp.shape == (M, M, 2) and normal.shape == (N, N, 2)
    assert np.array_equal(disp, ocean_chain.downsample_distribution(height, 1))
    assert height[0, 0, 0] == 0.0 and height[0, 0, 1] == 0.0 and np.any(height != 0.0)


@pytest.mark.parametrize("bad", [dict(fft_resolution=96), dict(fft_resolution=64, displacement_downsample=1), dict(grid_count=0), dict(grid_resolution=0),
                                 dict(wind_velocity=(0.0, 0.0))])
def test_refusals(application, bad):
    with pytest.raises(capi.GraniteHipError):
        Ocean(application, **{**CONFIG, **bad})
