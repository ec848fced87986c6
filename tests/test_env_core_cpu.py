"""CPU: granite_amd/csrc/env_core.hpp built for the host (tests/cpp/env_core_host.cpp) and held to the reference's shaders executed on the
CPU (tests/golden/env_bake_shader_v1.npz) within the standing bound of tests/util.assert_rgba16f_close (2 fp16 ulps + 1e-4; see
tests/test_gpu_env_bake.py for why that is the bound), with a texel's taps on one lane and split over 64 as the kernels split them; the
per-face matrices of host/math.* against the reference's; and the seamless edge rule probed at face edges and at a corner."""
import ctypes as C
import os

import numpy as np
import pytest

import env_ref
from host_program import ROOT, build_library
from util import assert_rgba16f_close

GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "env_bake_shader_v1.npz"))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = C.CDLL(build_library(tmp_path_factory.mktemp("env_core"), "libenv_core_host.so", "env_core_host.cpp", exact=True))
    lib.env_host_chain_offset.restype = C.c_uint64
    return lib


@pytest.fixture(scope="module")
def matrices(host):
    m = np.zeros((6, 16), np.float32)
    host.env_host_matrices(ptr(m))
    return m


def test_face_matrices_equal_the_reference_transforms(matrices):
    # the reference goes through quaternions (look_at -> mat4_cast), host/math.* through the basis vectors: rounding apart
    assert np.abs(matrices - GOLDEN["matrices"]).max() < 1e-6


def test_chain_offsets(host):
    for size, levels in ((5, 3), (24, 5), (128, 8)):
        for level in range(levels):
            for face in range(6):
                assert host.env_host_chain_offset(size, level, face) == env_ref.chain_offset(size, level, face)


@pytest.mark.parametrize("name", ["equirect_5", "equirect_16"])
def test_equirect_to_cube(host, matrices, name):
    size, levels = (int(v) for v in GOLDEN[name + "/params"])
    equirect = np.ascontiguousarray(GOLDEN[name + "/equirect"])
    out = np.zeros_like(GOLDEN[name + "/out"])
    host.env_host_equirect_to_cube(ptr(matrices), ptr(equirect), equirect.shape[1], equirect.shape[0], ptr(out), size, levels)
    assert_rgba16f_close(out.reshape(-1, 4), GOLDEN[name + "/out"].reshape(-1, 4), what=name)


@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("name", ["specular_24", "specular_16"])
def test_specular(host, matrices, name, lanes):
    src_size, src_levels, out_size, out_levels = (int(v) for v in GOLDEN[name + "/params"])
    src, out = np.ascontiguousarray(GOLDEN[name + "/src"]), np.zeros_like(GOLDEN[name + "/out"])
    host.env_host_specular(ptr(matrices), ptr(src), src_size, src_levels, ptr(out), out_size, out_levels, lanes)
    assert_rgba16f_close(out.reshape(-1, 4), GOLDEN[name + "/out"].reshape(-1, 4), what=f"{name} on {lanes} lanes")


@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("name", ["diffuse_8", "diffuse_4"])
def test_diffuse(host, matrices, name, lanes):
    src_size, src_levels, out_size = (int(v) for v in GOLDEN[name + "/params"])
    src, out = np.ascontiguousarray(GOLDEN[name + "/src"]), np.zeros_like(GOLDEN[name + "/out"])
    assert host.env_host_diffuse(ptr(matrices), ptr(src), src_size, src_levels, ptr(out), out_size, lanes) == 0  # 252 x 63 taps
    assert_rgba16f_close(out.reshape(-1, 4), GOLDEN[name + "/out"].reshape(-1, 4), what=f"{name} on {lanes} lanes")


def sample(host, chain_bits, size, levels, level, d):
    rgb, st, d = np.zeros(3, np.float32), np.zeros(2, np.float32), np.asarray(d, np.float32)
    face = host.env_host_sample(ptr(chain_bits), size, levels, level, ptr(d), ptr(rgb), ptr(st))
    return face, rgb, st


def test_seamless_edges_and_corner(host):
    """A cube whose texel (face, y, x) holds (face, y, x): the sampler's taps can be read off the result."""
    size = 4
    level = np.ones((6, size, size, 4))
    level[..., 0], level[..., 1], level[..., 2] = np.meshgrid(np.arange(6), np.arange(size), np.arange(size), indexing="ij")
    bits = np.ascontiguousarray(env_ref.pack_chain([level]))
    # face selection and ties: Z over Y over X
    for d, face in (((1, 0.2, 0.3), 0), ((-1, 0.2, 0.3), 1), ((0.1, 1, 0.3), 2), ((0.1, -1, 0.3), 3), ((0.1, 0.2, 1), 4), ((0.1, 0.2, -1), 5),
                    ((1, 1, 1), 4), ((1, 1, -1), 5), ((1, 1, 0.5), 2), ((1, -1, 0.5), 3), ((-1, 0.5, 1), 4)):
        assert sample(host, bits, size, 1, 0, d)[0] == face, d
    # on the edge between +X and +Z (x = z): the footprint straddles it and reads both faces' edge columns with equal weight.
    # +Z at s = 1: columns 3 of +Z and -- off the face -- the nearest texel of +X, its column 0 (sc = -z there).
    face, rgb, st = sample(host, bits, size, 1, 0, (1.0, -0.25 * 0.5, 1.0))  # tc = 0.125 -> t = 0.5625: row centre 2 (2.25 - 0.5 = 1.75 ..)
    assert face == 4 and st[0] == 1.0
    t = 0.5625 * size - 0.5  # 1.75: rows 1 and 2, weight 0.75 on row 2
    assert np.allclose(rgb, [0.5 * 4 + 0.5 * 0, 1 * 0.25 + 2 * 0.75, 0.5 * 3 + 0.5 * 0], atol=1e-6), rgb
    # the float64 model agrees on directions across every edge and at the corners
    rng = np.random.default_rng(5)
    noise = np.ones((6, size, size, 4))
    noise[..., :3] = rng.uniform(0.0, 4.0, (6, size, size, 3))
    noise = env_ref.round_half(noise)
    nbits = np.ascontiguousarray(env_ref.pack_chain([noise]))
    dirs = [(1, 1, 1), (1, -1, 1), (-1, 1, -1), (1, 0.999, 0.3), (0.999, 1, 0.3), (0.3, 1, 0.9999), (-0.3, -1, 1.0001), (1, 0.97, 0.98), (-1, -0.99, 0.97),
            (0.98, 0.99, -1)]
    for d in dirs:
        _, rgb, _ = sample(host, nbits, size, 1, 0, d)
        want = env_ref.sample_level(noise, np.array([d], np.float64))[0]
        assert np.allclose(rgb, want, rtol=1e-5, atol=1e-5), (d, rgb, want)
    # continuity across an edge: two directions a hair to either side of x = z give the same colour to fp32 accuracy
    a = sample(host, nbits, size, 1, 0, (1.0, 0.3, 1.0 - 1e-6))[1]
    b = sample(host, nbits, size, 1, 0, (1.0, 0.3, 1.0 + 1e-6))[1]
    assert np.allclose(a, b, atol=1e-4), (a, b)
