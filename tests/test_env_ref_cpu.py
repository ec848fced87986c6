"""CPU: tests/env_ref.py (float64, from the formulae) held to the reference's shaders executed on the CPU
(tests/golden/env_bake_shader_v1.npz), and exact probes of the model.

The distance between the two -- an fp32 evaluation's own error -- is what the GPU bound of tests/test_gpu_env_bake.py rests on.  As
recorded by tests/golden/make_env_bake_golden.py, in fp16 ulps beyond the standing absolute allowance of 1e-4: equirect_5 0.000,
equirect_16 0.949, specular_24 0.000, specular_16 0.000, diffuse_8 0.987, diffuse_4 0.000.  Asserted here: below one ulp in every case,
which the standing bound (2 ulps + 1e-4) covers with room."""
import os

import numpy as np
import pytest

import env_ref
from granite_amd import capi
from util import assert_rgba16f_close

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "env_bake_shader_v1.npz"))
MATRICES = GOLDEN["matrices"]


def held(name, ref_chain):
    got, want = env_ref.pack_chain(ref_chain).reshape(-1, 4), GOLDEN[name + "/out"].reshape(-1, 4)
    assert_rgba16f_close(got, want, what=name)
    assert env_ref.ulp_distance(got, want).max() < 1.0, name  # the measured distance: a rounding step, not a model difference


@pytest.mark.parametrize("name", ["equirect_5", "equirect_16"])
def test_equirect_to_cube_against_the_executed_shader(name):
    size, levels = (int(v) for v in GOLDEN[name + "/params"])
    held(name, env_ref.equirect_to_cube(MATRICES, GOLDEN[name + "/equirect"], size, levels))


@pytest.mark.parametrize("name", ["specular_24", "specular_16"])
def test_specular_against_the_executed_shader(name):
    src_size, src_levels, out_size, out_levels = (int(v) for v in GOLDEN[name + "/params"])
    env_ref.check_up_switch(MATRICES, out_size, out_levels)
    held(name, env_ref.specular(MATRICES, env_ref.unpack_chain(GOLDEN[name + "/src"], src_size, src_levels), out_size, out_levels))


@pytest.mark.parametrize("name", ["diffuse_8", "diffuse_4"])
def test_diffuse_against_the_executed_shader(name):
    src_size, src_levels, out_size = (int(v) for v in GOLDEN[name + "/params"])
    held(name, [env_ref.diffuse(MATRICES, env_ref.unpack_chain(GOLDEN[name + "/src"], src_size, src_levels), out_size)])


def constant_chain(size, levels, colour):
    return [np.broadcast_to(np.array(colour + (1.0,)), (6, env_ref.level_size(size, l), env_ref.level_size(size, l), 4)).copy() for l in range(levels)]


def test_constant_cube_bakes_to_the_constant():
    colour = (3.5, 0.25, 700.0)
    chain = constant_chain(8, 4, colour)
    for level in env_ref.specular(MATRICES, chain, 4, 3):
        assert np.array_equal(level, env_ref.round_half(np.broadcast_to(np.array(colour + (1.0,)), level.shape)))
    phi, theta = env_ref.diffuse_angles()
    factor = env_ref.SHADER_PI * phi.size * (np.cos(theta) * np.sin(theta)).sum() / (phi.size * theta.size)
    assert abs(factor - 1.0) < 0.02  # PI * sum(cos sin) / count: the Riemann sum of the cosine lobe, 1 in the limit
    got = env_ref.diffuse(MATRICES, chain, 4)
    want = np.broadcast_to(np.array(tuple(c * factor for c in colour) + (1.0,)), got.shape)
    assert_rgba16f_close(env_ref.to_half(got).view(np.uint16), env_ref.to_half(want).view(np.uint16), ulps=1.0, abs_tol=0.0, what="constant diffuse")


def test_one_lit_face_of_a_matching_equirect():
    """An equirect image painted by the face its direction selects bakes to a cube whose face f holds colour f (away from the edges,
    where the lat-long tap blends two colours)."""
    w, h, size = 256, 128, 8
    u, v = (np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h
    lon, lat = (u[None, :] - 0.5) / 0.1591, (v[:, None] - 0.5) / 0.3183  # atan(z, x), asin(-y)
    d = np.stack([np.cos(lat) * np.cos(lon), -np.sin(lat) * np.ones_like(lon), np.cos(lat) * np.sin(lon)], -1)
    face, _, _ = env_ref.select_face(d)
    image = np.ones((h, w, 4), np.float16)
    image[..., :3] = (face[..., None] == np.array([0, 2, 4])) * 1.0 + (face[..., None] == np.array([1, 3, 5])) * 0.5
    cube = env_ref.equirect_to_cube(MATRICES, image.view(np.uint16), size, 1)[0]
    for f in range(6):
        want = np.zeros(3)
        want[f // 2] = 1.0 if f % 2 == 0 else 0.5
        assert np.array_equal(cube[f, 2:-2, 2:-2, :3], np.broadcast_to(want, (size - 4, size - 4, 3))), f


def test_layout_offsets_match_the_c_abi():
    lib = capi.load_library()
    for size, levels in ((5, 3), (16, 5), (24, 5), (128, 8), (32, 1), (1, 1)):
        assert lib.gr_cube_chain_bytes(size, levels) == 8 * env_ref.chain_texels(size, levels)
        for level in range(levels):
            assert env_ref.chain_offset(size, level, 0) % 16 == 0
            for face in range(6):
                assert lib.gr_cube_chain_offset(size, level, face) == env_ref.chain_offset(size, level, face), (size, level, face)
    # hand-computed: 5 -> 2 -> 1 is 1200 + 192 + 48 bytes
    assert [env_ref.chain_offset(5, l, 0) for l in range(3)] == [0, 1200, 1392] and lib.gr_cube_chain_bytes(5, 3) == 1440
    assert lib.gr_cube_chain_offset(5, 1, 3) == 1200 + 3 * 32
