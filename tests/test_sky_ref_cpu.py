"""CPU: tests/sky_ref.py (numpy float32, single operations in the shader's order) against the reference's sky shaders executed on the CPU
(tests/golden/sky_shader_v1.npz).  The zero mask -- the two decisions of rayleigh_mie_scatter, made of + - * sqrt -- is the golden's exactly
on every procedural case and on both gr_sky_cube cases; the values differ through exp and pow alone, and the largest distance is asserted
to stay below one fp16 ulp beyond an absolute 1e-4: the premise of the GPU test's bound (tests/test_gpu_sky.py).  Measured when the golden
was recorded: at most 0.795 ulps (horizon/40x24, mie_peak/136x72), 0 on the other cases."""
import numpy as np
import pytest

import sky_cases as sc
import sky_ref

GOLDEN = sc.load_golden()


def test_the_golden_holds_the_cases_it_is_there_for():
    for name, (width, height, pattern, *_rest) in {**sc.PROCEDURAL, **sc.TEXTURED}.items():
        case = sc.apply_case(GOLDEN, name)
        far = case["depth"] == 0.0
        assert (case["width"], case["height"]) == (width, height)
        assert far.any() == (pattern != "none") and (pattern == "all") == bool(far.all()), name
        assert not case["out"][~far].any() and not case["zero"][~far].any(), name
    horizon = sc.apply_case(GOLDEN, "horizon/40x24")
    assert horizon["zero"].any() and ((horizon["depth"] == 0.0) & ~horizon["zero"]).any(), "both outcomes of the earth test in one image"
    assert sorted(float(GOLDEN[f"{n}/camera_height"]) for n in sc.PROCEDURAL) == [-5.0, 0.0, 2.0, 2.0, 1500.0]
    for name in sc.PROCEDURAL:
        values = GOLDEN[f"{name}/out"][GOLDEN[f"{name}/out"] != 0.0]
        assert values.size == 0 or (values > 0.125).mean() >= 0.9, name


@pytest.mark.parametrize("name", list(sc.PROCEDURAL))
def test_the_procedural_sky_against_the_executed_shader(name):
    case = sc.apply_case(GOLDEN, name)
    far = case["depth"] == 0.0
    got = sky_ref.apply_procedural(case["depth"], case["inv"], case["color"], case["camera_height"], case["sun_direction"])
    assert got.dtype == np.float32
    assert np.array_equal(sky_ref.zero_mask(got, far), case["zero"]), f"{name}: the zero mask is exact"
    distance = sky_ref.ulp_distance(got, case["out"]).max(initial=0.0)
    print(f"{name}: sky_ref.py against the executed shader: {distance:.3f} fp16 ulps beyond 1e-4")
    assert distance < 1.0, name


@pytest.mark.parametrize("name", list(sc.CUBES))
def test_the_sky_cube_against_the_executed_shader(name):
    case = sc.cube_case(GOLDEN, name)
    got = sky_ref.sky_cube(case["size"], case["sun_color"], case["camera_y"], case["sun_direction"])
    assert np.array_equal(got == 0.0, case["out"] == 0.0), f"{name}: the zero mask is exact"
    assert (got[..., 3] == 1.0).all()
    distance = sky_ref.ulp_distance(got, case["out"]).max()
    print(f"{name}: sky_ref.py against the executed shader: {distance:.3f} fp16 ulps beyond 1e-4")
    assert distance < 1.0, name


def test_the_direction_statement_is_the_matrix_at_the_pixel_centre():
    case = sc.apply_case(GOLDEN, "horizon/40x24")
    inv = case["inv"].reshape(4, 4)
    d = sky_ref.pixel_directions(case["inv"], 40, 24)
    px, py = np.float32(2.0) * np.float32(7.5) / np.float32(40) - np.float32(1.0), np.float32(2.0) * np.float32(3.5) / np.float32(24) - np.float32(1.0)
    assert np.array_equal(d[3, 7], inv[0, :3] * px + inv[1, :3] * py + inv[2, :3] + inv[3, :3])
