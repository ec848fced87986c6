"""CPU: granite_amd/csrc/sky_core.hpp built for the host (tests/cpp/sky_core_host.cpp, a stand-alone program, -ffp-contract=off, visiting the
far pixels of 16 x 16 tiles through a compacted list as k_sky_apply does) and held to the reference's sky shaders executed on the CPU
(tests/golden/sky_shader_v1.npz): the zero mask exactly on every procedural case, every far pixel visited exactly once and no other, the
cube colours bit for bit (the runner and the header state one sampler and LOD model), values within one fp16 ulp beyond 1e-4 where exp and
pow are involved (measured: 0 on every case -- both sides call the same libm).  The program is built plainly and with
-fsanitize=address,undefined and run directly (its own main; nothing is preloaded), on the golden's inputs and on hostile ones.  The same
cases run on the device in tests/test_gpu_sky.py."""
import numpy as np
import pytest

import sky_cases as sc
import sky_ref
from host_program import program_fixtures, run_program

GOLDEN = sc.load_golden()
plain, sanitized = program_fixtures("sky_core_host.cpp", exact=True)


def run(exe, tmp_path, data):
    return run_program(exe, input_bytes=data, tmp_path=tmp_path)


def check_apply(exe, tmp_path, name):
    case = sc.apply_case(GOLDEN, name)
    rgb, written = sc.parse_host_apply(run(exe, tmp_path, sc.host_apply_bytes(case)), case["width"], case["height"])
    far = case["depth"] == 0.0
    assert np.array_equal(written, far.astype(np.uint32)), f"{name}: every far pixel once, no other pixel"
    assert np.array_equal(sky_ref.zero_mask(rgb, far), case["zero"]), f"{name}: the zero mask is exact"
    if "cube" in case:
        assert np.array_equal(rgb.view(np.uint32), case["out"].view(np.uint32)), f"{name}: the cube colours, bit for bit"
    else:
        distance = sky_ref.ulp_distance(rgb, case["out"]).max(initial=0.0)
        print(f"{name}: the host build against the executed shader: {distance:.3f} fp16 ulps beyond 1e-4")
        assert distance < 1.0, name


def check_cube(exe, tmp_path, name):
    case = sc.cube_case(GOLDEN, name)
    got = np.frombuffer(run(exe, tmp_path, sc.host_cube_bytes(case)), np.float32).reshape(case["out"].shape)
    assert np.array_equal(got == 0.0, case["out"] == 0.0), f"{name}: the zero mask is exact"
    distance = sky_ref.ulp_distance(got, case["out"]).max()
    print(f"{name}: the host build against the executed shader: {distance:.3f} fp16 ulps beyond 1e-4")
    assert distance < 1.0, name


@pytest.mark.parametrize("name", list(sc.PROCEDURAL) + list(sc.TEXTURED))
def test_apply_against_the_golden(plain, tmp_path, name):
    check_apply(plain, tmp_path, name)


@pytest.mark.parametrize("name", list(sc.CUBES))
def test_sky_cube_against_the_golden(plain, tmp_path, name):
    check_cube(plain, tmp_path, name)


@pytest.mark.parametrize("name", list(sc.PROCEDURAL) + list(sc.TEXTURED))
def test_apply_under_address_and_undefined_behaviour_sanitizers(sanitized, tmp_path, name):
    check_apply(sanitized, tmp_path, name)


@pytest.mark.parametrize("name", list(sc.CUBES))
def test_sky_cube_under_address_and_undefined_behaviour_sanitizers(sanitized, tmp_path, name):
    check_cube(sanitized, tmp_path, name)


def hostile_cases():
    """Inputs no frame should produce: the program must stay inside its arrays and finish, whatever the values come to."""
    base = sc.apply_case(GOLDEN, "horizon/40x24")
    textured = sc.apply_case(GOLDEN, "cube8_two_levels/40x24")
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    out = {}
    for label, fill in (("nan_matrix", nan), ("inf_matrix", inf), ("negative_inf_matrix", -inf), ("zero_direction", np.float32(0.0)),
                        ("huge_matrix", np.float32(3e38))):
        for kind, case in (("procedural", base), ("textured", textured)):
            out[f"{label}/{kind}"] = dict(case, inv=np.full(16, fill, np.float32))
    mixed = base["inv"].copy()
    mixed[[0, 5, 9]] = [nan, inf, -inf]
    out["mixed_matrix/procedural"] = dict(base, inv=mixed)
    out["mixed_matrix/textured"] = dict(textured, inv=mixed)
    out["zero_sun"] = dict(base, sun_direction=np.zeros(3, np.float32))
    out["nan_sun"] = dict(base, sun_direction=np.full(3, nan, np.float32))
    out["height_plus_1e30"] = dict(base, camera_height=1e30)
    out["height_minus_1e30"] = dict(base, camera_height=-1e30)
    out["height_nan"] = dict(base, camera_height=float("nan"))
    one = np.array([0x3c00, 0x4000, 0x4200, 0x3c00] * 6, np.uint16)  # a cube of size 1: six texels
    out["cube_of_size_1"] = dict(textured, cube=one, cube_size=1, cube_levels=1)
    out["cube_of_size_1/nan_matrix"] = dict(textured, cube=one, cube_size=1, cube_levels=1, inv=np.full(16, nan, np.float32))
    infinite = textured["cube"].copy()
    infinite[::7] = 0x7c00
    out["cube_of_infinities"] = dict(textured, cube=infinite)
    return out


HOSTILE = hostile_cases()


@pytest.mark.parametrize("name", list(HOSTILE))
def test_hostile_inputs_under_the_sanitizers(sanitized, tmp_path, name):
    case = HOSTILE[name]
    rgb, written = sc.parse_host_apply(run(sanitized, tmp_path, sc.host_apply_bytes(case)), case["width"], case["height"])
    assert np.array_equal(written, (case["depth"] == 0.0).astype(np.uint32)), name
    if name == "cube_of_size_1":
        # four fp32 weights that sum to 1 within their roundings
        assert np.allclose(rgb, np.float32([1.0, 2.0, 3.0]), rtol=1e-6, atol=0.0), "one texel a face, every face the same colour"
    if name.startswith("zero_direction"):
        assert not rgb.any() or np.isnan(rgb).any(), "a zero direction reads no texel"


def test_hostile_sky_cube_under_the_sanitizers(sanitized, tmp_path):
    for camera_y, sun in ((1e30, (0.0, 0.0, 0.0)), (-1e30, (np.nan, 0.0, 1.0)), (np.inf, (0.0, 1.0, 0.0))):
        case = dict(size=3, sun_color=np.float32([1, 1, 1]), camera_y=camera_y, sun_direction=np.float32(sun))
        assert len(run(sanitized, tmp_path, sc.host_cube_bytes(case))) == 6 * 3 * 3 * 16
