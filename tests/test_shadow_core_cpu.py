"""CPU: granite_amd/csrc/shadow_core.hpp built for the host (tests/cpp/shadow_core_host.cpp, a stand-alone program, -ffp-contract=off) and held
to the reference's directional.frag with SHADOWS, resolve_vsm.frag and the two VSM blurs executed on the CPU
(tests/golden/shadow_shader_v1.npz).  Both sides state one sampler model and call one libm, so the cascade decisions -- layer_near, layer_far,
shadow_lerp == 0, white_lerp == 0 -- are asserted exactly, and so are the shadow term, the lit target, the moments and the blurs: measured
0 everywhere.  The value bound is nevertheless the one the GPU tests use (tests/test_gpu_shadows.py), not bit equality: exp2, log2 and pow
belong to the platform.  The program is built plainly and with -fsanitize=address,undefined and run directly (its own main; nothing is
preloaded), on the golden's cases and on hostile ones."""
import numpy as np
import pytest

import shadow_cases as sc
import shadow_ref
from host_program import program_fixtures, run_program
from util import assert_rgba16f_close

GOLDEN = sc.load_golden()
plain, sanitized = program_fixtures("shadow_core_host.cpp", exact=True)


def run(exe, tmp_path, data):
    return run_program(exe, input_bytes=data, tmp_path=tmp_path)


def check_directional(exe, tmp_path, name):
    case = sc.directional_case(GOLDEN, name)
    hdr, term, layers, lerps = sc.parse_host_directional(run(exe, tmp_path, sc.host_directional_bytes(case, GOLDEN["srgb_table"])), case["width"], case["height"])
    far = case["depth"] == 0.0
    assert np.array_equal(hdr[far], case["emissive"][far]), f"{name}: a far-plane pixel changed"
    assert np.array_equal(hdr[..., 3], case["emissive"][..., 3]), f"{name}: an alpha changed"
    if case["cascaded"]:
        live = ~far
        assert np.array_equal(layers[live], case["layers"][live].astype(np.int32)), f"{name}: layer_near / layer_far"
        assert np.array_equal(lerps[live] == 0.0, case["lerps"][live] == 0.0), f"{name}: the shadow_lerp == 0 and white_lerp == 0 decisions"
    assert np.array_equal((term == 0.0), (case["term"] == 0.0)) and np.array_equal((term == 1.0), (case["term"] == 1.0)), f"{name}: fully lit / fully shadowed"
    distance = shadow_ref.ulp_distance(hdr[..., :3].view(np.float16), case["hdr"][..., :3].view(np.float16)).max()
    print(f"{name}: the host build against the executed shader: {distance:.3f} fp16 ulps beyond 1e-4, shadow term {np.abs(term - case['term']).max():.3e}")
    assert_rgba16f_close(hdr, case["hdr"], what=name)


@pytest.mark.parametrize("name", list(sc.DIRECTIONAL))
def test_directional_against_the_golden(plain, tmp_path, name):
    check_directional(plain, tmp_path, name)


@pytest.mark.parametrize("name", list(sc.DIRECTIONAL))
def test_directional_under_address_and_undefined_behaviour_sanitizers(sanitized, tmp_path, name):
    check_directional(sanitized, tmp_path, name)


def check_chain(exe, tmp_path):
    for name in sc.MOMENTS:
        depth = GOLDEN[f"{name}/depth"]
        got = np.frombuffer(run(exe, tmp_path, sc.host_moments_bytes(depth)), np.float32).reshape(GOLDEN[f"{name}/out"].shape)
        assert np.array_equal(got.view(np.uint32), GOLDEN[f"{name}/out"].view(np.uint32)), f"{name}: (z, z * z) is two exact operations"
    for name in sc.BLURS:
        source, down, up = GOLDEN[f"{name}/in"], GOLDEN[f"{name}/down"], GOLDEN[f"{name}/up"]
        half = (sc.half_size(source.shape[2]), sc.half_size(source.shape[1]))
        assert down.shape[1:3] == (half[1], half[0]) == (8, 16)
        got_down = np.frombuffer(run(exe, tmp_path, sc.host_blur_bytes(source, *half, False)), np.float32).reshape(down.shape)
        got_up = np.frombuffer(run(exe, tmp_path, sc.host_blur_bytes(down, source.shape[2], source.shape[1], True)), np.float32).reshape(up.shape)
        # + - * / only, in the shader's order, without contraction
        assert np.array_equal(got_down.view(np.uint32), down.view(np.uint32)), f"{name}: the down blur, bit for bit"
        assert np.array_equal(got_up.view(np.uint32), up.view(np.uint32)), f"{name}: the up blur, bit for bit"


def test_vsm_chain_against_the_golden(plain, tmp_path):
    check_chain(plain, tmp_path)


def test_vsm_chain_under_address_and_undefined_behaviour_sanitizers(sanitized, tmp_path):
    check_chain(sanitized, tmp_path)


def hostile_cases():
    """Inputs no frame should produce: the program must stay inside its arrays and finish, whatever the values come to."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    out = {}
    for base_name in ("pcf_cascades/61x37", "wide_cascades/64x40", "vsm_cascades/61x37", "pcf/64x40", "wide/61x37", "vsm/64x40"):
        base = sc.directional_case(GOLDEN, base_name)
        for label, fill in (("nan", nan), ("inf", inf), ("minus_inf", -inf), ("huge", np.float32(3e38)), ("zero", np.float32(0.0))):
            out[f"{label}_transforms/{base_name}"] = dict(base, transforms=np.full(64, fill, np.float32))
        out[f"nan_matrix/{base_name}"] = dict(base, inv_view_projection=np.full(16, nan, np.float32))
        out[f"inf_front/{base_name}"] = dict(base, camera_front=np.float32([inf, -inf, nan]))
        out[f"huge_bias/{base_name}"] = dict(base, cascade_log_bias=3e38)
        out[f"nan_bias/{base_name}"] = dict(base, cascade_log_bias=float("nan"))
    one = sc.directional_case(GOLDEN, "wide/61x37")
    out["map_of_one_texel"] = dict(one, maps=np.full((1, 1, 1), 0.5, np.float32))
    return out


HOSTILE = hostile_cases()


@pytest.mark.parametrize("name", list(HOSTILE))
def test_hostile_inputs_under_the_sanitizers(sanitized, tmp_path, name):
    case = HOSTILE[name]
    hdr, term, layers, _ = sc.parse_host_directional(run(sanitized, tmp_path, sc.host_directional_bytes(case, GOLDEN["srgb_table"])), case["width"], case["height"])
    far = case["depth"] == 0.0
    assert np.array_equal(hdr[far], case["emissive"][far]), name
    assert ((layers >= 0) & (layers <= 3)).all(), name
    if name == "map_of_one_texel":
        live = term[~far]
        assert np.isin(live, [0.0, 1.0]).all() or np.allclose(live[(live != 0) & (live != 1)], 1.0, atol=1e-6), "one texel: every tap compares alike"
