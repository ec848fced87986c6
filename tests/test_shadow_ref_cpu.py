"""CPU: tests/shadow_ref.py (float64 numpy) against the reference's shaders executed in fp32 (tests/golden/shadow_shader_v1.npz).  The
distance between the two is the size of an fp32 evaluation's own error; tests/golden/make_shadow_golden.py printed, and this test asserts:
    lit target, fp16 ulps beyond 1e-4   pcf 0.898, pcf_cascades 0.949, wide 0.795, wide_cascades 0.974, vsm 0.949, vsm_cascades 0.000
    moments, fp32 ulps                  resolve 0.500; down blur 4.287; up blur 3.773
Pixels on a knife edge of the depth compare (shadow_ref.KNIFE_EDGE) are left out and capped at 1 % of a case."""
import numpy as np
import pytest

import shadow_cases as sc
import shadow_ref

GOLDEN = sc.load_golden()
RECORDED = {"pcf/64x40": 0.898, "pcf_cascades/61x37": 0.949, "wide/61x37": 0.795, "wide_cascades/64x40": 0.974, "vsm/64x40": 0.949, "vsm_cascades/61x37": 0.000}
KNIFE_EDGES = {"wide_cascades/64x40": 1}


@pytest.mark.parametrize("name", list(sc.DIRECTIONAL))
def test_directional_light_against_the_executed_shader(name):
    case = sc.directional_case(GOLDEN, name)
    ref = shadow_ref.directional_light(case, GOLDEN["srgb_table"])
    edge = ref["edge"] <= shadow_ref.KNIFE_EDGE
    assert edge.sum() == KNIFE_EDGES.get(name, 0) and edge.sum() <= sc.KNIFE_EDGE_CAP * edge.size
    got = case["hdr"][..., :3].view(np.float16).astype(np.float64)
    distance = shadow_ref.ulp_distance(got, ref["hdr"])[~edge].max()
    assert distance <= RECORDED[name] + 0.0005, (name, distance)
    assert RECORDED[name] < 1.0
    # a pixel on a knife edge still lies between the shadowed and the unshadowed value
    lo, hi = np.minimum(ref["dark"], ref["lit"])[edge], np.maximum(ref["dark"], ref["lit"])[edge]
    assert (shadow_ref.ulp_distance(got[edge], np.clip(got[edge], lo, hi)) <= 1.0).all()
    assert np.array_equal(case["term"][ref["far"]], np.ones(int(ref["far"].sum()), np.float32))
    if case["cascaded"]:
        near, far, lerp, white = ref["cascade"]
        live = ~ref["far"]
        assert np.array_equal(case["layers"][..., 0][live], near[live]) and np.array_equal(case["layers"][..., 1][live], far[live])
        assert set(case["layers"][live].reshape(-1).tolist()) == {0, 1, 2, 3}, "every cascade is reached"
        assert (case["lerps"][..., 0][live] > 0).any() and (case["lerps"][..., 1][live] >= 1).any() and ((case["lerps"][..., 1][live] > 0) & (case["lerps"][..., 1][live] < 1)).any()


def test_the_cases_reach_their_rules():
    behind = sc.directional_case(GOLDEN, "pcf_cascades/61x37")
    pos = shadow_ref.world_position(behind["inv_view_projection"], behind["width"], behind["height"], behind["depth"])
    view_z = (np.float64(behind["camera_front"]) * (pos - np.float64(behind["camera_pos"]))).sum(-1)
    assert (view_z[behind["depth"] != 0.0] < 0.0).any(), "pixels behind the camera plane"
    plain = sc.directional_case(GOLDEN, "pcf/64x40")
    clip = shadow_ref.light_clip(plain["transforms"][:16], shadow_ref.world_position(plain["inv_view_projection"], plain["width"], plain["height"], plain["depth"]))
    live = plain["depth"] != 0.0
    assert (clip[live][:, 0] < 0.0).any() and (clip[live][:, 0] > 1.0).any(), "light-space positions left and right of the map"
    vsm = sc.directional_case(GOLDEN, "vsm/64x40")
    assert ((vsm["term"] > 0) & (vsm["term"] < 1)).any() and (vsm["term"] == 0).any() and (vsm["term"][vsm["depth"] != 0.0] == 1).any()
    moments = vsm["maps"].astype(np.float64)
    assert ((moments[..., 1] - moments[..., 0] ** 2) < 1e-5).any(), "variances below the floor"


def test_vsm_chain_against_the_executed_shaders():
    for name in sc.MOMENTS:
        assert shadow_ref.ulp32_distance(GOLDEN[f"{name}/out"], shadow_ref.vsm_moments(GOLDEN[f"{name}/depth"])).max() <= 0.5005
    worst_down = worst_up = 0.0
    for name in sc.BLURS:
        source, down, up = GOLDEN[f"{name}/in"], GOLDEN[f"{name}/down"], GOLDEN[f"{name}/up"]
        worst_down = max(worst_down, shadow_ref.ulp32_distance(down, shadow_ref.vsm_blur(source, down.shape[2], down.shape[1], False)).max())
        worst_up = max(worst_up, shadow_ref.ulp32_distance(up, shadow_ref.vsm_blur(down, up.shape[2], up.shape[1], True)).max())
    assert worst_down <= 4.2875 and worst_up <= 3.7735, (worst_down, worst_up)


def test_half_size_is_the_graphs_absolute_size_times_a_half():
    assert [sc.half_size(n) for n in (1, 2, 3, 17, 33, 2048)] == [1, 1, 1, 8, 16, 1024]
