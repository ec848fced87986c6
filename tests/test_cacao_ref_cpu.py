"""CPU: tests/cacao_ref.py itself -- the yardstick of the SSAO kernels -- before anything is held to it.  Non-vacuity of the cases is
asserted, not assumed; a camera-facing plane, a concave and a convex corner check that the formulae were not misread twice; and the final
image of the float32 chain is measured against the float64 chain, which is where tests/cacao_chain.py's whole-pass bounds come from."""
import numpy as np
import pytest

import cacao_cases as cc
import cacao_chain as chain
import cacao_ref as cr


def test_constant_block_layout():
    names = cr.CONSTANTS_DTYPE.fields
    assert cr.CONSTANTS_DTYPE.itemsize == 384
    assert [names[n][1] for n in ("EffectRadius", "PassIndex", "PatternRotScaleMatrices", "NormalsUnpackMul", "SSAOBufferDimensions", "DepthBufferOffset",
                                  "ImportanceMapDimensions", "NormalsWorldToViewspaceMatrix")] == [48, 100, 112, 192, 208, 240, 272, 320]


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_flagged_share_and_edges(case):
    for quality in cc.QUALITIES:
        r = chain.reference(case, quality)
        assert r["info"]["flag"].mean() <= chain.FLAG_SHARE_LIMIT
        if quality == cr.QUALITY_HIGHEST:
            assert r["base_info"]["flag"].mean() <= chain.FLAG_SHARE_LIMIT
            assert r["importance"].max() > 0 and r["load_counter"] > 0
        assert (r["ping"][..., 1] != 255).any(), "packed edges are all 255"
        assert r["info"]["outside"], "no tap lands outside the image"
        assert r["output"].min() < 255, "no occlusion anywhere"


def test_cases_reach_every_mechanism():
    taps = np.concatenate([chain.reference(case, cr.QUALITY_HIGHEST)["info"]["taps"].reshape(-1) for case in cc.CASES])
    assert (taps == 1).any() and (taps == cr.FLEXIBLE_TAPS).any(), "Q3 texels at 5 + 1 and at 32 tap pairs"
    assert max(chain.reference(case, q)["info"]["max_mip"] for case in cc.CASES for q in cc.QUALITIES) >= 2, "no tap reads mip 2 or 3"
    odd = chain.reference(cc.CASES[3], cr.QUALITY_HIGH)  # 61 x 45
    assert [m.shape for m in odd["depth_mips"]] == [(4, 23, 31), (4, 11, 15), (4, 5, 7), (4, 2, 3)]
    tiny = chain.reference(cc.CASES[-1], cr.QUALITY_HIGH)  # 16 x 16
    assert tiny["depth_mips"][3].shape == (4, 1, 1)
    wide = chain.reference(cc.CASES[7], cr.QUALITY_HIGHEST)  # 130 x 98
    assert wide["importance"].shape == (25, 33)


def whole(scene, quality=cr.QUALITY_HIGHEST, size=(64, 48), blur_passes=2):
    w, h = size
    depth, normal = scene
    return cr.chain(depth, normal, cc.constants(w, h, "survey", "reference", quality), quality, blur_passes)["output"]


@pytest.mark.parametrize("quality", cc.QUALITIES, ids=lambda q: f"q{q}")
def test_camera_facing_plane_is_unoccluded(quality):
    out = whole(cc.plane_scene(cc.camera("survey", 64, 48)), quality)
    assert out.min() == 255 and out.max() == 255


@pytest.mark.parametrize("quality", cc.QUALITIES, ids=lambda q: f"q{q}")
def test_concave_corner_darkens_towards_the_crease_and_convex_does_not(quality):
    cam = cc.camera("survey", 64, 48)
    concave = whole(cc.corner_scene(cam, True), quality).astype(np.float64)
    convex = whole(cc.corner_scene(cam, False), quality)
    # column means over the middle rows, left half: monotonically darker towards the crease at column 32, and mirrored on the right
    rows = concave[12:36]
    left, right = rows[:, :32].mean(axis=0), rows[:, 32:][:, ::-1].mean(axis=0)
    for side in (left, right):
        assert np.all(np.diff(side) <= 0.5), side  # half a code of slack for the dither of the five rotations
        assert side[0] - side[-1] >= 20, side
    assert concave[:, 30:34].mean() < 200
    assert convex.min() >= 250, int(convex.min())


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_float32_against_float64(case):
    """the figures behind cacao_chain.WHOLE_PASS_MEASURED: how far the rounding of fp32 alone moves the final image"""
    for quality in cc.QUALITIES:
        a, b = chain.reference(case, quality)["output"], chain.reference(case, quality, 2, "float64")["output"]
        distance = chain.codes(a, b)
        largest, mean = int(distance.max()), float(distance.mean())
        print(f"{cc.case_id(case)} q{quality}: float32 against float64 largest {largest} code(s), mean {mean:.5f}")
        # another numpy may round pow and log2 in another last bit: the measurement taken again has to stay within what the device is given
        bound_largest, bound_mean = chain.whole_pass_bound(case, quality)
        assert largest <= bound_largest and mean <= bound_mean, (largest, mean, chain.WHOLE_PASS_MEASURED[(cc.case_id(case), quality)])
