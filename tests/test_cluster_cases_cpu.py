"""CPU: the cluster build on lights around, behind and beside the camera (tests/cluster_cases.py).

For every case: the oracle equals the reference's executed shaders bit for bit (all four shaders, binning in its plain, 64-lane and
32-lane forms); the case reaches the branches it was made for; and the final masks and ranges are conservative against float64
geometry -- the one check that is not the same algorithm again.  The GPU tests (test_gpu_cluster_cases.py) hold the kernels to the
same three statements."""
import ctypes as C

import numpy as np
import pytest

from granite_amd import synth
from oracle import oracle as orc
import cluster_cases as cc
from test_reference_shaders_cpu import ref, ptr  # noqa: F401  (the fixture: builds / loads oracle/_ref, skips without it)
from util import assert_words_equal_or_both_nan

P = C.c_void_p
NAMES = [n for n in cc.CASES if n != "box_dim"]


def shader_build(ref, b, subgroup):
    """The four reference shaders on the oracle-packed lights of build b, binning at `subgroup` (0: the plain form)."""
    for name, argtypes in (("ref_cluster_spot_transform", [P, P, C.c_int, P]), ("ref_cluster_setup", [P, P, P, P, P, C.c_int, P]),
                           ("ref_cluster_binning", [P, P, P, P, C.c_int]), ("ref_cluster_z_range", [P, C.c_int, C.c_int, P])):
        getattr(ref, name).argtypes = argtypes
    n = b["n"]
    spots, setup = np.zeros_like(b["spots"]), np.zeros_like(b["setup"])
    bitmask, ranges = np.zeros_like(b["bitmask"]), np.zeros_like(b["range"])
    ref.ref_cluster_spot_transform(ptr(b["rp"]), ptr(b["model"]), n, ptr(spots))
    ref.ref_cluster_setup(ptr(b["rp"]), ptr(b["prm"]), ptr(b["lights"]), ptr(b["type_mask"]), ptr(spots), n, ptr(setup))
    ref.ref_cluster_binning(ptr(b["prm"]), ptr(b["type_mask"]), ptr(setup), ptr(bitmask), subgroup)
    ref.ref_cluster_z_range(ptr(b["light_ranges"]), len(b["light_ranges"]), b["res"][2], ptr(ranges))
    return dict(spots=spots, setup=setup, bitmask=bitmask, range=ranges)


# The plain form runs one team of 32 real threads per cell and 32-light chunk: 50 s for 2000 lights.  It differs from the subgroup
# forms only in having no coarse tile test in front of the same per-cell test, so the larger sets run it on their first PLAIN_MAX lights.
PLAIN_MAX = 256


def check_shaders(ref, name, res, forms):
    for subgroup in forms:
        cam, descs = cc.case(name)
        if subgroup == 0:
            descs = descs[:PLAIN_MAX]
        b = cc.built(name, res) if subgroup == 64 else cc.build(cam, descs, res=res, subgroup_tile_h=subgroup // 8)
        got = shader_build(ref, b, subgroup)
        np.testing.assert_array_equal(got["spots"].view(np.uint32), b["spots"].view(np.uint32), err_msg="transformed spots")
        np.testing.assert_array_equal(got["setup"].view(np.uint32), b["setup"].view(np.uint32), err_msg="cull set-up")
        np.testing.assert_array_equal(got["bitmask"], b["bitmask"], err_msg=f"cell bitmask, subgroup size {subgroup}")
        np.testing.assert_array_equal(got["range"], b["range"], err_msg="slice ranges")
        c = cc.conservativeness(b, got["bitmask"], got["range"])
        assert c["point"][1] == 0 and c["spot"][1] == 0, f"executed shaders, subgroup size {subgroup}: {c}"


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_executed_shaders_bit_for_bit(ref, name):
    check_shaders(ref, name, cc.RES, (0, 64, 32))


def test_oracle_equals_executed_shaders_at_the_full_resolution(ref):
    check_shaders(ref, "box_around_camera", cc.RES_FULL, (64,))  # the form the kernels restate; 20 s


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_branches(name):
    got = cc.check_reach(name, cc.built(name))
    print(name, {k: (sorted(v) if isinstance(v, set) else v) for k, v in got.items()})


def test_lights_behind_the_camera():
    """Every slice interval and every slice's range is empty, and no spot is in any cell (all five vertices fail the w clip).  A POINT
    light behind the camera is in EVERY cell, in the reference shader as in the oracle: project_sphere_flat returns -1 / 0, +1 / 0, so
    the flag is 0 and the infinite bounding box passes everywhere; only its empty slice interval keeps it from being shaded."""
    b = cc.built("behind")
    cc.check_reach("behind", b)
    bits = cc.light_bits(b)
    n = b["n"]
    point = ((b["type_mask"][np.arange(n) >> 5] >> (np.arange(n) & 31)) & 1).astype(bool)
    assert point.any() and bits[..., point].all()
    assert (b["setup"][:n][point][:, 12] == 0).all()
    assert np.isinf(b["setup"][:n][point][:, :4]).all()


@pytest.mark.parametrize("name", NAMES)
def test_masks_and_ranges_are_conservative_against_float64_geometry(name):
    """Zero misses at SHRINK = 0.98 for points and for spots, but for the one class cluster_cases.SMALL_SPOT_AREA describes."""
    b = cc.built(name)
    c = cc.conservativeness(b)
    print(name, c)
    assert c["point"][1] == 0 and c["spot"][1] == 0, c
    if name in ("box_around_camera", "through_frustum", "on_axis"):
        assert c["point"][0] > 1000 and c["spot"][0] > 1000 and c["small_spot_samples"] == 0
    if name == "far_and_tiny":
        assert c["small_spot_samples"] > 0 and 0 < c["largest_area_missed"] < cc.SMALL_SPOT_AREA


def test_conservativeness_check_sees_a_dropped_bit_and_a_short_range():
    """The check itself: clear one light's bit in one cell it covers, or cut one slice's range short, and it reports misses."""
    b = cc.built("box_around_camera")
    bits = cc.light_bits(b)
    cover = bits.reshape(-1, b["n"]).sum(axis=0)
    zr = b["light_ranges"]
    # a light that is in a few cells and within the covered depth, so that samples do land in them
    clean = cc.conservativeness(b)
    assert clean["point"][1] == 0 and clean["spot"][1] == 0
    mask = b["bitmask"].copy()
    n32 = (b["n"] + 31) // 32
    words = mask.reshape(-1, n32)
    dropped = 0
    for light in np.flatnonzero((cover > 0) & (cover <= 8) & (zr[:b["n"], 0] <= zr[:b["n"], 1])):
        words[:, light >> 5] &= ~np.uint32(1 << (light & 31))
        dropped += 1
    assert dropped > 10
    c = cc.conservativeness(b, bitmask=mask)
    assert c["point"][1] + c["spot"][1] > 0
    ranges = b["range"].copy()
    ranges[:, 1] = np.minimum(ranges[:, 1], np.maximum(ranges[:, 0], 1) + 3)
    c = cc.conservativeness(b, ranges=ranges)
    assert c["point"][1] + c["spot"][1] > 0


def lit(cam, descs, gbuf, **kw):
    rp = cam.render_params()
    n, lights, model, tmask, _ = orc.pack_lights(descs, rp[99:102])
    prm = orc.cluster_params(rp, *cc.RES_FULL, n)
    cb = orc.cluster_build(rp, prm, lights, model, tmask, n, cc.RES_FULL[2])
    return orc.lighting(gbuf, rp, prm, lights, tmask, cb["bitmask"], cb["range"], synth.DIRECTIONAL_COLOR, synth.DIRECTIONAL_DIRECTION,
                        directional=False, **kw)


def test_clustered_lighting_equals_the_sum_over_all_lights():
    """Through the consumer, on the CPU: the oracle's clustered result on box_dim (lights around the camera, dim colours) under the
    far = 20 camera equals its brute-force sum over all lights.  Both add the same lights' terms in index order, so they are equal
    bit for bit unless culling dropped a light that contributes; the GPU test can then only fail through the kernels."""
    cam, descs = cc.case("box_dim")
    gbuf = synth.make_gbuffer(cam)
    clustered, brute = lit(cam, descs, gbuf), lit(cam, descs, gbuf, bruteforce=True)
    np.testing.assert_array_equal(clustered, brute)
    assert (clustered != gbuf["emissive"]).any(axis=-1).mean() > 0.5, "the lights must reach the surface"


def test_words_equal_or_both_nan():
    f = np.array([1.0, np.nan, 2.0, np.inf], np.float32)
    a, b = f.view(np.uint32).copy(), f.view(np.uint32).copy()
    assert assert_words_equal_or_both_nan(a, b) == 0
    b[1] = 0xffc00000
    a[1] = 0x7fc00001
    assert assert_words_equal_or_both_nan(a, b) == 1
    c = a.copy()
    c[2] ^= 1
    with pytest.raises(AssertionError):
        assert_words_equal_or_both_nan(c, b)
    c = a.copy()
    c[1] = 0x7f800000  # inf where the other side has NaN
    with pytest.raises(AssertionError):
        assert_words_equal_or_both_nan(c, b)
    # an integer word: 0xffffffff vs 0xffc00000 are both NaN patterns, but not the same integer
    integer = np.array([False, True, False, False])
    a[1], b[1] = 0xffffffff, 0xffc00000
    assert assert_words_equal_or_both_nan(a, b) == 1
    with pytest.raises(AssertionError):
        assert_words_equal_or_both_nan(a, b, integer_words=integer)
    b[1] = 0xffffffff
    assert assert_words_equal_or_both_nan(a, b, integer_words=integer) == 0
