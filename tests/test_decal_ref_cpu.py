"""CPU: tests/decal_ref.py against the reference's decal shaders executed on the CPU (tests/golden/decal_shader_v1.npz, recorded by
tests/golden/make_decal_golden.py): the binning masks and the z ranges word for word on every case and resolution, the apply as float colour
before the 8-bit store, bit for bit, and which pixels a decal was fetched for.  Also asserts, per apply case, the cap the GPU test relies
on: the pixels within the margin of a decal's faces are at most 0.5 % of the case's decal-covered pixels."""
import numpy as np
import pytest

import decal_cases as dc
import decal_ref as ref

GOLDEN = dc.load_golden()
LEFT_OUT_CAP = 0.005


@pytest.mark.parametrize("name", dc.BINNING_CASES + list(dc.APPLY_CASES))
def test_binning_and_ranges_equal_the_executed_shaders(name):
    case = dc.golden_case(GOLDEN, name)
    assert np.array_equal(ref.binning(case["prm"], case["mvps"]), GOLDEN[f"{name}/bitmask"])
    assert np.array_equal(ref.z_ranges(case["intervals"], dc.RES_Z), GOLDEN[f"{name}/range"])


@pytest.mark.parametrize("name", dc.APPLY_CASES)
def test_apply_equals_the_executed_shader(name):
    case = dc.golden_case(GOLDEN, name)
    got = ref.apply(case)
    assert np.array_equal(got["touched"], GOLDEN[f"{name}/touched"])
    assert np.array_equal(got["colour"].view(np.uint32), GOLDEN[f"{name}/colour"].view(np.uint32))
    covered, margin = int(got["touched"].sum()), 64.0 * got["uvw_error"]
    left_out = int((got["edge_distance"] < margin).sum())
    print(f"{name}: {covered} covered pixels, margin {margin:.3g}, {left_out} within it")
    assert covered > 0 and left_out <= LEFT_OUT_CAP * covered


@pytest.mark.parametrize("name", dc.APPLY_CASES)
def test_host_functions_equal_the_reference_math_library(name):
    """sort key, decal_z_range, mvp and world_to_texture against what the reference's SIMD::transform_aabb / get_center, SIMD::mul, to_mat4,
    inverse and mat_affine(mat4) gave on the same world transforms (stored by the generator), bit for bit"""
    from granite_amd import synth
    case = dc.golden_case(GOLDEN, name)
    rp = synth.Camera(case["width"], case["height"]).render_params()
    rows = GOLDEN[f"{name}/host/world_rows"]
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert np.array_equal(bits(ref.host_sort_keys(rows, rp[99:102])), bits(GOLDEN[f"{name}/host/sort_keys"]))
    assert np.array_equal(bits([ref.decal_z_range(r, rp[96:99], rp[99:102]) for r in rows]), bits(GOLDEN[f"{name}/host/z_range"]))
    assert np.array_equal(bits(np.stack([ref.host_mvp(rp[32:48], r) for r in rows])), bits(GOLDEN[f"{name}/host/mvps"]))
    assert np.array_equal(bits(np.stack([ref.host_world_to_texture(r) for r in rows])), bits(GOLDEN[f"{name}/host/world_to_texture"]))
    extent = ref.z_slice_extent(rp[103], dc.RES_Z)
    intervals = np.array([ref.compute_uint_range(lo, hi, extent, dc.RES_Z) for lo, hi in GOLDEN[f"{name}/host/z_range"]], np.uint32)
    assert np.array_equal(intervals, case["intervals"]), "the stored slice intervals are those of the reference's z ranges"


def test_cases_rebuild_to_the_stored_inputs():
    """the golden file's inputs are what tests/decal_cases.py builds today, up to the last bit of the float64 geometry they are rounded from"""
    for name in dc.APPLY_CASES:
        built, stored = dc.apply_case(name), dc.golden_case(GOLDEN, name)
        assert built["prm"]["num_decals"] == stored["prm"]["num_decals"] and built["albedo"].shape == stored["albedo"].shape
        np.testing.assert_allclose(built["decal_rows"], stored["decal_rows"], rtol=1e-5, atol=1e-6)


def test_mask_range_is_the_shader_function():
    """cluster_mask_range at its edges: an empty range, a range inside one chunk, one that spans chunks"""
    full = np.uint32(0xFFFFFFFF)
    assert ref.mask_range(full, 0xFFFFFFFF, 0, 0) == 0
    assert ref.mask_range(full, 3, 5, 0) == 0b111000
    assert ref.mask_range(full, 3, 40, 0) == 0xFFFFFFF8 and ref.mask_range(full, 3, 40, 32) == 0x1FF
    assert ref.mask_range(full, 0, 31, 0) == full and ref.mask_range(full, 64, 70, 32) == 0
