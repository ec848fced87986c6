"""GPU: gr_cluster_binning_decal, the decal z ranges (gr_cluster_z_range over a second pair of buffers) and gr_decal_apply on the cases of
tests/golden/decal_shader_v1.npz (the reference's decal shaders executed on the CPU).

Binning and z ranges: word for word on every case and resolution; the words past the end still hold poison.

Apply, against the stored float colour put through the sRGB store: pixels no decal reaches, far-plane pixels and every alpha byte equal the
input byte for byte; pixels inside decals are within 1 code value per channel.  A pixel is left out only if, for one of its candidate decals,
| |uvw| - 0.5 | is below a margin of 64 x the largest |uvw_fp32 - uvw_fp64| that tests/decal_ref.py shows on that case -- taken from the
reference alone and printed -- and at most 0.5 % of a case's decal-covered pixels may be left out (tests/test_decal_ref_cpu.py asserts
that every case meets the cap).  Each case runs twice in one process on a fresh copy of the albedo, with equal bytes both times."""
import ctypes as C

import numpy as np
import pytest

import decal_cases as dc
import decal_device as dev
import decal_ref as ref

pytestmark = pytest.mark.gpu
GOLDEN = dc.load_golden()
LEFT_OUT_CAP = 0.005


@pytest.mark.parametrize("name", dc.BINNING_CASES + list(dc.APPLY_CASES))
def test_binning_and_z_ranges_equal_the_executed_shaders(gr, name):
    case = dc.golden_case(GOLDEN, name)
    words, tail = dev.binning(gr, case)
    assert np.array_equal(words, GOLDEN[f"{name}/bitmask"]), f"{name}: {(words != GOLDEN[f'{name}/bitmask']).sum()} bitmask words differ"
    assert np.all(tail == dev.POISON), f"{name}: words past the bitmask's end were written"
    ranges, tail = dev.z_ranges(gr, case, dc.RES_Z)
    assert np.array_equal(ranges, GOLDEN[f"{name}/range"]), name
    assert np.all(tail == dev.POISON), f"{name}: words past the range buffer's end were written"


@pytest.mark.parametrize("name", dc.APPLY_CASES)
def test_apply_against_the_executed_shader(gr, name):
    case = dc.golden_case(GOLDEN, name)
    mine = ref.apply(case)
    margin = 64.0 * mine["uvw_error"]
    left_out = mine["edge_distance"] < margin
    touched = GOLDEN[f"{name}/touched"]
    covered = int(touched.sum())
    print(f"{name}: margin {margin:.3g} (largest |uvw_fp32 - uvw_fp64| {mine['uvw_error']:.3g}), {int(left_out.sum())} of {covered} covered pixels left out")
    assert int(left_out.sum()) <= LEFT_OUT_CAP * covered
    albedo = np.asarray(case["albedo"], np.uint32)
    want = dev.reference_bytes(GOLDEN[f"{name}/colour"], albedo, touched)
    scene = dev.ApplyScene(gr, case)
    first, second = scene.run(), scene.run()
    assert np.array_equal(first, second), f"{name}: two runs on the same input differ"
    assert np.array_equal(first >> 24, albedo >> 24), f"{name}: an alpha byte changed"
    far = np.asarray(case["depth"]) == 0
    assert np.array_equal(first[far], albedo[far]), f"{name}: a far-plane pixel was written"
    outside = ~touched & ~left_out
    assert np.array_equal(first[outside], albedo[outside]), f"{name}: {(first[outside] != albedo[outside]).sum()} pixels outside every decal changed"
    inside = touched & ~left_out
    channels = lambda a: np.stack([(a >> s) & 255 for s in (0, 8, 16)], -1).astype(np.int64)
    error = np.abs(channels(first[inside]) - channels(want[inside]))
    print(f"{name}: largest difference inside decals {int(error.max()) if error.size else 0} code values, {int((error > 0).sum())} of {error.size} channel values differ")
    assert error.max() <= 1


def test_zero_decals_and_refusals_on_the_device(gr):
    case = dc.golden_case(GOLDEN, "count_0/8x8")
    words, tail = dev.binning(gr, case)
    assert len(words) == 0 and np.all(tail == dev.POISON)
    scene = dev.ApplyScene(gr, dc.golden_case(GOLDEN, "two_overlap"))
    scene.args.cluster.num_decals = scene.args.cluster.num_decals_32 = 0
    assert np.array_equal(scene.run(), np.asarray(scene.case["albedo"], np.uint32))
    scene = dev.ApplyScene(gr, dc.golden_case(GOLDEN, "two_overlap"))
    scene.args.textures = None
    assert gr.lib.gr_decal_apply(gr.handle, None, C.byref(scene.args)) == -1  # GR_ERR_INVALID_ARGUMENT
    assert b"textures" in gr.lib.gr_last_error(gr.handle)
