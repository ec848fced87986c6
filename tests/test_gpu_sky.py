"""GPU: gr_sky_apply and gr_sky_cube on the cases of tests/golden/sky_shader_v1.npz (the reference's skybox.frag, both HAVE_EMISSIVE
settings, and lights/volumetric_light_setup_sky.comp executed on the CPU), through the C ABI, in both emissive formats.

The zero mask (the earth and atmosphere decisions, made of + - * sqrt) is exact.  Pixels with depth != 0 are bit-identical to what was
uploaded, the alpha of an RGBA16F texel is untouched, and the guard bytes behind every row and behind both images are unchanged.

The bound on the values is not chosen from the kernel's output.  Two fp32 evaluations of the shader's text in the shader's order differ
through exp and pow alone; recorded with the golden (tests/golden/make_sky_golden.py prints it, tests/test_sky_ref_cpu.py and
tests/test_sky_core_cpu.py assert it): the executed shader against tests/sky_ref.py is at most 0.795 fp16 ulps beyond an absolute 1e-4
(horizon/40x24 and mie_peak/136x72; 0 on every other case), against the host build of csrc/sky_core.hpp 0 on every case, cube colours
bit for bit.  Every figure is below one fp16 ulp, so the bound is the project's standing assert_rgba16f_close, 2 fp16 ulps + 1e-4, for
the reason given in tests/test_gpu_env_bake.py: one ulp of evaluation difference and the store's own rounding may fall on either side of
a half's rounding boundary.  For B10G11R11 the same argument gives one step of the stored channel (6 or 5 mantissa bits: a step is 16 or
32 half ulps)."""
import ctypes as C

import numpy as np
import pytest

import sky_cases as sc
import sky_device as dev
from granite_amd import capi
from util import assert_rgba16f_close

pytestmark = pytest.mark.gpu
GOLDEN = sc.load_golden()
RGBA16F, PACKED = capi.FORMAT_R16G16B16A16_SFLOAT, capi.FORMAT_B10G11R11_UFLOAT_PACK32
INVALID = -1


def check_apply(gr, name, fmt, pad, negative_zero=False):
    case = sc.apply_case(GOLDEN, name)
    h, w = case["height"], case["width"]
    far = case["depth"] == 0.0
    depth_values = np.where(far, np.float32(-0.0), case["depth"]).astype(np.float32) if negative_zero else None
    uploaded = dev.emissive_input(np.random.default_rng(7), w, h, fmt)
    texels, guard, depth_after = dev.apply(gr, case, fmt, uploaded, pad, depth_values)
    assert (guard == dev.GUARD).all(), f"{name}: bytes between rows or behind an image were written"
    assert np.array_equal(depth_after.view(np.float32).reshape(h, w).view(np.uint32), (case["depth"] if depth_values is None else depth_values).view(np.uint32))
    if fmt == RGBA16F:
        got = texels.view(np.uint16).reshape(h, w, 4)
        assert np.array_equal(got[~far], uploaded[~far]), f"{name}: a pixel with depth != 0 changed"
        assert np.array_equal(got[..., 3], uploaded[..., 3]), f"{name}: an alpha changed"
        assert np.array_equal((got[..., :3] == 0).all(axis=-1) & far, case["zero"]), f"{name}: the zero mask"
        want = sky_ref_half(case["out"])
        assert_rgba16f_close(got[far][:, :3], want[far], what=name)
    else:
        got = texels.view(np.uint32).reshape(h, w)
        assert np.array_equal(got[~far], uploaded[~far]), f"{name}: a pixel with depth != 0 changed"
        assert np.array_equal((got == 0) & far, case["zero"]), f"{name}: the zero mask"
        want = np.stack([dev.ufloat_codes(case["out"][..., 0], 6), dev.ufloat_codes(case["out"][..., 1], 6), dev.ufloat_codes(case["out"][..., 2], 5)], -1)
        steps = np.abs(dev.unpack_codes(got)[far] - want[far])
        print(f"{name}: largest difference {int(steps.max(initial=0))} steps of the stored channel")
        assert steps.max(initial=0) <= 1, name


def sky_ref_half(values):
    with np.errstate(over="ignore"):
        return np.asarray(values, np.float32).astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("fmt", [RGBA16F, PACKED], ids=["rgba16f", "b10g11r11"])
@pytest.mark.parametrize("name", list(sc.PROCEDURAL) + list(sc.TEXTURED))
def test_apply_against_the_executed_shader(gr, name, fmt):
    check_apply(gr, name, fmt, (0, 0))


@pytest.mark.parametrize("fmt", [RGBA16F, PACKED], ids=["rgba16f", "b10g11r11"])
@pytest.mark.parametrize("name", ["up_low_sun/67x35", "cube16_odd/67x35"])
def test_apply_with_padded_pitches(gr, name, fmt):
    check_apply(gr, name, fmt, (24, 12))


@pytest.mark.parametrize("name", ["below_dusk/67x35", "cube16_crossing/40x24"])
def test_a_depth_of_negative_zero_is_far(gr, name):
    check_apply(gr, name, RGBA16F, (8, 4), negative_zero=True)


def run_sky_cube(gr, case):
    texels = 6 * case["size"] ** 2
    out = capi.DeviceBuffer(gr, texels * 8 + dev.TAIL_BYTES).upload(np.full(texels * 8 + dev.TAIL_BYTES, dev.GUARD, np.uint8))
    gr.sky_cube(out, case["size"], case["sun_color"], case["camera_y"], case["sun_direction"])
    gr.sync()
    return out, out.download(np.uint8)


@pytest.mark.parametrize("name", list(sc.CUBES))
def test_sky_cube_against_the_executed_shader(gr, name):
    case = sc.cube_case(GOLDEN, name)
    texels = 6 * case["size"] ** 2
    _, raw = run_sky_cube(gr, case)
    assert (raw[texels * 8:] == dev.GUARD).all(), f"{name}: bytes behind the chain were written"
    got = raw[:texels * 8].view(np.uint16).reshape(6, case["size"], case["size"], 4)
    assert np.array_equal(got == 0, case["out"] == 0.0), f"{name}: the zero mask"
    assert (got[..., 3] == 0x3c00).all(), f"{name}: alpha is 1.0"
    assert_rgba16f_close(got, sky_ref_half(case["out"]), what=name)


def test_sky_cube_feeds_env_diffuse(gr):
    case = sc.cube_case(GOLDEN, "sky_cube/8")
    cube, _ = run_sky_cube(gr, case)
    out = capi.DeviceBuffer(gr, 6 * 4 * 4 * 8)
    gr.env_diffuse(cube, case["size"], 1, out, 4)
    gr.sync()
    irradiance = out.download(np.uint16).view(np.float16).reshape(6, 4, 4, 4).astype(np.float32)
    assert np.isfinite(irradiance).all() and (irradiance[..., :3] > 0.0).any() and (irradiance[..., :3] >= 0.0).all()


# ---- refusals: each returns before a launch, with the argument and the rule in gr_last_error -----------------------------------------------
def refused(gr, code, *words):
    message = gr.lib.gr_last_error(gr.handle).decode()
    assert code == INVALID, (code, message)
    for word in words:
        assert word in message, (word, message)


def test_apply_refusals(gr):
    case = sc.apply_case(GOLDEN, "cube8_two_levels/40x24")
    w, h = case["width"], case["height"]
    emissive = capi.DeviceImage(gr, w, h, RGBA16F)
    before = emissive.download().copy()
    depth = capi.DeviceImage(gr, w, h, capi.FORMAT_D32_SFLOAT).upload(np.ascontiguousarray(case["depth"]))
    cube = capi.DeviceBuffer(gr, case["cube"].nbytes).upload(case["cube"])
    call = lambda args: gr.lib.gr_sky_apply(gr.handle, None, C.byref(args))
    fresh = lambda: dev.sky_args(emissive, depth, case, cube)

    refused(gr, gr.lib.gr_sky_apply(gr.handle, None, None), "gr_sky_apply", "args")
    for fmt in (capi.FORMAT_R8G8B8A8_UNORM, capi.FORMAT_R32_SFLOAT, capi.FORMAT_D32_SFLOAT):
        a = fresh()
        a.emissive.format = fmt
        refused(gr, call(a), "gr_sky_apply", "emissive", "format")
    a = fresh()
    a.depth.format = capi.FORMAT_R32_SFLOAT
    refused(gr, call(a), "gr_sky_apply", "depth", "format")
    for field, value in (("width", w - 1), ("height", h + 1)):
        a = fresh()
        setattr(a.depth, field, value)
        refused(gr, call(a), "gr_sky_apply", "depth", "width and height")
    a = fresh()
    a.emissive.ptr = None
    refused(gr, call(a), "gr_sky_apply", "emissive", "null pointer")
    a = fresh()
    a.depth.ptr = None
    refused(gr, call(a), "gr_sky_apply", "depth", "null pointer")
    a = fresh()
    a.emissive.pitch_bytes = w * 8 - 8
    refused(gr, call(a), "gr_sky_apply", "emissive", "pitch_bytes")
    a = fresh()
    a.cube.ptr = None
    refused(gr, call(a), "gr_sky_apply", "cube.ptr", "null pointer")
    a = fresh()
    a.cube.size = 0
    refused(gr, call(a), "gr_sky_apply", "cube.size")
    a = fresh()
    a.cube.levels = 0
    refused(gr, call(a), "gr_sky_apply", "cube.levels")
    a = fresh()
    a.cube.levels = 5  # an 8-texel cube's full chain has 4
    refused(gr, call(a), "gr_sky_apply", "cube.levels", "beyond the chain")
    a = fresh()
    a.cube.ptr = cube.ptr + 8
    refused(gr, call(a), "gr_sky_apply", "cube.ptr", "16-byte aligned")
    gr.sync()
    assert np.array_equal(emissive.download(), before), "a refused call wrote"


def test_sky_cube_refusals(gr):
    out = capi.DeviceBuffer(gr, 6 * 8 * 8 * 8)
    params = capi.SkyCubeParams()
    refused(gr, gr.lib.gr_sky_cube(gr.handle, None, None, 8, C.byref(params)), "gr_sky_cube", "out_chain")
    refused(gr, gr.lib.gr_sky_cube(gr.handle, None, out.ptr, 8, None), "gr_sky_cube", "params")
    refused(gr, gr.lib.gr_sky_cube(gr.handle, None, out.ptr, 0, C.byref(params)), "gr_sky_cube", "size")
    refused(gr, gr.lib.gr_sky_cube(gr.handle, None, out.ptr, 16385, C.byref(params)), "gr_sky_cube", "size")
    refused(gr, gr.lib.gr_sky_cube(gr.handle, None, out.ptr + 8, 8, C.byref(params)), "gr_sky_cube", "16-byte aligned")
