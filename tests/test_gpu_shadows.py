"""GPU: gr_directional_light in the six shader variants, gr_vsm_moments and gr_vsm_blur on the cases of tests/golden/shadow_shader_v1.npz (the
reference's directional.frag with SHADOWS, resolve_vsm.frag and the two VSM blurs executed on the CPU), through the C ABI.

Far-plane pixels and every alpha are bit-identical to what was uploaded.

The bound on the values is not chosen from the kernel's output.  Recorded with the golden (tests/golden/make_shadow_golden.py prints it,
tests/test_shadow_ref_cpu.py asserts it): the executed shader (fp32) against tests/shadow_ref.py (float64), in fp16 ulps beyond an absolute
1e-4: pcf/64x40 0.898, pcf_cascades/61x37 0.949, wide/61x37 0.795, wide_cascades/64x40 0.974, vsm/64x40 0.949, vsm_cascades/61x37 0.000;
the host build of csrc/shadow_core.hpp against the executed shader 0 on every case.  Every figure is below one fp16 ulp; plus one ulp of the
output format that is the project's standing lighting bound, 2 fp16 ulps + 1e-4 (assert_rgba16f_close), which is what is asserted.  The wide
kernel's exp2 and division and the cascade's log2 did not need more.  Moments (fp32): resolve 0.500 fp32 ulps, down blur 4.287, up blur
3.773; plus one fp32 ulp each: 1.5, 5.287 and 4.773.

Knife edges: the depth compare is the one discontinuity.  A pixel is left out of the value comparison only if, in shadow_ref.py, a tap with a
non-zero weight has |ref_z - texel| <= 2^-20; it must still lie between the fully shadowed and the unshadowed value within the bound, and
such pixels may not exceed 1 % of a case (recorded: 1 of 2560 in wide_cascades/64x40, 0 in every other case)."""
import ctypes as C

import numpy as np
import pytest

import shadow_cases as sc
import shadow_device as dev
import shadow_ref
from granite_amd import capi, synth
from layout_images import Factory
from util import assert_rgba16f_close, rgba16f_mismatch

pytestmark = pytest.mark.gpu
GOLDEN = sc.load_golden()
MOMENTS_ULPS, DOWN_ULPS, UP_ULPS = 0.500 + 1.0, 4.287 + 1.0, 3.773 + 1.0
_REFERENCE = {}


def reference(name):
    """the float64 restatement of a case, computed once: the knife-edge mask and the two values a pixel on one must lie between"""
    if name not in _REFERENCE:
        ref = shadow_ref.directional_light(sc.directional_case(GOLDEN, name), GOLDEN["srgb_table"])
        _REFERENCE[name] = dict(edge=ref["edge"] <= shadow_ref.KNIFE_EDGE, lit=ref["lit"], dark=ref["dark"])
    return _REFERENCE[name]


def check_frame(name, case, got, layout=""):
    far = case["depth"] == 0.0
    assert np.array_equal(got[far], case["emissive"][far]), f"{name}: a far-plane pixel changed"
    assert np.array_equal(got[..., 3], case["emissive"][..., 3]), f"{name}: an alpha changed"
    ref = reference(name)
    edge = ref["edge"]
    name += layout
    assert edge.sum() <= sc.KNIFE_EDGE_CAP * edge.size, f"{name}: {edge.sum()} pixels on a knife edge"
    distance = shadow_ref.ulp_distance(got[..., :3].view(np.float16), case["hdr"][..., :3].view(np.float16))[~edge].max()
    print(f"{name}: the kernel against the executed shader: {distance:.3f} fp16 ulps beyond 1e-4; bit-identical channels {(got == case['hdr']).mean():.4f}; "
          f"{int(edge.sum())} pixels on a knife edge")
    assert_rgba16f_close(got[~edge], case["hdr"][~edge], what=name)
    if edge.any():
        value = got[edge][:, :3]
        lo, hi = np.minimum(ref["dark"], ref["lit"])[edge], np.maximum(ref["dark"], ref["lit"])[edge]
        inside = np.clip(value.view(np.float16).astype(np.float64), lo, hi)
        assert not rgba16f_mismatch(value, shadow_ref.to_half_bits(inside), 2.0, 1e-4).any(), f"{name}: a knife-edge pixel outside [shadowed, unshadowed]"


@pytest.mark.parametrize("name", list(sc.DIRECTIONAL))
def test_directional_light_against_the_executed_shader(gr, name):
    case = sc.directional_case(GOLDEN, name)
    args, imgs = dev.directional_args(case, dev.tight(gr))
    gr.directional_light(args)
    gr.sync()
    check_frame(name, case, dev.download_rgba16f(imgs["hdr"]))


def test_directional_light_into_a_target_of_its_own(gr):
    """hdr is not emissive: every pixel is written (the target starts as NaN), emissive is only read"""
    for name in ("pcf_cascades/61x37", "vsm/64x40"):
        case = sc.directional_case(GOLDEN, name)
        args, imgs = dev.directional_args(case, dev.tight(gr), in_place=False)
        gr.directional_light(args)
        gr.sync()
        check_frame(name, case, dev.download_rgba16f(imgs["hdr"]), " [own target]")
        assert np.array_equal(dev.download_rgba16f(imgs["emissive"]), case["emissive"]), name


def test_directional_light_on_padded_pitches_and_offset_pointers(gr):
    """every layout of tests/layout_images.py on four variants, guard bytes checked after each launch"""
    for assignment in ("wide256", "pad1", "mixed"):
        for name in ("wide_cascades/64x40", "pcf_cascades/61x37", "vsm_cascades/61x37", "wide/61x37"):
            case = sc.directional_case(GOLDEN, name)
            make = Factory(gr, assignment)
            args, imgs = dev.directional_args(case, make, in_place=assignment != "mixed")
            gr.directional_light(args)
            gr.sync()
            check_frame(name, case, dev.download_rgba16f(imgs["hdr"]), f" [{assignment}]")
            make.check()


def run_moments(gr, depth, make):
    h, w = depth.shape
    src = make(w, h, capi.FORMAT_D16_UNORM if depth.dtype == np.uint16 else capi.FORMAT_D32_SFLOAT, "in", "depth").upload(depth)
    out = make(w, h, capi.FORMAT_R32G32_SFLOAT, "out", "moments")
    gr.vsm_moments(src, out)
    gr.sync()
    return dev.download_moments(out)


def run_blur(gr, source, out_w, out_h, up, make):
    """one call per layer -> (layers, out_h, out_w, 2)"""
    planes = []
    for layer in source:
        src = make(layer.shape[1], layer.shape[0], capi.FORMAT_R32G32_SFLOAT, "in", "in").upload(layer)
        out = make(out_w, out_h, capi.FORMAT_R32G32_SFLOAT, "out", "out")
        gr.vsm_blur(src, out, up)
        gr.sync()
        planes.append(dev.download_moments(out))
    return np.stack(planes)


def assert_moments_close(got, want, ulps, what):
    distance = shadow_ref.ulp32_distance(got, want).max()
    print(f"{what}: {distance:.3f} fp32 ulps")
    assert distance <= ulps, what


def test_vsm_chain_against_the_executed_shaders(gr):
    for assignment in ("tight", "pad1", "mixed"):
        make = Factory(gr, assignment)
        for name in sc.MOMENTS:
            assert_moments_close(run_moments(gr, GOLDEN[f"{name}/depth"], make), GOLDEN[f"{name}/out"], MOMENTS_ULPS, f"{name} [{assignment}]")
        for name in sc.BLURS:
            source, down, up = GOLDEN[f"{name}/in"], GOLDEN[f"{name}/down"], GOLDEN[f"{name}/up"]
            assert_moments_close(run_blur(gr, source, down.shape[2], down.shape[1], False, make), down, DOWN_ULPS, f"{name} down [{assignment}]")
            assert_moments_close(run_blur(gr, down, up.shape[2], up.shape[1], True, make), up, UP_ULPS, f"{name} up [{assignment}]")
        make.check()


def test_unshadowed_directional_light_then_clustered_lighting_equals_the_fused_path(gr):
    """Moments with moments.x above every depth make vsm() exactly 1: gr_directional_light followed by gr_lighting(CLUSTERED) in place is then
    the frame the existing oracle lights in one go, under the existing lighting bound.  This ties the new kernel to the old path."""
    from gpu_scene import Scene
    from oracle import oracle as orc
    scene = Scene(333, 77, 700)
    clusters = orc.cluster_build(scene.rp, scene.prm, scene.lights, scene.model, scene.type_mask, scene.n, scene.res[2])
    want = orc.lighting(scene.gbuf, scene.rp, scene.prm, scene.lights, scene.type_mask, clusters["bitmask"], clusters["range"], synth.DIRECTIONAL_COLOR,
                        synth.DIRECTIONAL_DIRECTION)
    built = scene.build_clusters_gpu(gr)
    lighting, imgs = scene.lighting_args(gr, built, capi.LIGHTING_CLUSTERED_BIT)
    moments = capi.DeviceImage(gr, 4, 4, capi.FORMAT_R32G32_SFLOAT).upload(np.tile(np.float32([2.0, 4.0]), (4, 4, 1)))
    a = capi.DirectionalLightArgs()
    a.albedo, a.normal, a.pbr, a.depth, a.emissive, a.hdr = lighting.albedo, lighting.normal, lighting.pbr, lighting.depth, lighting.hdr, lighting.hdr
    a.inv_view_projection[:] = list(lighting.inv_view_projection)
    C.memmove(C.byref(a.directional), C.byref(lighting.directional), C.sizeof(capi.PushDirectional))
    a.flags = capi.LIGHTING_AMBIENT_FALLBACK_BIT
    a.mode, a.layers = capi.SHADOW_VSM, 1
    a.shadow_maps[0] = moments.desc
    a.transforms[0][:] = [0.0] * 12 + [0.5, 0.5, 0.5, 1.0]  # every position lands on (0.5, 0.5, 0.5)
    gr.directional_light(a)
    gr.check(gr.lib.gr_lighting(gr.handle, None, lighting))
    gr.sync()
    got = imgs["hdr"].download()
    sky = scene.gbuf["depth"] == 0.0
    np.testing.assert_array_equal(got[sky], scene.gbuf["emissive"][sky])
    np.testing.assert_array_equal(got[..., 3], scene.gbuf["emissive"][..., 3])
    assert_rgba16f_close(got, want, ulps=2.0, abs_tol=1e-4, what="directional + clustered against the oracle's fused frame")
