"""GPU: the launchers of the image-space chain on padded pitches and offset pointers (tests/layout_images.py), each against the CPU oracle with
the comparator of its own test file: lighting, the bloom / luminance / tonemap chain and its fused forms, FXAA, SMAA, TAA, blit, FSR, PQ10, HiZ, SPD,
SSR, the decal apply pass, the RGB888 transport form, and the image arguments of the environment bake and of the ocean's bake and mipmap passes.

Every case runs under four layout assignments: `tight` (the control: what capi.DeviceImage hands over), all images `wide256` (the alignment-gated
fast forms stay selected, pitch != width * texel), all images `pad1` (every other row misaligned at an even width), and `mixed` (inputs and
read-modify-write images `off1`, outputs `pad1`).  After the launches every output's guard bytes must hold their fill and every pure input must
be unchanged, guards and texels.  The references are computed once per family and size and never written to.

Which form each assignment selects at the even sizes, read from the launchers' own conditions (tight / wide256 / pad1 / mixed):

    gr_lighting, pairs_aligned (256 x 128, 130 x 75)           two-pixel / two-pixel / one-pixel / one-pixel
    gr_smaa_neighbor_blend, `wide` (320 x 180)                 four-pixel / four-pixel / one-pixel / one-pixel
    k_fxaa_fast, 8-byte staging of interior tiles (320 x 180)  on / on / off / off
    k_tonemap, `full` 16-byte rows (256 x 256)                 every row / every row / every other row of hdr, every fourth of out / the same
    gr_hiz, p.aligned (256 x 64)                               16-byte rows / 16-byte rows / single texels / single texels
    bloom threshold and downsample, *_is_exact (256 x 256)     2:1 stencils / 2:1 stencils / generic taps / generic taps
    gr_bloom_*_supported (256 x 256)                           all five / all five / all but down_head and pyramid / all but down_head and pyramid

(The anti-aliasing launchers pick their tile kernels by size, not by layout: all four sizes here take them.)"""
import ctypes as C

import numpy as np
import pytest

import decal_cases as dc
import decal_device
import decal_ref
from gpu_scene import Scene
from granite_amd import capi, synth
from granite_amd.data import expand_sssr_dither, load_brdf_lut, load_sssr_noise_base, load_smaa_luts
from layout_images import Factory
from ocean_cases import BAKE, MIPMAP
from ocean_cases import GOLDEN as OCEAN_GOLDEN
from ocean_chain import FORMATS as OCEAN_FORMATS
from ocean_chain import as_struct
from oracle import oracle as orc
from test_gpu_aa import taa_inputs
from test_gpu_env_bake import GOLDEN as ENV_GOLDEN
from test_gpu_env_bake import chain_buffer, close, read_chain
from test_gpu_fsr import image as fsr_image
from test_gpu_hiz import depth_image, z_transform
from test_gpu_lighting import ambient_occlusion_image
from test_gpu_packed_hdr import codes_close
from test_gpu_spd import source as spd_source
from util import assert_rgba16f_close, assert_rgba8_close, close_up_scene, half_bits_to_f32, rgba16f_mismatch

pytestmark = pytest.mark.gpu

ASSIGNMENTS = ("tight", "wide256", "pad1", "mixed")
F16, B10 = capi.FORMAT_R16G16B16A16_SFLOAT, capi.FORMAT_B10G11R11_UFLOAT_PACK32
SRGB, UNORM = capi.FORMAT_R8G8B8A8_SRGB, capi.FORMAT_R8G8B8A8_UNORM
D32, A2, RG8, R8 = capi.FORMAT_D32_SFLOAT, capi.FORMAT_A2B10G10R10_UNORM_PACK32, capi.FORMAT_R8G8_UNORM, capi.FORMAT_R8_UNORM
LEVELS = ("threshold", "d0", "d1", "d2", "d3", "u2", "u1", "u0")
SCALES = dict(threshold=0.5, d0=0.25, d1=0.125, d2=0.0625, d3=0.03125, u2=0.0625, u1=0.125, u0=0.25)

_REFERENCES = {}


def reference(key, compute):
    """The oracle's answer for `key`, computed on first use and shared by the layouts; read-only for the tests."""
    if key not in _REFERENCES:
        _REFERENCES[key] = compute()
    return _REFERENCES[key]


def per_assignment(*cases, ids=None):
    """One test per layout assignment -- the ids list each family against the four of them -- with the family's cases (sizes, qualities,
    formats) run inside it, each named on stdout before it runs so that a failure says which one it was."""
    def wrap(case_function):
        @pytest.mark.parametrize("assignment", ASSIGNMENTS)
        def test(gr, assignment):
            for index, case in enumerate(cases):
                print(f"{case_function.__name__}[{assignment}] case {ids[index] if ids else case}")
                case_function(gr, assignment, *case)
        test.__name__, test.__doc__ = case_function.__name__, case_function.__doc__
        return test
    return wrap


# ---- post chain ---------------------------------------------------------------------------------------------------------------------
def chain_reference(w, h, packed):
    def compute():
        hdr = synth.make_hdr(w, h)
        if packed:
            hdr = orc.quantize_b10g11r11(hdr)  # a packed texel is exactly a half float: the passes read it like its RGBA16F expansion
        state = {}
        return hdr, [orc.hdr_chain(hdr, state) for _ in range(2)]
    return reference(("chain", w, h, packed), compute)


def banded(height, bands):
    """The row bands one launch is split into: the whole level, or two bands that meet at a third of it."""
    first = max(height // 3, 1)
    return [(0, first), (first, height - first)] if bands and height > first else [None]


def run_chain_frame(gr, make, hdr_bits, packed, out_fmt, state, bands=False):
    """run_chain_gpu of tests/test_gpu_post.py with every image from `make`, and, with `bands`, every *_rows launch issued as two row bands."""
    h, w = hdr_bits.shape[:2]
    lum_lerp, fb_lerp = orc.frame_lerps(0.01)
    size = {name: orc.level_size(w, h, s) for name, s in SCALES.items()}
    hdr = make(w, h, B10 if packed else F16, "in", "hdr").upload(orc.pack_b10g11r11(hdr_bits) if packed else hdr_bits)
    l = {name: make(*size[name], F16, "out", name) for name in LEVELS if name != "d3"}
    out = make(w, h, out_fmt, "out", "tonemapped")
    if "lum" not in state:
        state.update(lum=capi.DeviceBuffer(gr, 12), d3=[make(*size["d3"], F16, "out", "d3.0"), make(*size["d3"], F16, "out", "d3.1")], frame=0)
    lum = state["lum"].ptr
    l["d3"] = state["d3"][state["frame"] & 1]
    history = state["d3"][(state["frame"] & 1) ^ 1] if state["frame"] > 0 else None
    for rows in banded(size["threshold"][1], bands):
        gr.bloom_threshold(hdr, l["threshold"], lum, rows=rows)
    for src, dst in zip(LEVELS[:4], LEVELS[1:5]):
        for rows in banded(size[dst][1], bands):
            gr.bloom_downsample(l[src], l[dst], history if dst == "d3" else None, fb_lerp if dst == "d3" else 0.0, rows=rows)
    gr.luminance(l["d3"], lum, lum_lerp)
    for src, dst in zip(LEVELS[4:7], LEVELS[5:8]):
        for rows in banded(size[dst][1], bands):
            gr.bloom_upsample(l[src], l[dst], rows=rows)
    for rows in banded(h, bands):
        gr.tonemap(hdr, l["u0"], out, lum, rows=rows)
    gr.sync()
    state["frame"] += 1
    got = {name: image.download() for name, image in l.items()}
    got["tonemapped"], got["lum"] = out.download(), state["lum"].download(np.float32)
    return got


def check_chain(got, ref, hdr_bits, out_fmt, what):
    for name in LEVELS:
        assert got[name].shape == ref[name].shape, name
        assert_rgba16f_close(got[name], ref[name], what=f"{what} {name}")
    np.testing.assert_allclose(got["lum"][0], ref["lum"][0], atol=1e-5, rtol=0)
    np.testing.assert_allclose(got["lum"][1:], ref["lum"][1:], rtol=2e-5)
    if out_fmt == SRGB:
        assert_rgba8_close(got["tonemapped"], ref["tonemapped"], 1, what=f"{what} tonemapped")
    else:  # tests/test_gpu_post.py::test_chain_into_a_unorm_target_matches_oracle: the oracle's store on the device's own bloom level and exposure
        want = orc.tonemap(hdr_bits, got["u0"], got["lum"], 1.0, "rgba8_unorm")
        assert_rgba8_close(got["tonemapped"], want, 1, what=f"{what} tonemapped (UNORM)")
        assert (got["tonemapped"] != want).mean() < 1e-3
        assert (got["tonemapped"][..., 3] == 255).all()


@per_assignment((256, 256, False, SRGB, False), (256, 256, True, UNORM, False), (250, 130, False, UNORM, False), (250, 130, True, SRGB, False),
                (250, 130, False, SRGB, True),
                ids=["256x256-rgba16f-srgb", "256x256-b10g11r11-unorm", "250x130-rgba16f-unorm", "250x130-b10g11r11-srgb", "250x130-rows"])
def test_post_chain(gr, assignment, w, h, packed, out_fmt, bands):
    """Threshold, four downsamples (+ feedback), luminance, three upsamples, tonemap over two frames.  256 x 256 under tight and wide256: every
    level on its 2:1 / 1:2 stencil form and the 16-byte tonemap rows (post.hip: threshold_is_exact, downsample_is_exact, k_tonemap's `full`);
    under pad1 and mixed the rows are 8-byte aligned only and the generic forms run at the same even sizes."""
    hdr_bits, frames = chain_reference(w, h, packed)
    make, state = Factory(gr, assignment), {}
    for frame, ref in enumerate(frames):
        got = run_chain_frame(gr, make, hdr_bits, packed, out_fmt, state, bands)
        make.check()
        check_chain(got, ref, hdr_bits, out_fmt, f"{assignment} {w}x{h} frame {frame}")


# ---- fused bloom forms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("assignment", ASSIGNMENTS)
def test_fused_bloom_forms(gr, assignment):
    """down_head, down_mid, down_tail + up_tail, up_all and pyramid at 256 x 256, on the second frame (feedback history and exposure in play).
    The separate launches on the same layout are within the comparator of the oracle; a form its *_supported query offers leaves the very
    bytes of the separate launches (what tests/test_gpu_post.py holds on tight images); a form the query refuses launches nothing.  tight and
    wide256 must be offered every form: no header asks a fused form for a tight pitch."""
    w = h = 256
    hdr_bits, frames = chain_reference(w, h, False)
    make = Factory(gr, assignment)
    lum_lerp, fb_lerp = orc.frame_lerps(0.01)
    size = {name: orc.level_size(w, h, s) for name, s in SCALES.items()}
    hdr = make(w, h, F16, "in", "hdr").upload(hdr_bits)

    def levels(tag, names=LEVELS):
        return {name: make(*size[name], F16, "out", f"{tag}.{name}") for name in names}

    def separate(l, history, lum):
        gr.bloom_threshold(hdr, l["threshold"], lum.ptr)
        for src, dst in zip(LEVELS[:4], LEVELS[1:5]):
            gr.bloom_downsample(l[src], l[dst], history if dst == "d3" else None, fb_lerp if dst == "d3" else 0.0)
        gr.luminance(l["d3"], lum.ptr, lum_lerp)
        for src, dst in zip(LEVELS[4:7], LEVELS[5:8]):
            gr.bloom_upsample(l[src], l[dst])
        gr.sync()

    first, lum_first = levels("frame0"), capi.DeviceBuffer(gr, 12)
    separate(first, None, lum_first)
    lum_before = lum_first.download(np.float32).copy()
    history = first["d3"]
    a, lum_a = levels("separate"), capi.DeviceBuffer(gr, 12).upload(lum_before)
    separate(a, history, lum_a)
    want = {name: image.download() for name, image in a.items()}
    want_lum = lum_a.download(np.float32)
    for name in LEVELS:
        assert_rgba16f_close(want[name], frames[1][name], what=f"{assignment} separate launches, frame 1 {name}")
    np.testing.assert_allclose(want_lum[0], frames[1]["lum"][0], atol=1e-5, rtol=0)
    np.testing.assert_allclose(want_lum[1:], frames[1]["lum"][1:], rtol=2e-5)

    def fused(form, names, launch, writes_lum):
        b, lum = levels(form, names), capi.DeviceBuffer(gr, 12).upload(lum_before)
        offered = launch(b, lum)
        gr.sync()
        print(f"fused bloom forms, {assignment}: {form} {'offered' if offered else 'refused'}")
        if assignment in ("tight", "wide256"):
            assert offered, f"{form} is offered on tight images and must be on {assignment} ones"
        if not offered:
            for name, image in b.items():
                image.check_unchanged(f"{form}.{name} (the form was refused: nothing may be launched)")
            np.testing.assert_array_equal(lum.download(np.float32), lum_before)
            return
        for name, image in b.items():
            np.testing.assert_array_equal(image.download(), want[name], err_msg=f"{assignment} {form} {name}")
        if writes_lum:
            np.testing.assert_array_equal(lum.download(np.float32), want_lum, err_msg=f"{assignment} {form} luminance")

    fused("down_head", ("threshold", "d0", "d1"), lambda b, lum: gr.bloom_down_head(hdr, b["threshold"], b["d0"], b["d1"], lum.ptr), False)
    fused("down_mid", ("d0", "d1"), lambda b, lum: gr.bloom_down_mid(a["threshold"], b["d0"], b["d1"]), False)
    fused("down_tail+up_tail", ("d2", "d3", "u2", "u1"),
          lambda b, lum: gr.bloom_tail(a["d1"], b["d2"], b["d3"], history, b["u2"], b["u1"], fb_lerp, lum.ptr, lum_lerp), True)
    fused("up_all", ("u2", "u1", "u0"), lambda b, lum: gr.bloom_up_all(a["d3"], b["u2"], b["u1"], b["u0"], lum.ptr, lum_lerp), True)
    fused("pyramid", LEVELS, lambda b, lum: gr.bloom_pyramid(hdr, b, history, fb_lerp, lum.ptr, lum_lerp), True)
    assert gr.pyramid_giveups() == 0
    make.check()


# ---- lighting -----------------------------------------------------------------------------------------------------------------------
ALL = capi.LIGHTING_DIRECTIONAL_BIT | capi.LIGHTING_CLUSTERED_BIT | capi.LIGHTING_AMBIENT_FALLBACK_BIT


def lighting_reference(w, h, lights, packed_with_ao):
    def compute():
        sc = Scene(w, h, lights)
        ao = None
        if packed_with_ao:
            sc.gbuf["emissive"] = orc.quantize_b10g11r11(sc.gbuf["emissive"])
            ao = ambient_occlusion_image(w // 2, h // 2)
        ref_c = orc.cluster_build(sc.rp, sc.prm, sc.lights, sc.model, sc.type_mask, sc.n, sc.res[2])
        want = orc.lighting(sc.gbuf, sc.rp, sc.prm, sc.lights, sc.type_mask, ref_c["bitmask"], ref_c["range"], synth.DIRECTIONAL_COLOR,
                            synth.DIRECTIONAL_DIRECTION, b10g11r11=packed_with_ao, ambient_occlusion=ao)
        return sc, ao, want
    return reference(("lighting", w, h, lights, packed_with_ao), compute)


@per_assignment((256, 128, 300), (130, 75, 64))
def test_lighting_aliased_emissive(gr, assignment, w, h, lights):
    """Clustered + directional, emissive aliased onto the RGBA16F target (read-modify-write).  Both widths are even: tight and wide256 run the
    two-pixel kernel (gr_lighting: pairs_aligned), wide256 over a pitch that is not the width; pad1 and mixed leave rows or pointers that are
    not multiples of two texels and run the one-pixel kernel."""
    sc, _, want = lighting_reference(w, h, lights, False)
    make = Factory(gr, assignment)
    dev = sc.build_clusters_gpu(gr)
    args, imgs = sc.lighting_args(gr, dev, ALL, make_image=make)
    gr.check(gr.lib.gr_lighting(gr.handle, None, args))
    gr.sync()
    make.check()
    got = imgs["hdr"].download()
    np.testing.assert_array_equal(got[..., 3], sc.gbuf["emissive"][..., 3])
    sky = sc.gbuf["depth"] == 0.0
    np.testing.assert_array_equal(got[sky], sc.gbuf["emissive"][sky])
    assert_rgba16f_close(got, want, ulps=2.0, abs_tol=1e-4, what=f"lighting {assignment} {w}x{h}")
    assert (got == want).mean() > 0.95


@pytest.mark.parametrize("assignment", ASSIGNMENTS)
def test_lighting_separate_emissive_packed_target_and_half_size_ao(gr, assignment):
    """A separate emissive input, a B10G11R11 target and the ambient-occlusion instantiation with its half-size image in pad1 under every assignment."""
    w, h = 256, 128
    sc, ao, want = lighting_reference(w, h, 300, True)
    make = Factory(gr, assignment)
    dev = sc.build_clusters_gpu(gr)
    args, imgs = sc.lighting_args(gr, dev, ALL | capi.LIGHTING_AMBIENT_OCCLUSION_BIT, alias_emissive=False, make_image=make)
    target = make(w, h, B10, "out", "hdr (B10G11R11)")
    emissive = make(w, h, B10, "in", "emissive (B10G11R11)").upload(orc.pack_b10g11r11(sc.gbuf["emissive"]))
    ao_image = make(w // 2, h // 2, R8, "in", "ambient_occlusion", layout="pad1").upload(ao)
    args.hdr, args.emissive, args.ambient_occlusion = target.desc, emissive.desc, ao_image.desc
    gr.check(gr.lib.gr_lighting(gr.handle, None, args))
    gr.sync()
    make.check()
    got = target.download()
    codes_close(got, orc.pack_b10g11r11(want), f"lighting {assignment} into a packed target with AO")
    sky = sc.gbuf["depth"] == 0.0
    np.testing.assert_array_equal(got[sky], orc.pack_b10g11r11(sc.gbuf["emissive"])[sky])


# ---- anti-aliasing and blit ---------------------------------------------------------------------------------------------------------
AA_SIZES = [(320, 180), (253, 127)]


@per_assignment(*AA_SIZES)
def test_fxaa(gr, assignment, w, h):
    src, want_srgb, want_unorm = reference(("fxaa", w, h), lambda: (lambda s: (s, orc.fxaa(s, True), orc.fxaa(s, False)))(synth.make_ldr_pattern(w, h)))
    make = Factory(gr, assignment)
    din, dout, dun = make(w, h, SRGB, "in", "in").upload(src), make(w, h, SRGB, "out", "out (sRGB)"), make(w, h, UNORM, "out", "out (UNORM)")
    gr.fxaa(din, dout)
    gr.fxaa(din, dun)
    gr.sync()
    make.check()
    assert_rgba8_close(dout.download(), want_srgb, 1, what=f"fxaa {assignment} srgb target")
    np.testing.assert_array_equal(dun.download(), want_unorm)


@per_assignment(*[(quality, w, h) for w, h in AA_SIZES for quality in (0, 3)])
def test_smaa_passes(gr, assignment, quality, w, h):
    """Edges and weights bit-exact, the blend within 1 LSB.  320 is a multiple of 4: tight and wide256 take gr_smaa_neighbor_blend's `wide` form
    (four pixels a lane through 16-byte accesses), pad1 and mixed the one-pixel form at the same width."""
    area, search = reference("smaa luts", load_smaa_luts)
    src, ref = reference(("smaa", w, h, quality), lambda: (lambda s: (s, orc.smaa(s, area, search, quality, True)))(synth.make_ldr_pattern(w, h)))
    gr.smaa_set_luts(area, search)
    make = Factory(gr, assignment)
    dsrc = make(w, h, SRGB, "in", "color").upload(src)
    dedge, dwt, dout = make(w, h, RG8, "out", "edges"), make(w, h, UNORM, "out", "weights"), make(w, h, SRGB, "out", "out")
    gr.smaa_edge_detection(dsrc, dedge, quality)
    gr.smaa_blend_weight(dedge, dwt, quality)
    gr.smaa_neighbor_blend(dsrc, dwt, dout)
    gr.sync()
    make.check()
    np.testing.assert_array_equal(dedge.download(), ref["edges"])
    np.testing.assert_array_equal(dwt.download(), ref["weights"])
    assert_rgba8_close(dout.download(), ref["out"], 1, what=f"smaa {assignment} q{quality} blend")
    assert ref["edges"].any() and ref["weights"].any()


def taa_reference(w, h, quality):
    def compute():
        cur, depth, mv, reproj = taa_inputs(w, h)
        first = orc.taa_resolve(cur, depth, mv, None, reproj, quality)
        cur2 = synth.make_hdr(w, h, seed=11)
        second = orc.taa_resolve(cur2, depth, mv, first[1], reproj, quality)
        return cur, cur2, depth, mv, reproj, first, second
    return reference(("taa", w, h, quality), compute)


@per_assignment(*[(quality, w, h) for w, h in AA_SIZES for quality in (0, 2)])
def test_taa_resolve(gr, assignment, quality, w, h):
    """A frame without history, then one with the oracle's history of the first."""
    cur, cur2, depth, mv, reproj, first, second = taa_reference(w, h, quality)
    make = Factory(gr, assignment)
    dcur = make(w, h, F16, "in", "current").upload(cur)
    ddepth, dmv = make(w, h, D32, "in", "depth").upload(depth), make(w, h, capi.FORMAT_R16G16_SFLOAT, "in", "mv").upload(mv)
    dcol, dhist = make(w, h, F16, "out", "out_color"), make(w, h, F16, "out", "out_history")
    gr.taa_resolve(dcur, ddepth, dmv, None, dcol, dhist, reproj, quality)
    gr.sync()
    make.check()
    assert_rgba16f_close(dcol.download(), first[0], what=f"taa {assignment} q{quality} f0 colour")
    assert_rgba16f_close(dhist.download(), first[1], what=f"taa {assignment} q{quality} f0 history")
    dcur2, dprev = make(w, h, F16, "in", "current (frame 1)").upload(cur2), make(w, h, F16, "in", "history").upload(first[1])
    dcol2, dhist2 = make(w, h, F16, "out", "out_color (frame 1)"), make(w, h, F16, "out", "out_history (frame 1)")
    gr.taa_resolve(dcur2, ddepth, dmv, dprev, dcol2, dhist2, reproj, quality)
    gr.sync()
    make.check()
    assert_rgba16f_close(dcol2.download(), second[0], ulps=2.0, abs_tol=1e-4, what=f"taa {assignment} q{quality} f1 colour")
    assert_rgba16f_close(dhist2.download(), second[1], ulps=2.0, abs_tol=1e-4, what=f"taa {assignment} q{quality} f1 history")


@per_assignment(*[(linear, w, h) for w, h in AA_SIZES for linear in (False, True)])
def test_blit(gr, assignment, linear, w, h):
    """point: RGBA16F -> RGBA8 sRGB at the same size; linear: RGBA8 sRGB -> RGBA16F, rescaled to 333 x 77.  Same arithmetic as the oracle: exact."""
    if linear:
        src_name, src_fmt, dst_name, dst_fmt, dw, dh = "rgba8_srgb", SRGB, "rgba16f", F16, 333, 77
    else:
        src_name, src_fmt, dst_name, dst_fmt, dw, dh = "rgba16f", F16, "rgba8_srgb", SRGB, w, h

    def compute():
        src = synth.make_hdr(w, h) if src_fmt == F16 else synth.make_ldr_pattern(w, h)
        return src, orc.blit(src, src_name, dw, dh, dst_name, linear)
    src, want = reference(("blit", w, h, linear), compute)
    make = Factory(gr, assignment)
    din, dout = make(w, h, src_fmt, "in", "in").upload(src), make(dw, dh, dst_fmt, "out", "out")
    gr.blit(din, dout, linear)
    gr.sync()
    make.check()
    np.testing.assert_array_equal(dout.download(), want)


# ---- FSR ------------------------------------------------------------------------------------------------------------------------------
@per_assignment(*[(fp16, *sizes) for sizes in ((160, 90, 240, 135), (7, 5, 30, 22)) for fp16 in (False, True)])
def test_fsr_easu(gr, assignment, fp16, w, h, ow, oh):
    def compute():
        src = fsr_image(w, h, "noise")
        return src, orc.fsr_easu(src, ow, oh, fp16), orc.fsr_easu(src, ow, oh, fp16, target_srgb=True)
    src, want_unorm, want_srgb = reference(("easu", w, h, ow, oh, fp16), compute)
    make = Factory(gr, assignment)
    din, dun, dsrgb = make(w, h, SRGB, "in", "in").upload(src), make(ow, oh, UNORM, "out", "out (UNORM)"), make(ow, oh, SRGB, "out", "out (sRGB)")
    gr.fsr_upscale(din, dun, fp16)
    gr.fsr_upscale(din, dsrgb, fp16)
    gr.sync()
    make.check()
    np.testing.assert_array_equal(dun.download(), want_unorm)
    assert_rgba8_close(dsrgb.download(), want_srgb, 1, what=f"easu {assignment} srgb target")


@pytest.mark.parametrize("assignment", ASSIGNMENTS)
def test_fsr_rcas(gr, assignment):
    w, h = 253, 127
    sharp = orc.fsr_rcas_sharpness(0.5)
    src, want_unorm, want_srgb = reference("rcas", lambda: (lambda s: (s, orc.fsr_rcas(s, sharp, False), orc.fsr_rcas(s, sharp, True)))(fsr_image(w, h, "noise", seed=9)))
    make = Factory(gr, assignment)
    din, dun, dsrgb = make(w, h, UNORM, "in", "in").upload(src), make(w, h, UNORM, "out", "out (UNORM)"), make(w, h, SRGB, "out", "out (sRGB)")
    gr.fsr_sharpen(din, dun, sharp)
    gr.fsr_sharpen(din, dsrgb, sharp)
    gr.sync()
    make.check()
    np.testing.assert_array_equal(dun.download(), want_unorm)
    assert_rgba8_close(dsrgb.download(), want_srgb, 1, what=f"rcas {assignment} srgb")


# ---- PQ10 -----------------------------------------------------------------------------------------------------------------------------
@per_assignment((333, 77), (256, 64))
def test_pq10(gr, assignment, w, h):
    conversion = orc.rec709_to_display()

    def compute():
        hdr = synth.make_hdr(w, h, 5)
        ui = np.random.default_rng(2).integers(0, 256, (h, w, 4), dtype=np.uint8)
        ui[: h // 2] = (0, 0, 0, 255)
        return hdr, ui, {mll: orc.pq10_encode(hdr, ui, conversion, 500.0, 400.0, mll) for mll in (1000.0, 400.0)}
    hdr, ui, want = reference(("pq10", w, h), compute)
    make = Factory(gr, assignment)
    dh, du = make(w, h, F16, "in", "hdr").upload(hdr), make(w, h, SRGB, "in", "ui").upload(ui)
    channels = lambda words: np.stack([(words >> s) & 1023 for s in (0, 10, 20)], axis=-1).astype(int)
    for mll in (1000.0, 400.0):
        do = make(w, h, A2, "out", f"out ({mll:g} nits)")
        gr.pq10_encode(dh, du, do, conversion, 500.0, 400.0, mll)
        gr.sync()
        make.check()
        got = do.download()
        assert ((got >> 30) == 3).all()
        diff = np.abs(channels(got) - channels(want[mll]))
        assert diff.max() <= 1, diff.max()
        assert (diff == 0).mean() > 0.9


# ---- HiZ, SPD -------------------------------------------------------------------------------------------------------------------------
@per_assignment((256, 64), (257, 131))
def test_hiz(gr, assignment, w, h):
    """The depth image laid out; the chain is a buffer.  256 wide under tight and wide256: 16-byte row loads (gr_hiz: p.aligned); pad1 and mixed:
    single texels at the same width."""
    depth, zt, want = reference(("hiz", w, h), lambda: (lambda d, z: (d, z, orc.hiz(d, z)))(depth_image(w, h), z_transform(w, h)))
    make = Factory(gr, assignment)
    image = make(w, h, D32, "in", "depth").upload(depth)
    chain, counter, layout = gr.hiz(image, zt)
    gr.sync()
    make.check()
    assert counter.download(np.uint32)[0] == 0
    got = gr.read_mip_chain(chain, layout)
    assert len(got) == len(want)
    for level, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"level {level} of {w}x{h} {assignment}")


@per_assignment((200, 120, 100, 60, 7, 4, False), (128, 128, 128, 128, 8, 1, True), ids=["colour", "depth"])
def test_spd(gr, assignment, iw, ih, w0, h0, mips, components, depth):
    src, want = reference(("spd", iw, ih, depth), lambda: (lambda s: (s, orc.spd(s, w0, h0, mips, components, depth, None, fill=0x3c00)))(spd_source(iw, ih)))
    make = Factory(gr, assignment)
    image = make(iw, ih, F16, "in", "input").upload(src)
    texels = orc.spd_chain_texels(w0, h0, mips)
    chain = capi.DeviceBuffer(gr, texels * 8).upload(np.full(texels * 4, 0x3c00, np.uint16))
    gr.spd_downsample(image, w0, h0, mips, components, depth, None, chain=chain)
    gr.sync()
    make.check()
    for level, (a, b) in enumerate(zip(want, orc.spd_split(chain.download(np.uint16), w0, h0, mips))):
        np.testing.assert_array_equal(b, a, err_msg=f"level {level} {assignment}")


# ---- SSR ------------------------------------------------------------------------------------------------------------------------------
def ssr_reference(w, h, frame):
    def compute():
        cam, depth, normal, pbr, albedo, light = close_up_scene(w, h, 0)
        rp = cam.render_params()
        zt = orc.hiz_z_transform(rp[48:64])
        noise = expand_sssr_dither(load_sssr_noise_base())
        traced = orc.ssr_trace(orc.hiz(depth, zt), pbr, normal, light, noise, frame, rp[32:48], rp[80:96], rp[96:99])
        return depth, normal, pbr, albedo, light, rp, zt, noise, traced, load_brdf_lut()
    return reference(("ssr", w, h, frame), compute)


@pytest.mark.parametrize("assignment", ASSIGNMENTS)
def test_ssr_trace_and_apply(gr, assignment):
    """gr_ssr_trace with its G-buffer and light inputs and its three output images laid out, then gr_ssr_apply on the device's traced image with
    every image laid out but brdf_lut, which gr_ssr_apply takes at a tight pitch only (granite_hip.h).  Ray list and counter exact."""
    w, h, frame = 256, 144, 0
    depth, normal, pbr, albedo, light, rp, zt, noise, ref, lut = ssr_reference(w, h, frame)
    make = Factory(gr, assignment)
    ddepth = make(w, h, D32, "in", "depth").upload(depth)
    dnormal, dpbr = make(w, h, A2, "in", "normal").upload(normal), make(w, h, RG8, "in", "pbr").upload(pbr)
    dlight = make(w, h, F16, "in", "light").upload(light)
    chain, _, layout = gr.hiz(ddepth, zt)
    outputs = {"output": make(w, h, F16, "out", "output"), "ray_length": make(w, h, capi.FORMAT_R16_SFLOAT, "out", "ray_length"),
               "confidence": make(w, h, R8, "out", "confidence")}
    # the trace writes a ray length only where a ray ran (output and confidence it clears itself): zero texels, as a fresh allocation has them
    outputs["ray_length"].upload(np.zeros((h, w), np.uint16))
    dev =gr.ssr_trace(chain, layout, dpbr, dnormal, dlight, capi.DeviceBuffer(gr, noise.nbytes).upload(noise), frame, rp[32:48], rp[80:96], rp[96:99],
                       images=outputs)
    gr.sync()
    make.check()
    counter = dev["ray_counter"].download(np.uint32)[:6]
    np.testing.assert_array_equal(counter, ref["ray_counter"])
    count = int(counter[5])
    assert count > 0.2 * w * h * 0.3, "the scene must produce rays"
    np.testing.assert_array_equal(dev["ray_list"].download(np.uint32)[:count], ref["ray_list"])
    got_conf, got_out, got_len = outputs["confidence"].download(), outputs["output"].download(), outputs["ray_length"].download()
    untouched = (ref["output"] == 0).all(axis=2) & (ref["confidence"] == 0)
    assert (got_out[untouched] == 0).all()
    np.testing.assert_array_equal(got_conf, ref["confidence"])
    assert not rgba16f_mismatch(got_out, ref["output"], 2.0, 1e-4).any()
    want_len = half_bits_to_f32(ref["ray_length"])
    assert not (np.abs(half_bits_to_f32(got_len) - want_len) > 1e-2 * (1.0 + np.abs(want_len))).any()
    assert (ref["confidence"] > 0).sum() > 30, "some rays must hit with confidence"

    # the apply pass on the device's traced image, so that it is checked on its own
    real_depth = depth.copy()
    real_depth[::17, ::13] = 1.0  # pixels the NOT_EQUAL depth test rejects
    want = orc.ssr_apply(light, got_out, albedo, normal, pbr, real_depth, lut, rp[80:96], rp[96:99])
    hdr = make(w, h, F16, "rmw", "hdr").upload(light)
    dalbedo, ddepth2 = make(w, h, SRGB, "in", "albedo").upload(albedo), make(w, h, D32, "in", "depth (apply)").upload(real_depth)
    gr.ssr_apply(hdr, outputs["output"], dalbedo, dnormal, dpbr, ddepth2, capi.DeviceImage(gr, 256, 256, capi.FORMAT_R16G16_SFLOAT).upload(lut), rp[80:96], rp[96:99])
    gr.sync()
    make.check()
    np.testing.assert_array_equal(outputs["output"].download(), got_out)  # `reflected` is an input of this pass
    got = hdr.download()
    assert not rgba16f_mismatch(got, want, 2.0, 1e-4).any()
    np.testing.assert_array_equal(got[::17, ::13], light[::17, ::13])
    assert (got != light).any(axis=2).mean() > 0.3
    np.testing.assert_array_equal(got[..., 3], light[..., 3])


# ---- decal apply ----------------------------------------------------------------------------------------------------------------------
GOLDEN = dc.load_golden()


@per_assignment(("two_overlap",), ("three_overlap_odd",))
def test_decal_apply(gr, assignment, name):
    """tests/test_gpu_decals.py::test_apply_against_the_executed_shader with albedo (read-modify-write) and depth laid out: the same golden colours,
    the same left-out pixels, the same 1 code value."""
    case = dc.golden_case(GOLDEN, name)
    mine = reference(("decal", name), lambda: decal_ref.apply(case))
    left_out = mine["edge_distance"] < 64.0 * mine["uvw_error"]
    touched = GOLDEN[f"{name}/touched"]
    assert int(left_out.sum()) <= 0.005 * int(touched.sum())
    albedo = np.asarray(case["albedo"], np.uint32)
    want = decal_device.reference_bytes(GOLDEN[f"{name}/colour"], albedo, touched)
    make = Factory(gr, assignment)
    scene = decal_device.ApplyScene(gr, case)
    w, h = case["width"], case["height"]
    scene.albedo = make(w, h, SRGB, "rmw", "albedo")
    scene.depth = make(w, h, D32, "in", "depth").upload(np.ascontiguousarray(case["depth"], np.float32))
    scene.args.albedo, scene.args.depth = scene.albedo.desc, scene.depth.desc
    first = scene.run()
    make.check()
    assert np.array_equal(first >> 24, albedo >> 24), "an alpha byte changed"
    far = np.asarray(case["depth"]) == 0
    assert np.array_equal(first[far], albedo[far]), "a far-plane pixel was written"
    outside, inside = ~touched & ~left_out, touched & ~left_out
    assert np.array_equal(first[outside], albedo[outside]), f"{(first[outside] != albedo[outside]).sum()} pixels outside every decal changed"
    channels = lambda a: np.stack([(a >> s) & 255 for s in (0, 8, 16)], -1).astype(np.int64)
    assert np.abs(channels(first[inside]) - channels(want[inside])).max() <= 1


# ---- the RGB888 transport form (ctx.hip) ----------------------------------------------------------------------------------------------
@per_assignment((64, 16), (333, 21))
def test_rgb888_transport(gr, assignment, w, h):
    """gr_pack_rgb8_rows from a laid-out image and gr_unpack_rgb8_rows into one, a band of rows: against the rows' own bytes."""
    lib = gr.lib
    lib.gr_pack_rgb8_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.Image), C.POINTER(capi.Rows), C.c_void_p]
    lib.gr_unpack_rgb8_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(capi.Image), C.POINTER(capi.Rows)]
    src = np.random.default_rng(w * 131 + h).integers(0, 256, (h, w, 4), dtype=np.uint8)
    src[..., 3] = 255
    make = Factory(gr, assignment)
    image = make(w, h, SRGB, "in", "image").upload(src)
    other = make(w, h, SRGB, "rmw", "unpacked").upload(np.full((h, w, 4), 7, np.uint8))
    packed = capi.DeviceBuffer(gr, w * h * 3)
    first, count = h // 3, max(h // 2, 1)
    rows = capi.Rows(first, count)
    gr.check(lib.gr_pack_rgb8_rows(gr.handle, None, image.desc, rows, packed.ptr))
    gr.check(lib.gr_unpack_rgb8_rows(gr.handle, None, packed.ptr, other.desc, rows))
    gr.sync()
    make.check()
    got = other.download()
    np.testing.assert_array_equal(got[first:first + count], src[first:first + count])
    assert (got[:first] == 7).all() and (got[first + count:] == 7).all()
    raw = packed.download(np.uint8).reshape(h, w, 3)
    np.testing.assert_array_equal(raw[first:first + count], src[first:first + count, :, :3])


# ---- environment bake and ocean: the image arguments of gr_env_equirect_to_cube, gr_ocean_bake_maps and gr_ocean_mipmap ----------------------------
@pytest.mark.parametrize("assignment", ASSIGNMENTS)
def test_equirect_to_cube(gr, assignment):
    """tests/test_gpu_env_bake.py's smallest case with the equirect image laid out: against the executed shader, the file's bound."""
    name = "equirect_5"
    size, levels = (int(v) for v in ENV_GOLDEN[name + "/params"])
    bits = ENV_GOLDEN[name + "/equirect"]
    make = Factory(gr, assignment)
    image = make(bits.shape[1], bits.shape[0], F16, "in", "equirect").upload(bits)
    cube, nbytes = chain_buffer(gr, size, levels)
    gr.env_equirect_to_cube(image, cube, size, levels)
    gr.sync()
    make.check()
    close(f"{name} {assignment}", read_chain(cube, nbytes), ENV_GOLDEN[name + "/out"])


@per_assignment(*[(name,) for name in BAKE[:2]])
def test_ocean_bake_maps(gr, assignment, name):
    """Bit for bit against the executed shader; height and displacement are sampled with wrap-around, the two outputs are written."""
    size, vertex = (int(v) for v in OCEAN_GOLDEN[name + "/spec"])
    make = Factory(gr, assignment)

    def laid_out(bits, channels, what):
        bits = np.ascontiguousarray(bits)
        return make(bits.shape[1], bits.shape[0], OCEAN_FORMATS[channels], "in", what).upload(bits)
    height, disp = laid_out(OCEAN_GOLDEN["bake/height"], 1, "height"), laid_out(OCEAN_GOLDEN[f"bake/displacement{size}"], 2, "displacement")
    gj = make(64, 64, OCEAN_FORMATS[4], "out", "grad_jacobian")
    hd = make(64, 64, OCEAN_FORMATS[4], "out", "height_displacement") if vertex else None
    gr.ocean_bake_maps(height, disp, gj, hd, as_struct(capi.PushOceanBake, OCEAN_GOLDEN[name + "/push"]))
    gr.sync()
    make.check()
    assert np.array_equal(gj.download(), OCEAN_GOLDEN[name + "/grad_jacobian"])
    if vertex:
        assert np.array_equal(hd.download(), OCEAN_GOLDEN[name + "/height_displacement"])


@per_assignment(*[(name,) for name in MIPMAP])
def test_ocean_mipmap(gr, assignment, name):
    w, h, channels = (int(v) for v in OCEAN_GOLDEN[name + "/spec"])
    make = Factory(gr, assignment)
    src = make(w, h, OCEAN_FORMATS[channels], "in", "in").upload(np.ascontiguousarray(OCEAN_GOLDEN[f"mipmap/in_{w}x{h}_c{channels}"]))
    out = make(w // 2, h // 2, OCEAN_FORMATS[channels], "out", "out")
    gr.ocean_mipmap(src, out, as_struct(capi.PushOceanMipmap, OCEAN_GOLDEN[name + "/push"]))
    gr.sync()
    make.check()
    assert np.array_equal(out.download().reshape(h // 2, w // 2, channels), OCEAN_GOLDEN[name + "/out"])
