"""GPU: the bloom launches over the sizes they accept (tests/post_sweep.py; its coverage and patch extents are asserted by
tests/test_post_sweep_cpu.py, on the CPU, before anything here is launched).

  * each fused launch against the separate launches, byte for byte: the parity sweep where the rules offer it, level pairs no frame has
    ("off-pyramid": on the boundaries of the ratio rules), the sizes whose committed answer in tests/golden/bloom_supported.json is 1;
  * the separate launches against the CPU oracle over the whole parity sweep, and stage by stage on the level pairs;
  * +0, the smallest denormal, 65504 and +inf through every stage and every fused form.

Tolerances are those of tests/test_gpu_post.py.  Which launch a case should be offered is stated in post_sweep.py from the rules; an entry point
that declines what it should take, or takes what it should decline, fails the case."""
import numpy as np
import pytest

import post_sweep as ps
from granite_amd import capi, synth
from oracle import oracle as orc
from test_gpu_post import run_chain_gpu
from util import assert_rgba16f_close, assert_rgba8_close, half_bits_to_f32

pytestmark = pytest.mark.gpu

F16 = capi.FORMAT_R16G16B16A16_SFLOAT
B10 = capi.FORMAT_B10G11R11_UFLOAT_PACK32
LUM0 = np.array([0.3, 1.7, 1.0 / 1.7], np.float32)
MID, TAIL = ("threshold", "d0", "d1"), ("d1", "d2", "d3")


def size_id(levels):
    return " ".join("%s=%dx%d" % (name, *levels[name]) for name in ("hdr", "threshold", "d0", "d1", "d2", "d3", "u2", "u1", "u0") if name in levels)


def image(gr, size, bits=None, fmt=F16):
    img = capi.DeviceImage(gr, size[0], size[1], fmt)
    return img.upload(bits) if bits is not None else img


def seed_of(levels):
    return sum((i + 1) * 7919 * (w * 4099 + h) for i, (w, h) in enumerate(levels[name] for name in sorted(levels))) & 0x7fffffff


def assert_same_bytes(got, want, what, specials=False):
    """Byte for byte; with planted special values: NaN in the same places (whatever its payload), every other texel byte for byte."""
    if specials and got.dtype == np.uint16:
        g, w = half_bits_to_f32(got), half_bits_to_f32(want)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=what + ": NaN in different places")
        got, want = np.where(np.isnan(g), 0x7e00, got), np.where(np.isnan(w), 0x7e00, want)
    elif specials:
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what + ": NaN in different places")
        got, want = np.nan_to_num(got, nan=0.0).view(np.uint32), np.nan_to_num(want, nan=0.0).view(np.uint32)
    np.testing.assert_array_equal(got, want, err_msg=what)


def hdr_input(gr, size, seed, b10, plant=False):
    bits = ps.random_level(size, seed, -6, 6)
    if plant:
        ps.plant_specials(bits)
    if b10:  # the packed format holds neither a denormal half nor 65504: what it holds instead goes through both forms alike
        return image(gr, size, orc.pack_b10g11r11(bits), B10)
    return image(gr, size, bits)


def lum_buffer(gr, dynamic):
    return capi.DeviceBuffer(gr, 12).upload(LUM0) if dynamic else None


# ---- one function per fused launch: runs both forms, compares ---------------------------------------------------------------------------------
def check_down_pair(gr, names, levels, plant=False):
    """gr_bloom_down_mid (threshold, d0, d1) / gr_bloom_down_tail (d1, d2, d3: with the feedback) against two gr_bloom_downsample calls."""
    src_n, fine_n, coarse_n = names
    feedback = names == TAIL
    seed = seed_of(levels)
    bits = ps.random_level(levels[src_n], seed)
    if plant:
        ps.plant_specials(bits)
    src = image(gr, levels[src_n], bits)
    hist_bits = ps.random_level(levels[coarse_n], seed + 1, -8, 4)
    if plant and levels[coarse_n][0] >= 38 and levels[coarse_n][1] >= 25:
        ps.plant_specials(hist_bits)  # an infinite alpha in the history: inf * 0 = NaN in the feedback mix, in both forms
    hist = image(gr, levels[coarse_n], hist_bits) if feedback else None
    _, fb_lerp = orc.frame_lerps(0.01)
    want_fine, want_coarse = image(gr, levels[fine_n]), image(gr, levels[coarse_n])
    gr.bloom_downsample(src, want_fine)
    gr.bloom_downsample(want_fine, want_coarse, hist, fb_lerp if feedback else 0.0)
    fine, coarse = image(gr, levels[fine_n]), image(gr, levels[coarse_n])
    p_a, p_b = capi.downsample_push(fine, src, fb_lerp if feedback else 0.0), capi.downsample_push(coarse, fine, fb_lerp if feedback else 0.0)
    if feedback:
        gr.check(gr.lib.gr_bloom_down_tail(gr.handle, None, src.desc, fine.desc, coarse.desc, hist.desc, p_a, p_b))
    else:
        gr.check(gr.lib.gr_bloom_down_mid(gr.handle, None, src.desc, fine.desc, coarse.desc, p_a, p_b, None))
    gr.sync()
    out = coarse.download()
    assert_same_bytes(fine.download(), want_fine.download(), fine_n, plant)
    assert_same_bytes(out, want_coarse.download(), coarse_n, plant)
    return out


def decline_down_pair(gr, names, levels):
    src, fine, coarse = (image(gr, levels[n]) for n in names)
    p_a, p_b = capi.downsample_push(fine, src), capi.downsample_push(coarse, fine)
    with pytest.raises(capi.GraniteHipError):
        if names == TAIL:
            gr.check(gr.lib.gr_bloom_down_tail(gr.handle, None, src.desc, fine.desc, coarse.desc, image(gr, levels[names[2]]).desc, p_a, p_b))
        else:
            gr.check(gr.lib.gr_bloom_down_mid(gr.handle, None, src.desc, fine.desc, coarse.desc, p_a, p_b, None))


def check_up_tail(gr, levels, dynamic, d3_bits=None, plant=False):
    """gr_bloom_up_tail against gr_luminance + two gr_bloom_upsample calls."""
    dynamic = dynamic and min(levels["d3"]) >= 2  # a luminance grid (downsample-3 / 2) with no texel is not launched
    if d3_bits is None:
        d3_bits = ps.random_level(levels["d3"], seed_of(levels) + 2, -8, 4)
        if plant:
            ps.plant_specials(d3_bits)
    d3 = image(gr, levels["d3"], d3_bits)
    lum_lerp, _ = orc.frame_lerps(0.01)
    got = {}
    for fused in (False, True):
        u2, u1 = image(gr, levels["u2"]), image(gr, levels["u1"])
        lum = lum_buffer(gr, dynamic)
        if fused:
            p_lum = capi.luminance_push(d3, lum_lerp) if dynamic else None
            gr.check(gr.lib.gr_bloom_up_tail(gr.handle, None, d3.desc, u2.desc, u1.desc, lum.ptr if dynamic else None, capi.upsample_push(u2, d3),
                                             capi.upsample_push(u1, u2), p_lum))
        else:
            if dynamic:
                gr.luminance(d3, lum.ptr, lum_lerp)
            gr.bloom_upsample(d3, u2)
            gr.bloom_upsample(u2, u1)
        gr.sync()
        got[fused] = (u2.download(), u1.download(), lum.download(np.float32) if dynamic else np.zeros(3, np.float32))
    for a, b, name in zip(got[True], got[False], ("upsample-2", "upsample-1", "luminance")):
        assert_same_bytes(a, b, name, plant)
    if dynamic and not plant:
        assert got[True][2][0] != LUM0[0]


def decline_up_tail(gr, levels):
    d3, u2, u1 = (image(gr, levels[n]) for n in ("d3", "u2", "u1"))
    with pytest.raises(capi.GraniteHipError):
        gr.check(gr.lib.gr_bloom_up_tail(gr.handle, None, d3.desc, u2.desc, u1.desc, None, capi.upsample_push(u2, d3), capi.upsample_push(u1, u2), None))


def check_up_all(gr, levels, dynamic, plant=False):
    """gr_bloom_up_all in both workgroup forms against gr_luminance + three gr_bloom_upsample calls."""
    dynamic = dynamic and min(levels["d3"]) >= 2
    d3_bits = ps.random_level(levels["d3"], seed_of(levels) + 3, -8, 4)
    if plant:
        ps.plant_specials(d3_bits)
    d3 = image(gr, levels["d3"], d3_bits)
    lum_lerp, _ = orc.frame_lerps(0.01)
    got = {}
    for form in ("separate", "1024 threads", "256 threads"):
        u2, u1, u0 = (image(gr, levels[n]) for n in ("u2", "u1", "u0"))
        lum = lum_buffer(gr, dynamic)
        if form == "separate":
            if dynamic:
                gr.luminance(d3, lum.ptr, lum_lerp)
            gr.bloom_upsample(d3, u2)
            gr.bloom_upsample(u2, u1)
            gr.bloom_upsample(u1, u0)
        else:
            p_lum = capi.luminance_push(d3, lum_lerp) if dynamic else None
            gr.check(gr.lib.gr_bloom_up_all(gr.handle, None, d3.desc, u2.desc, u1.desc, u0.desc, lum.ptr if dynamic else None, capi.upsample_push(u2, d3),
                                            capi.upsample_push(u1, u2), capi.upsample_push(u0, u1), p_lum, 1 if form == "256 threads" else 0))
        gr.sync()
        got[form] = (u2.download(), u1.download(), u0.download(), lum.download(np.float32) if dynamic else np.zeros(3, np.float32))
    for form in ("1024 threads", "256 threads"):
        for a, b, name in zip(got[form], got["separate"], ("upsample-2", "upsample-1", "upsample-0", "luminance")):
            assert_same_bytes(a, b, f"{name} ({form})", plant)


def decline_up_all(gr, levels):
    d3, u2, u1, u0 = (image(gr, levels[n]) for n in ("d3", "u2", "u1", "u0"))
    with pytest.raises(capi.GraniteHipError):
        gr.check(gr.lib.gr_bloom_up_all(gr.handle, None, d3.desc, u2.desc, u1.desc, u0.desc, None, capi.upsample_push(u2, d3), capi.upsample_push(u1, u2),
                                        capi.upsample_push(u0, u1), None, 0))


def check_head(gr, levels, b10, dynamic, plant=False):
    """gr_bloom_down_head against gr_bloom_threshold + two gr_bloom_downsample calls."""
    hdr = hdr_input(gr, levels["hdr"], seed_of(levels) + 4, b10, plant)
    lum = lum_buffer(gr, dynamic)
    lum_ptr = lum.ptr if dynamic else None
    want = [image(gr, levels[n]) for n in MID]
    gr.bloom_threshold(hdr, want[0], lum_ptr)
    gr.bloom_downsample(want[0], want[1])
    gr.bloom_downsample(want[1], want[2])
    got = [image(gr, levels[n]) for n in MID]
    assert gr.bloom_down_head(hdr, *got, lum_ptr), "the rules offer this frame the fused head"
    gr.sync()
    for a, b, name in zip(got, want, MID):
        assert_same_bytes(a.download(), b.download(), name, plant)


def check_pyramid(gr, levels, b10, dynamic, plant=False, ask=True):
    """gr_bloom_pyramid against the nine separate launches, two frames over the same images (the second launch finds the counters the first left)."""
    dynamic = dynamic and min(levels["d3"]) >= 2
    seed = seed_of(levels)
    hdr = hdr_input(gr, levels["hdr"], seed + 5, b10, plant)
    history_bits = ps.random_level(levels["d3"], seed + 6, -8, 2)
    if plant and levels["d3"][0] >= 38 and levels["d3"][1] >= 25:
        ps.plant_specials(history_bits)
    history = image(gr, levels["d3"], history_bits)
    lum_lerp, fb_lerp = orc.frame_lerps(0.01)
    down = ("threshold", "d0", "d1", "d2", "d3")
    results = {}
    for fused in (False, True):
        l = {name: image(gr, levels[name]) for name in ps.SCALES}
        lum = lum_buffer(gr, dynamic)
        lum_ptr = lum.ptr if dynamic else None
        for frame in range(2):
            if fused:
                assert gr.bloom_pyramid(hdr, l, history, fb_lerp, lum_ptr, lum_lerp, any_size=not ask), "the rules offer this frame the one-launch pyramid"
            else:
                gr.bloom_threshold(hdr, l["threshold"], lum_ptr)
                for src, dst in zip(down[:-1], down[1:]):
                    gr.bloom_downsample(l[src], l[dst], history if dst == "d3" else None, fb_lerp)
                if dynamic:
                    gr.luminance(l["d3"], lum_ptr, lum_lerp)
                gr.bloom_upsample(l["d3"], l["u2"])
                gr.bloom_upsample(l["u2"], l["u1"])
                gr.bloom_upsample(l["u1"], l["u0"])
        gr.sync()
        results[fused] = {name: img.download() for name, img in l.items()}
        results[fused]["luminance"] = lum.download(np.float32) if dynamic else np.zeros(3, np.float32)
    assert gr.pyramid_giveups() == 0
    for name in results[True]:
        assert_same_bytes(results[True][name], results[False][name], name, plant)


# ---- the queries on a case's real descriptors ---------------------------------------------------------------------------------------------------
def query(gr, function, levels):
    """gr_bloom_<function>_supported on descriptors of these level sizes (nothing is read through them)."""
    im = ps.fake_images(levels)
    down, up = capi.downsample_push, capi.upsample_push
    lib = gr.lib
    if function == "down_mid":
        return lib.gr_bloom_down_mid_supported(im["threshold"], im["d0"], im["d1"], down(im["d0"], im["threshold"]), down(im["d1"], im["d0"]))
    if function == "down_head":
        return lib.gr_bloom_down_head_supported(im["hdr"], im["threshold"], im["d0"], im["d1"], capi.threshold_push(im["threshold"]),
                                                down(im["d0"], im["threshold"]), down(im["d1"], im["d0"]))
    if function == "tail":
        return lib.gr_bloom_tail_supported(im["d1"], im["d2"], im["d3"], im["u2"], im["u1"], down(im["d2"], im["d1"]), down(im["d3"], im["d2"]),
                                           up(im["u2"], im["d3"]), up(im["u1"], im["u2"]))
    if function == "up_all":
        return lib.gr_bloom_up_all_supported(im["d3"], im["u2"], im["u1"], im["u0"], up(im["u2"], im["d3"]), up(im["u1"], im["u2"]), up(im["u0"], im["u1"]))
    raise ValueError(function)


# ---- B: the case lists ------------------------------------------------------------------------------------------------------------------------
def frame_cases(function):
    """ps.frame_cases as pytest parameters (how many there are of each kind is asserted by tests/test_post_sweep_cpu.py)."""
    return [pytest.param(origin, levels, option, id="%s %dx%d/%d" % (origin, w, h, option)) for origin, (w, h), levels, option in ps.frame_cases(function, ps.CROSS[function])]


def pair_cases(cases):
    return [pytest.param("pairs" if taken else "declined pairs", levels, taken, id=("pair " if taken else "declined ") + size_id(levels)) for levels, taken in cases]


@pytest.mark.parametrize("origin,levels,option", frame_cases("down_mid"))
def test_down_mid_on_frames(gr, origin, levels, option):
    assert query(gr, "down_mid", levels) == 1
    check_down_pair(gr, MID, levels)


@pytest.mark.parametrize("origin,levels,taken", pair_cases(ps.down_pair_cases(MID)))
def test_down_mid_on_level_pairs(gr, origin, levels, taken):
    assert query(gr, "down_mid", levels) == int(taken)
    if not taken:
        decline_down_pair(gr, MID, levels)
    else:
        check_down_pair(gr, MID, levels)


@pytest.mark.parametrize("origin,levels,option", frame_cases("down_head"))
def test_down_head_on_frames(gr, origin, levels, option):
    assert query(gr, "down_head", levels) == 1
    check_head(gr, levels, b10=bool(option & 1), dynamic=bool(option & 2))


def test_down_head_is_declined_where_a_level_is_not_an_exact_half(gr):
    for w, h in ps.PARITY_SWEEP:
        levels = ps.frame_levels(w, h)
        if not ps.head_offered(levels):
            assert query(gr, "down_head", levels) == 0, (w, h)
    for w, h in ((66, 128), (132, 128), (136, 100)):  # the half, the quarter, the eighth level is a ceil
        levels = ps.frame_levels(w, h)
        hdr, t, d0, d1 = (image(gr, levels[n]) for n in ("hdr",) + MID)
        assert not gr.bloom_down_head(hdr, t, d0, d1)
        with pytest.raises(capi.GraniteHipError):
            gr.check(gr.lib.gr_bloom_down_head(gr.handle, None, hdr.desc, t.desc, d0.desc, d1.desc, None, capi.threshold_push(t), capi.downsample_push(d0, t),
                                               capi.downsample_push(d1, d0)))


@pytest.mark.parametrize("origin,levels,option", frame_cases("tail"))
def test_down_tail_and_up_tail_on_frames(gr, origin, levels, option):
    assert query(gr, "tail", levels) == 1
    d3_bits = check_down_pair(gr, TAIL, levels)
    check_up_tail(gr, levels, dynamic=bool(option & 1), d3_bits=d3_bits)


@pytest.mark.parametrize("origin,levels,taken", pair_cases(ps.down_pair_cases(TAIL)))
def test_down_tail_on_level_pairs(gr, origin, levels, taken):
    full = dict(levels, u2=levels["d2"], u1=(2 * levels["d2"][0], 2 * levels["d2"][1]))  # an upsample side that fits: the query's answer is the down rule's
    assert query(gr, "tail", full) == int(taken)
    if not taken:
        decline_down_pair(gr, TAIL, levels)
    else:
        check_down_pair(gr, TAIL, levels)


@pytest.mark.parametrize("origin,levels,taken", pair_cases(ps.up_tail_cases()))
def test_up_tail_on_level_pairs(gr, origin, levels, taken):
    full = dict(levels, d2=levels["u2"], d1=(2 * levels["u2"][0], 2 * levels["u2"][1]))
    assert query(gr, "tail", full) == int(taken)
    if not taken:
        decline_up_tail(gr, levels)
    else:
        for dynamic in (False, True):
            check_up_tail(gr, levels, dynamic)


@pytest.mark.parametrize("origin,levels,option", frame_cases("up_all"))
def test_up_all_on_frames(gr, origin, levels, option):
    assert query(gr, "up_all", levels) == 1
    check_up_all(gr, levels, dynamic=bool(option & 1))


@pytest.mark.parametrize("origin,levels,taken", pair_cases(ps.up_all_cases()))
def test_up_all_on_level_pairs(gr, origin, levels, taken):
    assert query(gr, "up_all", levels) == int(taken)
    if not taken:
        decline_up_all(gr, levels)
    else:
        for dynamic in (False, True):
            check_up_all(gr, levels, dynamic)


@pytest.mark.parametrize("origin,levels,option", frame_cases("pyramid"))
def test_pyramid_on_frames(gr, origin, levels, option):
    check_pyramid(gr, levels, b10=bool(option & 1), dynamic=bool(option & 2))


@pytest.mark.parametrize("levels", [pytest.param(l, id=size_id(l)) for l in ps.pyramid_offpyramid_cases()])
def test_pyramid_on_levels_no_frame_has(gr, levels):
    """Upsample-1 one texel off downsample-1's size: D2_EXACT != U1_EXACT (ps.pyramid_offpyramid_cases)."""
    for dynamic in (False, True):
        check_pyramid(gr, levels, b10=False, dynamic=dynamic)


# ---- C: the separate launches against the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", ps.PARITY_SWEEP)
def test_separate_launches_match_the_oracle_over_the_parity_sweep(gr, w, h):
    """Two frames, so that the feedback and the exposure are on in the second.  (The fused forms equal these launches byte for byte: above.)"""
    hdr = synth.make_hdr(w, h, seed=w * 1000 + h)
    ostate, gstate = {}, {}
    for frame in range(2):
        ref = orc.hdr_chain(hdr, ostate)
        got = run_chain_gpu(gr, hdr, gstate)
        for name in ("threshold", "d0", "d1", "d2", "d3", "u2", "u1", "u0"):
            assert ref[name].shape == got[name].shape, name
            assert_rgba16f_close(got[name], ref[name], what=f"{w}x{h} frame {frame} {name}")
        np.testing.assert_allclose(got["lum"][0], ref["lum"][0], atol=1e-5, rtol=0)
        np.testing.assert_allclose(got["lum"][1:], ref["lum"][1:], rtol=2e-5)
        assert_rgba8_close(got["tonemapped"], ref["tonemapped"], 1, what=f"{w}x{h} frame {frame} tonemapped")


def stage_pairs():
    """(kind, input size, output size) of every single stage among the taken level pairs."""
    stages = set()
    for names in (MID, TAIL):
        for levels, taken in ps.down_pair_cases(names):
            if taken:
                stages.add(("down", levels[names[0]], levels[names[1]]))
                stages.add(("down", levels[names[1]], levels[names[2]]))
    for levels, taken in ps.up_tail_cases() + ps.up_all_cases():
        if taken:
            stages.add(("up", levels["d3"], levels["u2"]))
            stages.add(("up", levels["u2"], levels["u1"]))
            if "u0" in levels:
                stages.add(("up", levels["u1"], levels["u0"]))
    return sorted(stages)


@pytest.mark.parametrize("kind,src_size,out_size", [pytest.param(*s, id="%s %dx%d->%dx%d" % (s[0], *s[1], *s[2])) for s in stage_pairs()])
def test_single_stages_match_the_oracle_on_the_level_pairs(gr, kind, src_size, out_size):
    """Each stage on identical input bits (no error carried from the stage before), at the sizes of the off-pyramid pairs."""
    bits = ps.random_level(src_size, src_size[0] * 131 + src_size[1] + out_size[0])
    src, out = image(gr, src_size, bits), image(gr, out_size)
    if kind == "down":
        gr.bloom_downsample(src, out)
        assert_rgba16f_close(out.download(), orc.bloom_downsample(bits, *out_size), what="downsample")
        hist_bits = ps.random_level(out_size, out_size[0] * 17 + out_size[1], -8, 4)
        gr.bloom_downsample(src, out, image(gr, out_size, hist_bits), 0.0667)
        assert_rgba16f_close(out.download(), orc.bloom_downsample(bits, *out_size, hist_bits, 0.0667), what="downsample(feedback)")
    else:
        gr.bloom_upsample(src, out)
        assert_rgba16f_close(out.download(), orc.bloom_upsample(bits, *out_size), what="upsample")
    stencil = src_size == (2 * out_size[0], 2 * out_size[1]) if kind == "down" else out_size == (2 * src_size[0], 2 * src_size[1])


# ---- D: special values -----------------------------------------------------------------------------------------------------------------------
def assert_same_class_and_close(got, want, what):
    """NaN, +inf and -inf where the oracle has them, position by position; the finite texels at the file's tolerance."""
    g, w = half_bits_to_f32(got), half_bits_to_f32(want)
    np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=what + ": NaN")
    np.testing.assert_array_equal(np.isposinf(g), np.isposinf(w), err_msg=what + ": +inf")
    np.testing.assert_array_equal(np.isneginf(g), np.isneginf(w), err_msg=what + ": -inf")
    finite = np.isfinite(w)
    assert_rgba16f_close(np.where(finite, got, 0), np.where(finite, want, 0), what=what)


def planted(size, seed):
    bits = ps.random_level(size, seed)
    ps.plant_specials(bits)
    return bits


def test_special_values_through_every_stage_match_the_oracle(gr):
    """+0, the smallest denormal, 65504 and +inf (whole texels) at an image corner, in the last column, at a tile corner and in the interior of
    each stage's input; sizes with partial tiles.  The oracle is the statement of what is right, and on these values it is itself held to the
    reference's shaders run on the CPU (tests/test_reference_shaders_cpu.py): an infinite HDR texel makes inf / inf = NaN in the threshold's
    colour, which max(., 0) turns into 0 (and log2(inf) = +inf in alpha)."""
    lum3 = np.array([0.5, 2.0 ** 0.5, 2.0 ** -0.5], np.float32)
    lumbuf = capi.DeviceBuffer(gr, 12).upload(lum3)
    for hdr_size, out_size, form in (((139, 97), (70, 49), "bilinear"), ((136, 98), (68, 49), "2:1")):
        bits = planted(hdr_size, 1)
        hdr, out = image(gr, hdr_size, bits), image(gr, out_size)
        for lum_ptr, l in ((None, None), (lumbuf.ptr, lum3)):
            gr.bloom_threshold(hdr, out, lum_ptr)
            want = orc.bloom_threshold(bits, *out_size, l)
            assert np.isposinf(half_bits_to_f32(want)[..., 3]).any() and not np.isnan(half_bits_to_f32(want)).any()
            assert_same_class_and_close(out.download(), want, f"threshold ({form}, {'dynamic' if l is not None else 'static'})")
    for src_size, out_size, form in (((75, 49), (38, 25), "nine taps"), ((76, 50), (38, 25), "2:1 stencil"), ((43, 43), (19, 19), "nine taps, 2.3 : 1")):
        bits, hist_bits = planted(src_size, 2), ps.random_level(out_size, 3, -8, 4)
        if min(out_size) >= 25:
            ps.plant_specials(hist_bits)
        src, out, hist = image(gr, src_size, bits), image(gr, out_size), image(gr, out_size, hist_bits)
        gr.bloom_downsample(src, out)
        want = orc.bloom_downsample(bits, *out_size)
        assert np.isinf(half_bits_to_f32(want)).any()
        assert_same_class_and_close(out.download(), want, f"downsample ({form})")
        gr.bloom_downsample(src, out, hist, 0.0667)
        assert_same_class_and_close(out.download(), orc.bloom_downsample(bits, *out_size, hist_bits, 0.0667), f"downsample ({form}, feedback)")
    for src_size, out_size, form in (((38, 25), (75, 49), "nine taps"), ((38, 25), (76, 50), "1:2 stencil"), ((38, 25), (38, 25), "taps on texel centres")):
        bits = planted(src_size, 4)
        src, out = image(gr, src_size, bits), image(gr, out_size)
        gr.bloom_upsample(src, out)
        want = orc.bloom_upsample(bits, *out_size)
        assert np.isinf(half_bits_to_f32(want)).any()
        assert_same_class_and_close(out.download(), want, f"upsample ({form})")


@pytest.mark.parametrize("w,h", [(136, 128), (139, 97), (152, 128)])
def test_special_values_fused_forms_equal_the_separate_launches(gr, w, h):
    """The planted images of the test above into every fused launch the frame is offered: NaN in the same places, everything else byte for byte.
    136 x 128 and 152 x 128 (downsample-1 17 and 19 wide: partial tiles; every launch; the levels below downsample-1 on the nine taps and on the
    stencils respectively) and 139 x 97 (no exact level: middle and tail only)."""
    assert (w, h) in ps.PARITY_SWEEP
    levels = ps.frame_levels(w, h)
    # the level each launch starts from must hold the planted texels: the tail starts at downsample-1, too small at these frames, so its input is
    # planted at the size of the half level instead (the launch takes any levels within its ratios)
    check_down_pair(gr, MID, levels, plant=True)
    big = {"d1": levels["threshold"], "d2": levels["d0"], "d3": levels["d1"], "u2": levels["d0"], "u1": levels["threshold"]}
    assert ps.tail_offered(big) and ps.down_extent(big["d2"], big["d3"])[0] <= ps.TAIL_PATCH
    check_down_pair(gr, TAIL, big, plant=True)
    # ... and once more with a downsample-3 large enough to hold planted texels in the feedback history too (an infinite history alpha: NaN in both
    # forms), downsample-3 on the stencil and on the nine taps
    thr = levels["threshold"]
    for d2 in ((2 * thr[0], 2 * thr[1]), (2 * thr[0] - 1, 2 * thr[1] - 1)):
        with_history = {"d1": (2 * d2[0], 2 * d2[1]), "d2": d2, "d3": thr}
        assert ps.down_tail_fits(with_history) and ps.down_extent(d2, thr)[0] <= ps.TAIL_PATCH
        check_down_pair(gr, TAIL, with_history, plant=True)
    up = {"d3": levels["threshold"], "u2": (2 * levels["threshold"][0] - 1, 2 * levels["threshold"][1]), "u1": (4 * levels["threshold"][0] - 2, 4 * levels["threshold"][1])}
    up["u0"] = (2 * up["u1"][0], 2 * up["u1"][1])
    assert ps.up_all_fits(up)
    for dynamic in (False, True):
        check_up_tail(gr, up, dynamic, plant=True)
        check_up_all(gr, up, dynamic, plant=True)
    if ps.head_offered(levels):
        for option in range(4):
            check_head(gr, levels, b10=bool(option & 1), dynamic=bool(option & 2), plant=True)
            check_pyramid(gr, levels, b10=bool(option & 1), dynamic=bool(option & 2), plant=True)


def test_special_values_pyramid_with_a_planted_history(gr):
    """The one-launch pyramid at 1280 x 832 (the launcher asked directly, as tests/test_gpu_post.py does for 720p: the query offers it up to 640 x 384),
    where downsample-3 is 40 x 26 and its feedback history holds the planted texels: NaN alpha where the history's is infinite, in both forms."""
    levels = ps.frame_levels(1280, 832)
    assert ps.pyramid_fits(levels) and levels["d3"] == (40, 26)
    for dynamic in (False, True):
        check_pyramid(gr, levels, b10=False, dynamic=dynamic, plant=True, ask=False)


def test_an_infinite_texel_stays_in_the_feedback_alpha(gr):
    """Four frames of the chain over a frame with one +inf texel, against the oracle (which the executed shaders pin on these values).  Frame 0:
    log2(inf) = +inf in the alpha of the levels under it.  From frame 1 on the history's alpha is infinite there, mix(history, value, 1) is
    inf * 0 + value = NaN, and NaN * 0 keeps it NaN in every later frame: the reference's behaviour, which the kernels reproduce -- a frame does
    not recover from an overflowed texel by itself."""
    w, h = 136, 128
    hdr = synth.make_hdr(w, h, seed=77)
    hdr[61, 70, :3] = 0x7c00
    ostate, gstate = {}, {}
    for frame in range(4):
        ref = orc.hdr_chain(hdr, ostate)
        got = run_chain_gpu(gr, hdr, gstate)
        for name in ("threshold", "d0", "d1", "d2", "d3", "u2", "u1", "u0"):
            assert_same_class_and_close(got[name], ref[name], f"frame {frame} {name}")
        alpha = half_bits_to_f32(got["d3"])[..., 3]
        assert np.isnan(alpha).any() == (frame > 0) and (frame > 0 or np.isinf(alpha).any())
        np.testing.assert_array_equal(np.isnan(got["lum"]), np.isnan(ref["lum"]))
        if not np.isnan(ref["lum"]).any():
            np.testing.assert_allclose(got["lum"][0], ref["lum"][0], atol=1e-5, rtol=0)
            np.testing.assert_allclose(got["lum"][1:], ref["lum"][1:], rtol=2e-5)
        assert_rgba8_close(got["tonemapped"], ref["tonemapped"], 1, what=f"frame {frame} tonemapped")


@pytest.mark.parametrize("fmt,fmt_name", [(capi.FORMAT_R8G8B8A8_SRGB, "rgba8_srgb"), (capi.FORMAT_R8G8B8A8_UNORM, "rgba8_unorm")])
@pytest.mark.parametrize("w,h", [(139, 97), (136, 128)])
def test_tonemap_of_special_values(gr, w, h, fmt, fmt_name):
    """A frame holding 0, the smallest denormal, 65504 and +inf: within 1 LSB of the oracle, and not a byte changed but at the planted texels (the
    pass reads the frame at texel centres: a planted texel is its own whole neighbourhood).  139 x 97: bloom by the bilinear fetch; 136 x 128:
    the 4 x bloom form.  Both stores."""
    levels = ps.frame_levels(w, h)
    plain = ps.random_level((w, h), 9, -6, 6)
    bits = plain.copy()
    positions = ps.plant_specials(bits)
    bloom_bits = ps.random_level(levels["u0"], 10, -8, 2)
    bloom = image(gr, levels["u0"], bloom_bits)
    lum3 = np.array([0.5, 2.0 ** 0.5, 2.0 ** -0.5], np.float32)
    lumbuf = capi.DeviceBuffer(gr, 12).upload(lum3)
    touched = np.zeros((h, w), bool)
    for x, y in positions:
        touched[y, x] = True
    for lum_ptr, l, exposure in ((lumbuf.ptr, lum3, 1.3), (None, None, 0.7)):
        outs = []
        for frame_bits in (plain, bits):
            out = image(gr, (w, h), fmt=fmt)
            gr.tonemap(image(gr, (w, h), frame_bits), bloom, out, lum_ptr, exposure)
            gr.sync()
            outs.append(out.download())
            assert_rgba8_close(outs[-1], orc.tonemap(frame_bits, bloom_bits, l, exposure, fmt_name), 1, what=f"tonemap {fmt_name}")
        changed = (outs[0] != outs[1]).any(axis=2)
        assert not (changed & ~touched).any(), f"{int((changed & ~touched).sum())} pixels away from the planted texels changed"
        assert changed.any()
