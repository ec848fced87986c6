"""GPU: gr_video_scale (VideoScaler::rescale + scaler.comp) against tests/video_ref.py.

Bounds, per sample:
  * 8-bit planes at the same size: 1 code.  The reference and the kernel compute the same expression, the reference in float64,
    the kernel in fp32 (the shader in fp16); a difference below 1e-5 can still fall on either side of a rounding midpoint.
  * 8-bit planes when rescaled: 2 codes.  The filter's input and its vertical result are fp16 in both (the shader's LDS tiles);
    accumulation order and the fp32 transfer functions move a value by a few fp16 ulps (2^-11 relative), which the sRGB encode
    near black (slope 12.92) can bring to a little over one code.
  * 16-bit planes: 64 of 65535.  The shader rounds the OETF result and the YCbCr value to fp16: one fp16 ulp at [0.5, 1) is
    2^-11 = 32 codes of 65535; the kernel keeps fp32 there, so it may sit up to two half-ulps from the shader's value.
Chroma is compared against the 2 x 2 mean (4:2:0) of the reference's per-pixel Cb / Cr.  Every plane lies in a buffer with a padded
row pitch and a guard after its last row: no byte outside the plane's extent may change.

Where the kernel is compared with the reference's shader executed on the CPU (oracle/ref_build/ref_video.cpp), the bound is the sum of
this file's bound and the shader-against-video_ref bound of tests/test_video_shader_cpu.py (1 code at 8 bits, 64 at 16 bits).
"""
import ctypes as C

import numpy as np
import pytest

import video_ref as vr
from granite_amd import capi
from video_planes import EDGE_SIZES, GuardedImage, nv12, yuv

pytestmark = pytest.mark.gpu

S, HDR, LIN = capi.COLOR_SPACE_SRGB_NONLINEAR, capi.COLOR_SPACE_HDR10_ST2084, capi.COLOR_SPACE_EXTENDED_SRGB_LINEAR


def make_input(gr, fmt, w, h, seed, smooth=False, offset=0, pad=None):
    """Input texels and their image; `offset` / `pad` place the image `offset` bytes into its buffer with a pitch of row + pad bytes
    (a pitch or offset that is not a multiple of 16 takes the texel-by-texel loads)."""
    rng = np.random.default_rng(seed)
    if fmt in (vr.RGBA8, vr.RGBA8_SRGB):
        data = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        # smooth regions next to the noise: the filter's DC path and the chroma mean of flat blocks
        data[: h // 4] = (np.linspace(0, 255, w)[None, :, None] * np.array([1.0, 0.6, 0.3, 1.0])).astype(np.uint8)
    elif fmt == vr.A2B10G10R10:
        c = rng.integers(0, 1024, (h, w, 3), dtype=np.uint32)
        if smooth:  # diagonal ramps with +-8 codes of noise
            ramp = (np.arange(w)[None, :, None] * 700 // w + np.arange(h)[:, None, None] * 300 // h) * np.array([1, 1, 1])[None, None]
            c = np.clip(ramp + rng.integers(-8, 9, (h, w, 3)), 0, 1023).astype(np.uint32)
        data = c[..., 0] | (c[..., 1] << 10) | (c[..., 2] << 20) | np.uint32(3 << 30)
    elif smooth:  # RGBA16F ramps with 2 % noise
        ramp = np.arange(w)[None, :, None] * 0.7 / w + np.arange(h)[:, None, None] * 0.3 / h + np.array([0.05, 0.1, 0.15, 1.0])
        data = (ramp * rng.uniform(0.98, 1.02, (h, w, 4))).astype(np.float16).view(np.uint16)
    else:
        data = rng.uniform(0.0, 1.2, (h, w, 4)).astype(np.float16).view(np.uint16)
    if not offset and pad is None:
        return data, capi.DeviceImage(gr, w, h, fmt).upload(data)
    return data, GuardedImage(gr, w, h, fmt, data, offset, pad)


def run_case(gr, in_fmt, in_size, planes, src_space, dst_space, tol, seed=1, smooth=False, offset=0, pad=None, in_offset=0, in_pad=None):
    data, img = make_input(gr, in_fmt, in_size[0], in_size[1], seed, smooth, in_offset, in_pad)
    outs = [GuardedImage(gr, *p, offset=offset, pad=pad) for p in planes]
    arr = (capi.Image * len(outs))(*[o.desc for o in outs])
    gr.check(gr.lib.gr_video_scale(gr.handle, None, img.desc, arr, len(outs), src_space, dst_space))
    gr.sync()
    got = [o.samples() for o in outs]
    ref = vr.video_scale(data, in_fmt, planes, src_space, dst_space)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape, (i, g.shape, r.shape)
        err = np.abs(g.astype(np.int64) - r)
        worst = np.unravel_index(np.argmax(err), err.shape)
        assert err.max() <= tol, f"plane {i}: {int((err > tol).sum())} samples beyond {tol} codes, worst {err.max()} at {worst}"
    return got


SAME_SIZE_LAYOUTS = {
    "nv12": lambda w, h: nv12(w, h),
    "yuv420p": lambda w, h: yuv(w, h),
    "yuv444p": lambda w, h: yuv(w, h, sub=False),
    "rgba8_dither": lambda w, h: [(w, h, vr.RGBA8)],
    "bgra8_dither": lambda w, h: [(w, h, vr.BGRA8_SRGB)],
    "yuv420p16": lambda w, h: yuv(w, h, wide=True),
}


@pytest.mark.parametrize("layout", sorted(SAME_SIZE_LAYOUTS))
@pytest.mark.parametrize("size", [(3840, 2160), (1277, 719)], ids=["4k", "odd"])
def test_same_size_from_srgb_rgba8(gr, size, layout):
    planes = SAME_SIZE_LAYOUTS[layout](*size)
    run_case(gr, vr.RGBA8, size, planes, S, S, 64 if planes[0][2] == vr.R16 else 1)


@pytest.mark.parametrize("layout", ["nv12", "yuv420p", "yuv444p", "rgba8_dither", "yuv420p16"])
def test_unaligned_planes(gr, layout):
    # plane pointers 4 bytes into their buffers and pitches of row + 4: vector stores are off, every sample goes out on its own
    for size in ((3840, 2160), (1277, 719)):
        planes = SAME_SIZE_LAYOUTS[layout](*size)
        run_case(gr, vr.RGBA8, size, planes, S, S, 64 if planes[0][2] == vr.R16 else 1, offset=4, pad=4)
    run_case(gr, vr.RGBA8, (2560, 1440), nv12(1920, 1080), S, S, 2, offset=4, pad=4)


def test_same_size_srgb_view_input(gr):
    # an *_SRGB input decodes through the view and the sRGB OETF re-encodes: no cancellation
    run_case(gr, vr.RGBA8_SRGB, (1277, 719), nv12(1277, 719), S, S, 1)


def test_p010_from_hdr10_target(gr):
    run_case(gr, vr.A2B10G10R10, (3840, 2160), nv12(3840, 2160, wide=True), HDR, HDR, 64)


def test_srgb_to_hdr10_with_primary_conversion(gr):
    run_case(gr, vr.RGBA8, (1920, 1080), nv12(1920, 1080, wide=True), S, HDR, 64)


def test_hdr10_to_srgb(gr):
    # BT.2020 -> BT.709 of out-of-gamut colours in nits (sdr_scale 1): a channel can be the difference of terms of up to 10^4 that
    # cancel to below 1, where fp32 keeps ~1e-3 of absolute error and the sRGB encode (slope 12.92 near black) turns it into a few
    # codes.  The shader holds these nits in fp16 (ulp 4 at 8000), far coarser; 8 codes bound the fp32 kernel.
    run_case(gr, vr.A2B10G10R10, (1277, 719), nv12(1277, 719), HDR, S, 8)


def test_rgba16f_input(gr):
    # scRGB -> sRGB scales by 80 (sdr_scale) and saturates most colour: the sRGB -> sRGB run checks the colour channels of the
    # RGBA16F fetch, this one the primary conversion with alpha passed through; 4K takes the 32-B vector loads, the odd width the
    # texel-by-texel ones
    run_case(gr, vr.RGBA16F, (1277, 719), [(1277, 719, vr.RGBA8)], LIN, S, 1)
    run_case(gr, vr.RGBA16F, (3840, 2160), [(3840, 2160, vr.RGBA8)], S, S, 1)
    run_case(gr, vr.RGBA16F, (1277, 719), yuv(1277, 719), S, S, 1)


@pytest.mark.parametrize("case", [
    ((3840, 2160), nv12(1920, 1080)),
    ((2560, 1440), yuv(1920, 1080)),
    ((1280, 720), nv12(1920, 1080)),
    ((7680, 4320), nv12(1920, 1080)),
    ((1280, 720), yuv(1919, 1081, sub=False)),
], ids=["4k_to_1080p", "1440p_to_1080p", "720p_to_1080p", "8k_to_1080p_sampled", "720p_to_odd_444"])
def test_rescale(gr, case):
    in_size, planes = case
    run_case(gr, vr.RGBA8, in_size, planes, S, S, 2)


def test_rescale_to_rgba8(gr):
    # Per-channel sRGB output of a filtered noise frame: the fp16 tiles of kernel and reference can differ by one fp16 ulp where the
    # fp32 and float64 sums straddle a rounding point (2^-11 at magnitudes in [0.5, 1)); through a tap weight near 1 and the sRGB
    # encode's slope of 12.92 near black that is 12.92 * 255 / 2048 = 1.6 codes per differing tap, so two such taps reach 4.  The
    # YCbCr planes above average three channels and stay within 2.
    run_case(gr, vr.RGBA8, (2560, 1440), [(1917, 1083, vr.RGBA8)], S, S, 4)


def test_rescale_16_bit(gr):
    # PQ in, PQ out, filtered in nits: on full-range noise the sinc's negative lobes cancel terms of up to 10^4 nits down to near
    # black, where fp16 staging (ulp 8 at 10^4, in the shader as here) meets PQ's unbounded slope and any two roundings disagree by
    # thousands of codes.  A ramp with +-8 codes of noise keeps the filtered values away from that cliff.
    run_case(gr, vr.A2B10G10R10, (3840, 2160), nv12(1920, 1080, wide=True), HDR, HDR, 64, smooth=True)


def test_refusals_report_an_error(gr):
    data, img = make_input(gr, vr.RGBA8, 64, 32, 3)
    y = GuardedImage(gr, 64, 32, vr.R8)
    c = GuardedImage(gr, 31, 16, vr.R8G8)  # neither half nor full size
    arr = (capi.Image * 2)(y.desc, c.desc)
    rc = gr.lib.gr_video_scale(gr.handle, None, img.desc, arr, 2, S, S)
    assert rc == -1 and b"chroma" in gr.lib.gr_last_error(gr.handle)
    good = GuardedImage(gr, 32, 16, vr.R8G8)
    arr = (capi.Image * 2)(y.desc, good.desc)
    assert gr.lib.gr_video_scale(gr.handle, None, img.desc, arr, 2, S, LIN) == -1
    assert gr.lib.gr_video_scale(gr.handle, None, img.desc, arr, 2, 7, S) == -1
    gr.sync()
    # nothing was launched: the planes still hold the fill
    assert y.untouched()


# ---- edge shapes -----------------------------------------------------------------------------------------------------------------
# The direct path runs over EDGE_SIZES (tests/video_planes.py); the rescale path converts 16 x 16 outputs per group from a staging
# window of at most STAGE = 41 texels per axis, with the prefilter above a ratio of 2: RESCALE_EDGES below.
def assert_refused(gr, in_size, planes):
    """A 4:2:0 frame one pixel wide has chroma as wide as its luma: the plan (as VideoScaler::rescale) tells subsampling by the
    width alone, so the chroma height does not match and the conversion is refused, with nothing written."""
    data, img = make_input(gr, vr.RGBA8, in_size[0], in_size[1], 1)
    outs = [GuardedImage(gr, *p) for p in planes]
    arr = (capi.Image * len(outs))(*[o.desc for o in outs])
    assert gr.lib.gr_video_scale(gr.handle, None, img.desc, arr, len(outs), S, S) == -1
    assert b"chroma" in gr.lib.gr_last_error(gr.handle)
    gr.sync()
    for o in outs:
        assert o.untouched()


@pytest.mark.parametrize("layout", sorted(SAME_SIZE_LAYOUTS) + ["p010_pq"])
def test_same_size_edge_shapes(gr, layout):
    for size in EDGE_SIZES:
        if layout == "p010_pq":
            args = (vr.A2B10G10R10, size, nv12(*size, wide=True), HDR, HDR, 64)
        else:
            planes = SAME_SIZE_LAYOUTS[layout](*size)
            args = (vr.RGBA8, size, planes, S, S, 64 if planes[0][2] == vr.R16 else 1)
        if len(args[2]) > 1 and size[0] == 1 and args[2][1][1] < size[1]:
            assert_refused(gr, size, args[2])
            continue
        run_case(gr, *args)
        # input 4 bytes into its buffer with a pitch of row + 4 (its vector loads are off), planes likewise
        run_case(gr, *args, seed=2, offset=4, pad=4, in_offset=4, in_pad=4)


def test_same_size_unaligned_rgba16f_input(gr):
    for size in ((1023, 7), (257, 3), (1, 1)):
        run_case(gr, vr.RGBA16F, size, [(size[0], size[1], vr.RGBA8)], S, S, 1, in_offset=4, in_pad=12)
        run_case(gr, vr.RGBA16F, size, yuv(*size), S, S, 1, in_offset=4, in_pad=12)


RESCALE_EDGES = {
    # outputs of 1, 15, 16, 17, 31 and 33 on each axis: partial 16 x 16 tiles, one-pixel planes, odd 4:2:0
    **{f"out_{n}x17": ((3 * n // 2 + 1, 25), nv12(n, 17) if n > 1 else yuv(n, 17, sub=False)) for n in (1, 15, 16, 17, 31, 33)},
    **{f"out_17x{n}": ((25, 3 * n // 2 + 1), yuv(17, n)) for n in (1, 15, 16, 17, 31, 33)},
    # a ratio of exactly 2: the widest staging window without the prefilter
    "ratio2_64": ((64, 64), nv12(32, 32)),
    "ratio2_2048": ((2048, 32), nv12(1024, 16)),
    "ratio2_7680": ((7680, 16), nv12(3840, 8)),
    # just above 2: the prefilter at twice the output size
    "above2_129": ((129, 64), nv12(64, 32)),
    "above2_2049": ((2049, 33), yuv(1024, 16)),
    # anisotropic: one axis prefiltered, the other not
    "aniso_x_sampled": ((400, 90), nv12(120, 80)),
    "aniso_y_sampled": ((90, 400), yuv(80, 120)),
    "aniso_up_x_sampled_y": ((60, 300), nv12(90, 100)),
    # inputs smaller than the 8 taps
    "tiny_1x1": ((1, 1), nv12(64, 64)),
    "tiny_3x2": ((3, 2), nv12(64, 64)),
    "tiny_5x7": ((5, 7), yuv(64, 64)),
    # odd 4:2:0 from 4K
    "4k_to_odd_nv12": ((3840, 2160), nv12(1279, 719)),
    "4k_to_odd_yuv420p": ((3840, 2160), yuv(1279, 719)),
}


@pytest.mark.parametrize("case", sorted(RESCALE_EDGES))
def test_rescale_edge_shapes(gr, case):
    in_size, planes = RESCALE_EDGES[case]
    run_case(gr, vr.RGBA8, in_size, planes, S, S, 2)
    if case == "out_1x17":
        assert_refused(gr, in_size, nv12(1, 17))


@pytest.mark.parametrize("in_size", [(1, 1), (3, 2), (5, 7)], ids=["1x1", "3x2", "5x7"])
def test_tiny_input_upscaled_16_bit(gr, in_size):
    # 16 bits resolve a position one phase step (1/256 texel) off next to a texel step: the first outputs of an upscale sit at
    # negative positions, where int() truncates toward zero and floor() would not
    run_case(gr, vr.RGBA8, in_size, nv12(64, 64, wide=True), S, S, 64)
    run_case(gr, vr.RGBA8, in_size, yuv(64, 64, sub=False, wide=True), S, S, 64)


def test_rescale_dithered_rgba8_and_bgra8(gr):
    # bound 4: see test_rescale_to_rgba8
    run_case(gr, vr.RGBA8, (300, 170), [(71, 45, vr.RGBA8)], S, S, 4)
    run_case(gr, vr.RGBA8, (64, 48), [(96, 72, vr.BGRA8_SRGB)], S, S, 4)
    run_case(gr, vr.RGBA8, (1920, 1080), [(1279, 719, vr.BGRA8_SRGB)], S, S, 4)


def test_rescale_scrgb_to_p010(gr):
    # ramps with 2 % noise, as test_rescale_16_bit: filtered noise that cancels to near black meets PQ's unbounded slope there
    run_case(gr, vr.RGBA16F, (1921, 1081), nv12(1280, 720, wide=True), LIN, HDR, 64, smooth=True)


def test_dither_table_and_index_exact(gr):
    # tests/video_ref.py dither_probe: every code is decided by the dither term alone, 1/32 of a code from any midpoint
    data, want = vr.dither_probe()
    for fmt in (vr.RGBA8, vr.BGRA8):
        img = capi.DeviceImage(gr, 64, 16, vr.RGBA16F).upload(data)
        out = GuardedImage(gr, 64, 16, fmt)
        arr = (capi.Image * 1)(out.desc)
        gr.check(gr.lib.gr_video_scale(gr.handle, None, img.desc, arr, 1, LIN, LIN))
        gr.sync()
        assert np.array_equal(out.samples(), want), fmt


def _launch(gr, img, planes, src, dst, stream):
    outs = [GuardedImage(gr, *p) for p in planes]
    arr = (capi.Image * len(outs))(*[o.desc for o in outs])
    gr.check(gr.lib.gr_video_scale(gr.handle, stream, img.desc, arr, len(outs), src, dst))
    return outs


def test_weight_cache_switches_size_pairs_across_streams(gr):
    """One context runs size pair A, then B, then A again, the launches on two streams; each result equals a fresh context's output
    byte for byte (a table keyed or uploaded wrongly would filter with the other pair's weights)."""
    hip = C.CDLL("libamdhip64.so")
    streams = [C.c_void_p(), C.c_void_p()]
    for st in streams:
        assert hip.hipStreamCreate(C.byref(st)) == 0
    try:
        pairs = {"A": ((1920, 1080), nv12(1280, 720)), "B": ((1280, 720), nv12(1920, 1080))}
        inputs = {k: make_input(gr, vr.RGBA8, *v[0], seed=5) for k, v in pairs.items()}
        got = []
        for key, st in (("A", streams[0]), ("B", streams[1]), ("A", streams[1])):
            got.append((key, _launch(gr, inputs[key][1], pairs[key][1], S, S, st.value)))
        for st in streams:
            gr.sync(st.value)
        for key, outs in got:
            fresh = capi.Context(0)
            try:
                data, img = make_input(fresh, vr.RGBA8, *pairs[key][0], seed=5)
                want = _launch(fresh, img, pairs[key][1], S, S, None)
                fresh.sync()
                for o, w in zip(outs, want):
                    assert np.array_equal(o.samples(), w.samples()), key
            finally:
                fresh.close()
    finally:
        for st in streams:
            hip.hipStreamDestroy(st)


# ---- the kernel against the reference's shader, executed on the CPU ------------------------------------------------------------
SHADER_CASES = {
    "same_odd_nv12": (vr.RGBA8, (67, 35), nv12(67, 35), S, S, 1 + 1),
    "same_odd_yuv420p16": (vr.RGBA8, (67, 35), yuv(67, 35, wide=True), S, S, 64 + 64),
    "down2_odd_yuv420p": (vr.RGBA8, (258, 130), yuv(129, 65), S, S, 2 + 1),
    "up1.5_odd_nv12": (vr.RGBA8, (134, 90), nv12(201, 135), S, S, 2 + 1),
    "sampled_odd_nv12": (vr.RGBA8, (320, 180), nv12(97, 55), S, S, 2 + 1),
    "down1.5_rgba8_dither": (vr.RGBA8, (150, 90), [(100, 60, vr.RGBA8)], S, S, 4 + 1),
    "same_odd_p010_pq": (vr.A2B10G10R10, (67, 35), nv12(67, 35, wide=True), HDR, HDR, 64 + 64),
}


@pytest.mark.parametrize("case", sorted(SHADER_CASES))
def test_kernel_matches_executed_shader(gr, case):
    in_fmt, in_size, planes, src, dst, tol = SHADER_CASES[case]
    data, img = make_input(gr, in_fmt, in_size[0], in_size[1], 3, smooth=in_fmt == vr.A2B10G10R10)
    outs = _launch(gr, img, planes, src, dst, None)
    gr.sync()
    p = capi.video_scale_plan(in_size, in_fmt, planes, src, dst)
    want = vr.shader_scale(data, in_fmt, planes, p, capi.video_scaler_weights(in_size[0], in_size[1], planes[0][0], planes[0][1]))
    for i, (o, w) in enumerate(zip(outs, want)):
        err = np.abs(o.samples().astype(np.int64) - w)
        assert err.max() <= tol, f"plane {i}: {int((err > tol).sum())} samples beyond {tol}, worst {err.max()}"
