"""CPU: tests/video_ref.py against the reference's own scaler.comp, executed.

oracle/ref_build/ref_video.cpp runs util/scaler.comp (re-spelled by glsl2cpp.py, compiled against glsl_cpu.hpp) on the CPU: 64-thread
workgroups over the 8 x 8 output tiles, team barriers, quad swaps, fp16 arithmetic rounded after every operation.  It takes the
plan and the fp16 weight table of the product's host half (gr_video_scale_plan, gr_video_scaler_weights), so what is compared is
video_ref's reading of the shader's pixel arithmetic: sample positions, taps, staging, transfer functions, matrices, chroma mean,
dither and stores.  The GPU tests compare the kernel with video_ref; these tests pin video_ref to the shader.

Bounds, per sample (shader against video_ref):
  * 8-bit planes: 1 code, and at least 90 % of the samples of each plane exact.  The shader rounds to fp16 after every operation
    from the fetch on (the EOTF, the filter's products and sums, the primary conversion, the OETF, the YCbCr value); video_ref keeps
    float64 except at the filter's two fp16 tiles.  One rounding moves a value in [0, 1] by at most 2^-12 (half an ulp at [0.5, 1)),
    0.06 of a code; the roundings are of both signs and a few of them in series stay below one code, but any of them can carry a
    value across a code's midpoint.  A misread constant, position, tap, transfer or dither term moves whole codes on many samples
    and fails the share before the bound.
  * 16-bit planes: 64 of 65535, and at least 90 % within 32.  The shader's last two roundings are the OETF result and the YCbCr
    value, each up to 2^-12 = 16 codes at [0.5, 1); the fp16 input (2^-12 relative) and the fp16 filter sums add as much again on
    the samples where they line up.  64 is also the GPU tests' bound for the kernel, so the two bounds add to 128 where the kernel
    is compared with the shader directly.
Exact, with no tolerance: the dither table and its index (a flat-per-block RGBA16F frame whose codes depend only on the dither
term), and the 8.8 sample positions and taps (a one-hot weight table that turns the filter into a texel lookup of a frame whose
texels encode their own coordinates).
"""
import numpy as np
import pytest

import video_ref as vr
from granite_amd import capi
from video_planes import nv12, yuv

S, HDR, LIN = capi.COLOR_SPACE_SRGB_NONLINEAR, capi.COLOR_SPACE_HDR10_ST2084, capi.COLOR_SPACE_EXTENDED_SRGB_LINEAR


def make_input(fmt, w, h, seed, src, dst):
    """Noise with a smooth band (8-bit), a smooth ramp with +-8 codes of noise (A2B10G10R10: PQ's slope near black turns any two
    roundings of a filtered value that cancels to black into thousands of codes), or scRGB noise.  Inputs that would saturate the
    output are kept below it: scRGB below 1.2 / 80 (the 80-nit scale), PQ below code 160 (1 nit = 1.0 into sRGB): saturated white
    puts Cb / Cr on 0.5 exactly, a rounding midpoint of every format, where any two evaluations may round apart."""
    rng = np.random.default_rng(seed)
    if fmt in (vr.RGBA8, vr.RGBA8_SRGB):
        data = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        data[: h // 4] = (np.linspace(0, 255, w)[None, :, None] * np.array([1.0, 0.6, 0.3, 1.0])).astype(np.uint8)
        return data
    if fmt == vr.A2B10G10R10:
        peak = 160 if dst == S else 1000
        ramp = np.arange(w)[None, :, None] * 7 * peak // (10 * w) + np.arange(h)[:, None, None] * 3 * peak // (10 * h) + np.zeros((1, 1, 3), np.int64)
        c = np.clip(ramp + rng.integers(-8, 9, (h, w, 3)), 0, 1023).astype(np.uint32)
        return c[..., 0] | (c[..., 1] << 10) | (c[..., 2] << 20) | np.uint32(3 << 30)
    top = 1.2 / 80.0 if src == LIN else 1.0
    return rng.uniform(0.0, top, (h, w, 4)).astype(np.float16).view(np.uint16)


def shader(data, in_fmt, planes, src, dst, weights=None):
    in_h, in_w = data.shape[:2]
    p = capi.video_scale_plan((in_w, in_h), in_fmt, planes, src, dst)
    assert p is not None
    if weights is None:
        weights = capi.video_scaler_weights(in_w, in_h, planes[0][0], planes[0][1])
    return vr.shader_scale(data, in_fmt, planes, p, weights)


def check_bounds(got, ref, planes, what):
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape, (what, i, g.shape, r.shape)
        err = np.abs(g - r)
        wide = planes[min(i, len(planes) - 1)][2] in (vr.R16, vr.R16G16)
        bound, near, share = (64, 32, 0.9) if wide else (1, 0, 0.9)
        worst = np.unravel_index(np.argmax(err), err.shape)
        assert err.max() <= bound, f"{what} plane {i}: {int((err > bound).sum())} samples beyond {bound}, worst {err.max()} at {worst}"
        assert (err <= near).mean() >= share, f"{what} plane {i}: only {(err <= near).mean():.3f} of the samples within {near}"


# (input format, input size, planes, source space, destination space)
CASES = {
    # paths, NV12 from RGBA8 sRGB
    "same_odd_nv12": (vr.RGBA8, (67, 35), nv12(67, 35), S, S),
    "down1.5_nv12": (vr.RGBA8, (192, 108), nv12(128, 72), S, S),
    "down2_odd_nv12": (vr.RGBA8, (258, 130), nv12(129, 65), S, S),
    "up1.5_odd_nv12": (vr.RGBA8, (134, 90), nv12(201, 135), S, S),
    "up7_odd_nv12": (vr.RGBA8, (37, 23), nv12(259, 161), S, S),
    "sampled_odd_nv12": (vr.RGBA8, (480, 270), nv12(97, 55), S, S),
    "aniso_sampled_x_down_y": (vr.RGBA8, (400, 90), nv12(120, 80), S, S),
    "aniso_up_x_sampled_y": (vr.RGBA8, (60, 300), nv12(90, 100), S, S),
    # outputs
    "same_rgba8_dither": (vr.RGBA8, (67, 35), [(67, 35, vr.RGBA8)], S, S),
    "same_bgra8_dither": (vr.RGBA8, (67, 35), [(67, 35, vr.BGRA8)], S, S),
    "down1.5_rgba8_dither": (vr.RGBA8, (150, 90), [(100, 60, vr.RGBA8)], S, S),
    "up1.5_bgra8_srgb_dither": (vr.RGBA8, (64, 48), [(96, 72, vr.BGRA8_SRGB)], S, S),
    "sampled_rgba8_dither": (vr.RGBA8, (300, 170), [(71, 45, vr.RGBA8)], S, S),
    "same_odd_yuv420p": (vr.RGBA8, (67, 35), yuv(67, 35), S, S),
    "down2_odd_yuv420p": (vr.RGBA8, (258, 130), yuv(129, 65), S, S),
    "sampled_odd_yuv420p": (vr.RGBA8, (333, 200), yuv(77, 41), S, S),
    "same_odd_yuv444p": (vr.RGBA8, (67, 35), yuv(67, 35, sub=False), S, S),
    "up1.5_yuv444p": (vr.RGBA8, (64, 48), yuv(96, 72, sub=False), S, S),
    "same_odd_yuv420p16": (vr.RGBA8, (67, 35), yuv(67, 35, wide=True), S, S),
    # inputs and transfers
    "same_odd_p010_pq": (vr.A2B10G10R10, (67, 35), nv12(67, 35, wide=True), HDR, HDR),
    "down1.5_p010_pq": (vr.A2B10G10R10, (192, 108), nv12(128, 72, wide=True), HDR, HDR),
    "same_odd_srgb_view": (vr.RGBA8_SRGB, (67, 35), nv12(67, 35), S, S),
    "down1.5_srgb_view": (vr.RGBA8_SRGB, (192, 108), nv12(128, 72), S, S),
    "same_scrgb_to_rgba8": (vr.RGBA16F, (67, 35), [(67, 35, vr.RGBA8)], LIN, S),
    "down1.5_scrgb_to_nv12": (vr.RGBA16F, (192, 108), nv12(128, 72), LIN, S),
    "down1.5_scrgb_to_p010": (vr.RGBA16F, (193, 109), nv12(129, 73, wide=True), LIN, HDR),
    "same_srgb_to_p010_primary": (vr.RGBA8, (67, 35), nv12(67, 35, wide=True), S, HDR),
    "same_pq_to_nv12_primary": (vr.A2B10G10R10, (67, 35), nv12(67, 35), HDR, S),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_video_ref_matches_executed_shader(case):
    in_fmt, in_size, planes, src, dst = CASES[case]
    data = make_input(in_fmt, in_size[0], in_size[1], 7, src, dst)
    got = shader(data, in_fmt, planes, src, dst)
    ref = vr.video_scale(data, in_fmt, planes, src, dst)
    check_bounds(got, ref, planes, case)


def test_matrix_covers_every_path_layout_and_transfer():
    plans = [capi.video_scale_plan(c[1], c[0], c[2], c[3], c[4]) for c in CASES.values()]
    flags = [p["flags"] for p in plans]
    for bit in (vr.SKIP, vr.DOWN, vr.SAMPLED, vr.CHROMA, vr.PRIMARY, vr.DITHER):
        assert any(f & bit for f in flags) and any(not f & bit for f in flags), bit
    assert {(p["eotf"], p["oetf"]) for p in plans} >= {(vr.T_ID, vr.T_ID), (vr.T_SRGB, vr.T_SRGB), (vr.T_ID, vr.T_SRGB), (vr.T_PQ, vr.T_PQ),
                                                         (vr.T_SRGB, vr.T_PQ), (vr.T_PQ, vr.T_SRGB), (vr.T_ID, vr.T_PQ)}
    # odd 4:2:0 on both paths: the chroma mean of a 2 x 2 block that reaches past the frame
    assert any(p["flags"] & vr.SKIP and p["flags"] & vr.CHROMA for p, c in zip(plans, CASES.values()) if c[2][0][0] % 2)
    assert any(not p["flags"] & vr.SKIP and p["flags"] & vr.CHROMA for p, c in zip(plans, CASES.values()) if c[2][0][0] % 2)


# ---- exact: dither ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [vr.RGBA8, vr.BGRA8])
def test_dither_table_and_index_exact(fmt):
    data, want = vr.dither_probe()
    planes = [(64, 16, fmt)]
    assert np.array_equal(shader(data, vr.RGBA16F, planes, LIN, LIN)[0], want)
    assert np.array_equal(vr.video_scale(data, vr.RGBA16F, planes, LIN, LIN)[0], want)


# ---- exact: sample positions and taps ----------------------------------------------------------------------------------------
def one_hot_table():
    """(2, 256, 8) fp16 bits: phase p weighs tap p % 8 (horizontal) or tap (p * 3 + 1) % 8 (vertical) by 1.0 and the others by 0.
    The filter then returns one staged texel exactly, in fp16 and in float64 alike, and which one depends on the integer position
    and on the low bits of the phase: a position one phase step off reads a neighbouring texel."""
    t = np.zeros((2, 256, 8), np.uint16)
    p = np.arange(256)
    t[0, p, p % 8] = 0x3C00
    t[1, p, (p * 3 + 1) % 8] = 0x3C00
    return t


def coordinate_frame(w, h):
    """RGBA16F: R encodes the column, G the row, B both, as (2m + 1) / 128 (exact in fp16); 255 v + n / 16 is then never within 1/128
    of an integer, so every dithered code is decided away from a midpoint."""
    y, x = np.mgrid[0:h, 0:w]
    enc = lambda m: (2 * (m % 64) + 1) / 128
    rgba = np.stack([enc(x), enc(y), enc(3 * x + 5 * y), np.ones_like(x, np.float64)], axis=-1)
    return rgba.astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("sizes", [((40, 30), (60, 45)), ((9, 5), (64, 37)), ((96, 60), (64, 40)), ((128, 64), (64, 32)),
                                   ((96, 30), (48, 41)), ((3, 2), (64, 64))],
                         ids=["up1.5", "up7", "down1.5", "down2", "aniso_down2_up", "tiny_up"])
def test_sample_positions_and_taps_exact(sizes):
    (iw, ih), (ow, oh) = sizes
    data = coordinate_frame(iw, ih)
    planes = [(ow, oh, vr.RGBA8)]
    table = one_hot_table()
    got = shader(data, vr.RGBA16F, planes, LIN, LIN, weights=table)
    ref = vr.video_scale(data, vr.RGBA16F, planes, LIN, LIN, weights=table)[0]
    assert np.array_equal(got[0], ref), f"{int((got[0] != ref).sum())} samples differ"
