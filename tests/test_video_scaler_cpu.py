"""CPU: the host half of gr_video_scale (VideoScaler::rescale / update_weights, video/scaler.cpp) against tests/video_ref.py, and the
static resources of its kernels.  No device needed: gr_video_scaler_weights and gr_video_scale_plan are host-only."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import video_ref as vr
from granite_amd import capi
from video_planes import nv12, yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sizes", [(1920, 1080, 1920, 1080), (3840, 2160, 1920, 1080), (1920, 1080, 1280, 720), (1280, 720, 1920, 1080),
                                   (7680, 4320, 1920, 1080)], ids=["1to1", "2to1", "1.5to1", "1to1.5", "4to1_clamped"])
def test_weight_table_matches_update_weights(sizes):
    got = capi.video_scaler_weights(*sizes)
    ref = vr.scaler_weights(*sizes)
    assert got.shape == (2, 256, 8)
    assert (got == ref).mean() >= 0.999
    # within one fp16 ulp everywhere: neighbouring bit patterns of the same sign
    assert np.abs(got.astype(np.int64) - ref.astype(np.int64)).max() <= 1
    w = got.view(np.float16).astype(np.float64)
    # normalised per phase: 8 fp16 roundings of weights below 1.25 move the sum by at most 8 half-ulps of 1.25 (2^-11 each)
    assert np.abs(w.sum(axis=2) - 1.0).max() <= 8 * 2.0 ** -11
    # phase 0 of the same-size table is the identity tap (sinc at integers)
    if sizes[:2] == sizes[2:]:
        assert np.array_equal(w[:, 0], np.tile([0, 0, 0, 1, 0, 0, 0, 0], (2, 1)))


def test_float_to_half_rounds_ties_away_from_zero():
    v = np.array([1 + 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 3 * 2.0 ** -11, 2.0 ** -25, 0.1], np.float32)
    assert list(vr.float_to_half_away(v)) == [0x3c01, 0xbc01, 0x3c02, 0x0001, 0x2e66]


S, HDR, LIN = capi.COLOR_SPACE_SRGB_NONLINEAR, capi.COLOR_SPACE_HDR10_ST2084, capi.COLOR_SPACE_EXTENDED_SRGB_LINEAR
K4, K2, P1080 = (3840, 2160), (2560, 1440), (1920, 1080)


PLAN_CASES = {
    # the recorder's case: same size, same transfer -> SKIP with the EOTF / OETF cancelled
    "skip_nv12": (K4, vr.RGBA8, nv12(*K4), S, S, vr.SKIP | vr.CLAMP | vr.CHROMA, vr.T_ID, vr.T_ID),
    "skip_yuv444": (K4, vr.RGBA8, yuv(*K4, sub=False), S, S, vr.SKIP | vr.CLAMP, vr.T_ID, vr.T_ID),
    "skip_rgba8_dither": ((1277, 719), vr.RGBA8, [(1277, 719, vr.RGBA8)], S, S, vr.SKIP | vr.CLAMP | vr.DITHER, vr.T_ID, vr.T_ID),
    "skip_bgra8_srgb": (K2, vr.RGBA8, [(2560, 1440, vr.BGRA8_SRGB)], S, S, vr.SKIP | vr.CLAMP | vr.DITHER, vr.T_ID, vr.T_ID),
    # an *_SRGB input is decoded by the view: EOTF identity, OETF sRGB, so they do not cancel
    "skip_srgb_view": (K4, vr.RGBA8_SRGB, nv12(*K4), S, S, vr.SKIP | vr.CLAMP | vr.CHROMA, vr.T_ID, vr.T_SRGB),
    "skip_hdr10_p010": (K4, vr.A2B10G10R10, nv12(*K4, wide=True), HDR, HDR, vr.SKIP | vr.CLAMP | vr.CHROMA, vr.T_ID, vr.T_ID),
    "skip_srgb_to_hdr10": (K4, vr.RGBA8, nv12(*K4, wide=True), S, HDR, vr.SKIP | vr.CLAMP | vr.CHROMA | vr.PRIMARY, vr.T_SRGB, vr.T_PQ),
    "skip_hdr10_to_srgb": (K4, vr.A2B10G10R10, nv12(*K4), HDR, S, vr.SKIP | vr.CLAMP | vr.CHROMA | vr.PRIMARY, vr.T_PQ, vr.T_SRGB),
    "scrgb_to_srgb_rgba8": (K4, vr.RGBA16F, [(3840, 2160, vr.RGBA8)], LIN, S, vr.SKIP | vr.CLAMP | vr.PRIMARY | vr.DITHER, vr.T_ID, vr.T_SRGB),
    "srgb_to_scrgb_rgba8": (K4, vr.RGBA8, [(3840, 2160, vr.RGBA8)], S, LIN, vr.SKIP | vr.CLAMP | vr.PRIMARY | vr.DITHER, vr.T_SRGB, vr.T_ID),
    # rescaling keeps both transfer functions: the filter runs in linear light
    "down_4k_1080p": (K4, vr.RGBA8, nv12(*P1080), S, S, vr.DOWN | vr.CLAMP | vr.CHROMA, vr.T_SRGB, vr.T_SRGB),
    "down_1440p_1080p": (K2, vr.RGBA8, yuv(*P1080), S, S, vr.DOWN | vr.CLAMP | vr.CHROMA, vr.T_SRGB, vr.T_SRGB),
    "up_720p_1080p": ((1280, 720), vr.RGBA8, yuv(*P1080, sub=False), S, S, vr.CLAMP, vr.T_SRGB, vr.T_SRGB),
    "sampled_8k_1080p": ((7680, 4320), vr.RGBA8, nv12(*P1080), S, S, vr.DOWN | vr.SAMPLED | vr.CLAMP | vr.CHROMA, vr.T_SRGB, vr.T_SRGB),
    "sampled_one_axis": ((3841, 1080), vr.RGBA8, nv12(*P1080), S, S, vr.DOWN | vr.SAMPLED | vr.CLAMP | vr.CHROMA, vr.T_SRGB, vr.T_SRGB),
    "down_one_axis": ((1920, 2160), vr.RGBA8, [(1920, 1080, vr.RGBA8)], S, S, vr.DOWN | vr.CLAMP | vr.DITHER, vr.T_SRGB, vr.T_SRGB),
}


@pytest.mark.parametrize("case", sorted(PLAN_CASES))
def test_plan_matches_rescale_decisions(case):
    in_size, in_fmt, planes, src_space, dst_space, flags, eotf, oetf = PLAN_CASES[case]
    got = capi.video_scale_plan(in_size, in_fmt, planes, src_space, dst_space)
    ref = vr.plan(in_size, in_fmt, planes, src_space, dst_space)
    assert got is not None and ref is not None
    assert (got["flags"], got["eotf"], got["oetf"]) == (flags, eotf, oetf), case
    assert (ref["flags"], ref["eotf"], ref["oetf"]) == (flags, eotf, oetf), case
    assert got["num_planes"] == len(planes)
    assert got["resolution"] == tuple(in_size)
    assert got["scaling_to_input"] == pytest.approx(ref["scaling_to_input"], rel=1e-7, abs=0)
    assert max(got["scaling_to_input"]) <= 2.0
    assert got["inv_input_resolution"] == pytest.approx(ref["inv_input_resolution"], rel=1e-7, abs=0)
    assert got["dither_strength"] == pytest.approx(float(ref["dither_strength"]), rel=1e-7, abs=0)
    assert np.array_equal(got["gamma_space_transform"], ref["gamma_space_transform"])
    # float32 construction against the float64 restatement: 1e-6 of the matrix's scale
    scale = np.abs(ref["primary_transform"]).max()
    assert np.abs(got["primary_transform"] - ref["primary_transform"]).max() <= 1e-6 * scale, case


def test_plan_primary_matrices_are_the_known_conversions():
    p = capi.video_scale_plan(K4, vr.RGBA8, nv12(*K4, wide=True), S, HDR)["primary_transform"] / 200.0
    # BT.709 -> BT.2020 (ITU-R BT.2087 table 2, D65 both sides): rows sum to 1
    assert p[0] == pytest.approx([0.6274, 0.3293, 0.0433], abs=2e-4)
    assert p.sum(axis=1) == pytest.approx([1, 1, 1], abs=1e-5)
    back = capi.video_scale_plan(K4, vr.A2B10G10R10, nv12(*K4), HDR, S)["primary_transform"]
    assert back @ p == pytest.approx(np.eye(3), abs=1e-5)


@pytest.mark.parametrize("args", [
    (K4, vr.RGBA8, nv12(*K4), 12345, S),                               # unrecognised colour space
    (K4, vr.RGBA8, nv12(*K4), S, 1000104001),
    (K4, vr.RGBA8, nv12(*K4), S, LIN),                                  # YCbCr needs a nonlinear output
    (K4, vr.RGBA8, yuv(*K4), S, LIN),
    (K4, vr.RGBA8, [(3840, 2160, vr.R8), (1921, 1080, vr.R8G8)], S, S),  # chroma neither half nor full size
    (K4, vr.RGBA8, [(3840, 2160, vr.R8), (1920, 1080, vr.R16G16)], S, S),  # 8-bit luma with 16-bit chroma
    (K4, vr.RGBA8, [(3840, 2160, vr.R8), (1920, 1080, vr.R8), (1920, 1081, vr.R8)], S, S),
    (K4, vr.RGBA8, [(3840, 2160, vr.R8)], S, S),                        # one plane must be RGBA8 / BGRA8
    (K4, vr.R8, nv12(*K4), S, S),                                        # input format
    (K4, vr.RGBA8, [], S, S),
    # one pixel wide: 4:2:0 chroma (1 x 1) is as wide as the luma (1 x 2), and the plan tells subsampling by the width alone, as
    # VideoScaler::rescale does; gr_video_yuv_plan accepts the same planes (tests/test_yuv_ref_cpu.py)
    ((1, 2), vr.RGBA8, nv12(1, 2), S, S),
    ((1, 2), vr.RGBA8, yuv(1, 2), S, S),
], ids=["space_in", "space_out", "nv12_linear", "yuv_linear", "chroma_size", "chroma_depth", "plane3_size", "luma_alone",
        "input_format", "no_planes", "one_wide_420", "one_wide_420_three_planes"])
def test_plan_refuses_invalid_conversions(args):
    in_size, in_fmt, planes, src_space, dst_space = args
    assert capi.video_scale_plan(in_size, in_fmt, planes, src_space, dst_space) is None


def test_new_formats_are_declared_with_their_vkformat_values():
    assert (capi.FORMAT_B8G8R8A8_UNORM, capi.FORMAT_B8G8R8A8_SRGB, capi.FORMAT_R16_UNORM, capi.FORMAT_R16G16_UNORM) == (44, 50, 70, 77)
    text = open(os.path.join(ROOT, "include", "granite_hip.h")).read()
    for name, value in (("B8G8R8A8_UNORM", 44), ("B8G8R8A8_SRGB", 50), ("R16_UNORM", 70), ("R16G16_UNORM", 77)):
        assert re.search(rf"GR_FORMAT_{name} = {value},", text), name
    for name in ("gr_video_scale", "gr_video_scale_plan", "gr_video_scaler_weights"):
        assert name in capi.EXPORTED_SYMBOLS


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_video_kernels_do_not_spill(tmp_path):
    """Every instantiation of k_video_direct / k_video_rescale (9 plane layouts each) stays at eight waves per SIMD: at most 64 VGPRs,
    nothing spilled, no scratch; the rescale tiles fit eight groups in the 160 KiB of LDS."""
    out = tmp_path / "video.s"
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only",
                           os.path.join(ROOT, "granite_amd", "csrc", "video.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    kernels = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S*k_video_\w+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                         r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(kernels) == 18, [k[1] for k in kernels]
    for lds, name, vgprs, spilled in kernels:
        assert int(spilled) == 0, (name, spilled)
        assert int(vgprs) <= 64, (name, vgprs)
        assert int(lds) * 8 <= 160 * 1024, (name, lds)
    assert ".private_segment_fixed_size: 0" in text and not re.search(r"\.private_segment_fixed_size:\s+[1-9]", text)
