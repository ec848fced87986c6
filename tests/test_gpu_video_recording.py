"""GPU: frame recording on the application (gra_video_*, the headless runner's --video-encode-path).

The end-to-end tests render with sync=False throughout and read recorded frames lazily, several frames behind, so that the recorder's
conversions overlap the frames that follow them.  Every recorded frame must equal, byte for byte, gr_video_scale applied to the same
frame's backbuffer taken from a second application that renders frame by frame with sync=True.  A conversion that ran before the
frame's last writer (the generic stream's tonemap, or the tail stream's SMAA under split_tail) finished, or a swapchain image
rewritten four frames later before its conversion read it, would make some frame differ."""

import numpy as np
import pytest

import video_ref as vr
from granite_amd import app as gapp
from granite_amd import capi, headless, png, synth

pytestmark = pytest.mark.gpu

S, HDR = capi.COLOR_SPACE_SRGB_NONLINEAR, capi.COLOR_SPACE_HDR10_ST2084
PLANE_FORMATS = {"nv12": (capi.FORMAT_R8_UNORM, capi.FORMAT_R8G8_UNORM), "yuv420p": (capi.FORMAT_R8_UNORM,) * 3,
                 "p010": (capi.FORMAT_R16_UNORM, capi.FORMAT_R16G16_UNORM)}


def make(cam, gbuf, descs, motion, **kw):
    a = gapp.Application(cam.width, cam.height, **kw)
    P, V = np.ascontiguousarray(cam.P.T, np.float32).reshape(16), np.ascontiguousarray(cam.V.T, np.float32).reshape(16)
    a.set_camera(P, V)
    a.set_lights(descs)
    a.upload_gbuffer(gbuf, motion_vectors=synth.make_motion_vectors(cam.width, cam.height))
    a.set_camera_motion(motion)
    return a


def convert(gr, backbuffer, layout, fmt, in_space, out_space):
    """gr_video_scale of one backbuffer (as gra_read_backbuffer returned it) into planes of the recorder's layout."""
    h, w = backbuffer.shape[:2]
    in_fmt = capi.FORMAT_A2B10G10R10_UNORM_PACK32 if backbuffer.dtype == np.uint32 else capi.FORMAT_R8G8B8A8_SRGB
    src = capi.DeviceImage(gr, w, h, in_fmt).upload(backbuffer)
    planes = [capi.DeviceImage(gr, layout.width[i], layout.height[i], PLANE_FORMATS[fmt][i]) for i in range(layout.num_planes)]
    gr.video_scale(src, planes, in_space, out_space)
    gr.sync()
    return [p.download() for p in planes]


def record_against_frame_by_frame(gr, size, fmt, frames=12, lag=5, lights=4096, **kw):
    cam = synth.Camera(*size)
    gbuf, descs = synth.make_gbuffer(cam), synth.make_lights(cam, lights)
    motion = (0.02, 0.0, 0.01)
    a = make(cam, gbuf, descs, motion, **kw)
    b = make(cam, gbuf, descs, motion, **kw)
    layout = a.start_video(fmt)
    recorded = []
    for f in range(frames):
        a.render_frames(1, sync=False)
        if f >= lag:
            got = a.read_video_frame()
            assert got is not None
            recorded.append(got)
    while (got := a.read_video_frame()) is not None:
        recorded.append(got)
    assert [n for _, n in recorded] == list(range(frames))
    for f in range(frames):
        b.render_frames(1, sync=True)
        want = convert(gr, b.read_backbuffer(), layout, fmt, S, S)
        for i, (g, w) in enumerate(zip(recorded[f][0], want)):
            np.testing.assert_array_equal(g, w.reshape(g.shape), err_msg=f"frame {f}, plane {i}")
    # the frames really move: a stale or repeated frame would not be caught otherwise
    assert not np.array_equal(recorded[0][0][0], recorded[-1][0][0])
    a.stop_video()
    a.close()
    b.close()


def test_recording_4k_config3_nv12(gr):
    record_against_frame_by_frame(gr, (3840, 2160), "nv12")


def test_recording_tail_stream_taa_smaa_yuv420p(gr):
    # taaHigh + smaaUltra: the SMAA passes run on the tail stream (split_tail), so the swapchain image's last writer is not on the
    # generic stream
    record_against_frame_by_frame(gr, (1920, 1080), "yuv420p", lights=1024, pre_aa=gapp.POST_AA_TAA_HIGH, post_aa=gapp.POST_AA_SMAA_ULTRA)


def test_recording_hdr10_p010_matches_reference():
    w, h = 480, 270
    cam = synth.Camera(w, h)
    a = make(cam, synth.make_gbuffer(cam), synth.make_lights(cam, 500), (0.01, 0.0, 0.0), hdr10=True, hdr_bloom=False)
    layout = a.start_video("p010", hdr10=True)
    assert (layout.num_planes, layout.bytes_per_sample) == (2, 2)
    for _ in range(3):
        a.render_frames(1, sync=True)
        planes, _ = a.read_video_frame()
        ref = vr.video_scale(a.read_backbuffer(), vr.A2B10G10R10, [(w, h, vr.R16), (w // 2, h // 2, vr.R16G16)], HDR, HDR)
        for g, r in zip(planes, ref):
            # 64 of 65535: the bound of tests/test_gpu_video_scaler.py for 16-bit planes
            assert np.abs(g.astype(np.int64) - r.reshape(g.shape)).max() <= 64
    a.stop_video()
    a.close()


def test_recording_does_not_change_the_backbuffer():
    w, h = 640, 360
    cam = synth.Camera(w, h)
    gbuf, descs = synth.make_gbuffer(cam), synth.make_lights(cam, 600)
    a = make(cam, gbuf, descs, (0.01, 0.0, 0.0), post_aa=gapp.POST_AA_FXAA)
    b = make(cam, gbuf, descs, (0.01, 0.0, 0.0), post_aa=gapp.POST_AA_FXAA)
    a.start_video("yuv444p", ring_frames=16)
    for f in range(6):
        a.render_frames(1, sync=True)
        b.render_frames(1, sync=True)
        np.testing.assert_array_equal(a.read_backbuffer(), b.read_backbuffer(), err_msg=f"frame {f}")
    a.stop_video()
    a.close()
    b.close()


def test_full_ring_fails_the_frame_and_drops_nothing():
    w, h = 320, 180
    cam = synth.Camera(w, h)
    a = make(cam, synth.make_gbuffer(cam), synth.make_lights(cam, 100), (0.01, 0.0, 0.0))
    a.start_video("nv12", ring_frames=2)
    assert a.read_video_frame() is None
    a.render_frames(2, sync=False)
    with pytest.raises(capi.GraniteHipError, match="unread"):
        a.render_frames(1, sync=False)
    assert a.read_video_frame()[1] == 0
    a.render_frames(1, sync=False)   # room again: this is frame 2, nothing was skipped or overwritten
    assert [a.read_video_frame()[1], a.read_video_frame()[1]] == [1, 2]
    assert a.read_video_frame() is None
    a.stop_video()
    with pytest.raises(capi.GraniteHipError):
        a.read_video_frame()
    a.close()


def test_headless_writes_y4m(tmp_path):
    out, last = str(tmp_path / "out.y4m"), str(tmp_path / "last.png")
    w, h = 320, 180
    assert headless.main(["synthetic", "--frames", "3", "--width", str(w), "--height", str(h), "--lights", "200",
                          "--video-encode-path", out, "--png-reference-path", last]) == 0
    data = open(out, "rb").read()
    header, _, body = data.partition(b"\n")
    assert header.split()[:4] == [b"YUV4MPEG2", b"W320", b"H180", b"F100:1"] and b"C420jpeg" in header and b"XCOLORRANGE=FULL" in header
    frame = w * h + 2 * (w // 2) * (h // 2)
    frames = body.split(b"FRAME\n")[1:]
    assert len(frames) == 3 and all(len(f) == frame for f in frames)
    # the last frame's luma against the reference conversion of the last backbuffer (within the same-size bound of 1 code)
    y = np.frombuffer(frames[-1][:w * h], np.uint8).reshape(h, w)
    ref = vr.video_scale(png.read_png(last), vr.RGBA8_SRGB, [(w, h, vr.R8), (w // 2, h // 2, vr.R8), (w // 2, h // 2, vr.R8)], S, S)
    assert np.abs(y.astype(np.int64) - ref[0]).max() <= 1
