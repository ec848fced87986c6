"""GPU: recording and playback end to end.  A few frames are rendered with recording on; the recorded bytes go to gra_video_play_frame
as they came out of gra_video_read_frame, and every image read back is compared with tests/yuv_ref.py applied to the same recorded
bytes, at the kernel's bounds of tests/test_gpu_yuv_to_rgb.py (1 code for R8G8B8A8; 2 fp16 ulp + 1e-4 + the fp32 allowance for
R16G16B16A16_SFLOAT).  That checks the packed layout, the order of frames, the reuse of ring slots and the frame numbers; it needs no
tolerance of its own.  Recording writes full-range planes with centre-sited chroma, BT.709 (BT.2020 for HDR10), 8 or 16 bits."""
import numpy as np
import pytest

import yuv_ref as yr
from granite_amd import app as gapp
from granite_amd import capi, synth
from test_gpu_yuv_to_rgb import compare, plane_format

pytestmark = pytest.mark.gpu

W, H = 322, 182


def render_and_record(fmt, frames, hdr10=False):
    cam = synth.Camera(W, H)
    a = gapp.Application(W, H, hdr10=True, hdr_bloom=False) if hdr10 else gapp.Application(W, H)
    a.set_render_parameters(cam.render_params())
    a.set_lights(synth.make_lights(cam, 64))
    a.upload_gbuffer(synth.make_gbuffer(cam))
    a.start_video(fmt, hdr10=hdr10, ring_frames=frames)
    a.render_frames(frames, sync=False)
    recorded = []
    for k in range(frames):
        raw, number = a.read_video_frame(raw=True)
        assert number == k
        raw = raw.copy()
        raw[:W * 2] += np.uint8(16 * k)  # a stripe of luma bytes that tells the frames apart whatever the scene does
        recorded.append(raw)
    layout = a.video_layout()
    a.stop_video()
    return a, layout, recorded


def expected(layout, raw, out_fmt, inf):
    planes = gapp.video_planes(layout, raw)
    p = yr.plan([(q.shape[1], q.shape[0], plane_format(q)) for q in planes], (W, H, out_fmt), yr.info(**inf))
    return yr.store(yr.shade(planes, p), out_fmt), (yr.pq_fp32_allowance(planes, p) if out_fmt == yr.RGBA16F else None)


@pytest.mark.parametrize("fmt", ["yuv444p", "nv12"])
def test_recorded_sdr_frames_play_back(fmt):
    frames = 5
    a, layout, recorded = render_and_record(fmt, frames)
    play = a.start_playback(fmt, (W, H), ring_frames=2)  # fewer slots than frames: slots are reused
    assert play.frame_bytes == layout.frame_bytes and list(play.offset) == list(layout.offset)
    inf = dict(bit_depth=8, full_range=1)
    got = []
    for k in range(0, frames, 2):  # two in flight, then read both
        batch = recorded[k:k + 2]
        for raw in batch:
            a.play_frame(raw)
        for _ in batch:
            got.append(a.read_playback())
    assert a.read_playback() is None
    assert [n for _, n in got] == list(range(frames))
    for k, (img, _) in enumerate(got):
        ref, _ = expected(layout, recorded[k], yr.RGBA8, inf)
        compare(img, ref, yr.RGBA8, W, H, f"{fmt} frame {k}")
    a.end_playback()
    a.close()


def test_recorded_hdr10_p010_frames_play_back():
    frames = 3
    a, layout, recorded = render_and_record("p010", frames, hdr10=True)
    # recording stores UNORM16 words: sixteen significant bits
    inf = dict(bit_depth=16, full_range=1, matrix=yr.M_BT2020, pq=1)
    a.start_playback("p010", (W, H), info=capi.video_yuv_info(**inf), output_format=capi.FORMAT_R16G16B16A16_SFLOAT)
    for raw in recorded:
        a.play_frame(raw)
    for k in range(frames):
        img, number = a.read_playback()
        assert number == k
        ref, allowance = expected(layout, recorded[k], yr.RGBA16F, inf)
        compare(img, ref, yr.RGBA16F, W, H, f"p010 frame {k}", allowance)
    a.end_playback()
    a.close()


def test_full_ring_is_reported_and_end_drains_frames_in_flight():
    a = gapp.Application(W, H)
    layout = a.start_playback("nv12", (W, H), ring_frames=2)
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, layout.frame_bytes, dtype=np.uint8) for _ in range(3)]
    a.play_frame(frames[0])
    a.play_frame(frames[1])
    with pytest.raises(capi.GraniteHipError, match="unread"):
        a.play_frame(frames[2])
    img, number = a.read_playback()
    assert number == 0
    planes = gapp.video_planes(layout, frames[0])
    compare(img, yr.yuv_to_rgb(planes, yr.RGBA8, yr.info(full_range=1)), yr.RGBA8, W, H, "frame 0")
    a.play_frame(frames[2])  # the slot just handed back; frames 1 and 2 are in flight
    a.end_playback()
    # a new player starts from frame 0 with an empty ring
    a.start_playback("nv12", (W, H), ring_frames=2)
    assert a.read_playback() is None
    a.play_frame(frames[1])
    img, number = a.read_playback()
    assert number == 0
    compare(img, yr.yuv_to_rgb(gapp.video_planes(layout, frames[1]), yr.RGBA8, yr.info(full_range=1)), yr.RGBA8, W, H, "frame 0 of the second player")
    a.end_playback()
    a.close()
