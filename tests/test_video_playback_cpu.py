"""CPU: the playback side that needs no device: the bindings, the player's refusals, and -- against the device-less HIP stand-in of
tests/hip_stub (preloaded in front of the HIP runtime; kernels do not run, "device memory" is host memory) -- what one played frame
asks the runtime to do: one upload and one read-back copy, one launch, one event record, and no synchronisation of any kind until the
image is read, which waits for that frame's event alone."""
import json
import os
import subprocess
import sys

import pytest

from granite_amd import app as gapp
from granite_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hip_stub", "libhip_stub.so")

WORKER = r'''
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, %(root)r)
from granite_amd import app as gapp, capi
stub = C.CDLL(%(stub)r); stub.hip_stub_count.restype = C.c_uint64; stub.hip_stub_count.argtypes = [C.c_char_p]
keys = ["launches", "event_records", "stream_waits", "event_queries", "memcpys", "memsets", "syncs"]
count = lambda: {k: stub.hip_stub_count(k.encode()) for k in keys}
diff = lambda a, b: {k: b[k] - a[k] for k in keys}
a = gapp.Application(64, 64, lighting=False)
layout = a.start_playback("nv12", (70, 38), ring_frames=3)
frame = np.zeros(layout.frame_bytes, np.uint8)
out = {"frame_bytes": int(layout.frame_bytes)}
c0 = count(); a.play_frame(frame); c1 = count()
out["per_frame"] = diff(c0, c1)
a.play_frame(frame); a.play_frame(frame)
try:
    a.play_frame(frame)
    out["full_ring"] = None
except capi.GraniteHipError as e:
    out["full_ring"] = str(e)
c2 = count(); img, number = a.read_playback(); c3 = count()
out["per_read"] = diff(c2, c3)
out["first"] = [list(img.shape), number]
a.play_frame(frame)  # the slot just handed back
numbers = []
while True:
    r = a.read_playback()
    if r is None:
        break
    numbers.append(r[1])
out["numbers"] = numbers
a.play_frame(frame)
a.end_playback()  # one frame in flight
try:
    a.play_frame(frame)
    out["after_end"] = None
except capi.GraniteHipError as e:
    out["after_end"] = str(e)
a.close()
print(json.dumps(out))
'''


def test_one_played_frame_is_one_upload_one_launch_one_event_and_no_sync():
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(os.path.join(os.path.dirname(STUB), "hip_stub.cpp")):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(STUB)])
    r = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT, "stub": STUB}], env=dict(os.environ, LD_PRELOAD=STUB),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["frame_bytes"] == 70 * 38 + 35 * 19 * 2
    f = out["per_frame"]
    # the upload of the planes and the read-back of the image; the conversion; the frame's event
    assert f["memcpys"] == 2 and f["launches"] == 1 and f["event_records"] == 1, f
    assert f["syncs"] == 0 and f["stream_waits"] == 0 and f["memsets"] == 0, f
    assert out["full_ring"] and "unread" in out["full_ring"]
    rd = out["per_read"]
    assert rd["syncs"] == 1 and rd["launches"] == 0 and rd["memcpys"] == 0, rd  # hipEventSynchronize on that frame's event
    assert out["first"] == [[38, 70, 4], 0]
    assert out["numbers"] == [1, 2, 3]
    assert out["after_end"] and "not playing" in out["after_end"]


def test_playback_symbols_are_bound():
    lib = gapp.load_library()
    for name in ("gra_video_play_begin", "gra_video_play_layout", "gra_video_play_frame", "gra_video_play_read_rgb", "gra_video_play_end"):
        assert name in gapp.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "gr_video_yuv_to_rgb" in capi.EXPORTED_SYMBOLS and "gr_video_yuv_plan" in capi.EXPORTED_SYMBOLS


def test_playback_refuses_row_bands():
    a = gapp.Application(320, 180, device=-1, strip_index=0, strip_count=2)
    with pytest.raises(capi.GraniteHipError, match="row bands"):
        a.start_playback("nv12", (320, 180))
    a.close()


def test_playback_refusals_need_no_device():
    a = gapp.Application(320, 180, device=-1)
    with pytest.raises(capi.GraniteHipError, match="width and height"):
        a.start_playback("nv12", (0, 180))
    with pytest.raises(capi.GraniteHipError, match="output format"):
        a.start_playback("nv12", (320, 180), output_format=capi.FORMAT_B8G8R8A8_UNORM)
    with pytest.raises(capi.GraniteHipError, match="not supported"):  # 8-bit planes described as 10-bit
        a.start_playback("nv12", (320, 180), info=capi.video_yuv_info(bit_depth=10))
    with pytest.raises(capi.GraniteHipError, match="not supported"):  # RGBA16F needs PQ content
        a.start_playback("p010", (320, 180), output_format=capi.FORMAT_R16G16B16A16_SFLOAT)
    opts = gapp.VideoPlayOptions(99, 320, 180, capi.video_yuv_info(), capi.FORMAT_R8G8B8A8_UNORM, 0)
    assert a.lib.gra_video_play_begin(a.handle, opts) < 0
    for call in (a.playback_layout, a.end_playback, a.read_playback):
        with pytest.raises(capi.GraniteHipError, match="not playing"):
            call()
    a.close()
