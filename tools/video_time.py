"""gr_video_scale launch times (hipEvents around each launch: 5 warm-up launches, then 50 timed), bytes moved and the fraction of the
8 TB/s HBM peak and of the copy ceiling measured in the same run (gr_bandwidth_probe), plus the device-to-host copy of one packed frame
into pinned memory: NV12 (1.5 B/px) against RGBA8 (4 B/px) at 3840x2160."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C  # noqa: E402

from granite_amd import app as gapp  # noqa: E402
from granite_amd import capi, synth  # noqa: E402

S, HDR = capi.COLOR_SPACE_SRGB_NONLINEAR, capi.COLOR_SPACE_HDR10_ST2084


def planes_nv12(gr, w, h, wide=False, sub=True):
    """Luma and interleaved chroma; sub=False: chroma at full size (two-plane 4:4:4)."""
    cw, ch = ((w + 1) // 2, (h + 1) // 2) if sub else (w, h)
    return [capi.DeviceImage(gr, w, h, capi.FORMAT_R16_UNORM if wide else capi.FORMAT_R8_UNORM),
            capi.DeviceImage(gr, cw, ch, capi.FORMAT_R16G16_UNORM if wide else capi.FORMAT_R8G8_UNORM)]


CASES = [
    ("4K sRGB -> NV12 (same size)", (3840, 2160), capi.FORMAT_R8G8B8A8_UNORM, (3840, 2160), dict(), S, S),
    ("4K -> 1080p NV12", (3840, 2160), capi.FORMAT_R8G8B8A8_UNORM, (1920, 1080), dict(), S, S),
    ("2560x1440 -> 1920x1080 NV12", (2560, 1440), capi.FORMAT_R8G8B8A8_UNORM, (1920, 1080), dict(), S, S),
    ("1280x720 -> 1920x1080 NV12", (1280, 720), capi.FORMAT_R8G8B8A8_UNORM, (1920, 1080), dict(), S, S),
    ("7680x4320 -> 1920x1080 NV12 (sampled)", (7680, 4320), capi.FORMAT_R8G8B8A8_UNORM, (1920, 1080), dict(), S, S),
    ("4K HDR10 -> P010 (same size)", (3840, 2160), capi.FORMAT_A2B10G10R10_UNORM_PACK32, (3840, 2160), dict(wide=True), HDR, HDR),
    # interleaved chroma at full size: k_video_direct<2, false, *>, which no recording format reaches
    ("4K sRGB -> 2-plane 4:4:4 8 bit", (3840, 2160), capi.FORMAT_R8G8B8A8_UNORM, (3840, 2160), dict(sub=False), S, S),
    ("4K sRGB -> 2-plane 4:4:4 16 bit", (3840, 2160), capi.FORMAT_R8G8B8A8_UNORM, (3840, 2160), dict(wide=True, sub=False), S, S),
]


def main():
    gr = capi.Context(0)
    copy = C.c_double()
    triad = C.c_double()
    gr.check(gr.lib.gr_bandwidth_probe(gr.handle, 1 << 30, 20, C.byref(copy), C.byref(triad)))
    ceiling = copy.value / 1e3
    print(f"copy ceiling {ceiling:.2f} TB/s (gr_bandwidth_probe, 1 GiB, best of 20)")
    rng = np.random.default_rng(0)
    for name, (iw, ih), fmt, (ow, oh), layout, src_space, dst_space in CASES:
        src = capi.DeviceImage(gr, iw, ih, fmt).upload(rng.integers(0, 256, (ih, iw * 4), dtype=np.uint8))
        planes = planes_nv12(gr, ow, oh, **layout)
        for _ in range(5):
            gr.video_scale(src, planes, src_space, dst_space)
        gr.sync()
        gr.timing_reset()
        gr.timing_enable(True)
        for _ in range(50):
            gr.video_scale(src, planes, src_space, dst_space)
        gr.sync()
        n, ms = gr.timing_query()["video_scale"]
        best = gr.timing_max_ms("video_scale")
        gr.timing_enable(False)
        us = 1e3 * ms / n
        moved = iw * ih * 4 + sum(p.pitch * p.height for p in planes)
        tbs = moved / (us * 1e-6) / 1e12
        print(f"{name:40s} mean {us:7.2f} us (max {1e3 * best:7.2f})  {moved / 1e6:6.1f} MB  {tbs:5.2f} TB/s = "
              f"{tbs / 8.0:5.1%} of 8 TB/s, {tbs / ceiling:5.1%} of the copy ceiling")
        for p in planes:
            p.buffer.free()
        src.buffer.free()

    # device -> host copy of one frame into pinned memory (gr_download on the default stream, wall clock around a sync)
    for label, nbytes in (("NV12 3840x2160 (1.5 B/px)", 3840 * 2160 * 3 // 2), ("RGBA8 3840x2160 (4 B/px)", 3840 * 2160 * 4)):
        dev = capi.DeviceBuffer(gr, nbytes)
        host = C.c_void_p()
        gr.check(gr.lib.gr_alloc_host(gr.handle, nbytes, C.byref(host)))
        times = []
        for i in range(25):
            gr.sync()
            t0 = time.perf_counter()
            gr.check(gr.lib.gr_download(gr.handle, None, host, dev.ptr, nbytes))
            gr.sync()
            if i >= 5:
                times.append(time.perf_counter() - t0)
        gr.check(gr.lib.gr_free_host(gr.handle, host))
        dev.free()
        t = np.median(times)
        print(f"D2H {label:28s} {nbytes / 1e6:5.1f} MB  median {t * 1e3:6.3f} ms  {nbytes / t / 1e9:5.1f} GB/s")
    gr.close()
    frame_periods()


def frame_periods(steps=200, rounds=2):
    """Config 3 (3840x2160, 4096 lights, bloom + tonemap): frame period with NV12 recording (frames read three behind) and without,
    alternated in one process, and the period of render + gra_read_backbuffer (RGBA8, 4 B/px) per frame."""
    cam = synth.Camera(3840, 2160)
    a = gapp.Application(cam.width, cam.height)
    a.set_render_parameters(cam.render_params())
    a.set_lights(synth.make_lights(cam, 4096))
    a.upload_gbuffer(synth.make_gbuffer(cam))
    a.render_frames(20)

    def run(record):
        if record:
            a.start_video("nv12")
        t0 = time.perf_counter()
        for i in range(steps):
            a.render_frames(1, sync=False)
            if record and i >= 3:
                a.read_video_frame(raw=True)
        a.sync()
        t = (time.perf_counter() - t0) / steps
        if record:
            while a.read_video_frame(raw=True) is not None:
                pass
            a.stop_video()
        return t

    results = {"off": [], "nv12": []}
    for _ in range(rounds):
        results["off"].append(run(False))
        results["nv12"].append(run(True))
    t0 = time.perf_counter()
    for _ in range(50):
        a.render_frames(1, sync=False)
        a.read_backbuffer()
    rb = (time.perf_counter() - t0) / 50
    for k, v in results.items():
        print(f"config 3 frame period, recording {k:4s}: " + ", ".join(f"{1e3 * t:.4f}" for t in v) + " ms")
    print(f"config 3 frame period with gra_read_backbuffer (RGBA8) every frame: {1e3 * rb:.4f} ms")
    a.close()


if __name__ == "__main__":
    main()
