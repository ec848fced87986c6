"""gr_video_yuv_to_rgb launch times (hipEvents around each launch: 5 warm-up launches, then 30 timed), bytes moved and the fraction of
the copy ceiling measured in the same run (gr_bandwidth_probe): NV12 -> RGBA8 and P010 (PQ, BT.2020) -> RGBA16F at 3840x2160."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from granite_amd import capi  # noqa: E402

CASES = [
    ("4K NV12 -> RGBA8", False, capi.FORMAT_R8G8B8A8_UNORM, dict(bit_depth=8, full_range=1)),
    ("4K P010 (PQ) -> RGBA16F", True, capi.FORMAT_R16G16B16A16_SFLOAT,
     dict(bit_depth=10, msb_aligned=1, matrix=capi.VIDEO_MATRIX_BT2020, pq=1)),
]


def main():
    w, h = 3840, 2160
    gr = capi.Context(0)
    copy = C.c_double()
    triad = C.c_double()
    gr.check(gr.lib.gr_bandwidth_probe(gr.handle, 1 << 30, 20, C.byref(copy), C.byref(triad)))
    ceiling = copy.value / 1e3
    print(f"copy ceiling {ceiling:.2f} TB/s (gr_bandwidth_probe, 1 GiB, best of 20)")
    rng = np.random.default_rng(0)
    for name, wide, out_fmt, inf in CASES:
        planes = [capi.DeviceImage(gr, w, h, capi.FORMAT_R16_UNORM if wide else capi.FORMAT_R8_UNORM),
                  capi.DeviceImage(gr, w // 2, h // 2, capi.FORMAT_R16G16_UNORM if wide else capi.FORMAT_R8G8_UNORM)]
        for p in planes:
            p.upload(rng.integers(0, 256, (p.height, p.pitch), dtype=np.uint8))
        out = capi.DeviceImage(gr, w, h, out_fmt)
        info = capi.video_yuv_info(**inf)
        for _ in range(5):
            gr.video_yuv_to_rgb(planes, out, info)
        gr.sync()
        gr.timing_reset()
        gr.timing_enable(True)
        for _ in range(30):
            gr.video_yuv_to_rgb(planes, out, info)
        gr.sync()
        n, ms = gr.timing_query()["video_yuv_to_rgb"]
        worst = gr.timing_max_ms("video_yuv_to_rgb")
        gr.timing_enable(False)
        us = 1e3 * ms / n
        moved = sum(p.pitch * p.height for p in planes) + out.pitch * out.height
        tbs = moved / (us * 1e-6) / 1e12
        print(f"{name:28s} mean {us:7.2f} us (max {1e3 * worst:7.2f}, {n} launches)  {moved / 1e6:6.1f} MB  {tbs:5.2f} TB/s = "
              f"{tbs / ceiling:5.1%} of the copy ceiling")
        for p in planes + [out]:
            p.buffer.free()
    gr.close()


if __name__ == "__main__":
    main()
