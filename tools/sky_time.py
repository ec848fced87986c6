"""The sky pass (csrc/sky.hip) at 3840 x 2160: device-event times of gr_sky_apply for three shares of sky -- every pixel far, the upper
third far, and a checkerboard of far and near 8 x 8 pixel tiles (half the pixels, every 16 x 16 workgroup tile half full) -- in both
emissive formats, procedural (sun at 30 degrees, camera 2 m up, looking level: the horizon crosses the image) and with a 256-texel cube
of 9 levels; and of gr_sky_cube at 32 and 128 texels.

The library's own event brackets around each entry point (gr_timing_*): 2 warm-up calls, then 20 calls, three rounds, every one printed.
The calls run in place on one emissive image (the work per call does not depend on what emissive holds).

Beside the procedural times stands what the instruction count would give at one vector instruction per SIMD and quad-cycle:
VALU_PER_MARCHED_PIXEL instructions for every far pixel whose ray misses the earth (counted in the gfx950 code of k_sky_apply: 16 x (46 +
8 x 115 + 162) in the two loops and about 300 around them), over 64 lanes, times 4 cycles, over 1024 SIMDs at CLOCK_HZ.  Lanes that idle
beside a marching lane, scalar instructions and the clock the chip really holds are not in the figure: it is a yardstick, not a bound
(the marching pixels are counted on every 8th pixel each way, and plain fp32 operations issue faster than one per quad-cycle).

    timeout -k 10 600 python tools/sky_time.py > profiles/sky_time.txt
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sky_cases as sc  # noqa: E402
import sky_ref  # noqa: E402
from granite_amd import capi, synth  # noqa: E402

W, H = 3840, 2160
VALU_PER_MARCHED_PIXEL = 16 * (46 + 8 * 115 + 162) + 300
SIMDS, CLOCK_HZ = 1024, 2.4e9
CALLS = 20


def event_us(gr, name, run):
    run()
    run()
    gr.sync()
    gr.timing_reset()
    for _ in range(CALLS):
        run()
    gr.sync()
    count, ms = gr.timing_query().get(name, (0, 0.0))[:2]
    assert count == CALLS, (name, count)
    return ms * 1e3 / count


def far_patterns():
    y, x = np.mgrid[0:H, 0:W]
    return {"all": np.ones((H, W), bool), "upper third": y < H // 3, "8x8 checkerboard": (((x >> 3) + (y >> 3)) & 1) == 0}


def main():
    gr = capi.Context(0)
    cam = synth.Camera(W, H, eye=(0.0, 2.0, 8.0), center=(0.0, 2.0, 0.0))
    view = cam.V.copy()
    view[:3, 3] = 0.0
    inv = synth._cm(np.linalg.inv(cam.P @ view)).astype(np.float32)
    sun, color, height = sc.sun(30.0, 20.0), (20.0, 20.0, 20.0), 2.0
    rng = np.random.default_rng(1)
    size, levels = 256, 9
    chain_words = gr.lib.gr_cube_chain_bytes(size, levels) // 2
    cube = capi.DeviceBuffer(gr, chain_words * 2).upload(rng.uniform(0.0, 4.0, chain_words).astype(np.float16).view(np.uint16))
    # which far pixels march: sky_ref's decision, on a coarse grid of the same view (every 8th pixel)
    directions = sky_ref.normalize(sky_ref.pixel_directions(inv, W, H)[::8, ::8].reshape(-1, 3))
    marched_grid = sky_ref.scatter_mask(directions, height)[0].reshape(H // 8, W // 8)
    gr.timing_enable(True)
    for fmt, fmt_name in ((capi.FORMAT_R16G16B16A16_SFLOAT, "RGBA16F"), (capi.FORMAT_B10G11R11_UFLOAT_PACK32, "B10G11R11")):
        emissive = capi.DeviceImage(gr, W, H, fmt)
        for pattern, far in far_patterns().items():
            depth = capi.DeviceImage(gr, W, H, capi.FORMAT_D32_SFLOAT).upload(np.where(far, np.float32(0.0), np.float32(0.5)).astype(np.float32))
            marched = int((far[::8, ::8] & marched_grid).sum()) * 64
            floor_us = marched * VALU_PER_MARCHED_PIXEL / 64 * 4 / SIMDS / CLOCK_HZ * 1e6
            for textured in (False, True):
                run = lambda: gr.sky_apply(emissive, depth, inv, color, 0.0 if textured else height, (0.0, 0.0, 0.0) if textured else sun,
                                           cube if textured else None, size if textured else 0, levels if textured else 0)
                for round_ in range(3):
                    us = event_us(gr, "sky_apply", run)
                    model = "" if textured else f";  {marched} pixels march, {VALU_PER_MARCHED_PIXEL} VALU each: {floor_us:8.1f} us at one per SIMD and quad-cycle, {CLOCK_HZ / 1e9:.1f} GHz"
                    print(f"{W} x {H} {fmt_name:9s} far: {pattern:16s} ({int(far.sum()):7d} px) {'cube 256/9 ' if textured else 'procedural '} round {round_}: {us:9.1f} us{model}")
    for n in (32, 128):
        out = capi.DeviceBuffer(gr, 6 * n * n * 8)
        run = lambda: gr.sky_cube(out, n, color, height, sun)
        for round_ in range(3):
            print(f"gr_sky_cube {n:3d}: round {round_}: {event_us(gr, 'sky_cube', run):9.1f} us")
    gr.timing_enable(False)
    gr.close()


if __name__ == "__main__":
    main()
