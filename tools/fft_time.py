"""gr_fft_execute launch times beside a device copy (gr_copy) of the bytes the plan's passes move (every pass reads its input and writes
its output once: the sum over the passes, copied as one block of half that size, which reads and writes it).  Both are timed the same
way: 2 warm-up calls, then the wall clock over 10 back-to-back calls between two synchronisations; three such rounds, every one printed.
The C2R case is the reference ocean's default fft_resolution (renderer/ocean.hpp: 1024) into an R16 image.

    timeout -k 10 300 python tools/fft_time.py > profiles/fft_time.txt
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from granite_amd import capi, fft  # noqa: E402

OCEAN_FFT_RESOLUTION = 1024


def per_call_ms(gr, call, warmup=2, calls=10):
    for _ in range(warmup):
        call()
    gr.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    gr.sync()
    return 1e3 * (time.perf_counter() - t0) / calls


def side_units(nx, mode, output):
    real_side = mode == (capi.FFT_C2R if output else capi.FFT_R2C)
    return (nx, 1) if real_side else ((nx // 2 + 1 if mode in (capi.FFT_R2C, capi.FFT_C2R) else nx), 2)


def main():
    gr = capi.Context(0)
    rng = np.random.default_rng(0)
    cases = (("2-D C2C 1024 x 1024 fp32", 1024, 1024, 2, capi.FFT_FORWARD_C2C, capi.FFT_FP32, False),
             ("2-D C2R 1024 x 1024 fp16 -> R16 image", OCEAN_FFT_RESOLUTION, OCEAN_FFT_RESOLUTION, 2, capi.FFT_C2R, capi.FFT_FP16, True),
             ("2-D R2C 2048 x 1024 fp32", 2048, 1024, 2, capi.FFT_R2C, capi.FFT_FP32, False),
             ("1-D C2C 2^20 fp32", 1 << 20, 1, 1, capi.FFT_FORWARD_C2C, capi.FFT_FP32, False),
             ("1-D R2C 2^16 x 16 fp32", 1 << 16, 16, 1, capi.FFT_R2C, capi.FFT_FP32, False))
    for name, nx, ny, dims, mode, data_type, image in cases:
        scalar = np.float16 if data_type == capi.FFT_FP16 else np.float32
        size = np.dtype(scalar).itemsize
        (in_units, in_per), (out_units, out_per) = side_units(nx, mode, False), side_units(nx, mode, True)
        in_bytes, out_bytes = ny * in_units * in_per * size, ny * out_units * out_per * size
        options = capi.fft_options(nx, ny, 1, dims, mode, data_type, output_resource=capi.FFT_RESOURCE_TEXTURE if image else capi.FFT_RESOURCE_BUFFER)
        passes = capi.fft_describe(options)
        # scratch rows: nx complex numbers, or nx / 2 + 1 rounded up to 16 in a real mode (fft_core.hpp: scratch_row_stride)
        scratch_bytes = ny * (nx if mode < capi.FFT_R2C else (nx // 2 + 1 + 15) & ~15) * 2 * size
        moved = sum({capi.FFT_BUFFER_SRC: in_bytes}.get(p.reads, scratch_bytes) + {capi.FFT_BUFFER_DST: out_bytes}.get(p.writes, scratch_bytes) for p in passes)
        src = capi.DeviceBuffer(gr, in_bytes).upload(rng.uniform(-1.0, 1.0, in_bytes // size).astype(scalar))
        dst = capi.DeviceBuffer(gr, out_bytes)
        a, b = capi.DeviceBuffer(gr, moved // 2), capi.DeviceBuffer(gr, moved // 2)
        plan = fft.Plan(gr, options)
        r_src = capi.fft_buffer_resource(src.ptr, in_bytes, in_units, in_units * ny)
        if image:
            r_dst = capi.fft_image_resource(capi.Image(dst.ptr, nx, ny, nx * size, capi.FORMAT_R16_SFLOAT if data_type else capi.FORMAT_R32_SFLOAT))
        else:
            r_dst = capi.fft_buffer_resource(dst.ptr, out_bytes, out_units, out_units * ny)
        for round_ in range(3):
            ms = per_call_ms(gr, lambda: plan.execute(r_dst, r_src))
            copy_ms = per_call_ms(gr, lambda: gr.check(gr.lib.gr_copy(gr.handle, None, b.ptr, a.ptr, moved // 2)))
            print(f"{name:38s} round {round_}: {ms:8.4f} ms in {len(passes)} passes ({'+'.join(str(p.points) if p.points else 'resolve' for p in passes)}), "
                  f"{moved / 1e6:6.1f} MB moved, {moved / (ms * 1e-3) / 1e9:7.1f} GB/s;  copy of those bytes {copy_ms:7.4f} ms;  ratio {ms / copy_ms:5.2f}")
        plan.close()
        for buf in (src, dst, a, b):
            buf.free()
    gr.close()


if __name__ == "__main__":
    main()
