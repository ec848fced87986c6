"""gr_texture_decode launch times at 4096 x 4096 for BC1, BC5, BC7 and BC6H, beside a device copy (gr_copy) of the same number of output
bytes.  Both are timed the same way: 10 warm-up calls, then the wall clock over 100 back-to-back calls between two synchronisations;
three such rounds, every one printed."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from granite_amd import capi  # noqa: E402

CASES = [("BC1 RGBA", capi.FORMAT_BC1_RGBA_UNORM_BLOCK), ("BC5", capi.FORMAT_BC5_UNORM_BLOCK), ("BC7", capi.FORMAT_BC7_UNORM_BLOCK),
         ("BC6H UFLOAT", capi.FORMAT_BC6H_UFLOAT_BLOCK)]


def per_call_us(gr, call, warmup=10, calls=100):
    for _ in range(warmup):
        call()
    gr.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    gr.sync()
    return 1e6 * (time.perf_counter() - t0) / calls


def main():
    w = h = 4096
    gr = capi.Context(0)
    rng = np.random.default_rng(0)
    for name, fmt in CASES:
        nb = gr.lib.gr_texture_block_bytes(fmt)
        blocks = capi.DeviceBuffer(gr, (w // 4) * (h // 4) * nb).upload(rng.integers(0, 256, (w // 4) * (h // 4) * nb, dtype=np.uint8))
        out = capi.DeviceImage(gr, w, h, gr.lib.gr_texture_decoded_format(fmt))
        other = capi.DeviceBuffer(gr, out.pitch * h)
        written = out.pitch * h
        for round_ in range(3):
            us = per_call_us(gr, lambda: gr.texture_decode(fmt, blocks.ptr, (w // 4) * nb, out))
            copy_us = per_call_us(gr, lambda: gr.check(gr.lib.gr_copy(gr.handle, None, other.ptr, out.ptr, written)))
            print(f"{name:12s} round {round_}: decode {us:8.2f} us  ({written / 1e6:6.1f} MB out, {blocks.nbytes / 1e6:5.1f} MB in, "
                  f"{written / (us * 1e-6) / 1e12:5.2f} TB/s written);  copy of the output bytes {copy_us:8.2f} us;  decode / copy = {us / copy_us:5.2f}")
        for b in (blocks, out.buffer, other):
            b.free()
    gr.close()


if __name__ == "__main__":
    main()
