"""gr_texture_decode launch times at 4096 x 4096 for BC1, BC5, BC7 and BC6H, beside a device copy (gr_copy) of the same number of output
bytes.  Both are timed the same way: 10 warm-up calls, then the wall clock over 100 back-to-back calls between two synchronisations;
three such rounds, every one printed.  Then ASTC 4 x 4, 6 x 6, 8 x 8 and 12 x 12 in the same run (BC7 above is their yardstick), each on two
payloads: the legal blocks of the test suite's case sets (tests/astc_cases.py, every class that is no error class or void extent) tiled
up, and void extents only -- the floor: one header, no endpoints, no weights."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
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


def astc_payloads(bw, bh, count):
    """(name, (count, 16) blocks): the legal mix and the void extents of the golden's case sets for the footprint, tiled up."""
    import astc_cases
    import astc_ref
    mine = {n: c for n, c in astc_cases.golden().items() if astc_ref.format_footprint(c[0]) == (bw, bh)}
    legal = np.concatenate([c[3].reshape(-1, 16) for n, c in mine.items() if not astc_cases.is_error_class(n) and "_void_" not in n])
    void = astc_cases.golden()["f4x4_void_ldr"][3].reshape(-1, 16)  # a void extent does not depend on the footprint
    return [(name, np.resize(b, (count, 16))) for name, b in (("legal mix", legal), ("void extent", void))]


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
    for bw, bh in ((4, 4), (6, 6), (8, 8), (12, 12)):
        fmt = 157 + 2 * capi.ASTC_FOOTPRINTS.index((bw, bh))
        bx, by = (w + bw - 1) // bw, (h + bh - 1) // bh
        out = capi.DeviceImage(gr, w, h, capi.FORMAT_R8G8B8A8_UNORM)
        other = capi.DeviceBuffer(gr, out.pitch * h)
        written = out.pitch * h
        for payload, host_blocks in astc_payloads(bw, bh, bx * by):
            blocks = capi.DeviceBuffer(gr, host_blocks.size).upload(host_blocks.reshape(-1))
            for round_ in range(3):
                us = per_call_us(gr, lambda: gr.texture_decode(fmt, blocks.ptr, bx * 16, out))
                copy_us = per_call_us(gr, lambda: gr.check(gr.lib.gr_copy(gr.handle, None, other.ptr, out.ptr, written)))
                print(f"ASTC {bw}x{bh} {payload:11s} round {round_}: decode {us:8.2f} us  ({written / 1e6:6.1f} MB out, {blocks.nbytes / 1e6:5.1f} MB in, "
                      f"{written / (us * 1e-6) / 1e12:5.2f} TB/s written);  copy of the output bytes {copy_us:8.2f} us;  decode / copy = {us / copy_us:5.2f}")
            blocks.free()
        for b in (out.buffer, other):
            b.free()
    gr.close()


if __name__ == "__main__":
    main()
