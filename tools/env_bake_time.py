"""gr_env_specular (128 texels a side, 8 levels) and gr_env_diffuse (32 texels a side) launch times from a 512-texel cube with its full
chain, beside a device copy (gr_copy) of the same number of output bytes.  Both are timed the same way: 2 warm-up calls, then the wall
clock over 10 back-to-back calls between two synchronisations; three such rounds, every one printed.

    timeout -k 10 300 python tools/env_bake_time.py > profiles/env_bake_time.txt
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from granite_amd import capi  # noqa: E402


def per_call_ms(gr, call, warmup=2, calls=10):
    for _ in range(warmup):
        call()
    gr.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    gr.sync()
    return 1e3 * (time.perf_counter() - t0) / calls


def main():
    gr = capi.Context(0)
    size, levels = 512, 10
    nbytes = gr.lib.gr_cube_chain_bytes(size, levels)
    rng = np.random.default_rng(0)
    src = capi.DeviceBuffer(gr, nbytes).upload(rng.uniform(0.0, 4.0, nbytes // 2).astype(np.float16))
    for name, out_size, out_levels, taps, call in (
            ("specular 128 / 8", 128, 8, 1024, lambda out: gr.env_specular(src, size, levels, out, 128, 8)),
            ("diffuse 32", 32, 1, 15876, lambda out: gr.env_diffuse(src, size, levels, out, 32))):
        written = gr.lib.gr_cube_chain_bytes(out_size, out_levels)
        out, other = capi.DeviceBuffer(gr, written), capi.DeviceBuffer(gr, written)
        total = taps * written // 8
        for round_ in range(3):
            ms = per_call_ms(gr, lambda: call(out))
            copy_ms = per_call_ms(gr, lambda: gr.check(gr.lib.gr_copy(gr.handle, None, other.ptr, out.ptr, written)))
            print(f"{name:16s} round {round_}: {ms:9.3f} ms  ({total / 1e6:6.1f} M cube taps, {total / (ms * 1e-3) / 1e9:6.2f} G taps/s, "
                  f"{written / 1e6:5.2f} MB out);  copy of the output bytes {copy_ms:7.4f} ms")
        out.free()
        other.free()
    src.free()
    gr.close()


if __name__ == "__main__":
    main()
