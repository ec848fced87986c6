"""gr_texture_encode and gr_texture_generate_mipmap times at 4096 x 4096, from the hipEvent brackets of the launchers (gr_timing_*).
BC4 from R8 and BC5 from RG8, each on uniform-, gradient- and masks-like content (tests/texture_encode_cases.py's families): the share of
blocks that are searched, and of those that are replaced, changes the work by an order of magnitude, so the class mix of a 4096-block
sample (tests/texture_encode_ref.py) is printed beside every time.  Then a full RG8 4096 x 4096 mip chain, 12 launches.
Every shape is warmed up with 5 calls; then three rounds of 50 calls, every round printed as the mean event time of a call.  The CRC-32
of the blocks is printed so that two builds (another lane mapping: make EXTRA_texture_encode=-DGR_RGTC_GROUP=32) can be held to each other.

    python tools/texture_encode_time.py [--output profiles/texture_encode_time.txt]"""
import argparse
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from granite_amd import capi  # noqa: E402
import texture_encode_cases as tc  # noqa: E402
import texture_encode_ref as ref  # noqa: E402

SIZE = 4096
WARMUP, CALLS, ROUNDS = 5, 50, 3


def event_ms(gr, name, call):
    """Mean hipEvent time of one launch under `name`, over CALLS calls."""
    gr.timing_reset()
    for _ in range(CALLS):
        call()
    gr.sync()
    count, total = gr.timing_query()[name]
    return total / count


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--output", default=None)
    args = parser.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    gr = capi.Context(0)
    gr.check(gr.lib.gr_timing_set_filter(gr.handle, b"texture_encode,texture_mip_level"))
    gr.timing_enable(True)
    say(f"# {SIZE} x {SIZE}; {WARMUP} warm-up calls, then {ROUNDS} rounds of {CALLS} calls, hipEvent time of a call (ms); lib dir {os.environ.get('GRANITE_LIB_DIR', 'granite_amd/lib')}")
    for family in ("uniform", "gradient", "masks"):
        rng = np.random.default_rng(tc.SEED + 7)
        planes = [tc.blocks_to_image(tc.family_blocks(family, rng, SIZE // 4, SIZE // 4)) for _ in range(2)]
        form = ref.encode_channel_blocks(ref.fetch_blocks(planes[0][:256, :256, None], 0).reshape(-1, 16))[1]["form"]
        mix = "/".join(str(int((form == k).sum())) for k in range(4))
        for target, fmt, src_fmt, image in (("BC4 from R8", tc.BC4, tc.R8, planes[0]), ("BC5 from RG8", tc.BC5, tc.RG8, np.stack(planes, axis=2))):
            src = capi.DeviceImage(gr, SIZE, SIZE, src_fmt).upload(image)
            pitch = SIZE // 4 * tc.BLOCK_BYTES[fmt]
            blocks = capi.DeviceBuffer(gr, pitch * SIZE // 4)
            call = lambda: gr.texture_encode(fmt, src, blocks.ptr, pitch)
            for _ in range(WARMUP):
                call()
            rounds = [event_ms(gr, "texture_encode", call) for _ in range(ROUNDS)]
            crc = zlib.crc32(blocks.download().tobytes())
            say(f"{family:9s} {target:13s} " + "  ".join(f"{ms:8.4f}" for ms in rounds) + f"   crc32 {crc:08x}   flat/small/kept/switched of 4096 sampled blocks: {mix}")
            blocks.free()
            src.buffer.free()

    rng = np.random.default_rng(tc.SEED + 8)
    levels = 13
    layout, size = tc.chain_layout(tc.RG8, SIZE, SIZE, 1, levels)
    chain = capi.DeviceBuffer(gr, size)
    level0 = rng.integers(0, 256, SIZE * SIZE * 2, dtype=np.uint8)
    gr.check(gr.lib.gr_upload(gr.handle, None, chain.ptr, level0.ctypes.data, level0.nbytes))
    gr.sync()
    views = [capi.Image(chain.ptr + offset, w, h, 2 * w, tc.RG8) for offset, w, h in layout]

    def make_chain():
        for above, below in zip(views, views[1:]):
            gr.texture_generate_mipmap(above, below)
    for _ in range(WARMUP):
        make_chain()
    rounds = [event_ms(gr, "texture_mip_level", make_chain) * (levels - 1) for _ in range(ROUNDS)]
    say(f"RG8 mip chain, {levels - 1} launches: " + "  ".join(f"{ms:8.4f}" for ms in rounds) + f"   crc32 {zlib.crc32(chain.download().tobytes()):08x}")
    gr.close()
    if args.output:
        with open(args.output, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
