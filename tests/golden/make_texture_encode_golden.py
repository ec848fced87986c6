"""Records tests/golden/texture_encode_v1.npz: the reference's RGTC compressor (scene-export/rgtc_compressor.cpp, compiled as it is) and its
mip filter (scene-export/texture_utils.cpp, generate_mipmaps<Ops>) run on the CPU over the cases of tests/texture_encode_cases.py.

Needs the reference's sources (REF, default /root/reference).  Everything is compiled in a temporary directory that is removed afterwards;
only inputs (fixed seed) and outputs are kept.

    python tests/golden/make_texture_encode_golden.py [output.npz]
    python tests/golden/make_texture_encode_golden.py --time [output.txt]

The mip filter: texture_utils.cpp cannot be compiled whole here -- its layout classes need the Vulkan headers -- so the part of it that is
the filter, from `struct TextureFormatUnorm8` to the end of the generate_mipmaps<Ops> template, is copied into the temporary directory
and compiled inside tests/golden/texture_encode_runner.cpp, which instantiates the template over a minimal layout of its own (a GTX
payload).  It is the same arithmetic because it is the same text: sample, mix, round and clamp are the reference's lines calling the
reference's muglm, built with -ffp-contract=off; the layout only answers where a texel lies.

The conditions on the encode cases (tests/texture_encode_ref.py names the classes and the ties) are asserted here and again, from the
fixture, by tests/test_texture_encode_ref_cpu.py.

--time: the reference compressor's single-thread time on 4096 x 4096 inputs of the uniform, gradient and masks families, BC4 from R8 and
BC5 from RG8 -- the scale tools/texture_encode_time.py's device times are read against."""
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "ref_build")]
import shader_runner as sr  # noqa: E402
import texture_encode_cases as tc  # noqa: E402
import texture_encode_ref as ref  # noqa: E402
from shader_runner import REF  # noqa: E402


def build(tmp):
    source = open(os.path.join(REF, "scene-export", "texture_utils.cpp")).read()
    begin, end = source.index("struct TextureFormatUnorm8"), source.index("static void copy_dimensions")
    with open(os.path.join(tmp, "mip_template.inc"), "w") as f:
        f.write(source[begin:end])
    flags = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-w", "-I" + tmp, "-I" + os.path.join(REF, "math"), "-I" + os.path.join(REF, "util"),
             "-I" + os.path.join(REF, "scene-export")]
    objs = sr.compile_objects(tmp, flags, [("runner", os.path.join(HERE, "texture_encode_runner.cpp"), []),
                                           ("rgtc", os.path.join(REF, "scene-export", "rgtc_compressor.cpp"), []), ("muglm", sr.MUGLM, [])])
    return C.CDLL(sr.link(os.path.join(tmp, "libtexture_encode_runner.so"), objs), mode=os.RTLD_LAZY)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def compress(lib, image, block_format):
    h, w, c = image.shape
    channels = 2 if block_format == tc.BC5 else 1
    blocks = np.zeros(((h + 3) // 4, (w + 3) // 4, 8 * channels), np.uint8)
    image = np.ascontiguousarray(image)
    lib.ref_rgtc_compress_image(ptr(image), w, h, c, channels, ptr(blocks))
    return blocks


def decompress(lib, blocks):
    """(4 by, 4 bx, channels): every channel block through the reference's decompress_rgtc_red_block."""
    by, bx, nbytes = blocks.shape
    channels = nbytes // 8
    out = np.zeros((by, bx, channels, 16), np.uint8)
    flat = np.ascontiguousarray(blocks.reshape(by, bx, channels, 8))
    for y in range(by):
        for x in range(bx):
            for c in range(channels):
                lib.ref_rgtc_decompress_block(ptr(flat[y, x, c]), ptr(out[y, x, c]))
    return np.ascontiguousarray(out.reshape(by, bx, channels, 4, 4).transpose(0, 3, 1, 4, 2).reshape(4 * by, 4 * bx, channels))


def check_conditions(infos):
    form = np.concatenate([i["form"] for i in infos])
    counts = [int((form == k).sum()) for k in range(4)]
    endpoint = int(sum(i["endpoint_tie"].sum() for i in infos))
    incumbent = int(sum(i["incumbent_tie"].sum() for i in infos))
    print(f"classes flat / range < 16 / kept / switched: {counts}; endpoint ties {endpoint}; equal-to-incumbent ties {incumbent}")
    assert min(counts) >= 16 and endpoint >= 16 and incumbent >= 16, "the case set misses a condition: change the seed"


def generate(path):
    record = {}
    with sr.scratch("texture_encode_golden_") as tmp:
        lib = build(tmp)
        infos = []
        for name, image in tc.make_encode_inputs().items():
            record[f"enc/{name}/input"] = image
            for fmt in tc.ENCODE_CASES[name][3]:
                blocks = compress(lib, image, fmt)
                record[f"enc/{name}/{fmt}/blocks"] = blocks
                record[f"enc/{name}/{fmt}/decoded"] = decompress(lib, blocks)
                mine, info = ref.encode_image(image, fmt)
                assert np.array_equal(mine, blocks), f"{name}: tests/texture_encode_ref.py differs from the reference"
                infos.append(info)
                if name in tc.FAMILIES:
                    print(name, [int((info["form"] == k).sum()) for k in range(4)], int(info["endpoint_tie"].sum()), int(info["incumbent_tie"].sum()))
        check_conditions(infos)
        for i, (_, ends, bits) in enumerate(tc.HAND_BLOCKS):
            block = record[f"enc/hand/{tc.BC4}/blocks"][0, i]
            assert (int(block[0]), int(block[1])) == ends and int.from_bytes(bytes(block[2:]), "little") == bits, (i, block)

        for name, level0 in tc.make_mip_inputs().items():
            fmt, w, h, layers, levels = tc.MIP_CASES[name]
            _, size = tc.chain_layout(fmt, w, h, layers, levels)
            payload = np.zeros(size, np.uint8)
            assert lib.ref_generate_mipmaps(ptr(payload), ptr(level0), tc.CHANNELS[fmt], w, h, layers, levels) == 0
            record[f"mip/{name}/level0"], record[f"mip/{name}/payload"] = level0, payload
            assert np.array_equal(ref.pack_chain(ref.mip_chain(level0, levels), fmt), payload), f"{name}: tests/texture_encode_ref.py differs from the reference"
            if name == "rg8_16x16":
                v = ref.mip_level_float(level0[0])
                halves = (v - np.floor(v) == 0.5) & (np.floor(v) % 2 == 0)  # roundf goes up, rintf to the even integer below
                print(f"{name}: {int(halves.sum())} values of level 1 are an even integer + .5 before rounding")
                assert halves.sum() >= 16

        # what gtx_convert --mipgen --format bc5_unorm makes of the edge_rg8 image: the chain, then every level's blocks and their decode
        fmt, w, h = tc.RG8, *tc.ENCODE_CASES["edge_rg8"][:2]
        level0 = np.ascontiguousarray(record["enc/edge_rg8/input"][None])
        _, size = tc.chain_layout(fmt, w, h, 1, tc.GTX_LEVELS)
        payload = np.zeros(size, np.uint8)
        assert lib.ref_generate_mipmaps(ptr(payload), ptr(level0), 2, w, h, 1, tc.GTX_LEVELS) == 0
        record["gtx/chain"] = payload
        for level in range(tc.GTX_LEVELS):
            blocks = compress(lib, tc.chain_level(payload, fmt, w, h, 1, tc.GTX_LEVELS, level)[0], tc.BC5)
            record[f"gtx/{level}/blocks"], record[f"gtx/{level}/decoded"] = blocks, decompress(lib, blocks)
    np.savez_compressed(path, **record)
    print(f"{path}: {os.path.getsize(path)} bytes")


def measure(path):
    lines = ["# The reference's RGTC compressor (scene-export/rgtc_compressor.cpp, g++ -O2), one thread of the recording machine's CPU, 4096 x 4096 texels,",
             "# best of 3 runs.  Written by tests/golden/make_texture_encode_golden.py --time.", "# family  target  ms"]
    with sr.scratch("texture_encode_golden_") as tmp:
        lib = build(tmp)
        for family in ("uniform", "gradient", "masks"):
            rng = np.random.default_rng(tc.SEED + 7)
            planes = [tc.blocks_to_image(tc.family_blocks(family, rng, 1024, 1024)) for _ in range(2)]
            for target, image in (("bc4_from_r8", planes[0][:, :, None]), ("bc5_from_rg8", np.stack(planes, axis=2))):
                image = np.ascontiguousarray(image)
                best = 1e30
                for _ in range(3):
                    start = time.perf_counter()
                    compress(lib, image, tc.BC5 if target.startswith("bc5") else tc.BC4)
                    best = min(best, time.perf_counter() - start)
                lines.append(f"{family:9s} {target:13s} {best * 1e3:9.1f}")
                print(lines[-1])
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--time":
        measure(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "texture_encode_reference_cpu.txt"))
    else:
        generate(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "texture_encode_v1.npz"))
