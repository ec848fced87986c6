"""Records tests/golden/astc_decode_shader_v1.npz: the reference's decode/astc.comp, executed on the CPU with DECODE_8BIT = true and the
LDR error colour, on the block sets of tests/astc_cases.py, and the contents of the lookup tables the shader reads.

Needs the reference's sources (REF, as oracle/ref_build/Makefile: default /root/reference).  The shader is re-spelled with
oracle/ref_build/glsl2cpp.py and gen_swizzles.py into a temporary directory; the functions that build the shader's tables are static
functions of vulkan/texture/texture_decoder.cpp, a file that needs Vulkan headers, so the lines that hold them (from
`struct ASTCQuantizationMode` to the end of `ASTCLutHolder::init_trits_quints`) are cut into the same directory.  Both are compiled
against oracle/ref_build/glsl_cpu.hpp with the runner next to this file, run, and the directory is removed: only block inputs, decoded
outputs and table contents are kept.

    python tests/golden/make_astc_decode_golden.py [output.npz]

Prints, per class, the share of blocks that hold a texel of the error colour and how many texels tests/astc_ref.py decodes otherwise,
and asserts what keeps the sets honest: at most a quarter of the blocks of a class that is no error class hold an error texel, and every
block of an error class does.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "ref_build")]
import astc_cases  # noqa: E402
import astc_ref  # noqa: E402
import shader_runner as sr  # noqa: E402

SHADER = os.path.join(sr.SHADERS, "decode", "astc.comp")
TABLES = os.path.join(sr.REF, "vulkan", "texture", "texture_decoder.cpp")


def build(tmp):
    gen = os.path.join(tmp, "gen")
    sr.respell(gen, [SHADER])
    lines = open(TABLES).read().split("\n")
    first = next(i for i, l in enumerate(lines) if l.startswith("struct ASTCQuantizationMode"))
    start = next(i for i, l in enumerate(lines) if l.startswith("void ASTCLutHolder::init_trits_quints"))
    last = next(i for i in range(start, len(lines)) if lines[i] == "}")
    open(os.path.join(gen, "astc_tables.inc"), "w").write("\n".join(lines[first:last + 1]) + "\n")
    objs = sr.compile_runner(tmp, os.path.join(HERE, "astc_decode_runner.cpp"), [("runner", ["-DSPEC_DECODE_8BIT=true"])])
    return sr.link(os.path.join(tmp, "libastc_decode_runner.so"), objs)


def generate(path):
    for needed in (SHADER, TABLES):
        if not os.path.isfile(needed):
            raise FileNotFoundError(needed)
    record = {}
    with sr.scratch("astc_golden_") as tmp:
        lib = C.CDLL(build(tmp))
        sizes = (C.c_int(), C.c_int())
        lib.ref_astc_table_sizes(C.byref(sizes[0]), C.byref(sizes[1]))
        tables = {"endpoint_quantiser": np.zeros((9, 128, 4), np.uint16), "endpoint_unquant": np.zeros(sizes[0].value, np.uint8),
                  "weight_quantiser": np.zeros((16, 4), np.uint8), "weight_unquant": np.zeros(sizes[1].value, np.uint8), "trits_quints": np.zeros(384, np.uint16)}
        lib.ref_astc_tables(*(tables[k].ctypes.data_as(C.c_void_p) for k in ("endpoint_quantiser", "endpoint_unquant", "weight_quantiser", "weight_unquant", "trits_quints")))
        for bw, bh in astc_cases.FULL:  # 4 x 4 is the one footprint hashed as a small block
            tables[f"partition_{bw}x{bh}"] = np.zeros((32 * bh, 32 * bw), np.uint8)
            lib.ref_astc_partition_table(bw, bh, tables[f"partition_{bw}x{bh}"].ctypes.data_as(C.c_void_p))
        for k, v in tables.items():
            record["tables/" + k] = v
        for name, (fmt, w, h, blocks) in sorted(astc_cases.cases().items()):
            bw, bh = astc_ref.format_footprint(fmt)
            blocks = np.ascontiguousarray(blocks, np.uint8)
            out = np.zeros((h, w, 4), np.uint8)
            assert lib.ref_astc_decode(blocks.ctypes.data_as(C.c_void_p), bw, bh, w, h, out.ctypes.data_as(C.c_void_p)) == 0, name
            share = astc_cases.blocks_with_error(out, bw, bh).mean()
            differ = int((astc_ref.decode(fmt, blocks, w, h) != out).any(-1).sum())
            print(f"{name:40s} {blocks.shape[0] * blocks.shape[1]:4d} blocks, {100 * share:6.2f} % hold an error texel; astc_ref differs on {differ} texels")
            assert share == 1.0 if astc_cases.is_error_class(name) else share <= 0.25, name
            record[f"{name}/format"] = np.array([fmt, w, h], np.int32)
            record[f"{name}/blocks"] = blocks
            record[f"{name}/out"] = out
    np.savez_compressed(path, **record)
    print(f"{path}: {os.path.getsize(path)} bytes, {sum(k.endswith('/out') for k in record)} cases")


if __name__ == "__main__":
    generate(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "astc_decode_shader_v1.npz"))
