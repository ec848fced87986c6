"""Records tests/golden/bc_decode_shader_v1.npz: the reference's decode/{s3tc,rgtc,bc7,bc6}.comp, executed on the CPU, on the block
sets of tests/bc_cases.py (every BC7 mode and the reserved pattern, every value of BC6H's low five bits in both signednesses, BC1's equal
and tie-sum endpoints, RGTC's equal and ascending endpoints, the mip-tail sizes).

Needs the reference's sources (REF, as oracle/ref_build/Makefile: default /root/reference).  The shaders are re-spelled with
oracle/ref_build/glsl2cpp.py and gen_swizzles.py into a temporary directory -- where the one construct the re-spelling leaves as GLSL, the
`ivec2[](...)` array constructor, is rewritten as a braced initialiser -- compiled against oracle/ref_build/glsl_cpu.hpp with the runner
next to this file (one object per shader and set of specialisation constants), run, and the directory is removed: only block inputs and
decoded outputs are kept.

    python tests/golden/make_bc_decode_golden.py [output.npz]

Prints, per case, the share of samples tests/bc_ref.py flags as ties and how many samples differ from the shader's, on ties and off.
"""
import ctypes as C
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "ref_build")]
import bc_cases  # noqa: E402
import bc_ref  # noqa: E402
import shader_runner as sr  # noqa: E402

SHADERS = os.path.join(sr.SHADERS, "decode")

# (shader, spec0, spec1, defines): dispatch_kernel_s3tc / _rgtc / _bc7 / _bc6 (texture_decoder.cpp)
VARIANTS = [(0, 0, 1, ["-DSPEC_USE_ALPHA=false", "-DSPEC_BC_VERSION=1"]), (0, 1, 1, ["-DSPEC_USE_ALPHA=true", "-DSPEC_BC_VERSION=1"]),
            (0, 1, 2, ["-DSPEC_USE_ALPHA=true", "-DSPEC_BC_VERSION=2"]), (0, 1, 3, ["-DSPEC_USE_ALPHA=true", "-DSPEC_BC_VERSION=3"]),
            (1, 0, 0, ["-DSPEC_DUAL_COMPONENT=false"]), (1, 1, 0, ["-DSPEC_DUAL_COMPONENT=true"]), (2, 0, 0, []),
            (3, 0, 0, ["-DSPEC_SIGNED=false"]), (3, 1, 0, ["-DSPEC_SIGNED=true"])]
# format -> (shader, spec0, spec1)
DISPATCH = {131: (0, 0, 1), 133: (0, 1, 1), 135: (0, 1, 2), 137: (0, 1, 3), 139: (1, 0, 0), 141: (1, 1, 0), 145: (2, 0, 0), 143: (3, 0, 0), 144: (3, 1, 0)}


def build(tmp):
    sr.respell(os.path.join(tmp, "gen"), [f"decode/{name}.comp" for name in ("s3tc", "rgtc", "bc7", "bc6")],
               patch=lambda text: re.sub(r"= ivec2\[\]\((.*?)\);", lambda m: "= {" + m.group(1) + "};", text, flags=re.S))
    variants = [(f"runner_{shader}_{spec0}_{spec1}", [f"-DBC_SHADER={shader}", f"-DBC_SPEC0={spec0}", f"-DBC_SPEC1={spec1}", *defines])
                for shader, spec0, spec1, defines in VARIANTS]
    objs = sr.compile_runner(tmp, os.path.join(HERE, "bc_decode_runner.cpp"), [*variants, ("runner_entry", ["-DBC_ENTRY"])])
    return sr.link(os.path.join(tmp, "libbc_decode_runner.so"), objs)


def generate(path):
    if not os.path.isdir(SHADERS):
        raise FileNotFoundError(SHADERS)
    record = {}
    with sr.scratch("bc_golden_") as tmp:
        lib = C.CDLL(build(tmp))
        lib.ref_bc_decode.restype = C.c_int
        for name, (fmt, w, h, blocks) in sorted(bc_cases.cases().items()):
            blocks = np.ascontiguousarray(blocks, np.uint8)
            ref, ties = bc_ref.decode(fmt, blocks, w, h)
            out = np.zeros_like(ref)
            shader, spec0, spec1 = DISPATCH[fmt]
            rc = lib.ref_bc_decode(shader, spec0, spec1, blocks.ctypes.data_as(C.c_void_p), bc_ref.BLOCK_BYTES[fmt], w, h, out.ctypes.data_as(C.c_void_p))
            assert rc == 0, name
            diff = out.astype(np.int64) != ref.astype(np.int64)
            print(f"{name:22s} ties {100 * ties.mean():6.2f} % of the samples; bc_ref differs on {int(diff[ties].sum())} tie samples, {int(diff[~ties].sum())} others")
            record[f"{name}/format"] = np.array([fmt, w, h], np.int32)
            record[f"{name}/blocks"] = blocks
            record[f"{name}/out"] = out
    np.savez_compressed(path, **record)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(record) // 3} cases")


if __name__ == "__main__":
    generate(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "bc_decode_shader_v1.npz"))
