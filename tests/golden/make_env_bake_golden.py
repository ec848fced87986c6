"""Records tests/golden/env_bake_shader_v1.npz: the reference's skybox_latlon.frag (HAVE_EMISSIVE), util/ibl_specular.frag and
util/ibl_diffuse.frag, executed on the CPU for every texel, face and level of the cases below, and the linear blit of generate_mipmap.

Needs the reference's sources (REF, as oracle/ref_build/Makefile: default /root/reference).  The shaders are re-spelled with
oracle/ref_build/glsl2cpp.py and gen_swizzles.py into a temporary directory and compiled against oracle/ref_build/glsl_cpu.hpp with the
runner next to this file; the per-face matrices come from the reference's math/transforms.cpp and math/muglm/muglm.cpp, compiled into the
same directory.  The directory is removed afterwards: only inputs (fixed seed) and outputs (fp16 bits) are kept.

    python tests/golden/make_env_bake_golden.py [output.npz]

Cases (the smallest that reach every rule):
    equirect_5     16 x 8  -> cube 5, 3 levels       odd blit sizes 5 -> 2 -> 1
    equirect_16    48 x 24 -> cube 16, full chain    the v.x guard column and the +-pi seam of atan
    specular_24    cube 24 (24, 12, 6, 3, 1) -> 8, 4 levels   fractional LODs 1.585 .. 4.585: trilinear, and the clamp at the last level
    specular_16    cube 16 -> 8, 2 levels            roughness 0.001, every H ~ N
    diffuse_8      cube 16 -> 8                      LOD 0
    diffuse_4      cube 16 -> 4                      the +-Y face centres, where cross(up, dir) is smallest

Prints, per case, the distance between the executed shaders (fp32) and tests/env_ref.py (float64) in fp16 ulps: the size of an fp32
evaluation's own error, which tests/test_gpu_env_bake.py's bound is derived from.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "ref_build")]
import env_ref  # noqa: E402
import shader_runner as sr  # noqa: E402
from shader_runner import SHADERS  # noqa: E402

SEED = 20260117


def build(tmp):
    sr.respell(os.path.join(tmp, "gen"), ["skybox_latlon.frag", "util/ibl_specular.frag", "util/ibl_diffuse.frag"])
    runner = os.path.join(HERE, "env_bake_runner.cpp")
    objs = sr.compile_runner(tmp, runner, [("shaders", [])])
    objs += sr.reference_math_objects(tmp, [("matrices", runner, ["-DENV_MATRICES"]), ("transforms", os.path.join(sr.MATH, "transforms.cpp"), []),
                                            ("muglm", sr.MUGLM, [])])
    return sr.link(os.path.join(tmp, "libenv_bake_runner.so"), objs)


def hdr(rng, shape):
    """Positive, HDR-like texels as fp16 bits: log-normal around 0.5 with a few near 1e3; alpha 1."""
    v = (0.5 * np.exp(rng.normal(0.0, 1.0, shape + (4,)))).astype(np.float32)
    flat = v.reshape(-1, 4)
    hot = rng.choice(flat.shape[0], max(flat.shape[0] // 97, 2), replace=False)
    flat[hot, :3] = rng.uniform(600.0, 1200.0, (hot.size, 3))
    flat[:, 3] = 1.0
    return flat.reshape(shape + (4,)).astype(np.float16).view(np.uint16)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def generate(path):
    if not os.path.isdir(SHADERS):
        raise FileNotFoundError(SHADERS)
    rng = np.random.default_rng(SEED)
    record = {}
    with sr.scratch("env_golden_") as tmp:
        lib = C.CDLL(build(tmp), mode=os.RTLD_LAZY)
        matrices = np.zeros((6, 16), np.float32)
        lib.ref_env_matrices(ptr(matrices))
        record["matrices"] = matrices

        def source_cube(size):
            """A full chain: random level 0, levels below by the blit rule (what equirect_to_cube would leave)."""
            levels = env_ref.full_chain_levels(size)
            chain = np.zeros(env_ref.chain_texels(size, levels) * 4, np.uint16)
            chain[:6 * size * size * 4] = hdr(rng, (6, size, size)).reshape(-1)
            got = env_ref.unpack_chain(chain, size, levels)
            for l in range(1, levels):
                got[l] = env_ref.blit_level(got[l - 1], env_ref.level_size(size, l))
            return env_ref.pack_chain(got), levels

        for name, (w, h, size, levels) in (("equirect_5", (16, 8, 5, 3)), ("equirect_16", (48, 24, 16, 5))):
            equirect = hdr(rng, (h, w))
            cube = np.zeros(env_ref.chain_texels(size, levels) * 4, np.uint16)
            lib.ref_env_equirect_to_cube(ptr(matrices), ptr(equirect), w, h, ptr(cube), size, levels)
            record[name + "/equirect"], record[name + "/params"], record[name + "/out"] = equirect, np.array([size, levels], np.int32), cube
            env_ref.report(name, cube, env_ref.pack_chain(env_ref.equirect_to_cube(matrices, equirect, size, levels)))
        for name, (src_size, out_size, out_levels) in (("specular_24", (24, 8, 4)), ("specular_16", (16, 8, 2))):
            src, src_levels = source_cube(src_size)
            out = np.zeros(env_ref.chain_texels(out_size, out_levels) * 4, np.uint16)
            lib.ref_env_specular(ptr(matrices), ptr(src), src_size, src_levels, ptr(out), out_size, out_levels)
            record[name + "/src"], record[name + "/params"], record[name + "/out"] = src, np.array([src_size, src_levels, out_size, out_levels], np.int32), out
            env_ref.check_up_switch(matrices, out_size, out_levels)
            env_ref.report(name, out, env_ref.pack_chain(env_ref.specular(matrices, env_ref.unpack_chain(src, src_size, src_levels), out_size, out_levels)))
        for name, (src_size, out_size) in (("diffuse_8", (16, 8)), ("diffuse_4", (16, 4))):
            src, src_levels = source_cube(src_size)
            out = np.zeros(6 * out_size * out_size * 4, np.uint16)
            lib.ref_env_diffuse(ptr(matrices), ptr(src), src_size, src_levels, ptr(out), out_size)
            record[name + "/src"], record[name + "/params"], record[name + "/out"] = src, np.array([src_size, src_levels, out_size], np.int32), out
            env_ref.report(name, out, env_ref.pack_chain([env_ref.diffuse(matrices, env_ref.unpack_chain(src, src_size, src_levels), out_size)]))
    np.savez_compressed(path, **record)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    generate(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "env_bake_shader_v1.npz"))
