"""Records tests/golden/yuv_to_rgb_shader_v1.npz: the reference's util/yuv_to_rgb.comp, executed on the CPU, on small frames.

Needs the reference's sources (REF, as oracle/ref_build/Makefile: default /root/reference).  The shader is re-spelled with
oracle/ref_build/glsl2cpp.py and gen_swizzles.py into a temporary directory, compiled against oracle/ref_build/glsl_cpu.hpp with the
runner next to this file (one object per set of specialisation constants), run, and the directory is removed: only inputs, push blocks
and outputs are kept.  glsl_cpu.hpp samples R8 and R8G8 textures but no 16-bit UNORM ones, so the golden covers 8-bit planes only.

    python tests/golden/make_yuv_to_rgb_golden.py [output.npz]

Prints, per case, the share of samples on which tests/yuv_ref.py (float64) gives exactly the shader's code: tests/test_yuv_ref_cpu.py
demands 99 %.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "ref_build")]
import shader_runner as sr  # noqa: E402
import yuv_ref as yr  # noqa: E402

SHADER = os.path.join(sr.SHADERS, "util", "yuv_to_rgb.comp")

# (pq, num_planes, nv21)
VARIANTS = [(0, 1, 0), (0, 2, 0), (0, 2, 1), (0, 3, 0), (1, 1, 0), (1, 2, 0), (1, 2, 1), (1, 3, 0)]


def cases():
    """name -> (size, planes, 4:2:0, nv21, info): 1, 2 and 3 planes, NV12 and NV21, 4:2:0 and 4:4:4, the six sitings, both ranges,
    every matrix, PQ into RGBA16F and off into RGBA8, at odd and even small sizes."""
    out = {}
    for loc in range(6):
        out[f"yuv420p_67x35_siting{loc}"] = ((67, 35), 3, True, 0, yr.info(chroma_location=loc, full_range=0))
        out[f"nv{21 if loc & 1 else 12}_34x18_siting{loc}"] = ((34, 18), 2, True, loc & 1, yr.info(chroma_location=loc, full_range=1, nv21=loc & 1))
        out[f"yuv444p_34x18_siting{loc}"] = ((34, 18), 3, False, 0, yr.info(chroma_location=loc, full_range=loc & 1, matrix=yr.M_BT601_625))
    for m in range(6):
        out[f"yuv420p_34x18_matrix{m}_limited"] = ((34, 18), 3, True, 0, yr.info(matrix=m, full_range=0))
        out[f"nv12_35x19_matrix{m}_full"] = ((35, 19), 2, True, 0, yr.info(matrix=m, full_range=1))
    # gray is recorded in limited range only: in full range r = g = b = y exactly, so the dither entry of +0.5 code puts every sixteenth
    # pixel on a rounding midpoint, where fp32 and float64 part by chance (4 % of the samples), not by error
    out["gray_67x35_limited_bt2020"] = ((67, 35), 1, False, 0, yr.info(full_range=0, matrix=yr.M_BT2020))
    out["gray_34x18_limited"] = ((34, 18), 1, False, 0, yr.info(full_range=0))
    out["pq_nv12_67x35_bt2020"] = ((67, 35), 2, True, 0, yr.info(pq=1, matrix=yr.M_BT2020, full_range=0))
    out["pq_nv21_34x18_bt2020"] = ((34, 18), 2, True, 1, yr.info(pq=1, matrix=yr.M_BT2020, full_range=1, nv21=1, chroma_location=yr.C_TOPLEFT))
    out["pq_yuv444p_34x18_bt2020"] = ((34, 18), 3, False, 0, yr.info(pq=1, matrix=yr.M_BT2020, full_range=0))
    out["pq_yuv420p_35x19_bt601_625"] = ((35, 19), 3, True, 0, yr.info(pq=1, matrix=yr.M_BT601_625, full_range=0, chroma_location=yr.C_LEFT))
    out["pq_gray_34x18_bt709"] = ((34, 18), 1, False, 0, yr.info(pq=1, full_range=1))
    return out


def make_planes(size, n, sub, seed):
    w, h = size
    rng = np.random.default_rng(seed)
    cw, ch = ((w + 1) // 2, (h + 1) // 2) if sub else (w, h)
    planes = [rng.integers(0, 256, (h, w), dtype=np.uint8)]
    planes[0][: h // 3] = (np.arange(w) * 255 // max(1, w - 1)).astype(np.uint8)
    if n == 2:
        planes.append(rng.integers(0, 256, (ch, cw, 2), dtype=np.uint8))
    elif n == 3:
        planes += [rng.integers(0, 256, (ch, cw), dtype=np.uint8) for _ in range(2)]
    return planes


def build(tmp):
    sr.respell(os.path.join(tmp, "gen"), [SHADER])
    variants = [(f"runner_{pq}_{n}_{nv21}", [f"-DSPEC_PQ={pq}", f"-DSPEC_NUM_PLANES={n}", f"-DSPEC_NV21={nv21}"]) for pq, n, nv21 in VARIANTS]
    objs = sr.compile_runner(tmp, os.path.join(HERE, "yuv_to_rgb_runner.cpp"), [*variants, ("runner_entry", ["-DYUV_ENTRY"])])
    return sr.link(os.path.join(tmp, "libyuv_to_rgb_runner.so"), objs)


def ubo_floats(p):
    return np.concatenate([p["yuv_to_rgb"].ravel(), p["primary_conversion"].ravel(), np.float32(p["inv_resolution"]), np.float32(p["chroma_siting"]),
                           np.float32(p["chroma_clamp"]), np.float32([p["unorm_rescale"]])]).astype(np.float32)


def generate(path):
    if not os.path.exists(SHADER):
        raise FileNotFoundError(SHADER)
    record = {}
    with sr.scratch("yuv_golden_") as tmp:
        lib = C.CDLL(build(tmp))
        lib.ref_yuv_to_rgb.restype = C.c_int
        for seed, (name, (size, n, sub, nv21, inf)) in enumerate(sorted(cases().items())):
            w, h = size
            planes = make_planes(size, n, sub, 100 + seed)
            dims = [(q.shape[1], q.shape[0], yr.R8G8 if q.ndim == 3 else yr.R8) for q in planes]
            out_fmt = yr.RGBA16F if inf["pq"] else yr.RGBA8
            p = yr.plan(dims, (w, h, out_fmt), inf)
            ubo = ubo_floats(p)
            out = np.zeros((h, w, 4), np.uint16 if inf["pq"] else np.uint8)
            ptrs = (C.c_void_p * 3)(*[q.ctypes.data for q in planes], *([None] * (3 - n)))
            pw = (C.c_int * 3)(*[d[0] for d in dims], *([0] * (3 - n)))
            ph = (C.c_int * 3)(*[d[1] for d in dims], *([0] * (3 - n)))
            rc = lib.ref_yuv_to_rgb(int(p["spec_pq"]), n, int(p["spec_nv21"]), ptrs, pw, ph, w, h, ubo.ctypes.data_as(C.POINTER(C.c_float)),
                                    out.ctypes.data_as(C.c_void_p))
            assert rc == 0, name
            ref = yr.store(yr.shade(planes, p), out_fmt)
            if inf["pq"]:
                share = float((ref == out).mean())
            else:
                share = min(float((ref[..., c] == out[..., c]).mean()) for c in range(3))
            print(f"{name:36s} yuv_ref exact on {100 * share:7.3f} % of the samples")
            for i, q in enumerate(planes):
                record[f"{name}/plane{i}"] = q
            record[f"{name}/ubo"] = ubo
            record[f"{name}/spec"] = np.array([p["spec_pq"], p["spec_num_planes"], p["spec_nv21"]], np.int32)
            record[f"{name}/info"] = np.array([inf[k] for k in ("bit_depth", "msb_aligned", "full_range", "matrix", "chroma_location", "pq", "nv21")], np.int32)
            record[f"{name}/out"] = out
    np.savez_compressed(path, **record)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(cases())} cases")


if __name__ == "__main__":
    generate(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "yuv_to_rgb_shader_v1.npz"))
