"""Records tests/golden/ocean_shader_v1.npz: the reference's ocean/generate_fft.comp, ocean/bake_maps.comp and ocean/mipmap.comp, executed
on the CPU, on small inputs.

Needs the reference's sources (REF, as oracle/ref_build/Makefile: default /root/reference).  The shaders are re-spelled with
oracle/ref_build/glsl2cpp.py and gen_swizzles.py into a temporary directory, compiled against oracle/ref_build/glsl_cpu.hpp with the
runner next to this file (one object per set of #defines, -ffp-contract=off), run, and the directory is removed: only inputs, push
blocks and outputs are kept.

    python tests/golden/make_ocean_golden.py [output.npz]

Prints, per generate case, the largest distance between the executed fp32 shader and tests/ocean_ref.py's float64 in fp16 ulps of
(|a| + |b|) g band -- the figure tests/ocean_ref.py's GENERATE_BOUND_UNITS is one unit above -- and checks that ocean_ref's fp32
restatements of bake_maps and mipmap give the shaders' bytes.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "ref_build")]
import ocean_ref as ocr  # noqa: E402
import shader_runner as sr  # noqa: E402

SHADERS = os.path.join(sr.SHADERS, "ocean")

VARIANT_DEFINES = {ocr.HEIGHT: [], ocr.GRADIENT_NORMAL: ["-DGRADIENT_NORMAL"], ocr.GRADIENT_DISPLACEMENT: ["-DGRADIENT_DISPLACEMENT"]}
MIPMAP_DEFINES = {1: "-DMIPMAP_R16F", 2: "-DMIPMAP_RG16F", 4: "-DMIPMAP_RGBA16F"}
BANDS = np.array([1.0, 0.25, 1.75, 0.5, 3.0, 0.125, 2.0, 0.75], np.float32)  # eight distinct amplitudes
PERIOD = np.float32(256.0 / (2.0 * np.pi))
# 2 pi / world size of the default configuration (1024 / 64 * 1024 / 128 = 128), and of its normal map (/ 7.3)
MOD_DEFAULT = np.float32(2.0) * np.float32(np.pi) / np.float32(128.0)
MOD_NORMAL = np.float32(2.0) * np.float32(np.pi) / (np.float32(128.0) / np.float32(7.3))


def build(tmp):
    sr.respell(os.path.join(tmp, "gen"), [f"ocean/{name}.comp" for name in ("generate_fft", "bake_maps", "mipmap")])
    sets = []
    for variant, defines in VARIANT_DEFINES.items():
        for bands in (0, 1):
            sets.append((f"ref_ocean_generate_{variant}_{bands}", ["-DOCEAN_GENERATE", f"-DFREQ_BAND_MODULATION={bands}", *defines]))
    for vertex in (0, 1):
        sets.append((f"ref_ocean_bake_{vertex}", ["-DOCEAN_BAKE", f"-DVERTEX_TEXTURE={vertex}"]))
    for channels, define in MIPMAP_DEFINES.items():
        sets.append((f"ref_ocean_mipmap_{channels}", ["-DOCEAN_MIPMAP", define]))
    objs = sr.compile_runner(tmp, os.path.join(HERE, "ocean_runner.cpp"), [(fn, [f"-DOCEAN_FN={fn}", *defines]) for fn, defines in sets])
    return sr.link(os.path.join(tmp, "libocean_runner.so"), objs)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def distribution(seed=7, n=128):
    """(n, n, 2) float32: unit normals times magnitudes spread over four decades, the DC bin zero as Phillips leaves it"""
    rng = np.random.default_rng(seed)
    d = (rng.standard_normal((n, n, 2)) * 10.0 ** rng.uniform(-4.0, 0.0, (n, n, 1))).astype(np.float32)
    d[0, 0] = 0.0
    return d


def generate_cases():
    """name -> (N.x, N.y, variant, bands on, time, mod).  64 x 64: one group a row, every variant with bands off under the world's mod
    factor and on under the normal map's, and the three times; 128 x 64: non-square; 128 x 128.  (The whole cross product would not fit
    the size a committed file may have.)"""
    out = {}
    names = {ocr.HEIGHT: "height", ocr.GRADIENT_NORMAL: "normal", ocr.GRADIENT_DISPLACEMENT: "displacement"}
    for variant, vname in names.items():
        out[f"generate_64x64_{vname}_bands0_world_t1.5"] = (64, 64, variant, 0, 1.5, MOD_DEFAULT)
        out[f"generate_64x64_{vname}_bands1_normalmap_t1.5"] = (64, 64, variant, 1, 1.5, MOD_NORMAL)
        out[f"generate_64x64_{vname}_bands1_world_t0"] = (64, 64, variant, 1, 0.0, MOD_DEFAULT)
        out[f"generate_64x64_{vname}_bands0_world_t255.9"] = (64, 64, variant, 0, 255.9, MOD_DEFAULT)
    out["generate_64x64_height_bands0_world_t0"] = (64, 64, ocr.HEIGHT, 0, 0.0, MOD_DEFAULT)
    out["generate_128x64_height_bands0_world_t255.9"] = (128, 64, ocr.HEIGHT, 0, 255.9, MOD_DEFAULT)
    out["generate_128x64_normal_bands1_normalmap_t1.5"] = (128, 64, ocr.GRADIENT_NORMAL, 1, 1.5, MOD_NORMAL)
    out["generate_128x64_displacement_bands1_world_t0"] = (128, 64, ocr.GRADIENT_DISPLACEMENT, 1, 0.0, MOD_DEFAULT)
    out["generate_128x128_height_bands1_world_t1.5"] = (128, 128, ocr.HEIGHT, 1, 1.5, MOD_DEFAULT)
    out["generate_128x128_normal_bands0_normalmap_t255.9"] = (128, 128, ocr.GRADIENT_NORMAL, 0, 255.9, MOD_NORMAL)
    return out


def half_image(rng, shape):
    """fp16 bits: values in (-2, 2), negatives included, and a few near +-100"""
    v = rng.uniform(-2.0, 2.0, shape)
    flat = v.reshape(-1)
    where = rng.choice(flat.size, max(4, flat.size // 64), replace=False)
    flat[where] = rng.choice([-100.0, 100.0], where.size) + rng.uniform(-1.0, 1.0, where.size)
    return ocr.float_to_half(v)


def bake_cases():
    """name -> (displacement size, scale, vertex texture).  Height 64 x 64.  scale: that of the default grid (sample distance 1024 / 64 /
    128 = 0.125, the displacement map's times 2^downsample) and an anisotropic pair."""
    f = np.float32
    default = lambda shift: (f(1) / f(0.125), f(1) / f(0.125), f(1) / (f(0.125) * f(1 << shift)), f(1) / (f(0.125) * f(1 << shift)))
    anisotropic = (f(3.0), f(0.7), f(1.3), f(2.5))
    return {
        "bake_64_d32_default_vertex1": (32, default(1), 1), "bake_64_d32_default_vertex0": (32, default(1), 0),
        "bake_64_d64_default_vertex1": (64, default(0), 1),
        "bake_64_d32_anisotropic_vertex1": (32, anisotropic, 1), "bake_64_d64_anisotropic_vertex0": (64, anisotropic, 0),
    }


def mipmap_cases():
    """name -> (in width, in height, channels, result_mod)"""
    out = {}
    for channels in (1, 2, 4):
        for mname, mod in (("ones", (1.0, 1.0, 1.0, 1.0)), ("zero_first", (0.0, 1.0, 1.0, 1.0))):
            for w, h in ((64, 64), (2, 2), (8, 4)):
                out[f"mipmap_{w}x{h}_c{channels}_{mname}"] = (w, h, channels, mod)
    return out


def generate(path):
    if not os.path.isdir(SHADERS):
        raise FileNotFoundError(SHADERS)
    record = {}
    with sr.scratch("ocean_golden_") as tmp:
        lib = C.CDLL(build(tmp))
        dist = distribution()
        record["generate/distribution"] = dist  # a case of N.x x N.y reads rows 0 .. N.y - 1, columns 0 .. N.x - 1 of it
        record["generate/bands"] = BANDS
        worst = 0.0
        for name, (nx, ny, variant, bands, time, mod) in sorted(generate_cases().items()):
            d = np.ascontiguousarray(dist[:ny, :nx])
            push = ocr.generate_push((mod, mod), (nx, ny), np.float32(14.0) / np.float32(nx), time, PERIOD)
            out = np.zeros((ny, nx), np.uint32)
            getattr(lib, f"ref_ocean_generate_{variant}_{bands}")(ptr(d), ptr(out), ptr(push), ptr(BANDS))
            spectrum, s = ocr.generate(d, push, variant, BANDS if bands else None)
            distance = ocr.generate_distance(out, spectrum, s)
            worst = max(worst, distance)
            print(f"{name:56s} shader vs float64: {distance:6.3f} fp16 ulps of (|a| + |b|) g band")
            record[name + "/push"] = push
            record[name + "/spec"] = np.array([variant, bands], np.int32)
            record[name + "/out"] = out
        print(f"largest: {worst:.3f}")
        record["generate/measured_units"] = np.float64(worst)

        rng = np.random.default_rng(11)
        height = half_image(rng, (64, 64))
        record["bake/height"] = height
        for size in (32, 64):
            record[f"bake/displacement{size}"] = half_image(rng, (size, size, 2))
        for name, (size, scale, vertex) in sorted(bake_cases().items()):
            disp = record[f"bake/displacement{size}"]
            push = ocr.bake_push((1.0 / 64, 1.0 / 64, 1.0 / size, 1.0 / size), scale)
            gj, hd = np.zeros((64, 64, 4), np.uint16), np.zeros((64, 64, 4), np.uint16)
            getattr(lib, f"ref_ocean_bake_{vertex}")(ptr(height), 64, 64, ptr(disp), size, size, ptr(push), ptr(gj), ptr(hd))
            ref_gj, ref_hd = ocr.bake_maps(height, disp, push)
            assert np.array_equal(ref_gj, gj) and (not vertex or np.array_equal(ref_hd, hd)), name
            record[name + "/push"] = push
            record[name + "/spec"] = np.array([size, vertex], np.int32)
            record[name + "/grad_jacobian"] = gj
            if vertex:
                record[name + "/height_displacement"] = hd
            print(f"{name:56s} ocean_ref fp32 gives the shader's bytes")

        for name, (w, h, channels, mod) in sorted(mipmap_cases().items()):
            key = f"mipmap/in_{w}x{h}_c{channels}"
            if key not in record:
                record[key] = half_image(rng, (h, w, channels))
            push = ocr.mipmap_push(mod, (np.float32(1) / np.float32(w), np.float32(1) / np.float32(h)), (w // 2, h // 2))
            out = np.zeros((h // 2, w // 2, channels), np.uint16)
            getattr(lib, f"ref_ocean_mipmap_{channels}")(ptr(record[key]), w, h, ptr(push), ptr(out))
            assert np.array_equal(ocr.mipmap(record[key], push), out), name
            record[name + "/push"] = push
            record[name + "/spec"] = np.array([w, h, channels], np.int32)
            record[name + "/out"] = out
            print(f"{name:56s} ocean_ref fp32 gives the shader's bytes")
    np.savez_compressed(path, **record)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    generate(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ocean_shader_v1.npz"))
