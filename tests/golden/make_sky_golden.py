"""Records tests/golden/sky_shader_v1.npz: the reference's skybox.frag (without and with HAVE_EMISSIVE) and
lights/volumetric_light_setup_sky.comp, executed on the CPU for every far pixel / texel of the cases of tests/sky_cases.py.

Needs the reference's sources (REF, as oracle/ref_build/Makefile: default /root/reference).  The shaders are re-spelled with
oracle/ref_build/glsl2cpp.py and gen_swizzles.py into a temporary directory and compiled against oracle/ref_build/glsl_cpu.hpp with the
runner next to this file (-ffp-contract=off); inv_local_view_projection comes from the reference's math/transforms.cpp and
math/muglm/muglm.cpp, compiled into the same directory.  The directory is removed afterwards: only inputs, parameters and outputs are kept
-- the float colour per pixel before any format store, and the mask of far pixels whose result is exactly 0.

    python tests/golden/make_sky_golden.py [output.npz]

The generator asserts each property its cases are there for (tests/sky_cases.py), and prints per case the largest distance between the
executed shader and (a) tests/sky_ref.py, (b) the host build of granite_amd/csrc/sky_core.hpp, in fp16 ulps beyond an absolute 1e-4:
what the GPU test's bound is derived from (tests/test_gpu_sky.py).  The same record gives the same bytes.
"""
import ctypes as C
import io
import math
import os
import pathlib
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "ref_build")]
import env_ref  # noqa: E402
import host_program  # noqa: E402
import shader_runner as sr  # noqa: E402
import sky_cases as sc  # noqa: E402
import sky_ref  # noqa: E402
from shader_runner import SHADERS  # noqa: E402


def braced_vec3_arrays(text):
    """`= vec3[](a, b, ...)` initialising an array declaration: the braced list `= {a, b, ...}` (glsl2cpp.py does this for scalar arrays)."""
    out, pos = [], 0
    while True:
        at = text.find("= vec3[](", pos)
        if at < 0:
            return "".join(out) + text[pos:]
        depth, end = 1, at + len("= vec3[](")
        while depth:
            depth += {"(": 1, ")": -1}.get(text[end], 0)
            end += 1
        out.append(text[pos:at] + "= {" + text[at + len("= vec3[]("):end - 1] + "}")
        pos = end


def build(tmp):
    sr.respell(os.path.join(tmp, "gen"), ["skybox.frag", "lights/volumetric_light_setup_sky.comp"], patch=braced_vec3_arrays)
    runner = os.path.join(HERE, "sky_runner.cpp")
    objs = sr.compile_runner(tmp, runner, [("shaders", [])])
    objs += sr.reference_math_objects(tmp, [("matrices", runner, ["-DSKY_MATRICES"]), ("transforms", os.path.join(sr.MATH, "transforms.cpp"), []),
                                            ("muglm", sr.MUGLM, [])])
    return sr.link(os.path.join(tmp, "libsky_runner.so"), objs), host_program.build_program(tmp, "sky_core_host", "sky_core_host.cpp", exact=True)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def f3(v):
    return np.asarray(v, np.float32).reshape(3)


def hdr_cube(rng, size, levels):
    """HDR-like texels (log-normal around 0.5, a few near 1e3) at level 0, the levels below by the blit rule; fp16 bits."""
    v = (0.5 * np.exp(rng.normal(0.0, 1.0, (6, size, size, 4)))).astype(np.float32)
    flat = v.reshape(-1, 4)
    hot = rng.choice(flat.shape[0], max(flat.shape[0] // 97, 2), replace=False)
    flat[hot, :3] = rng.uniform(600.0, 1200.0, (hot.size, 3))
    flat[:, 3] = 1.0
    chain = np.zeros(env_ref.chain_texels(size, levels) * 4, np.uint16)
    chain[:6 * size * size * 4] = v.astype(np.float16).view(np.uint16).reshape(-1)
    got = env_ref.unpack_chain(chain, size, levels)
    for l in range(1, levels):
        got[l] = env_ref.blit_level(got[l - 1], env_ref.level_size(size, l))
    return env_ref.pack_chain(got)


def run_host(host, tmp, data):
    return host_program.run_program(host, input_bytes=data, tmp_path=pathlib.Path(tmp))


def save(path, record):
    """np.savez_compressed with fixed time stamps: the same record gives the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(record):
            raw = io.BytesIO()
            np.lib.format.write_array(raw, np.asanyarray(record[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, raw.getvalue())


def bright_share(out):
    values = out[out != 0.0]
    return float((values > 0.125).mean()) if values.size else 1.0


def generate(path):
    if not os.path.isdir(SHADERS):
        raise FileNotFoundError(SHADERS)
    rng = np.random.default_rng(sc.SEED)
    record = {}
    with sr.scratch("sky_golden_") as tmp:
        lib_path, host = build(tmp)
        lib = C.CDLL(lib_path, mode=os.RTLD_LAZY)
        lib.ref_sky_camera.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]
        lib.ref_sky_apply.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        lib.ref_sky_cube.argtypes = [C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]

        def camera(name, cam, position_y, width, height):
            direction, up, position = f3(cam["direction"]), f3(cam["up"]), f3((3.0, position_y, -7.0))
            out = np.zeros(48, np.float32)
            lib.ref_sky_camera(ptr(direction), ptr(up), ptr(position), math.radians(cam["fovy"]), width / height, 0.1, 500.0, ptr(out))
            record[name + "/camera"] = np.concatenate([direction, up, position, np.float32([math.radians(cam["fovy"]), width / height, 0.1, 500.0])])
            record[name + "/view"], record[name + "/projection"], record[name + "/inv"] = out[:16].copy(), out[16:32].copy(), out[32:].copy()
            return record[name + "/inv"]

        def apply(name, width, height, pattern, inv, color, camera_height, sun_direction, cube=None, cube_size=0, cube_levels=0):
            depth = sc.depth_pattern(pattern, width, height, rng)
            color, sun_direction = f3(color), f3(sun_direction)
            out = np.zeros((height, width, 3), np.float32)
            raw_lambda = np.full((height, width), np.nan, np.float32)
            lib.ref_sky_apply(ptr(depth), width, height, ptr(inv), ptr(color), camera_height, ptr(sun_direction), None if cube is None else ptr(cube), cube_size,
                              cube_levels, ptr(out), ptr(raw_lambda))
            far = depth == 0.0
            assert np.isfinite(out).all(), name
            record[name + "/depth"], record[name + "/color"], record[name + "/camera_height"] = depth, color, np.float32(camera_height)
            record[name + "/sun_direction"], record[name + "/out"], record[name + "/zero"] = sun_direction, out, sky_ref.zero_mask(out, far)
            if cube is not None:
                record[name + "/cube"], record[name + "/cube_params"] = cube, np.array([cube_size, cube_levels], np.int32)
            case = sc.apply_case(record_view(record), name)
            host_rgb, written = sc.parse_host_apply(run_host(host, tmp, sc.host_apply_bytes(case)), width, height)
            assert np.array_equal(written != 0, far) and written.max(initial=0) <= 1, name
            return case, far, out, raw_lambda, host_rgb

        class record_view:  # what np.load gives the tests, over the record being built
            def __init__(self, r):
                self.r, self.files = r, list(r)

            def __getitem__(self, k):
                return self.r[k]

        for name, (width, height, pattern, cam, position_y, sun_direction, color) in sc.PROCEDURAL.items():
            inv = camera(name, cam, position_y, width, height)
            case, far, out, _, host_rgb = apply(name, width, height, pattern, inv, color, position_y, sun_direction)
            zero = record[name + "/zero"]
            ref = sky_ref.apply_procedural(case["depth"], inv, case["color"], position_y, case["sun_direction"])
            assert np.array_equal(sky_ref.zero_mask(ref, far), zero), f"{name}: sky_ref.py's zero mask"
            assert np.array_equal(sky_ref.zero_mask(host_rgb, far), zero), f"{name}: the host build's zero mask"
            share = bright_share(out)
            assert share >= 0.9, f"{name}: only {share:.3f} of the non-zero values exceed 0.125"
            if name.startswith("horizon"):
                assert zero.any() and (far & ~zero).any(), f"{name}: both outcomes of the earth test"
            if pattern == "none":
                assert not far.any() and not out.any(), name
            print(f"{name:26s} far {int(far.sum()):5d} zero {int(zero.sum()):5d} max {out.max():9.3f} bright {share:.3f}  "
                  f"sky_ref {sky_ref.ulp_distance(ref, out).max():.3f}  host {sky_ref.ulp_distance(host_rgb, out).max():.3f} fp16 ulps beyond 1e-4")

        for name, (width, height, pattern, cam, size, levels, color, side) in sc.TEXTURED.items():
            inv = camera(name, cam, 2.0, width, height)
            cube = hdr_cube(rng, size, levels)
            case, far, out, raw_lambda, host_rgb = apply(name, width, height, pattern, inv, color, 0.0, (0.0, 0.0, 0.0), cube, size, levels)
            lam = raw_lambda[far]
            assert np.isfinite(lam).all(), name
            if side == "below":
                assert (lam < 0.0).all(), f"{name}: lambda {lam.min()} .. {lam.max()}"
            elif side == "both":
                assert (lam < 0.0).any() and ((lam > 0.0) & (lam < levels - 1)).any(), f"{name}: lambda {lam.min()} .. {lam.max()}"
            else:
                assert (lam > levels - 1).any(), f"{name}: lambda {lam.min()} .. {lam.max()}"
            assert np.array_equal(host_rgb.view(np.uint32), out.view(np.uint32)), f"{name}: the host build is the runner's model bit for bit"
            print(f"{name:26s} far {int(far.sum()):5d} lambda {lam.min():7.3f} .. {lam.max():6.3f} max {out.max():9.3f}  host: bit for bit")

        for name, (size, sun_color, camera_y, sun_direction) in sc.CUBES.items():
            sun_color, sun_direction = f3(sun_color), f3(sun_direction)
            out = np.zeros((6, size, size, 4), np.float32)
            lib.ref_sky_cube(size, ptr(sun_color), camera_y, ptr(sun_direction), ptr(out))
            record[name + "/size"], record[name + "/sun_color"], record[name + "/camera_y"] = np.int32(size), sun_color, np.float32(camera_y)
            record[name + "/sun_direction"], record[name + "/out"] = sun_direction, out
            assert np.isfinite(out).all() and (out[..., 3] == 1.0).all(), name
            ref = sky_ref.sky_cube(size, sun_color, camera_y, sun_direction)
            host_rgba = np.frombuffer(run_host(host, tmp, sc.host_cube_bytes(sc.cube_case(record_view(record), name))), np.float32).reshape(out.shape)
            assert np.array_equal(ref == 0.0, out == 0.0) and np.array_equal(host_rgba == 0.0, out == 0.0), f"{name}: zero masks"
            assert (out[..., :3] == 0.0).any() and (out[..., :3] != 0.0).any(), f"{name}: the -Y face sees the earth"
            print(f"{name:26s} zero texels {int((out[..., :3] == 0.0).all(axis=-1).sum()):4d} max {out[..., :3].max():9.3f} bright {bright_share(out[..., :3]):.3f}  "
                  f"sky_ref {sky_ref.ulp_distance(ref, out).max():.3f}  host {sky_ref.ulp_distance(host_rgba, out).max():.3f} fp16 ulps beyond 1e-4")
    save(path, record)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    generate(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sky_shader_v1.npz"))
