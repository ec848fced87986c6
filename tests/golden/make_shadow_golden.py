"""Records tests/golden/shadow_shader_v1.npz: the reference's lights/directional.frag with SHADOWS in six define sets, lights/resolve_vsm.frag
and post/vsm_{down,up}_blur.frag (LAYERED 0 and 1), executed on the CPU for every pixel of the cases below.

Needs the reference's sources (REF, as oracle/ref_build/Makefile: default /root/reference).  The shaders are re-spelled with
oracle/ref_build/glsl2cpp.py and gen_swizzles.py into a temporary directory and compiled against oracle/ref_build/glsl_cpu.hpp with the
runner next to this file, once per define set; the runner supplies the shadow and array samplers.  The directory is removed
afterwards: only inputs (fixed seed) and outputs are kept.

    python tests/golden/make_shadow_golden.py [output.npz]

Cases (the smallest that reach every rule; VOLUMETRIC_DIFFUSE_FALLBACK in all):
    pcf/64x40            SHADOWS                                  16 x 16 x 1 D32   light-space positions left and right of [0, 1]: clamp to edge
    pcf_cascades/61x37   + SHADOW_CASCADES, AMBIENT_OCCLUSION     32 x 24 x 4 D16   view_z over all four cascades, fract > 0.8 (both layers),
                                                                                    cascade > 3.96 (white_lerp), a camera_front that puts the left of
                                                                                    the frame behind the camera plane (view_z = 0, log2 -> -inf -> 0)
    wide/61x37           + SHADOW_MAP_PCF_KERNEL_WIDE, AO         16 x 16 x 1 D32   6 x 6 footprints over steps and over the map's edge
    wide_cascades/64x40  + SHADOW_CASCADES, ..._WIDE              32 x 24 x 4 D16
    vsm/64x40            + DIRECTIONAL_SHADOW_VSM                 32 x 32 x 1 RG32F depth <= moments.x, the 1e-5 variance floor, the 0.25 leak band
    vsm_cascades/61x37   + SHADOW_CASCADES, ..._VSM               32 x 32 x 4 RG32F
Every frame has a patch of far-plane pixels; every map has hard steps on a smooth ramp.
    moments_d16/33x17, moments_d32/16x16                          resolve_vsm.frag
    blur/1, blur/4       33 x 17 -> 16 x 8 -> 33 x 17             the LAYERED 0 form on one layer, the LAYERED 1 form on four

Prints, per case, the distance between the executed shaders (fp32) and tests/shadow_ref.py (float64) -- fp16 ulps beyond 1e-4 for the lit
target, fp32 ulps for moments: the size of an fp32 evaluation's own error, which the bounds of tests/test_gpu_shadows.py are derived from --
and the number of pixels on a knife edge of the depth compare (|ref - texel| <= 2^-20 at a tap with a non-zero weight), which are left out
of that distance.  Asserts that they are at most 1 % of a case's pixels.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "ref_build")]
import shadow_cases as sc  # noqa: E402
import shadow_ref  # noqa: E402
import shader_runner as sr  # noqa: E402
from shader_runner import SHADERS  # noqa: E402

SEED = 20261021
FALLBACK = "-DVOLUMETRIC_DIFFUSE_FALLBACK"
VARIANTS = {
    "pcf/64x40": ("pcf", ["-DSHADOWS", FALLBACK]),
    "pcf_cascades/61x37": ("pcf_cascades", ["-DSHADOWS", "-DSHADOW_CASCADES", FALLBACK, "-DAMBIENT_OCCLUSION"]),
    "wide/61x37": ("wide", ["-DSHADOWS", "-DSHADOW_MAP_PCF_KERNEL_WIDE", FALLBACK, "-DAMBIENT_OCCLUSION"]),
    "wide_cascades/64x40": ("wide_cascades", ["-DSHADOWS", "-DSHADOW_CASCADES", "-DSHADOW_MAP_PCF_KERNEL_WIDE", FALLBACK]),
    "vsm/64x40": ("vsm", ["-DSHADOWS", "-DDIRECTIONAL_SHADOW_VSM", FALLBACK]),
    "vsm_cascades/61x37": ("vsm_cascades", ["-DSHADOWS", "-DSHADOW_CASCADES", "-DDIRECTIONAL_SHADOW_VSM", FALLBACK]),
}


class ShadowRun(C.Structure):
    """ShadowRun of shadow_runner.cpp"""
    _fields_ = [(n, C.c_void_p) for n in ("albedo", "normal", "pbr", "depth", "emissive", "ambient_occlusion", "maps", "hdr", "colour", "term", "layers", "lerps")] + \
               [(n, C.c_int32) for n in ("width", "height", "ao_width", "ao_height", "map_width", "map_height", "map_layers", "map_format")] + \
               [("inv_view_projection", C.c_float * 16), ("transforms", C.c_float * 64), ("color", C.c_float * 3), ("camera_pos", C.c_float * 3),
                ("direction", C.c_float * 3), ("camera_front", C.c_float * 3), ("cascade_log_bias", C.c_float)]


def build(tmp):
    sr.respell(os.path.join(tmp, "gen"), ["lights/directional.frag", "lights/resolve_vsm.frag", "post/vsm_down_blur.frag", "post/vsm_up_blur.frag"])
    variants = [(symbol, ["-DSHADOW_VARIANT=" + symbol, *defines]) for symbol, defines in VARIANTS.values()] + [("vsm_chain", ["-DSHADOW_VSM_CHAIN"])]
    objs = sr.compile_runner(tmp, os.path.join(HERE, "shadow_runner.cpp"), variants, jobs=4)
    return sr.link(os.path.join(tmp, "libshadow_runner.so"), objs)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------
EYE, FORWARD, NEAR = np.array([3.0, 2.0, 10.0]), unit([0.1, -0.2, -1.0]), 0.1
RIGHT = unit(np.cross(FORWARD, [0.0, 1.0, 0.0]))
UP = np.cross(RIGHT, FORWARD)
LIGHT = unit([0.4, 0.8, 0.45])  # towards the light
LIGHT_X = unit(np.cross(LIGHT, [0.0, 0.0, 1.0]))
LIGHT_Y = np.cross(LIGHT, LIGHT_X)


def inverse_view_projection(width, height):
    """reverse-Z, infinite far plane: depth = NEAR / view distance; column-major fp32"""
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = RIGHT, UP, -FORWARD
    view[:3, 3] = -view[:3, :3] @ EYE
    f = 1.0 / np.tan(np.radians(30.0))
    proj = np.array([[f * height / width, 0, 0, 0], [0, -f, 0, 0], [0, 0, 0, NEAR], [0, 0, -1, 0]], np.float64)
    return np.linalg.inv(proj @ view).T.reshape(16).astype(np.float32)


def frame(rng, width, height, nearest, farthest):
    """G-buffer and emissive: the view distance runs from `nearest` to `farthest` along a diagonal, with noise; a patch on the far plane"""
    x, y = np.meshgrid((np.arange(width) + 0.5) / width, (np.arange(height) + 0.5) / height)
    t = np.clip(0.75 * x + 0.25 * y + rng.normal(0.0, 0.02, (height, width)), 0.0, 1.0)
    depth = (NEAR / (nearest * (farthest / nearest) ** t)).astype(np.float32)
    depth[height // 5:height // 5 + 6, width // 2:width // 2 + 9] = 0.0
    depth[-1, -3:] = 0.0
    n = unit(-FORWARD + 0.6 * LIGHT)[None, None, :] + rng.normal(0.0, 0.45, (height, width, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    q = np.rint((n * 0.5 + 0.5) * 1023.0).astype(np.uint32)
    normal = q[..., 0] | (q[..., 1] << 10) | (q[..., 2] << 20) | (np.uint32(3) << 30)
    albedo = rng.integers(0, 1 << 32, (height, width), dtype=np.uint64).astype(np.uint32)
    pbr = rng.integers(0, 1 << 16, (height, width), dtype=np.uint32).astype(np.uint16)
    emissive = rng.uniform(0.0, 2.0, (height, width, 4)).astype(np.float16).view(np.uint16)
    return dict(albedo=albedo, normal=normal, pbr=pbr, depth=depth, emissive=emissive)


def transform(centre, radius, depth_radius):
    """world -> (u, v, z): [centre - radius, centre + radius] across the light's axes onto [0, 1], column-major fp32"""
    m = np.eye(4)
    for row, (axis, r) in enumerate(((LIGHT_X, radius), (LIGHT_Y, radius), (LIGHT, depth_radius))):
        m[row, :3] = axis / (2.0 * r)
        m[row, 3] = 0.5 - axis @ centre / (2.0 * r)
    return m.T.reshape(16).astype(np.float32)


def occluder_field(rng, layers, height, width):
    """hard steps (blocks of 3 x 4 texels) on a smooth ramp, around the receivers' z of 0.5"""
    x, y = np.meshgrid(np.arange(width) / width, np.arange(height) / height)
    ramp = 0.42 + 0.12 * x + 0.05 * y
    blocks = rng.choice([-0.2, 0.0, 0.0, 0.15], (layers, (height + 2) // 3, (width + 3) // 4))
    steps = np.repeat(np.repeat(blocks, 3, 1), 4, 2)[:, :height, :width]
    return ramp[None] + steps + rng.normal(0.0, 0.004, (layers, height, width))


def shadow_maps(rng, mode, layers, height, width, d16):
    field = occluder_field(rng, layers, height, width)
    if mode != shadow_ref.MODE_VSM:
        return np.rint(np.clip(field, 0.0, 1.0) * 65535.0).astype(np.uint16) if d16 else field.astype(np.float32)
    # moments: variance far below the 1e-5 floor, and of the size of d * d (the leak band); a corner no receiver is behind
    variance = np.repeat(np.repeat(rng.choice([1e-8, 1e-4, 2e-3, 2e-2], (layers, (height + 3) // 4, (width + 3) // 4)), 4, 1), 4, 2)[:, :height, :width]
    mx = field.astype(np.float32)
    mx[:, :height // 4, :width // 4] = 1.5
    return np.stack([mx, (mx.astype(np.float64) ** 2 + variance).astype(np.float32)], -1)


def directional_inputs(rng, name):
    mode, cascaded, ao = sc.DIRECTIONAL[name]
    width, height = (int(v) for v in name.split("/")[1].split("x"))
    case = frame(rng, width, height, 0.6, 110.0 if cascaded else 40.0)
    case["inv_view_projection"] = inverse_view_projection(width, height)
    case["color"], case["camera_pos"], case["direction"] = np.float32([3.0, 2.8, 2.5]), EYE.astype(np.float32), LIGHT.astype(np.float32)
    # pcf_cascades: a front vector that is not the camera's, so that the left of the frame has a negative view_z
    front = unit(0.3 * FORWARD + RIGHT) if name.startswith("pcf_cascades") else FORWARD
    case["camera_front"] = front.astype(np.float32)
    case["cascade_log_bias"] = np.float32(1.0 - np.log2(10.0))  # cascade i begins at view_z = 5 * 2^i
    if cascaded:
        case["transforms"] = np.concatenate([transform(EYE + FORWARD * 4.0 * 2.0 ** i, 9.0 * 2.0 ** i, 130.0) for i in range(4)])
    else:
        # a map far smaller than the frame's extent in light space, off its middle: the frame leaves it on the left and on the right and clamps
        case["transforms"] = np.concatenate([transform(EYE + FORWARD * 12.0 + LIGHT_X * 14.0, 11.0, 60.0), np.zeros(48, np.float32)])
    if mode == shadow_ref.MODE_VSM:
        case["maps"] = shadow_maps(rng, mode, 4 if cascaded else 1, 32, 32, False)
    elif cascaded:
        case["maps"] = shadow_maps(rng, mode, 4, 24, 32, True)
    else:
        case["maps"] = shadow_maps(rng, mode, 1, 16, 16, False)
    if ao:
        case["ambient_occlusion"] = rng.integers(0, 256, ((height + 1) // 2, (width + 1) // 2), dtype=np.uint16).astype(np.uint8)
    return dict(case, mode=mode, cascaded=cascaded, fallback=True, width=width, height=height)


def run_directional(lib, case, symbol):
    h, w = case["height"], case["width"]
    out = dict(hdr=np.zeros((h, w, 4), np.uint16), colour=np.zeros((h, w, 3), np.float32), term=np.zeros((h, w), np.float32),
               layers=np.zeros((h, w, 2), np.int32), lerps=np.zeros((h, w, 2), np.float32))
    run = ShadowRun()
    for key in ("albedo", "normal", "pbr", "depth", "emissive", "maps"):
        case[key] = np.ascontiguousarray(case[key])
        setattr(run, key, case[key].ctypes.data)
    for key, array in out.items():
        setattr(run, key, array.ctypes.data)
    ao = case.get("ambient_occlusion")
    if ao is not None:
        run.ambient_occlusion, run.ao_height, run.ao_width = ao.ctypes.data, *ao.shape
    run.width, run.height = w, h
    run.map_layers, run.map_height, run.map_width = case["maps"].shape[:3]
    run.map_format = sc.map_format_code(case["maps"], case["mode"])
    for key in ("inv_view_projection", "transforms", "color", "camera_pos", "direction", "camera_front"):
        getattr(run, key)[:] = [float(v) for v in case[key]]
    run.cascade_log_bias = float(case["cascade_log_bias"])
    getattr(lib, "ref_shadow_directional_" + symbol)(C.byref(run))
    return out


def report_directional(name, case, out, srgb_table):
    ref = shadow_ref.directional_light(case, srgb_table)
    edge = ref["edge"] <= shadow_ref.KNIFE_EDGE
    pixels = edge.size
    assert edge.sum() <= sc.KNIFE_EDGE_CAP * pixels, f"{name}: {edge.sum()} of {pixels} pixels on a knife edge: choose another seed"
    got = out["hdr"][..., :3].view(np.float16).astype(np.float64)
    distance = shadow_ref.ulp_distance(got, ref["hdr"])[~edge].max()
    term = np.abs(out["term"] - ref["term"])[~edge].max()
    print(f"{name}: executed shader against shadow_ref: {distance:.3f} fp16 ulps beyond 1e-4, shadow term {term:.3e}; {int(edge.sum())} of {pixels} pixels on a "
          f"knife edge (cap {int(sc.KNIFE_EDGE_CAP * pixels)})")
    if case["cascaded"]:
        near, far, lerp, white = ref["cascade"]
        live = ~ref["far"]
        both = int((out["lerps"][..., 0][live] > 0).sum())
        print(f"    layers {sorted(set(out['layers'][live].reshape(-1).tolist()))}, both layers at {both} pixels, white_lerp > 0 at {int((out['lerps'][..., 1][live] > 0).sum())}, "
              f"= 1 at {int((out['lerps'][..., 1][live] >= 1).sum())}; layer decisions differing from float64: {int((out['layers'][..., 0][live] != near[live]).sum())}")
    lit = np.abs(ref["lit"] - ref["dark"]).max(-1) > 1e-3
    print(f"    term 0 at {int((out['term'] == 0).sum())}, 1 at {int((out['term'] == 1).sum())} (far plane {int(ref['far'].sum())}), between at "
          f"{int(((out['term'] > 0) & (out['term'] < 1)).sum())} of {pixels}; the term changes the target at {int(lit.sum())}")


def generate(path):
    if not os.path.isdir(SHADERS):
        raise FileNotFoundError(SHADERS)
    rng = np.random.default_rng(SEED)
    record = {}
    with sr.scratch("shadow_golden_") as tmp:
        lib = C.CDLL(build(tmp), mode=os.RTLD_LAZY)
        table = np.zeros(256, np.float32)
        lib.ref_srgb_table(ptr(table))
        record["srgb_table"] = table
        for name, (symbol, _) in VARIANTS.items():
            case = directional_inputs(rng, name)
            out = run_directional(lib, case, symbol)
            for key in ("albedo", "normal", "pbr", "depth", "emissive", "maps"):
                record[f"{name}/{key}"] = case[key]
            if case.get("ambient_occlusion") is not None:
                record[f"{name}/ambient_occlusion"] = case["ambient_occlusion"]
            record[f"{name}/params"] = sc.pack_params(case)
            record[f"{name}/hdr"], record[f"{name}/term"] = out["hdr"], out["term"]
            if case["cascaded"]:
                record[f"{name}/layers"], record[f"{name}/lerps"] = out["layers"].astype(np.int8), out["lerps"]
            report_directional(name, case, out, table)

        for name in sc.MOMENTS:
            width, height = (int(v) for v in name.split("/")[1].split("x"))
            d16 = "d16" in name
            depth = shadow_maps(rng, shadow_ref.MODE_PCF, 1, height, width, d16)[0]
            moments = np.zeros((height, width, 2), np.float32)
            lib.ref_vsm_moments(ptr(depth), 0 if d16 else 1, width, height, ptr(moments))
            record[f"{name}/depth"], record[f"{name}/out"] = depth, moments
            print(f"{name}: executed shader against shadow_ref: {shadow_ref.ulp32_distance(moments, shadow_ref.vsm_moments(depth)).max():.3f} fp32 ulps")

        for name in sc.BLURS:
            layers = int(name.split("/")[1])
            source = shadow_maps(rng, shadow_ref.MODE_VSM, layers, 17, 33, False)
            half_w, half_h = sc.half_size(33), sc.half_size(17)
            down = np.zeros((layers, half_h, half_w, 2), np.float32)
            up = np.zeros((layers, 17, 33, 2), np.float32)
            lib.ref_vsm_blur(ptr(source), 33, 17, layers, ptr(down), half_w, half_h, 0, int(layers > 1))
            lib.ref_vsm_blur(ptr(down), half_w, half_h, layers, ptr(up), 33, 17, 1, int(layers > 1))
            record[f"{name}/in"], record[f"{name}/down"], record[f"{name}/up"] = source, down, up
            d_down = shadow_ref.ulp32_distance(down, shadow_ref.vsm_blur(source, half_w, half_h, False)).max()
            d_up = shadow_ref.ulp32_distance(up, shadow_ref.vsm_blur(down, 33, 17, True)).max()
            print(f"{name}: executed shaders against shadow_ref: down {d_down:.3f}, up {d_up:.3f} fp32 ulps")
    np.savez_compressed(path, **record)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    generate(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "shadow_shader_v1.npz"))
