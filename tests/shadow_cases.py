"""The cases of tests/golden/shadow_shader_v1.npz (tests/golden/make_shadow_golden.py records them and says what each is for) as the CPU and
GPU tests read them, and the case file of tests/cpp/shadow_core_host.cpp."""
import os

import numpy as np

import shadow_ref

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shadow_shader_v1.npz")

# name -> (mode, cascaded, ambient occlusion); VOLUMETRIC_DIFFUSE_FALLBACK is on in all six
DIRECTIONAL = {
    "pcf/64x40": (shadow_ref.MODE_PCF, False, False),
    "pcf_cascades/61x37": (shadow_ref.MODE_PCF, True, True),
    "wide/61x37": (shadow_ref.MODE_PCF_WIDE, False, True),
    "wide_cascades/64x40": (shadow_ref.MODE_PCF_WIDE, True, False),
    "vsm/64x40": (shadow_ref.MODE_VSM, False, False),
    "vsm_cascades/61x37": (shadow_ref.MODE_VSM, True, False),
}
MOMENTS = ("moments_d16/33x17", "moments_d32/16x16")
BLURS = ("blur/1", "blur/4")  # 33 x 17 -> 16 x 8 -> 33 x 17, one and four layers
KNIFE_EDGE_CAP = 0.01         # the share of a case's pixels that may lie on a knife edge

PARAMS = (("inv_view_projection", 16), ("transforms", 64), ("color", 3), ("camera_pos", 3), ("direction", 3), ("camera_front", 3), ("cascade_log_bias", 1))


def load_golden():
    with np.load(GOLDEN_PATH) as z:
        return {k: z[k] for k in z.files}


def pack_params(case):
    return np.concatenate([np.asarray(case[name], np.float32).reshape(-1) for name, _ in PARAMS])


def directional_case(golden, name):
    mode, cascaded, ao = DIRECTIONAL[name]
    case = dict(name=name, mode=mode, cascaded=cascaded, fallback=True)
    for key in ("albedo", "normal", "pbr", "depth", "emissive", "maps", "hdr", "term"):
        case[key] = golden[f"{name}/{key}"]
    case["ambient_occlusion"] = golden[f"{name}/ambient_occlusion"] if ao else None
    at = 0
    for key, count in PARAMS:
        value = golden[f"{name}/params"][at:at + count]
        case[key] = value if count > 1 else float(value[0])
        at += count
    if cascaded:
        case["layers"], case["lerps"] = golden[f"{name}/layers"], golden[f"{name}/lerps"]
    case["height"], case["width"] = case["depth"].shape
    return case


def map_format_code(maps, mode):
    """the code of tests/golden/shadow_runner.cpp and tests/cpp/shadow_core_host.cpp: 0 D16_UNORM, 1 D32_SFLOAT, 2 R32G32_SFLOAT"""
    return 2 if mode == shadow_ref.MODE_VSM else (0 if maps.dtype == np.uint16 else 1)


def words(*parts):
    """32-bit little-endian words of ints, floats and arrays; 16-bit and 8-bit arrays are padded to whole words"""
    out = []
    for p in parts:
        if isinstance(p, (int, np.integer)):
            out.append(np.array([p], np.uint32).tobytes())
        elif isinstance(p, float):
            out.append(np.array([p], np.float32).tobytes())
        else:
            raw = np.ascontiguousarray(p).tobytes()
            out.append(raw + b"\0" * (-len(raw) % 4))
    return b"".join(out)


def host_directional_bytes(case, srgb_table):
    """kind 0 of shadow_core_host"""
    ao = case["ambient_occlusion"]
    ao_h, ao_w = ao.shape if ao is not None else (0, 0)
    layers, map_h, map_w = case["maps"].shape[:3]
    return words(0, case["width"], case["height"], case["mode"], int(case["cascaded"]), int(case["fallback"]), ao_w, ao_h, map_w, map_h, layers,
                 map_format_code(case["maps"], case["mode"]), pack_params(case), np.asarray(srgb_table, np.float32), case["albedo"], case["normal"],
                 case["depth"], case["emissive"], case["pbr"], *([ao] if ao is not None else []), case["maps"])


def parse_host_directional(raw, width, height):
    """-> hdr (h, w, 4) uint16, term (h, w) float32, layers (h, w, 2) int32, lerps (h, w, 2) float32"""
    n = width * height
    hdr = np.frombuffer(raw, np.uint16, n * 4).reshape(height, width, 4)
    term = np.frombuffer(raw, np.float32, n, n * 8).reshape(height, width)
    layers = np.frombuffer(raw, np.int32, n * 2, n * 12).reshape(height, width, 2)
    lerps = np.frombuffer(raw, np.float32, n * 2, n * 20).reshape(height, width, 2)
    assert len(raw) == n * 28
    return hdr, term, layers, lerps


def host_moments_bytes(depth):
    h, w = depth.shape
    return words(1, w, h, 0 if depth.dtype == np.uint16 else 1, depth)


def host_blur_bytes(moments, out_w, out_h, up):
    layers, h, w, _ = moments.shape
    return words(2, w, h, layers, out_w, out_h, int(up), np.asarray(moments, np.float32))


def half_size(size):
    """the VSM chain's middle image: the graph's absolute size * 0.5, converted to unsigned (truncated), at least 1"""
    return max(int(np.float32(size) * np.float32(0.5)), 1)
