"""The sky pass's cases: what tests/golden/make_sky_golden.py records into tests/golden/sky_shader_v1.npz and what the CPU and GPU tests
replay from it.  Every input a test needs is in the file; the definitions here are what the generator builds them from."""
import math
import os

import numpy as np

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sky_shader_v1.npz")
SEED = 20261020


def sun(elevation_deg, azimuth_deg=0.0):
    """Unit vector towards the sun: azimuth 0 is -Z, the way the default camera looks."""
    e, a = math.radians(elevation_deg), math.radians(azimuth_deg)
    return (math.cos(e) * math.sin(a), math.sin(e), -math.cos(e) * math.cos(a))


# camera: direction, up, position, fovy (degrees), z_near, z_far; the aspect is width / height
LEVEL = dict(direction=(0.0, -0.05, -1.0), up=(0.0, 1.0, 0.0), fovy=60.0)
UP = dict(direction=(0.0, 1.0, 0.0), up=(0.0, 0.0, -1.0), fovy=70.0)
RAISED = dict(direction=(0.3, 0.35, -1.0), up=(0.0, 1.0, 0.0), fovy=50.0)

# name -> (width, height, depth pattern, camera, camera_position.y, sun direction, colour)
# The colours are chosen per case so that at least 90 % of the non-zero channel values exceed 0.125 (the generator asserts it): below
# that the absolute allowance of 1e-4 would hide errors of several percent.
PROCEDURAL = {
    # the horizon crosses the image: both outcomes of the earth test; sun high
    "horizon/40x24": (40, 24, "all", LEVEL, 2.0, sun(50.0, 20.0), (18.0, 18.0, 18.0)),
    # none far: nothing is written
    "none/40x24": (40, 24, "none", LEVEL, 2.0, sun(50.0, 20.0), (18.0, 18.0, 18.0)),
    # straight up, the sun at 1 degree of elevation, single-pixel checkerboard, partial tiles both ways
    "up_low_sun/67x35": (67, 35, "checker", UP, 0.0, sun(1.0, 0.0), (100.0, 100.0, 100.0)),
    # camera below the ground (clamped), sun 6 degrees below the horizon, one far pixel in every 8 x 8 tile
    "below_dusk/67x35": (67, 35, "isolated", RAISED, -5.0, sun(-6.0, 10.0), (6000.0, 6000.0, 6000.0)),
    # the sun inside the view (the Mie peak), the upper rows far, 1500 m up
    "mie_peak/136x72": (136, 72, "upper", RAISED, 1500.0, tuple(np.array(RAISED["direction"]) / np.linalg.norm(RAISED["direction"])), (20.0, 25.0, 30.0)),
}

# name -> (width, height, depth pattern, camera, cube size, cube levels, colour, lambda property)
# fovy sets the pixel's footprint on the cube: lambda is below 0 (clamped to 0) for a narrow view on a large screen, crosses 0 in a wide
# view on a small one, and exceeds levels - 1 when a pixel spans several texels.
TEXTURED = {
    "cube16_magnified/136x72": (136, 72, "upper", dict(LEVEL, fovy=60.0), 16, 5, (1.0, 0.5, 2.0), "below"),
    "cube16_crossing/40x24": (40, 24, "all", dict(LEVEL, fovy=150.0), 16, 5, (1.0, 1.0, 1.0), "both"),
    "cube16_odd/67x35": (67, 35, "checker", dict(RAISED, fovy=160.0), 16, 5, (0.5, 1.0, 1.5), "both"),
    "cube8_two_levels/40x24": (40, 24, "all", dict(UP, fovy=170.0), 8, 2, (1.0, 1.0, 1.0), "above"),
}

# name -> (size, sun colour, camera_y, sun direction)
CUBES = {
    "sky_cube/8": (8, (30.0, 30.0, 30.0), 2.0, sun(35.0, 40.0)),
    "sky_cube/16": (16, (120.0, 120.0, 120.0), 1500.0, sun(2.0, -120.0)),
}


def depth_pattern(kind, width, height, rng):
    """D32 values: 0 where the G-buffer left the far plane, a depth in (0, 1) elsewhere."""
    near = rng.uniform(0.05, 0.95, (height, width)).astype(np.float32)
    y, x = np.mgrid[0:height, 0:width]
    far = {"all": np.ones((height, width), bool), "none": np.zeros((height, width), bool), "upper": y < (height * 2) // 5,
           "isolated": ((x & 7) == 3) & ((y & 7) == 5), "checker": ((x + y) & 1) == 0}[kind]
    return np.where(far, np.float32(0.0), near).astype(np.float32)


def load_golden():
    return np.load(GOLDEN_PATH)


def apply_case(golden, name):
    keys = ("depth", "inv", "color", "camera_height", "sun_direction", "out", "zero")
    case = {k: golden[f"{name}/{k}"] for k in keys}
    case["height"], case["width"] = case["depth"].shape
    case["camera_height"] = float(case["camera_height"])
    if f"{name}/cube" in golden.files:
        case["cube"] = golden[f"{name}/cube"]
        case["cube_size"], case["cube_levels"] = (int(v) for v in golden[f"{name}/cube_params"])
    return case


def cube_case(golden, name):
    size, = (int(v) for v in golden[f"{name}/size"].reshape(-1))
    return dict(size=size, sun_color=golden[f"{name}/sun_color"], camera_y=float(golden[f"{name}/camera_y"]), sun_direction=golden[f"{name}/sun_direction"],
                out=golden[f"{name}/out"])


def host_apply_bytes(case):
    """The case file of tests/cpp/sky_core_host.cpp, kind 0."""
    cube = np.asarray(case.get("cube", np.zeros(0, np.uint16)), np.uint16)
    cube_words = np.frombuffer(cube.tobytes(), np.uint32)
    parts = [np.uint32(0), np.uint32(case["width"]), np.uint32(case["height"]), np.asarray(case["inv"], np.float32), np.asarray(case["color"], np.float32),
             np.float32(case["camera_height"]), np.asarray(case["sun_direction"], np.float32), np.uint32(case.get("cube_size", 0)),
             np.uint32(case.get("cube_levels", 0)), np.uint32(len(cube_words)), cube_words, np.asarray(case["depth"], np.float32)]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def host_cube_bytes(case):
    parts = [np.uint32(1), np.uint32(case["size"]), np.asarray(case["sun_color"], np.float32), np.float32(case["camera_y"]),
             np.asarray(case["sun_direction"], np.float32)]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def parse_host_apply(raw, width, height):
    pixels = width * height
    rgb = np.frombuffer(raw[:pixels * 12], np.float32).reshape(height, width, 3)
    written = np.frombuffer(raw[pixels * 12:], np.uint32).reshape(height, width)
    return rgb, written
