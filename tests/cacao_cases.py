"""The cases of the SSAO tests: sizes, cameras, settings and scenes, shared by the CPU and GPU tests and by tests/golden/make_cacao_golden.py.
Constants come from tests/golden/cacao_constants_v1.npz, which the reference's own ffx_cacao.cpp wrote: the reference chain of
tests/cacao_ref.py never depends on the code under test."""
import os

import numpy as np

import cacao_ref as cr
from granite_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "cacao_constants_v1.npz")

# width, height: what each exercises (half resolution in brackets)
SIZES = (
    (64, 48),    # [32 x 24] one blur tile
    (61, 45),    # [31 x 23] odd extents at every level, guarded mip stores, gathers at the edge
    (130, 98),   # [65 x 49] two blur tiles each way, mirrored apron, 33 x 25 importance map with the every-ninth counter rule
    (16, 16),    # [8 x 8] mip 3 is 1 x 1, most taps off the image
)
CAMERAS = {
    "survey": {},  # synth.Camera's: 60 degrees, 0.1 .. 100, eye (0, 2, 8) looking at (0, 1, 0)
    "oblique": {"fovy_deg": 45.0, "near": 0.5, "far": 50.0, "eye": (3.0, 4.0, 6.0), "center": (0.0, 0.5, 0.0)},
}
# FFX_CACAO_Settings as 17 dwords.  "reference" is what setup_ffx_cacao installs (renderer/post/ssao.cpp:73-91); "wide" has five times the
# radius, so that geometry close to the camera is sampled tens of texels away and the higher depth mips are read at these small sizes.
SETTINGS_FIELDS = ("radius", "shadow_multiplier", "shadow_power", "shadow_clamp", "horizon_angle_threshold", "fade_out_from", "fade_out_to",
                   "quality_level", "adaptive_quality_limit", "blur_pass_count", "sharpness", "temporal_supersampling_angle_offset",
                   "temporal_supersampling_radius_offset", "detail_shadow_strength", "generate_normals", "bilateral_sigma_squared",
                   "bilateral_similarity_distance_sigma")
SETTINGS_INTEGERS = ("quality_level", "blur_pass_count", "generate_normals")
REFERENCE_SETTINGS = {"radius": 0.6, "shadow_multiplier": 1.0, "shadow_power": 1.5, "shadow_clamp": 0.98, "horizon_angle_threshold": 0.06,
                      "fade_out_from": 20.0, "fade_out_to": 40.0, "quality_level": cr.QUALITY_HIGHEST, "adaptive_quality_limit": 0.75,
                      "blur_pass_count": 2, "sharpness": 0.98, "temporal_supersampling_angle_offset": 0.0,
                      "temporal_supersampling_radius_offset": 0.0, "detail_shadow_strength": 0.5, "generate_normals": 0,
                      "bilateral_sigma_squared": 5.0, "bilateral_similarity_distance_sigma": 0.1}
SETTINGS = {"reference": {}, "wide": {"radius": 3.0}}
QUALITIES = (cr.QUALITY_HIGHEST, cr.QUALITY_HIGH)


def settings_words(variant, quality, blur_passes=2):
    values = dict(REFERENCE_SETTINGS, **SETTINGS[variant], quality_level=quality, blur_pass_count=blur_passes)
    words = np.zeros(17, np.uint32)
    for i, name in enumerate(SETTINGS_FIELDS):
        words[i] = np.uint32(values[name]) if name in SETTINGS_INTEGERS else np.float32(values[name]).view(np.uint32)
    return words


def camera(name, width, height):
    return synth.Camera(width, height, **CAMERAS[name])


def matrices(cam):
    """RenderParameters::projection and ::view as 16 floats each, column-major as muglm keeps them"""
    rp = cam.render_params()
    return np.ascontiguousarray(rp[0:16]), np.ascontiguousarray(rp[16:32])


def key(width, height, cam_name, variant, quality):
    return f"{width}x{height}/{cam_name}/{variant}/q{quality}"


_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN_PATH))
    return _golden


def constants(width, height, cam_name, variant, quality):
    """The four FFX_CACAO_Constants blocks the reference's code computed: (4,) records of cacao_ref.CONSTANTS_DTYPE"""
    return golden()[key(width, height, cam_name, variant, quality) + "/constants"].view(cr.CONSTANTS_DTYPE).reshape(4)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def pack_normal(n):
    q = np.clip(np.rint((0.5 * n + 0.5) * 1023.0), 0, 1023).astype(np.uint32)
    return (q[..., 0] | (q[..., 1] << 10) | (q[..., 2] << 20) | np.uint32(3 << 30)).astype(np.uint32)


def _rays(cam):
    w, h = cam.width, cam.height
    x = ((np.arange(w) + 0.5) / w * 2.0 - 1.0)[None, :] + np.zeros((h, 1))
    y = ((np.arange(h) + 0.5) / h * 2.0 - 1.0)[:, None] + np.zeros((1, w))
    clip = np.stack([x, y, np.full((h, w), 0.5), np.ones((h, w))], axis=-1)
    world = clip @ cam.invVP.T
    world = world[..., :3] / world[..., 3:4]
    d = world - cam.position
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _box_hit(origin, d, lo, hi):
    """slab test; returns (t, normal) with t = inf where the ray misses"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - origin) / d, (hi - origin) / d
    near, far = np.minimum(t0, t1), np.maximum(t0, t1)
    t_in, t_out = near.max(axis=-1), far.min(axis=-1)
    hit = (t_in < t_out) & (t_in > 0)
    axis = near.argmax(axis=-1)
    normal = np.zeros(d.shape)
    np.put_along_axis(normal, axis[..., None], -np.sign(np.take_along_axis(d, axis[..., None], axis=-1)), axis=-1)
    return np.where(hit, t_in, np.inf), normal


def scene_from_hits(cam, t, normal):
    """depth (h, w) float32 D32F and normal (h, w) uint32 A2B10G10R10 of hits at distance t along the pixel rays (inf: sky, depth 0)"""
    d = _rays(cam)
    view_z = t * (d @ cam.front)
    sky = ~np.isfinite(t)
    depth = cam.depth_from_view_distance(np.where(sky, 1.0, view_z))
    depth[sky] = 0.0
    n = np.where(sky[..., None], -cam.front, normal)
    return depth.astype(np.float32), pack_normal(n)


def box_scene(cam, near_block=True, rough_patch=True):
    """A box on a floor, hand-made: depth steps at the box's silhouette, normal creases where it meets the floor and between its faces, sky
    behind.  near_block adds a small block a few tenths of a unit in front of the camera, low and to the left (about a twentieth of the
    image): under the "wide" settings its texels sample tens of texels away, through the higher depth mips.  rough_patch moves every
    pixel of the floor right of the box a few percent towards or away from the camera, at random: occlusion differs from texel to texel
    there, which is what drives the importance map -- and with it the adaptive tap count -- to its maximum."""
    d = _rays(cam)
    origin = cam.position
    with np.errstate(divide="ignore", invalid="ignore"):
        t_floor = -origin[1] / d[..., 1]
    p = origin + t_floor[..., None] * d
    floor_ok = (t_floor > 0) & (np.abs(p[..., 0]) < 30) & (np.abs(p[..., 2]) < 30)
    t = np.where(floor_ok, t_floor, np.inf)
    if rough_patch:
        bumps = np.random.Generator(np.random.PCG64(5)).choice([-1.0, 1.0], t.shape)
        t = np.where(floor_ok & (p[..., 0] > 1.5), t * (1.0 + 0.03 * bumps), t)
    normal = np.zeros(d.shape)
    normal[..., 1] = 1.0
    boxes = [(np.array([-1.2, 0.0, -1.2]), np.array([1.2, 1.5, 1.2]))]
    if near_block:
        right, up = cam.invV[:3, 0], cam.invV[:3, 1]
        centre = origin + 0.4 * cam.front - 0.2 * right - 0.12 * up
        boxes.append((centre - 0.05, centre + 0.05))
    for lo, hi in boxes:
        tb, nb = _box_hit(origin, d, lo, hi)
        closer = tb < t
        t = np.where(closer, tb, t)
        normal = np.where(closer[..., None], nb, normal)
    return scene_from_hits(cam, t, normal)


def synthetic_scene(cam):
    """the synthetic G-buffer of tests/gpu_scene.py / granite_amd/synth.py: a wavy surface, random normals, 2 % sky"""
    g = synth.make_gbuffer(cam)
    return g["depth"], g["normal"]


def plane_scene(cam, distance=5.0):
    """a plane facing the camera at a constant view distance"""
    d = _rays(cam)
    t = distance / (d @ cam.front)
    return scene_from_hits(cam, t, np.broadcast_to(-cam.front, d.shape))


def corner_scene(cam, concave):
    """Two vertical planes meeting at 90 degrees in a crease straight ahead of the camera (the image's middle column), six units away:
    concave -- a room's corner seen from inside, the crease is the farthest column -- or convex -- a building's corner seen from outside."""
    d = _rays(cam)
    right = cam.invV[:3, 0]
    s = np.sqrt(0.5)
    towards_right, towards_left = (right - cam.front) * s, (-right - cam.front) * s  # both face the camera
    left_normal, right_normal = (towards_right, towards_left) if concave else (towards_left, towards_right)
    side = d @ right
    n = np.where((side < 0)[..., None], left_normal, right_normal)
    t = (6.0 * (cam.front @ left_normal)) / np.einsum("hwk,hwk->hw", d, n)  # front . normal is the same for both planes
    return scene_from_hits(cam, np.where(t > 0, t, np.inf), n)


SCENES = {"synthetic": synthetic_scene, "box": box_scene}

# (width, height, camera, settings, scene): every size with both scenes; the wide radius on the box scene, whose near block it is for
CASES = tuple((w, h, cam, variant, scene) for (w, h) in SIZES
              for cam, variant, scene in (("survey", "reference", "synthetic"), ("survey", "wide", "box"), ("oblique", "reference", "box")))


def case_id(case):
    w, h, cam, variant, scene = case
    return f"{w}x{h}-{cam}-{variant}-{scene}"


def case_inputs(case):
    w, h, cam_name, _, scene = case
    return SCENES[scene](camera(cam_name, w, h))
