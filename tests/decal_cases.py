"""Named volumetric-decal cases: what tests/golden/make_decal_golden.py records, and what the CPU and GPU tests run.  Every case is tiny:
cluster resolutions 8x8x64, 32x16x64 and 24x40x64 (not a power of two), images 64x32 and 37x19 (odd: quads are cut at both edges).
Built from float64 geometry rounded once to float32: the rounded arrays are the inputs, and they are stored in the golden file, so a test
never depends on rebuilding them bit for bit."""
import math
import os

import numpy as np

import decal_ref as ref
from granite_amd import synth

F = np.float32
RES_Z = 64
RESOLUTIONS = ((8, 8), (32, 16), (24, 40))
PRM_DTYPE = np.dtype([("transform", "<f4", 16), ("clip_scale", "<f4", 4), ("camera_base", "<f4", 3), ("pad0", "<f4"), ("camera_front", "<f4", 3), ("pad1", "<f4"),
                      ("xy_scale", "<f4", 2), ("resolution_xy", "<i4", 2), ("inv_resolution_xy", "<f4", 2), ("num_lights", "<i4"), ("num_lights_32", "<i4"),
                      ("num_decals", "<i4"), ("num_decals_32", "<i4"), ("decals_texture_offset", "<i4"), ("z_max_index", "<i4"), ("z_scale", "<f4"), ("pad2", "<f4", 3)])
assert PRM_DTYPE.itemsize == 176
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decal_shader_v1.npz")


def cluster_params(cam, res, num_decals, texture_offset=0):
    """ClustererParametersBindless as LightClusterer::refresh fills it (clusterer.cpp:1133-1176), the light fields at zero."""
    p = np.zeros(1, PRM_DTYPE)[0]
    vp = cam.VP
    t = np.array([[0.5, 0, 0, 0.5], [0, 0.5, 0, 0.5], [0, 0, 1, 0], [0, 0, 0, 1]]) @ vp
    p["transform"] = np.ascontiguousarray(t.T, F).reshape(16)
    p["clip_scale"] = F([cam.P[0, 0], -cam.P[1, 1], cam.invP[0, 0], -cam.invP[1, 1]])
    p["camera_base"], p["camera_front"] = F(cam.position), F(cam.front)
    p["xy_scale"] = F(res)
    p["resolution_xy"] = res
    p["inv_resolution_xy"] = F(1.0) / F(res)
    p["num_decals"], p["num_decals_32"], p["decals_texture_offset"] = num_decals, (num_decals + 31) // 32, texture_offset
    p["z_max_index"] = RES_Z - 1
    p["z_scale"] = F(1.0) / ref.z_slice_extent(cam.far, RES_Z)
    return p


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * k + (1.0 - math.cos(angle)) * (k @ k)


def box(centre, size, axis=(0.0, 1.0, 0.0), angle=0.0):
    """world transform of a unit box: translate(centre) * rotate * scale(size), 4 x 4 float64"""
    m = np.eye(4)
    m[:3, :3] = rotation(axis, angle) @ np.diag(np.broadcast_to(np.asarray(size, np.float64), 3))
    m[:3, 3] = centre
    return m


def point_at(cam, u, v, distance):
    """world position under normalised screen coordinates (u, v) at view distance `distance`"""
    clip = np.array([2.0 * u - 1.0, 2.0 * v - 1.0, float(cam.depth_from_view_distance(np.float64(distance))), 1.0])
    p = cam.invVP @ clip
    return p[:3] / p[3]


def pack_decals(cam, worlds):
    """mvps (n, 16) column-major, world rows (n, 12), world_to_texture rows (n, 12), slice intervals (max(n, 1), 2)"""
    n = len(worlds)
    mvps = np.zeros((n, 16), F)
    world_rows, rows = np.zeros((n, 12), F), np.zeros((n, 12), F)
    intervals = np.zeros((max(n, 1), 2), np.uint32)
    intervals[0] = ref.EMPTY_RANGE
    extent = ref.z_slice_extent(cam.far, RES_Z)
    for i, world in enumerate(worlds):
        mvps[i] = np.ascontiguousarray((cam.VP @ world).T, F).reshape(16)
        world_rows[i] = F(world[:3]).reshape(12)
        rows[i] = F(np.linalg.inv(world)[:3]).reshape(12)
        lo, hi = ref.decal_z_range(world_rows[i], F(cam.position), F(cam.front))
        intervals[i] = ref.compute_uint_range(lo, hi, extent, RES_Z)
    return mvps, world_rows, rows, intervals


def random_boxes(cam, count, stream, size=(0.3, 2.5)):
    r = np.random.Generator(np.random.PCG64([synth.SEED, 7000 + stream]))
    worlds = []
    for _ in range(count):
        # centres on screen: for a decal wholly right of or below the screen the shader's two forms differ at a resolution whose reciprocal is not
        # exact (the last cell's u + stride rounds above 1.0, its tile's does not), and the stored cases are ones on which they agree
        centre = point_at(cam, r.uniform(0.05, 0.95), r.uniform(0.05, 0.95), r.uniform(1.0, 36.0))
        worlds.append(box(centre, r.uniform(*size, 3), r.normal(size=3), r.uniform(0, math.pi)))
    return worlds


# ---- binning ---------------------------------------------------------------------------------------------------------------------------------
BINNING_SETS = ("in_view", "near_straddle", "behind", "sub_cell", "cell_border", "count_0", "count_1", "count_32", "count_33", "count_70")
BINNING_CASES = [f"{s}/{rx}x{ry}" for s in BINNING_SETS for rx, ry in RESOLUTIONS]


def binning_case(name):
    kind, res = name.split("/")
    res = tuple(int(v) for v in res.split("x"))
    cam = synth.Camera(64, 32)
    direct_mvps = None
    if kind == "in_view":
        worlds = [box(point_at(cam, 0.45, 0.55, 6.0), (2.0, 1.0, 1.5), (1, 2, 3), 0.7)]
    elif kind == "near_straddle":  # corners on both sides of w = 0: the whole screen
        worlds = [box(cam.position + 0.2 * cam.front, 3.0, (0, 1, 0), 0.3), box(point_at(cam, 0.2, 0.3, 5.0), 0.5)]
    elif kind == "behind":  # every corner at w <= 0: vec4(-10), in no cell
        worlds = [box(cam.position - 10.0 * cam.front, 2.0), box(point_at(cam, 0.7, 0.6, 9.0), 1.0, (1, 0, 0), 0.4)]
    elif kind == "sub_cell":
        worlds = [box(point_at(cam, 0.333, 0.611, 7.0), 0.03), box(point_at(cam, 0.9, 0.1, 3.0), 0.01)]
    elif kind == "cell_border":
        # w = 1 everywhere and corners at exactly +-0.5, +-0.25: edges on cell borders of the 8 x 8 and 32 x 16 grids, where only strict comparisons
        # keep the neighbouring cells out
        worlds = [np.eye(4), np.eye(4)]
        direct_mvps = F([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0.1, 0, 0, 0, 0.5, 1], [0.5, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 0.1, 0, 0.25, -0.25, 0.5, 1]])
    else:
        worlds = random_boxes(cam, int(kind.split("_")[1]), len(kind))
    mvps, world_rows, rows, intervals = pack_decals(cam, worlds)
    if direct_mvps is not None:
        mvps = direct_mvps
    return {"name": name, "prm": cluster_params(cam, res, len(worlds)), "mvps": mvps, "intervals": intervals}


# ---- apply -------------------------------------------------------------------------------------------------------------------------------------
def make_texture(width, height, levels, fmt, stream):
    """random RGBA8 with partial alpha and a box-filtered chain: level i is max(1, w >> i) x max(1, h >> i)"""
    r = np.random.Generator(np.random.PCG64([synth.SEED, 9000 + stream]))
    top = r.integers(0, 256, (height, width, 4)).astype(np.float64)
    top[..., 3] = r.integers(64, 231, (height, width))
    chain, level = [], top
    for i in range(levels):
        chain.append(np.clip(np.rint(level), 0, 255).astype(np.uint32))
        h, w = level.shape[:2]
        nh, nw = max(1, h >> 1), max(1, w >> 1)
        level = level[:nh * min(2, h), :nw * min(2, w)].reshape(nh, min(2, h), nw, min(2, w), 4).mean(axis=(1, 3))
    texels = np.concatenate([(c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16) | (c[..., 3] << 24)).reshape(-1) for c in chain]).astype(np.uint32)
    return {"width": width, "height": height, "num_levels": levels, "format": fmt, "texels": texels}


def texture_set():
    return [make_texture(16, 4, 5, ref.FORMAT_RGBA8_SRGB, 0), make_texture(8, 8, 1, ref.FORMAT_RGBA8_UNORM, 1), make_texture(1, 1, 1, ref.FORMAT_RGBA8_SRGB, 2),
            make_texture(16, 4, 5, ref.FORMAT_RGBA8_UNORM, 3), make_texture(8, 8, 1, ref.FORMAT_RGBA8_SRGB, 4)]


def gbuffer(cam, distance, stream):
    """albedo RGBA8_SRGB words with a random alpha (ambient) and reverse-Z depth of a surface at view distance `distance` (h, w)"""
    r = np.random.Generator(np.random.PCG64([synth.SEED, 8000 + stream]))
    h, w = cam.height, cam.width
    c = r.integers(0, 256, (h, w, 4)).astype(np.uint32)
    albedo = c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16) | (c[..., 3] << 24)
    return albedo.astype(np.uint32), cam.depth_from_view_distance(np.broadcast_to(np.asarray(distance, np.float64), (h, w)))


APPLY_CASES = ("two_overlap", "three_overlap_odd", "far_plane", "depth_step", "beyond_slices", "texture_offset_3", "texture_outside", "many")


def apply_case(name):
    odd = name in ("three_overlap_odd", "depth_step", "many")
    w, h = (37, 19) if odd else (64, 32)
    cam = synth.Camera(w, h)
    u = (np.arange(w) + 0.5) / w
    v = (np.arange(h) + 0.5) / h
    distance = 6.0 + 0.5 * np.sin(5.0 * u)[None, :] + 0.25 * np.cos(4.0 * v)[:, None]
    res, offset, textures = (32, 16), 0, texture_set()
    surface = lambda su, sv: point_at(cam, su, sv, 6.0 + 0.5 * math.sin(5.0 * su) + 0.25 * math.cos(4.0 * sv))
    if name == "two_overlap":
        # the first decal is a few pixels wide under the 16 x 4 texture with its full chain: lambda reaches the last level
        worlds = [box(surface(0.45, 0.5), (0.2, 0.3, 1.0), (0, 0, 1), 0.2), box(surface(0.4, 0.5), (3.0, 2.0, 2.5), (0, 0, 1), 0.3),
                  box(surface(0.55, 0.45), (2.0, 2.4, 2.0), (1, 1, 0), 0.5)]
    elif name == "three_overlap_odd":
        res = (8, 8)
        worlds = [box(surface(0.5, 0.5), (5.0, 4.0, 3.0), (0, 0, 1), -0.2), box(surface(0.3, 0.4), (2.5, 2.0, 2.5), (0, 1, 0), 0.6),
                  box(surface(0.45, 0.55), (1.2, 1.4, 2.0), (1, 0, 1), 1.1)]
    elif name == "far_plane":
        worlds = [box(surface(0.5, 0.5), (4.1, 3.1, 3.0), (0, 0, 1), 0.15), box(surface(0.2, 0.7), 0.9, (1, 2, 0), 0.8)]
    elif name == "depth_step":  # the right half of the image is a wall behind the decal; quads across the step difference two depths
        res = (24, 40)
        distance = np.where(u[None, :] < 0.5, distance, 9.5)
        worlds = [box(point_at(cam, 0.5, 0.5, 7.0), (3.0, 2.5, 3.0), (0, 1, 0), 0.4), box(point_at(cam, 0.7, 0.4, 9.5), (2.0, 2.0, 1.0), (0, 0, 1), 0.9)]
    elif name == "beyond_slices":  # the top rows lie at view distance 40, past slice 63's end at 32; the third decal's interval is clamped to slice 63
        distance = np.where(v[:, None] < 0.3, 40.0, distance)
        worlds = [box(surface(0.5, 0.7), (3.0, 1.5, 2.0)), box(point_at(cam, 0.3, 0.1, 40.0), (14.0, 9.0, 6.0), (0, 0, 1), 0.2), box(point_at(cam, 0.7, 0.15, 36.0), (12.0, 12.0, 16.0), (0, 1, 0), 0.3)]
    elif name == "texture_offset_3":
        res, offset = (24, 40), 3
        worlds = [box(surface(0.4, 0.5), (3.0, 2.0, 2.5), (0, 0, 1), 0.3), box(surface(0.6, 0.5), (2.0, 2.4, 2.0), (1, 1, 0), 0.5)]
    elif name == "texture_outside":  # a table of four: decal 1 names entry 4 and is skipped, decal 0 and 2 are not
        offset, textures = 2, texture_set()[:4]
        worlds = [box(surface(0.4, 0.5), (3.0, 2.0, 2.5), (0, 0, 1), 0.3), box(surface(0.6, 0.5), (2.0, 2.4, 2.0), (1, 1, 0), 0.5), box(surface(0.5, 0.3), (1.0, 1.0, 2.0))]
        worlds = [worlds[0], worlds[2], worlds[1]]
    else:  # many: three chunks, decals from a few pixels to a quarter of the screen
        res = (24, 40)
        textures = [texture_set()[i % 5] for i in range(70)]
        r = np.random.Generator(np.random.PCG64([synth.SEED, 7100]))
        worlds = [box(surface(r.uniform(0.05, 0.95), r.uniform(0.05, 0.95)), r.uniform(0.8, 2.5, 3) * (1.0, 1.0, 3.0), r.normal(size=3), r.uniform(0, math.pi)) for _ in range(70)]
        centre = (cam.V @ np.stack([np.append(wd[:3, 3], 1.0) for wd in worlds], 1))[2]
        worlds = [worlds[i] for i in np.argsort(-centre, kind="stable")]  # front to back, as the host layer sorts
    albedo, depth = gbuffer(cam, distance, len(name))
    if name == "far_plane":
        depth = depth.copy()
        depth[h // 2 - 4:h // 2 + 3, w // 2 - 7:w // 2 + 6] = 0.0
        depth[::5, ::7] = 0.0
    mvps, world_rows, rows, intervals = pack_decals(cam, worlds)
    prm = cluster_params(cam, res, len(worlds), offset)
    return {"name": name, "width": w, "height": h, "prm": prm, "world_rows": world_rows, "mvps": mvps, "intervals": intervals, "decal_rows": rows, "albedo": albedo, "depth": F(depth),
            "inv_view_projection": np.ascontiguousarray(cam.invVP.T, F).reshape(16), "textures": textures,
            "bitmask_decal": ref.binning(prm, mvps), "range_decal": ref.z_ranges(intervals, RES_Z)}


# ---- the golden file -----------------------------------------------------------------------------------------------------------------------------
TEXTURE_FIELDS = ("width", "height", "num_levels", "format")


def pack_case(case):
    """the arrays of a case as the golden file keeps them"""
    out = {"prm": np.frombuffer(case["prm"].tobytes(), np.uint32), "mvps": case["mvps"], "intervals": case["intervals"]}
    if "albedo" in case:
        out.update({k: case[k] for k in ("decal_rows", "albedo", "depth", "inv_view_projection")})
        out["size"] = np.array([case["width"], case["height"]], np.int32)
        out["texture_table"] = np.array([[t[f] for f in TEXTURE_FIELDS] for t in case["textures"]], np.uint32).reshape(-1, 4)
        out["texture_texels"] = np.concatenate([t["texels"] for t in case["textures"]]) if case["textures"] else np.zeros(0, np.uint32)
    return out


def golden_case(golden, name):
    get = lambda k: golden[f"{name}/{k}"]
    case = {"name": name, "prm": np.frombuffer(get("prm").tobytes(), PRM_DTYPE)[0], "mvps": get("mvps"), "intervals": get("intervals")}
    if f"{name}/albedo" in golden:
        case.update({k: get(k) for k in ("decal_rows", "albedo", "depth", "inv_view_projection")})
        case["width"], case["height"] = (int(v) for v in get("size"))
        case["textures"], at = [], 0
        for row in get("texture_table"):
            t = dict(zip(TEXTURE_FIELDS, (int(v) for v in row)))
            count = ref.level_offset(t, t["num_levels"])
            t["texels"] = get("texture_texels")[at:at + count]
            at += count
            case["textures"].append(t)
        case["bitmask_decal"], case["range_decal"] = get("bitmask"), get("range")
    return case


def load_golden():
    return np.load(GOLDEN_PATH)
