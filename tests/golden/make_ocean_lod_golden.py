"""Records tests/golden/ocean_lod_shader_v1.npz: the reference's ocean/update_lod.comp, ocean/init_counter_buffer.comp and
ocean/cull_blocks.comp, executed on the CPU, on small grids.

Same recipe as make_ocean_golden.py: needs the reference's sources (REF, default /root/reference); the shaders are re-spelled with
oracle/ref_build/glsl2cpp.py and gen_swizzles.py into a temporary directory, compiled against oracle/ref_build/glsl_cpu.hpp with the
runner next to this file (-ffp-contract=off), run, and the directory is removed: only push blocks, planes and outputs are kept.

    python tests/golden/make_ocean_lod_golden.py [output.npz]

Cases: grid_count 4 (one partial 8 x 8 group), 8 (one group) and 16 (four groups) with every camera, frustum and mode below, and the default
grid_count 64 once.  Cameras: at the origin; at negative x and z (a negative image_offset); 500 units up (every LOD at max_lod); 10^4 units
out.  Frusta: planes that accept everything, a perspective frustum from the camera, planes that keep nothing.  Modes: moving and
fixed-position.  Push blocks are those Ocean::update_lod_pass derives (tests/ocean_lod_ref.pass_pushes).

The small grids have grid_resolution 32, 64 and 128 (max_lod 4, 5, 6) and lod_bias -1.5; the default grid has the default bias.

A case is recorded only if, in float64,
  (a) the five taps' integer addressing selects the texels of the float uv route;
  (b) every plane distance that is evaluated for a box has a magnitude of at least 1e-3 * (1 + sum |p_i c_i|);
  (c) at most 2 % of its texels lie in ocean_lod_ref.near_tie_mask of the unrounded float64 LOD, which is stored;
and if ocean_lod_ref's fp32 restatement gives the shaders' counters and patch sets and, outside the mask, the LOD image's bytes.
The camera is nudged, a fraction of a unit at a time, until (c) holds (one texel of sixteen is already 6 %).  The perspective frustum is turned about the vertical, a few degrees at a time, until (b) holds; with the camera 10^4 units out no
turn satisfies it (the bound is then 10 to 20 units, more than a block is wide), and that combination is not recorded."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "ref_build")]
import ocean_lod_ref as olr  # noqa: E402
import shader_runner as sr  # noqa: E402

SHADERS = os.path.join(sr.SHADERS, "ocean")

BLOCK = 16.0  # world units per block, as the default 1024 / 64
LOD_BIAS = -3.5   # the default, for the default grid
SMALL_BIAS = -1.5  # the small grids span 64 to 256 units: a bias that spreads their LODs over 0 .. max_lod
CAMERAS = {"origin": (1.3, 4.0, -2.1), "negative": (-171.7, 6.5, -93.4), "up": (3.1, 500.0, 5.7), "far": (10003.7, 12.0, -10000.9)}
FRUSTA = ("all", "perspective", "none")
COUNTS16 = np.array([8 * 17 + i for i in range(8)] + [0xdead0000 + i for i in range(8)], np.uint32)  # the shader reads the first eight


def build(tmp):
    sr.respell(os.path.join(tmp, "gen"), [f"ocean/{name}.comp" for name in ("update_lod", "init_counter_buffer", "cull_blocks")])
    sets = (("ref_ocean_update_lod", ["-DOCEAN_UPDATE_LOD"]), ("ref_ocean_init_counters", ["-DOCEAN_INIT_COUNTERS", "-DNUM_COUNTERS=8"]),
            ("ref_ocean_cull", ["-DOCEAN_CULL"]))
    objs = sr.compile_runner(tmp, os.path.join(HERE, "ocean_lod_runner.cpp"), [(fn, [f"-DOCEAN_FN={fn}", *defines]) for fn, defines in sets])
    return sr.link(os.path.join(tmp, "libocean_lod_runner.so"), objs)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def perspective(eye, yaw_degrees, pitch_degrees=-12.0, half_fov_degrees=50.0, near=0.5, far=400.0):
    """six inward planes (n, d), n . x + d >= 0 inside: near, far, left, right, bottom, top"""
    yaw, pitch, half = np.radians(yaw_degrees), np.radians(pitch_degrees), np.radians(half_fov_degrees)
    forward = np.array([np.cos(pitch) * np.cos(yaw), np.sin(pitch), np.cos(pitch) * np.sin(yaw)])
    right = np.cross(forward, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, forward)
    eye = np.asarray(eye, np.float64)
    normals = [forward, -forward, np.cos(half) * right + np.sin(half) * forward, -np.cos(half) * right + np.sin(half) * forward,
               np.cos(half) * up + np.sin(half) * forward, -np.cos(half) * up + np.sin(half) * forward]
    points = [eye + near * forward, eye + far * forward, eye, eye, eye, eye]
    return np.array([[*n, -np.dot(n, p)] for n, p in zip(normals, points)], np.float32)


def frustum_of(kind, eye, yaw):
    if kind == "all":
        return np.tile(np.array([0.0, 0.0, 0.0, 1.0], np.float32), (6, 1))
    if kind == "none":
        planes = np.tile(np.array([0.0, 0.0, 0.0, 1.0], np.float32), (6, 1))
        planes[2] = (0.0, 0.0, 0.0, -1.0)  # two planes are evaluated before the break
        return planes
    return perspective(eye, yaw)


def evaluated(dist):
    """(n, n, 6) bool: the planes the loop reaches for each box, the one that breaks included"""
    negative = dist < 0
    before = np.cumsum(negative, axis=-1) - negative
    return before == 0


def margins_hold(push, frustum):
    dist, scale = olr.box_distances(push, frustum)
    reached = evaluated(dist)
    return bool(np.all(np.abs(dist.astype(np.float64))[reached] >= 1e-3 * (1.0 + scale[reached])))


def float_route_taps(push, wrap):
    """texels the shader's nearest sampler selects, in float64 from the fp32 push block"""
    n = int(push[6])
    off = push[4:6].view(np.int32)
    inv = push[8:10].view(np.float32).astype(np.float64)
    x, y = np.meshgrid(np.arange(n), np.arange(n))
    u, v = ((x + int(off[0])).astype(np.float64) + 0.5) * inv[0], ((y + int(off[1])).astype(np.float64) + 0.5) * inv[1]
    out = []
    for ox, oy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
        tx, ty = np.floor(u * n).astype(np.int64) + ox, np.floor(v * n).astype(np.int64) + oy
        out.append((np.mod(tx, n), np.mod(ty, n)) if wrap else (np.clip(tx, 0, n - 1), np.clip(ty, 0, n - 1)))
    return out


def cases():
    """name -> (grid_count, grid_resolution, camera name, frustum kind, fixed, lod_bias)"""
    out = {}
    for gc, gr in ((4, 32), (8, 64), (16, 128)):
        for cname in CAMERAS:
            for kind in FRUSTA:
                if cname == "far" and kind == "perspective":
                    continue
                for fixed in (0, 1):
                    out[f"lod_g{gc}_{cname}_{kind}_{'fixed' if fixed else 'moving'}"] = (gc, gr, cname, kind, fixed, SMALL_BIAS)
    out["lod_g64_default_origin_all_moving"] = (64, 128, "origin", "all", 0, LOD_BIAS)
    return out


def generate(path):
    if not os.path.isdir(SHADERS):
        raise FileNotFoundError(SHADERS)
    record = {"init/counts16": COUNTS16}
    with sr.scratch("ocean_lod_golden_") as tmp:
        lib = C.CDLL(build(tmp))
        draws0 = np.full((8, 8), 0xcdcdcdcd, np.uint32)
        lib.ref_ocean_init_counters(ptr(COUNTS16), ptr(draws0))
        assert np.array_equal(draws0, olr.init_counters(COUNTS16))
        record["init/draws"] = draws0
        worst_mask = 0.0
        for name, (gc, gr, cname, kind, fixed, bias) in sorted(cases().items()):
            size = (BLOCK * gc, BLOCK * gc)
            center = (20.0, -3.0, 40.0)
            for nudge in range(64):  # (c): the camera is moved, 0.37 and 0.23 units at a time, until few enough texels are near a tie
                camera = tuple(np.array(CAMERAS[cname]) + nudge * np.array([0.37, 0.0, 0.23]))
                pushes = olr.pass_pushes(gc, gr, size, bias, camera, bool(fixed), center)
                if olr.near_tie_mask(olr.update_lod(pushes["update"], np.float64)[1]).mean() <= 0.02:
                    break
            update, cull, wrap = pushes["update"], pushes["cull"], pushes["wrap"]
            for turn in range(0, 360, 7):
                frustum = frustum_of(kind, camera, 20.0 + turn)
                if margins_hold(cull, frustum):  # (b)
                    break
            else:
                raise RuntimeError(f"{name}: no turn of the frustum keeps every plane distance clear of zero")
            image = np.full((gc, gc), 0xffff, np.uint16)
            lib.ref_ocean_update_lod(ptr(update), ptr(image), gc)
            _, lod64 = olr.update_lod(update, np.float64)
            mask = olr.near_tie_mask(lod64)
            worst_mask = max(worst_mask, float(mask.mean()))
            if mask.mean() > 0.02:  # (c)
                raise RuntimeError(f"{name}: {mask.mean():.3%} of the texels are near an fp16 tie")
            ref_image, _ = olr.update_lod(update)
            differ = ref_image != image
            assert not np.any(differ & ~mask), name
            assert np.all(np.abs(ref_image.astype(np.int32) - image.astype(np.int32))[differ] <= 1), name
            n = gc
            for (ax, ay), (bx, by) in zip(olr.taps(*[g + int(o) for g, o in zip(np.meshgrid(np.arange(n), np.arange(n)), cull[4:6].view(np.int32))], n, wrap),
                                          float_route_taps(cull, wrap)):  # (a)
                assert np.array_equal(ax, bx) and np.array_equal(ay, by), name
            draws = draws0.copy()
            patches = np.zeros((gc * gc * 8, 8), np.float32)
            lib.ref_ocean_cull(ptr(cull), ptr(frustum), ptr(image), gc, wrap, ptr(patches), ptr(draws))
            ref_draws, ref_patches = olr.cull_blocks(image, cull, frustum, wrap, draws0)
            assert np.array_equal(draws, ref_draws), name
            got = olr.buckets_of(patches, draws, gc * gc)
            for l in range(8):
                assert np.array_equal(got[l].view(np.uint32), olr.sorted_bucket(ref_patches[l]).view(np.uint32)), (name, l)
            kept = int(draws[:, 1].sum())
            print(f"{name:44s} kept {kept:4d} of {gc * gc:4d}  buckets {draws[:, 1].tolist()}  near ties {int(mask.sum())}  ref differs in {int(differ.sum())}")
            record[name + "/spec"] = np.array([gc, gr, fixed, wrap], np.int32)
            record[name + "/config"] = np.array([*size, bias, *camera, *center], np.float32)
            record[name + "/update_push"] = update
            record[name + "/cull_push"] = cull
            record[name + "/frustum"] = frustum
            record[name + "/lods"] = image
            record[name + "/lod64"] = lod64
            record[name + "/draws"] = draws
            record[name + "/patches"] = np.concatenate(got)  # each bucket's first instance_count entries, sorted, bucket after bucket
        print(f"largest share of near-tie texels: {worst_mask:.3%}")
    np.savez_compressed(path, **record)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    generate(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ocean_lod_shader_v1.npz"))
