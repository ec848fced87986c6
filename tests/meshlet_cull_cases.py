"""Scenes for meshlet culling: the cases of tests/golden/meshlet_cull_shader_v1.npz (built here, recorded by
tests/golden/make_meshlet_cull_golden.py from the executed shader) and seeded random scenes for the GPU tests.

A case is small on purpose: the task counts cross the wave and half-wave boundaries (0, 1, 31, 32, 33, 63, 64, 65, 130), tasks have 1,
31 or 32 chunks (and a few in between), one case dispatches from a non-zero offset, one writes two draw lists into one output buffer, and
one directed case per cause places an element just inside and just outside what decides it.  Every case of three tasks or more except `all` and
those named `none_*` also carries two ballast tasks: one in front of everything with occluder word 0x55555555 and one behind the camera,
so that no specialisation set leaves its list empty or full.

Each case is built once per projection (o0 perspective, o1 orthographic); the random cases hold the same world for both.  Positions are chosen in the shader's view space after
view_transform_yz_flip (x right, y down, z ahead) and carried to the world through the inverse camera in float64; what is stored is
float32, and the decisions are whatever the shader makes of those.

Depth: 100 x 60 and 200 x 40 linear view depth, a near wall over part of the screen in front of a far plane.  The chain is what
setup_depth_hierarchy_pass(..., true) keeps: the size rounded up to multiples of 64 and halved (64 x 32, 128 x 32), floor_log2(max) - 1
levels (5, 6), every texel the maximum of its 2 x 2 (edge texels repeat), min LOD 1."""
import os
import zlib

import numpy as np

import meshlet_cull_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_PATH = os.path.join(HERE, "golden", "meshlet_cull_shader_v1.npz")
PHASES = (0, 1, 2)
COUNT_WORDS = 4          # dwords 0..3 of the output buffer are count words; list A uses 0, list B uses 1
NEAR, FAR = 0.5, 200.0
WALL_Z, FAR_Z = 8.0, 150.0


def sets():
    """(phase, flags): phase x ORTHO x SKINNED, and FORCE_VISIBLE for phase 2"""
    out = []
    for phase in PHASES:
        for ortho in (0, ref.ORTHO):
            for skinned in (0, ref.SKINNED):
                out.append((phase, ortho | skinned))
                if phase == 2:
                    out.append((phase, ortho | skinned | ref.FORCE_VISIBLE))
    return out


def set_name(phase, flags):
    return f"p{phase}f{flags}"


# ---- depth and its chain -----------------------------------------------------------------------------------------------------------------
def synthetic_depth(width, height):
    """linear view depth: a wall at WALL_Z over the left half and a block on the right, the far plane elsewhere"""
    d = np.full((height, width), FAR_Z, np.float32)
    d[:, :width // 2] = WALL_Z
    d[height // 4:height // 2, (3 * width) // 4:(7 * width) // 8] = WALL_Z + 4.0
    return d


def chain_shape(width, height):
    cw, ch = (width + 63) // 64 * 64 // 2, (height + 63) // 64 * 64 // 2
    levels = int(np.floor(np.log2(max(width, height)))) - 1
    return cw, ch, levels


def max_chain(depth):
    """(flat chain, chain_width, chain_height, levels)"""
    h, w = depth.shape
    cw, ch, levels = chain_shape(w, h)
    ys, xs = np.minimum(np.arange(2 * ch), h - 1), np.minimum(np.arange(2 * cw), w - 1)
    level = depth[np.ix_(ys, xs)]
    out = []
    def halve(a, axis):
        """pairs along `axis`; an odd last element is folded into the last pair (a single element stays)"""
        n = a.shape[axis]
        if n == 1:
            return a
        a = np.moveaxis(a, axis, 0)
        r = np.maximum(a[0:2 * (n // 2):2], a[1:2 * (n // 2):2])
        if n & 1:
            r[-1] = np.maximum(r[-1], a[-1])
        return np.moveaxis(r, 0, axis)

    for _ in range(levels):
        level = halve(halve(level, 0), 1)
        out.append(level.astype(np.float32).ravel())
    sizes = ref.level_sizes(cw, ch, levels)
    assert [len(o) for o in out] == [a * b for a, b in sizes]
    return np.concatenate(out), cw, ch, levels


SCREENS = {"a": (100, 60), "b": (200, 40)}


def chains():
    return {key: max_chain(synthetic_depth(*size)) for key, size in SCREENS.items()}


# ---- camera ------------------------------------------------------------------------------------------------------------------------------
class Camera:
    """World -> view is a rotation about y and a translation; projection[1].y is negative, as Granite's Vulkan projection has it."""

    def __init__(self, ortho, screen, position=(1.0, 2.0, 3.0), yaw=0.35):
        self.ortho, self.screen = bool(ortho), screen
        self.width, self.height = SCREENS[screen]
        c, s = np.cos(yaw), np.sin(yaw)
        self.rotation = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]], np.float64)
        self.position = np.array(position, np.float64)
        view = np.eye(4)
        view[:3, :3] = self.rotation
        view[:3, 3] = -self.rotation @ self.position
        self.view = view
        aspect = self.width / self.height
        p = np.zeros((4, 4))
        if self.ortho:
            half_w = 10.0
            half_h = half_w / aspect
            p[0, 0], p[1, 1], p[2, 2], p[2, 3], p[3, 3] = 1.0 / half_w, -1.0 / half_h, 1.0 / (NEAR - FAR), NEAR / (NEAR - FAR), 1.0
        else:
            t = np.tan(np.radians(30.0))
            p[0, 0], p[1, 1], p[2, 2], p[2, 3], p[3, 2] = 1.0 / (aspect * t), -1.0 / t, FAR / (NEAR - FAR), NEAR * FAR / (NEAR - FAR), -1.0
        self.projection = p
        vp = p @ view
        planes = np.stack([vp[3] + vp[0], vp[3] - vp[0], vp[3] + vp[1], vp[3] - vp[1], vp[2], vp[3] - vp[2]])
        self.planes = (planes / np.linalg.norm(planes[:, :3], axis=1)[:, None]).astype(np.float32)

    def scale_bias(self):
        """bind_meshlet_culling_ubo's arithmetic (renderer.cpp:553-563) in fp32; the projection as column-major [column][row]"""
        F = np.float32
        p = self.projection.T.astype(np.float32)
        half = (F(0.5) * F(self.width), F(0.5) * F(self.height))
        sb = [half[0], half[1], half[0], half[1]]
        sb[2] = sb[2] + sb[0] * p[3][0]
        sb[3] = sb[3] + sb[1] * p[3][1]
        sb[0] = sb[0] * p[0][0]
        sb[1] = sb[1] * -p[1][1]
        return np.array(sb, np.float32)

    def frustum(self, chain):
        _, cw, ch, levels = chain
        F = np.float32
        viewport = [F(0.5) * F(self.width) - F(0.5), F(0.5) * F(self.height) - F(0.5), F(0.5) * F(self.width), F(0.5) * F(self.height)]
        return ref.pack_frustum(self.planes, self.view.T.astype(np.float32), self.scale_bias(), viewport, (cw << 1, ch << 1), 1.0, 1, levels - 1 + 1)

    def world(self, v):
        """the world position of a point of the shader's view space (x right, y down, z ahead)"""
        v = np.asarray(v, np.float64)
        return self.position + self.rotation.T @ np.array([v[0], -v[1], -v[2]])

    def pixels_per_unit(self, z):
        sb = self.scale_bias().astype(np.float64)
        return (sb[0], sb[1]) if self.ortho else (sb[0] / z, sb[1] / z)

    def at_pixel(self, px, py, z):
        """view-space point that lands on pixel (px, py) at depth z"""
        sb = self.scale_bias().astype(np.float64)
        x, y = (px - sb[2]) / sb[0], (py - sb[3]) / sb[1]
        return np.array([x, y, z]) if self.ortho else np.array([x * z, y * z, z])


# ---- scene builder -----------------------------------------------------------------------------------------------------------------------
def random_affine(rng, uniform=False):
    """rotation x scale (non-uniform unless asked) and a translation, float64 3 x 4"""
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    scale = np.full(3, rng.uniform(0.5, 2.0)) if uniform else rng.uniform(0.4, 2.5, 3)
    m = np.zeros((3, 4))
    m[:, :3] = r * scale[None, :]
    m[:, 3] = rng.uniform(-3, 3, 3)
    return m


class Builder:
    def __init__(self, camera, rng):
        self.camera, self.rng = camera, rng
        self.place = Camera(False, camera.screen)  # random tasks and the ballast lie where the perspective camera sees them, for both projections
        self.aabbs, self.transforms, self.bounds, self.draws, self.tasks, self.occluders = [], [], [], [], [], []
        self.next_index, self.next_vertex = 0, 0

    def add(self, spheres, affine=None, aabb=None, words=None, cones=None):
        """One instance: `spheres` are (world centre, world radius) per chunk, in world space; they are carried into the instance's local
        space through `affine`.  aabb: (lo, hi) in world space, default the spheres' box.  words: the occluder word per task, or one value.
        cones: per chunk (world axis, cutoff) or None for cutoff 1 (no cone test).  One task per 32 chunks at a 32-aligned offset."""
        m = random_affine(self.rng) if affine is None else np.asarray(affine, np.float64)
        inv = np.linalg.inv(m[:, :3])
        max_scale = np.sqrt(max((m[:, :3] ** 2).sum(axis=0)))
        node, box = len(self.transforms), len(self.aabbs)
        self.transforms.append(m.astype(np.float32).ravel())
        centres = np.array([c for c, _ in spheres], np.float64).reshape(-1, 3)
        radii = np.array([r for _, r in spheres], np.float64)
        if aabb is None:
            aabb = ((centres - radii[:, None]).min(axis=0), (centres + radii[:, None]).max(axis=0))
        self.aabbs.append(np.array([*aabb[0], 0.0, *aabb[1], 0.0], np.float32))
        first = len(self.bounds)
        assert first % 32 == 0
        for k, (c, r) in enumerate(spheres):
            local = inv @ (np.asarray(c, np.float64) - m[:, 3])
            axis, cutoff = (np.array([0.0, 0.0, 1.0]), 1.0) if cones is None or cones[k] is None else cones[k]
            # cone.xyz * M3 must come out along the world axis: local axis = M3 applied backwards, M3[i] = row i
            local_axis = np.linalg.solve(m[:, :3], np.asarray(axis, np.float64))
            local_axis /= np.linalg.norm(local_axis)
            self.bounds.append(np.array([*local, r / max_scale, *local_axis, cutoff], np.float32))
            prims = int(self.rng.integers(1, 257))
            self.draws.append(np.array([3 * prims, self.next_index, self.next_vertex], np.uint32))
            self.next_index += 3 * prims
            self.next_vertex += int(self.rng.integers(3, 256))
        count = len(spheres)
        while len(self.bounds) % 32:
            self.bounds.append(np.zeros(8, np.float32))
            self.draws.append(np.zeros(3, np.uint32))
        for t, j in enumerate(range(0, count, 32)):
            word = words[t] if isinstance(words, (list, tuple)) else (int(self.rng.integers(0, 1 << 32)) | int(self.rng.integers(0, 1 << 32)) if words is None else words)
            self.tasks.append(np.array([box, len(self.occluders), node, first + j + (min(count - j, 32) - 1), int(self.rng.integers(0, 1 << 24))], np.uint32))
            self.occluders.append(word & 0xFFFFFFFF)

    def ballast(self):
        cam = self.place
        near = [(cam.world(cam.at_pixel(cam.width * f, cam.height * 0.5, 2.0)), 0.15) for f in (0.3, 0.5, 0.7)]
        self.add(near, words=0x55555555, affine=random_affine(self.rng, uniform=True))
        self.add([(cam.world([0.0, 0.0, -30.0]), 0.5)], words=0xFFFFFFFF)

    def scene(self, chain_key, chain, dispatches, capacity=None):
        total = sum((int(t[3]) & 31) + 1 for t in self.tasks)
        capacity = total if capacity is None else capacity
        lists = len(dispatches_lists(dispatches))
        output = np.full(COUNT_WORDS + 5 * capacity * lists + 7, ref.POISON_WORD, np.uint32)
        output[:COUNT_WORDS] = 0

        def arr(rows, width, dtype):
            return np.array(rows, dtype).reshape(-1, width)
        return {"tasks": arr(self.tasks, 5, np.uint32), "aabbs": arr(self.aabbs, 8, np.float32), "transforms": arr(self.transforms, 12, np.float32),
                "bounds": arr(self.bounds, 8, np.float32), "draws": arr(self.draws, 3, np.uint32), "occluders": np.array(self.occluders, np.uint32),
                "output": output, "frustum": self.camera.frustum(chain), "camera": self.camera.position.astype(np.float32),
                "chain_key": chain_key, "chain": chain[0], "chain_width": chain[1], "chain_height": chain[2], "chain_levels": chain[3],
                "dispatches": np.array(dispatches, np.uint32).reshape(-1, 4)}


def dispatches_lists(dispatches):
    return sorted({int(d[2]) for d in dispatches})


def one_list(count, offset=0):
    return [(offset, count, 0, COUNT_WORDS)]


def random_sphere(cam, rng, z_range=(1.0, 40.0), r_pixels=(0.2, 12.0), margin=0.35):
    """a sphere somewhere around the screen, some of them off it"""
    z = float(np.exp(rng.uniform(np.log(z_range[0]), np.log(z_range[1]))))
    px, py = rng.uniform(-margin, 1 + margin) * cam.width, rng.uniform(-margin, 1 + margin) * cam.height
    r = rng.uniform(*r_pixels) / abs(cam.pixels_per_unit(z)[0])
    return cam.world(cam.at_pixel(px, py, z)), float(r)


def random_cone(cam, rng, centre):
    """facing the camera, facing away, or none"""
    kind = rng.integers(0, 3)
    if kind == 0:
        return None
    to_camera = cam.position - centre
    to_camera /= np.linalg.norm(to_camera)
    axis = to_camera if kind == 1 else -to_camera
    axis = axis + rng.normal(scale=0.3, size=3)
    return axis / np.linalg.norm(axis), float(rng.uniform(0.1, 0.9))


def random_tasks(b, rng, tasks, chunk_counts=(1, 31, 32, 2, 5, 1, 3, 2, 8, 1, 4)):
    cam = b.place
    made, k = 0, 0
    while made < tasks:
        chunks = chunk_counts[k % len(chunk_counts)]
        k += 1
        anchor, _ = random_sphere(cam, rng)
        spheres = []
        for _ in range(chunks):
            c, r = random_sphere(cam, rng)
            spheres.append((anchor + 0.15 * (c - anchor), r))
        cones = [random_cone(cam, rng, c) for c, _ in spheres]
        kind = made % 3
        b.add(spheres, cones=cones, words=[0, None, 0xFFFFFFFF][kind])
        made += 1


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
TASK_COUNTS = (0, 1, 31, 32, 33, 63, 64, 65, 130)
BIG = 500.0


def big_box(cam):
    """an AABB that holds the whole frustum: always visible, and in phase 2 its sphere straddles the near plane (perspective) or has
    closest_z far behind the camera (orthographic)"""
    return cam.position - BIG, cam.position + BIG


def _counts(cam, rng, b, n):
    """n tasks in all, the ballast among them; a lone task is one of 32 chunks scattered over and around the screen"""
    if n == 1:
        spheres = [random_sphere(cam, rng, z_range=(2.0, 6.0)) for _ in range(32)]
        b.add(spheres, aabb=big_box(cam), words=0x0F0F3355)
    elif n:
        random_tasks(b, rng, n - len(b.tasks))
    assert len(b.tasks) == n
    return one_list(n)


def _directed(name):
    def build(cam, rng, b):
        DIRECTED[name](cam, rng, b)
        return one_list(len(b.tasks))
    return build


def d_aabb_planes(cam, rng, b):
    """one box outside each plane, one box across each plane, one inside"""
    w, h = cam.width, cam.height
    outside = {0: (-0.5 * w, 0.5 * h, 10.0), 1: (1.5 * w, 0.5 * h, 10.0), 2: (0.5 * w, 1.6 * h, 10.0), 3: (0.5 * w, -0.6 * h, 10.0), 4: (0.5 * w, 0.5 * h, -3.0),
               5: (0.5 * w, 0.5 * h, FAR + 30.0)}
    across = {0: (0.0, 0.5 * h, 10.0), 1: (1.0 * w, 0.5 * h, 10.0), 2: (0.5 * w, 1.0 * h, 10.0), 3: (0.5 * w, 0.0, 10.0), 4: (0.5 * w, 0.5 * h, NEAR),
              5: (0.5 * w, 0.5 * h, FAR)}
    for table in (outside, across):
        for i in range(6):
            px, py, z = table[i]
            v = cam.at_pixel(px, py, abs(z))
            v[2] = z
            c = cam.world(v)
            b.add([(c, 0.3), (c + 0.2, 0.2)], aabb=(c - 0.6, c + 0.6))
    c = cam.world(cam.at_pixel(0.75 * w, 0.8 * h, 6.0))
    b.add([(c, 0.3)], aabb=(c - 0.5, c + 0.5))


def d_sphere_planes(cam, rng, b):
    """in one always-visible box: a sphere outside each plane, one touching each from outside and from inside"""
    w, h = cam.width, cam.height
    spheres = []
    for i, n in enumerate(cam.planes.astype(np.float64)):
        inside = cam.world(cam.at_pixel(0.75 * w, 0.5 * h, 20.0))
        dist = inside @ n[:3] + n[3]
        on_plane = inside - dist * n[:3]
        for out, r in ((3.0, 1.0), (1.0, 1.02), (1.0, 0.98), (-0.5, 0.2)):
            spheres.append((on_plane - out * n[:3], r))
    b.add(spheres, aabb=big_box(cam))


def d_cone(cam, rng, b):
    """cones facing the camera, facing away, at the limit, and cutoff >= 1 (no test) -- all on screen in front of the wall"""
    spheres, cones = [], []
    for k in range(24):
        c = cam.world(cam.at_pixel(cam.width * (0.55 + 0.4 * (k % 6) / 6), cam.height * (0.55 + 0.4 * (k // 6) / 4), 6.0))
        to_camera = (cam.position - c) / np.linalg.norm(cam.position - c)
        tilt = rng.normal(size=3)
        tilt -= tilt @ to_camera * to_camera
        tilt /= np.linalg.norm(tilt)
        angle = [0.0, 0.6, 1.2, 1.5, 1.6, 2.0, 2.6, 3.1][k % 8]
        axis = np.cos(angle) * -to_camera + np.sin(angle) * tilt  # angle 0: facing away
        cutoff = [0.2, 0.5, 0.8, 1.0, 1.5, 0.0][k % 6]
        spheres.append((c, 0.05))
        cones.append((axis, cutoff))
    b.add(spheres, cones=cones, aabb=big_box(cam))


def d_transforms(cam, rng, b):
    """non-uniformly scaled and rotated instances: the radius grows by the largest column scale, so a sphere just outside a plane by its
    own radius is inside with the scaled one"""
    n = cam.planes[0].astype(np.float64)
    for k in range(6):
        m = random_affine(rng)
        inside = cam.world(cam.at_pixel(0.6 * cam.width, 0.6 * cam.height, 12.0))
        on_plane = inside - (inside @ n[:3] + n[3]) * n[:3]
        spheres = [(on_plane - d * n[:3], 1.0) for d in (0.9, 1.1, 1.6, 2.4, 3.5, -2.0)]
        b.add(spheres, affine=m, aabb=big_box(cam))


def d_near(cam, rng, b):
    """spheres straddling the near plane and just beyond the acceptance distance r + 0.1, behind nothing and in front of the wall"""
    spheres = []
    for z, r in ((0.6, 0.3), (0.9, 1.0), (1.05, 1.0), (1.15, 1.0), (1.5, 0.5), (0.55, 0.449), (0.55, 0.451)):
        for fx in (0.25, 0.75):
            spheres.append((cam.world(cam.at_pixel(fx * cam.width, 0.5 * cam.height, z)), r))
    b.add(spheres, aabb=big_box(cam))


def d_occlusion(cam, rng, b):
    """behind the wall (occluded), in front of it, and over the far plane; boxes of their own, so the crude AABB test decides too"""
    w, h = cam.width, cam.height
    for fx, fy, z, r in ((0.2, 0.5, 12.0, 0.5), (0.2, 0.5, 5.0, 0.5), (0.7, 0.8, 40.0, 0.5), (0.8, 0.35, 10.0, 0.3), (0.8, 0.35, 14.0, 0.3), (0.2, 0.3, 8.4, 0.5),
                         (0.2, 0.3, 8.6, 0.5), (0.49, 0.5, 20.0, 0.6), (0.3, 0.7, WALL_Z + 0.5, 0.5)):
        c = cam.world(cam.at_pixel(fx * w, fy * h, z))
        b.add([(c, r), (c + 0.1, 0.5 * r)], aabb=(c - 1.2 * r, c + 1.2 * r))
    spheres = [(cam.world(cam.at_pixel(fx * w, 0.6 * h, z)), 0.4) for fx in (0.1, 0.3, 0.45, 0.55, 0.7, 0.9) for z in (6.0, 9.0, 30.0)]
    b.add(spheres, aabb=big_box(cam))


def d_spans(cam, rng, b):
    """pixel spans of 0, 1, 2, 3 and many texels: small spheres at pixel phases, then growing ones"""
    w, h = cam.width, cam.height
    spheres = []
    for k in range(32):
        z = 6.0 if k % 2 else 20.0
        r_pixels = [0.05, 0.3, 0.6, 1.1, 1.6, 2.4, 5.0, 11.0][k % 8]
        px, py = (0.1 + 0.8 * ((k * 7) % 32) / 32) * w + 0.37 * k, (0.15 + 0.7 * ((k * 5) % 32) / 32) * h + 0.21 * k
        spheres.append((cam.world(cam.at_pixel(px, py, z)), r_pixels / abs(cam.pixels_per_unit(z)[0])))
    b.add(spheres, aabb=big_box(cam))


def d_lod_clamp(cam, rng, b):
    """LOD clamped at hiz_min_lod (spans of 0 .. 2) and at hiz_max_lod (spans beyond 2^max_lod)"""
    w, h = cam.width, cam.height
    spheres = []
    for r_pixels, z in ((0.1, 6.0), (0.4, 6.0), (0.9, 30.0), (1.4, 6.0), (8.0, 6.0), (18.0, 6.0), (30.0, 30.0), (45.0, 6.0), (70.0, 5.0), (45.0, 30.0)):
        spheres.append((cam.world(cam.at_pixel(0.5 * w + 0.3, 0.5 * h + 0.3, z)), r_pixels / abs(cam.pixels_per_unit(z)[0])))
    b.add(spheres, aabb=big_box(cam))


def d_span_sides(cam, rng, b):
    """spans leaving the screen on each side, the sphere still crossing the side's plane"""
    w, h = cam.width, cam.height
    spheres = []
    for px, py in ((-1.0, 0.5 * h), (w + 1.0, 0.5 * h), (0.5 * w, -1.0), (0.5 * w, h + 1.0), (-2.0, -2.0), (w + 2.0, h + 2.0), (w + 20.0, 0.3 * h), (0.8 * w, h + 6.0)):
        for z in (6.0, 25.0):
            spheres.append((cam.world(cam.at_pixel(px, py, z)), 6.0 / abs(cam.pixels_per_unit(z)[0])))
    b.add(spheres, aabb=big_box(cam))


def d_phase_words(cam, rng, b):
    """visible tasks whose occluder word is zero, partial and full; invisible tasks with a non-zero word (phase 2 clears it)"""
    w, h = cam.width, cam.height
    for word in (0, 0x0000FFFF, 0xA5A5A5A5, 0xFFFFFFFF, 1, 0x80000000):
        spheres = [(cam.world(cam.at_pixel((0.55 + 0.012 * k) * w, (0.6 + 0.01 * k) * h, 5.0 + 0.05 * k)), 0.1) for k in range(32)]
        b.add(spheres, words=word)
    for word in (0xFFFFFFFF, 0x00F0F000, 0):
        c = cam.world([0.0, 0.0, -20.0])
        b.add([(c, 0.5), (c + 0.3, 0.2)], words=word)
    c = cam.world(cam.at_pixel(0.2 * w, 0.5 * h, 30.0))  # behind the wall: visible to the planes, occluded in phase 2
    b.add([(c, 0.5), (c + 0.3, 0.2)], words=0xFFFFFFFF, aabb=(c - 1.0, c + 1.0))


DIRECTED = {"aabb_planes": d_aabb_planes, "sphere_planes": d_sphere_planes, "cone": d_cone, "transforms": d_transforms, "near_straddle": d_near,
            "occlusion": d_occlusion, "pixel_spans": d_spans, "lod_clamp": d_lod_clamp, "span_sides": d_span_sides, "phase_words": d_phase_words}


def _all(cam, rng, b):
    for k in range(5):
        spheres = [(cam.world(cam.at_pixel((0.55 + 0.01 * j) * cam.width, (0.3 + 0.1 * k) * cam.height, 4.0)), 0.1) for j in range([1, 31, 32, 7, 32][k])]
        b.add(spheres, words=0xFFFFFFFF)
    return one_list(len(b.tasks))


def _none_outside(cam, rng, b):
    for k in range(5):
        c = cam.world([3.0 * k, 1.0, -10.0 - k])
        b.add([(c + 0.1 * j, 0.2) for j in range([1, 31, 32, 7, 32][k])], words=0xFFFFFFFF)
    return one_list(len(b.tasks))


def _offset(cam, rng, b):
    random_tasks(b, rng, 30)
    b.ballast()
    random_tasks(b, rng, 38)
    return one_list(50, 5)


def _two_lists(cam, rng, b):
    random_tasks(b, rng, 38)
    total = sum((int(t[3]) & 31) + 1 for t in b.tasks)
    return [(0, 25, 0, COUNT_WORDS), (25, len(b.tasks) - 25, 1, COUNT_WORDS + 5 * total)]


def case_table():
    """name -> (screen, builder, ballast)"""
    table = {}
    for n in TASK_COUNTS:
        name = "none_tasks_0" if n == 0 else f"tasks_{n}"
        table[name] = ("b" if n in (33, 65) else "a", (lambda cam, rng, b, n=n: _counts(cam, rng, b, n)), n >= 3)
    table["offset_nonzero"] = ("a", _offset, False)
    table["two_lists"] = ("b", _two_lists, True)
    table["all"] = ("a", _all, False)
    table["none_outside"] = ("a", _none_outside, False)
    for name in DIRECTED:
        table[name] = ("b" if name in ("pixel_spans", "occlusion") else "a", _directed(name), True)
    table["pixel_spans_a"] = ("a", _directed("pixel_spans"), True)
    return table


CASE_NAMES = tuple(case_table())


def build_case(name, ortho, chain_table=None):
    """the scene of a golden case for one projection"""
    screen, build, ballast = case_table()[name]
    chain_table = chains() if chain_table is None else chain_table
    cam = Camera(ortho, screen)
    rng = np.random.default_rng(zlib.crc32(name.encode()))  # the same for both projections: random scenes differ in the frustum block only
    b = Builder(cam, rng)
    if ballast:
        b.ballast()
    dispatches = build(cam, rng, b)
    return b.scene(screen, chain_table[screen], dispatches)


def random_scene(seed, ortho, tasks=40, screen="a", chain=None):
    """a seeded scene beyond the stored ones; chain: (flat, width, height, levels), default the synthetic one"""
    cam = Camera(ortho, screen)
    rng = np.random.default_rng(seed)
    b = Builder(cam, rng)
    random_tasks(b, rng, tasks)
    return b.scene(screen, chains()[screen] if chain is None else chain, one_list(len(b.tasks)))


def run_reference(scene, phase, flags):
    """every dispatch of the scene through meshlet_cull_ref, one after the other: (output, occluders, summed info)"""
    s = dict(scene)
    total = ref.Info()
    for offset, count, mdi, draw in scene["dispatches"]:
        s["output"], s["occluders"], info = ref.cull(s, phase, flags, int(offset), int(count), int(mdi), int(draw))
        for k, v in info.items():
            total[k] += v
    return s["output"], s["occluders"], total


# ---- the golden ---------------------------------------------------------------------------------------------------------------------------
SCENE_ARRAYS = ("tasks", "aabbs", "transforms", "bounds", "draws", "occluders", "output", "frustum", "camera", "dispatches")
CHAIN_KEYS = tuple(sorted(SCREENS))


def pack_scene(scene):
    """name -> array, the small arrays in one: {chain, camera bits, frustum, dispatches}"""
    params = np.concatenate([[CHAIN_KEYS.index(scene["chain_key"])], scene["camera"].view(np.uint32), scene["frustum"], scene["dispatches"].ravel()]).astype(np.uint32)
    return {"params": params, **{a: scene[a] for a in ("tasks", "aabbs", "transforms", "bounds", "draws", "occluders")}, "output_dwords": np.array(len(scene["output"]), np.uint32)}


def load_golden():
    return np.load(GOLDEN_PATH)


def golden_scene(golden, name, ortho):
    """arrays an orthographic scene shares with the perspective one are stored once, under o0"""
    def get(a):
        key = f"{name}/o{int(bool(ortho))}/{a}"
        return golden[key] if key in golden else golden[f"{name}/o0/{a}"]
    s = {a: get(a) for a in ("tasks", "aabbs", "transforms", "bounds", "draws", "occluders")}
    params = get("params")
    s["chain_key"] = CHAIN_KEYS[int(params[0])]
    s["camera"], s["frustum"], s["dispatches"] = params[1:4].view(np.float32), params[4:60], params[60:].reshape(-1, 4)
    s["output"] = np.full(int(get("output_dwords")), ref.POISON_WORD, np.uint32)
    s["output"][:COUNT_WORDS] = 0
    s["chain"] = golden[f"chain/{s['chain_key']}"]
    s["chain_width"], s["chain_height"], s["chain_levels"] = (int(v) for v in golden[f"chain/{s['chain_key']}/shape"])
    return s


def compact_output(scene, output):
    """What an output buffer holds beyond the scene's own data: per list the count word and, per record in buffer order, {chunk, task}.
    expand_output() gives the buffer back; the generator asserts that it does, dword for dword."""
    draws = np.asarray(scene["draws"], np.uint32).reshape(-1, 3)
    first = {int(d[1]): k for k, d in enumerate(draws) if d[0]}
    counts, rows = [], []
    for mdi in dispatches_lists(scene["dispatches"]):
        draw = int([d for d in scene["dispatches"] if int(d[2]) == mdi][0][3])
        count, r = ref.records(output, mdi, draw)
        counts.append(count)
        rows += [(mdi, first.get(int(rec[2]), 0xFFFFFFFF), int(rec[4])) for rec in r]
    return np.array(counts, np.uint32), np.array(rows, np.uint32).reshape(-1, 3)


def expand_output(scene, counts, rows):
    output = np.array(scene["output"], np.uint32)
    draws = np.asarray(scene["draws"], np.uint32).reshape(-1, 3)
    for mdi, count in zip(dispatches_lists(scene["dispatches"]), counts):
        draw = int([d for d in scene["dispatches"] if int(d[2]) == mdi][0][3])
        output[mdi] = count
        mine = rows[rows[:, 0] == mdi]
        for k, (_, chunk, task) in enumerate(mine):
            output[draw + 5 * k:draw + 5 * k + 5] = (draws[chunk, 0], 1, draws[chunk, 1], draws[chunk, 2], task)
    return output


def pack_result(scene, output, occluders):
    counts, rows = compact_output(scene, output)
    return np.concatenate([counts, occluders, rows.ravel()]).astype(np.uint32)


def golden_result(golden, name, phase, flags):
    """(output buffer, occluder words) of the executed shader"""
    scene = golden_scene(golden, name, bool(flags & ref.ORTHO))
    r = golden[f"{name}/{set_name(phase, flags)}"]
    lists, words = len(dispatches_lists(scene["dispatches"])), len(scene["occluders"])
    return expand_output(scene, r[:lists], r[lists + words:].reshape(-1, 3)), r[lists:lists + words]


def canonical(scene, output):
    """what is specified of an output buffer: per list (count, records sorted by (task_index, first_index)), and the rest of the buffer"""
    rest = np.array(output, np.uint32)
    lists = []
    for mdi in dispatches_lists(scene["dispatches"]):
        draw = int([d for d in scene["dispatches"] if int(d[2]) == mdi][0][3])
        count, r = ref.records(output, mdi, draw)
        lists.append((count, ref.sorted_records(r)))
        rest[mdi] = 0
        rest[draw:draw + 5 * len(r)] = 0
    return lists, rest


def assert_same(scene, got_output, got_occluders, want_output, want_occluders, what):
    got, got_rest = canonical(scene, got_output)
    want, want_rest = canonical(scene, want_output)
    for (gc, gr), (wc, wr) in zip(got, want):
        assert gc == wc, f"{what}: count {gc}, expected {wc}"
        assert np.array_equal(gr, wr), f"{what}: {int((gr != wr).any(axis=1).sum())} records differ"
    assert np.array_equal(got_rest, want_rest), f"{what}: dwords outside the records and count words differ (poison overwritten, or another list's count)"
    assert np.array_equal(got_occluders, want_occluders), f"{what}: {int((got_occluders != want_occluders).sum())} occluder words differ"
    for mdi in dispatches_lists(scene["dispatches"]):
        draw = int([d for d in scene["dispatches"] if int(d[2]) == mdi][0][3])
        ref.assert_task_order(ref.records(got_output, mdi, draw)[1], scene["draws"], scene["tasks"])


def hostile_scene(ortho, seed=7):
    """a random scene whose device data points outside its arrays, whose output is too small, and whose bounds hold values no int holds"""
    s = random_scene(seed, ortho, tasks=24)
    tasks = s["tasks"].copy()
    tasks[1, 0] = len(s["aabbs"]) + 3            # AABB past the array
    tasks[2, 2] = 0xFFFFFFFF                     # transform past the array
    tasks[3, 3] = (len(s["bounds"]) & ~31) + 40  # chunks past bounds and draws
    tasks[4, 1] = len(s["occluders"]) + 100      # occluder word past the array
    tasks[5, 3] = (len(s["bounds"]) - 32) + 31   # the last 32 slots, all of them
    s["tasks"] = tasks
    bounds = s["bounds"].copy()
    bounds[int(tasks[6, 3]) & ~31] = [1e30, -1e30, 1e30, 1e30, 0, 0, 1, 1]
    bounds[(int(tasks[7, 3]) & ~31)] = [np.nan, 0, 0, 1, 0, 0, 1, 1]
    bounds[(int(tasks[8, 3]) & ~31)] = [np.inf, 0, 0, 1, 0, 0, 1, 1]
    bounds[(int(tasks[9, 3]) & ~31)] = [0, 0, 0, 3e9, 0, 0, 1, 1]
    s["bounds"] = bounds
    s["output"] = s["output"][:COUNT_WORDS + 5 * 9 + 3].copy()  # nine records fit, the tenth would end past the buffer
    s["dispatches"] = np.array([[2, len(tasks) + 50, 0, COUNT_WORDS]], np.uint32)  # reaches past the task array
    return s
