"""The ocean's LOD update restated in numpy (ocean/update_lod.comp, init_counter_buffer.comp, cull_blocks.comp), the push
blocks Ocean::update_lod_pass derives from a configuration and a camera, and the static meshes of Ocean::build_buffers.

update_lod() and cull_blocks() repeat the shaders' fp32 operations one by one (sums in dot()'s left-to-right order); log2 alone is taken in
float64 and rounded to fp32.  The five LOD taps address texels -- (coord + offset) mod N or clamped -- which for a power-of-two N is what
the shader's uv = (coord + 0.5) / N selects with a nearest sampler; tests/golden/make_ocean_lod_golden.py checks that on every case."""
import numpy as np

f32 = np.float32
MAX_LOD_INDIRECT = 8
HEIGHTMAP_RANGE = (-10.0, 10.0)
GUARD_BAND = 5.0
NEAR_TIE = 2.0 ** -16  # see near_tie_mask


# ---- push blocks, as dwords ----------------------------------------------------------------------------------------------------------
def update_lod_push(camera, max_lod, image_offset, n, grid_base, grid_size, lod_bias):
    """gr_push_ocean_update_lod, 16 dwords"""
    p = np.zeros(16, np.uint32)
    p[0:3] = np.array(camera, f32).view(np.uint32)
    p[3:4] = np.array([max_lod], f32).view(np.uint32)
    p[4:6] = np.array(image_offset, np.int32).view(np.uint32)
    p[6:8] = n
    p[8:10] = np.array(grid_base, f32).view(np.uint32)
    p[10:12] = np.array(grid_size, f32).view(np.uint32)
    p[12:13] = np.array([lod_bias], f32).view(np.uint32)
    return p


def cull_push(world_offset, image_offset, n, grid_base, grid_size, grid_resolution, lod_stride, max_lod, handle_edge_lods,
              heightmap_range=HEIGHTMAP_RANGE, guard_band=GUARD_BAND):
    """gr_push_ocean_cull, 24 dwords"""
    p = np.zeros(24, np.uint32)
    p[0:3] = np.array(world_offset, f32).view(np.uint32)
    p[4:6] = np.array(image_offset, np.int32).view(np.uint32)
    p[6:8] = n
    p[8:10] = (f32(1.0) / np.array([n, n], f32)).view(np.uint32)
    p[10:12] = np.array(grid_base, f32).view(np.uint32)
    p[12:14] = np.array(grid_size, f32).view(np.uint32)
    p[14:16] = np.array(grid_resolution, f32).view(np.uint32)
    p[16:18] = np.array(heightmap_range, f32).view(np.uint32)
    p[18:19] = np.array([guard_band], f32).view(np.uint32)
    p[19] = lod_stride
    p[20:21] = np.array([max_lod], f32).view(np.uint32)
    p[21] = handle_edge_lods
    return p


# ---- what the host derives (renderer/ocean.cpp:263-393, 960-974) -----------------------------------------------------------------------
def lod_count(grid_resolution):
    """quad_lod.size(): one LOD per halving of grid_resolution down to 2"""
    return int(grid_resolution).bit_length() - 1


def round_half_away(v):
    v = np.asarray(v, f32)
    return (np.sign(v) * np.floor(np.abs(v).astype(np.float64) + 0.5)).astype(f32)


def pass_pushes(grid_count, grid_resolution, ocean_size, lod_bias, camera, fixed_position=False, center=(0.0, 0.0, 0.0)):
    """-> dict(update=, cull=, wrap=, world_offset=, coord_offset=, base_coord=) for a camera position, fp32 as the host computes it"""
    size = np.array(ocean_size, f32)
    cam = np.array(camera, f32)
    grid_size = size / f32(grid_count)
    max_lod = float(lod_count(grid_resolution) - 1)
    if fixed_position:
        world_offset = np.array(center, f32) - np.array([size[0] * f32(0.5), 0.0, size[1] * f32(0.5)], f32)
        base_coord = np.zeros(2, np.int32)
        image_offset, grid_base, coord_offset = (0, 0), np.zeros(2, f32), np.zeros(2, f32)
    else:
        world_offset = np.zeros(3, f32)
        snapped = round_half_away(cam[[0, 2]] * (np.array([grid_count, grid_count], f32) / size))
        base_coord = snapped.astype(np.int32) - (grid_count >> 1)
        image_offset, grid_base = base_coord, base_coord.astype(f32) * grid_size
        coord_offset = (base_coord * int(grid_resolution)).astype(f32)
    update = update_lod_push(cam - world_offset, max_lod, image_offset, grid_count, grid_base, grid_size, lod_bias)
    cull = cull_push(world_offset, image_offset, grid_count, grid_base, grid_size, (grid_resolution, grid_resolution), grid_count * grid_count, max_lod,
                     0 if fixed_position else 1)
    return dict(update=update, cull=cull, wrap=0 if fixed_position else 1, world_offset=world_offset, coord_offset=coord_offset, base_coord=base_coord)


# ---- update_lod.comp -----------------------------------------------------------------------------------------------------------------
def float_to_half(values):
    return np.asarray(values).astype(np.float16).view(np.uint16)


def half_to_float(bits, dtype=f32):
    return np.ascontiguousarray(bits).view(np.float16).astype(dtype)


def update_lod(push, dtype=f32):
    """-> (image (n, n) of fp16 bits, stored at (id + image_offset) & (n - 1); the LOD before the fp16 rounding, same layout).  dtype
    float64 gives the formula, float32 the shader's operations."""
    pf = push.view(f32).astype(dtype)
    off = push[4:6].view(np.int32)
    n = int(push[6])
    cam, max_lod, base, size, bias = pf[0:3], pf[3], pf[8:10], pf[10:12], pf[12]
    x, y = np.meshgrid(np.arange(n), np.arange(n))
    one, zero, half = dtype(1.0), dtype(0.0), dtype(0.5)
    x00, y00 = base[0] + x.astype(dtype) * size[0], base[1] + y.astype(dtype) * size[1]

    def dist(px, pz):
        dx, dy, dz = cam[0] - px, cam[1] - zero, cam[2] - pz
        return (dx * dx + dy * dy) + dz * dz

    d = dist(x00 + half * size[0], y00 + half * size[1])
    for fx, fy in ((zero, zero), (one, zero), (zero, one), (one, one)):
        d = np.minimum(d, dist(x00 + fx * size[0], y00 + fy * size[1]))
    lod = half * np.log2((d + one).astype(np.float64)).astype(dtype) + bias
    lod = np.minimum(np.maximum(lod, zero), max_lod)
    assert lod.dtype == dtype
    image, raw = np.zeros((n, n), np.uint16), np.zeros((n, n), dtype)
    ix, iy = (x + int(off[0])) & (n - 1), (y + int(off[1])) & (n - 1)
    image[iy, ix] = float_to_half(lod)
    raw[iy, ix] = lod
    return image, raw


def near_tie_mask(lod64):
    """texels whose float64 LOD lies within 2^-16 of a midpoint between adjacent fp16 values: there an fp32 chain that differs from
    another in its last bits (a few ulps of d2, one of log2, about 1e-6 at values up to 8) may round to the other fp16 neighbour.  2^-16
    is more than ten times that error."""
    v = np.asarray(lod64, np.float64)
    with np.errstate(over="ignore"):
        lo = v.astype(np.float16)
    lo = np.where(lo.astype(np.float64) > v, np.nextafter(lo, np.float16(-np.inf)), lo).astype(np.float16)
    hi = np.nextafter(lo, np.float16(np.inf))
    mid = 0.5 * (lo.astype(np.float64) + hi.astype(np.float64))
    return np.abs(v - mid) <= NEAR_TIE


# ---- init_counter_buffer.comp --------------------------------------------------------------------------------------------------------
def init_counters(counts16):
    draws = np.zeros((MAX_LOD_INDIRECT, 8), np.uint32)
    draws[:, 0] = np.asarray(counts16, np.uint32)[:MAX_LOD_INDIRECT]
    return draws


# ---- cull_blocks.comp ----------------------------------------------------------------------------------------------------------------
def box_distances(push, frustum):
    """-> (n, n, 6) fp32 plane distances of each block's deciding corner, and (n, n, 6) float64 sums of |p_i c_i| + |p_w|"""
    pf = push.view(f32)
    n = int(push[6])
    wo, base, size, rng, guard = pf[0:3], pf[10:12], pf[12:14], pf[16:18], pf[18]
    planes = np.asarray(frustum, f32).reshape(6, 4)
    x, y = np.meshgrid(np.arange(n), np.arange(n))
    min_x, min_z = base[0] + x.astype(f32) * size[0], base[1] + y.astype(f32) * size[1]
    max_x, max_z = min_x + size[0], min_z + size[1]
    lo = [(min_x - guard) + wo[0], np.full_like(min_x, rng[0] + wo[1]), (min_z - guard) + wo[2]]
    hi = [(max_x + guard) + wo[0], np.full_like(min_x, rng[1] + wo[1]), (max_z + guard) + wo[2]]
    dist, scale = np.zeros((n, n, 6), f32), np.zeros((n, n, 6), np.float64)
    for i, p in enumerate(planes):
        c = [hi[k] if p[k] > 0 else lo[k] for k in range(3)]
        dist[..., i] = ((c[0] * p[0] + c[1] * p[1]) + c[2] * p[2]) + f32(1.0) * p[3]
        scale[..., i] = sum(np.abs(c[k].astype(np.float64) * float(p[k])) for k in range(3)) + abs(float(p[3]))
    assert dist.dtype == f32
    return dist, scale


def taps(coord_x, coord_y, n, wrap):
    """the five texel coordinates (centre, -x, +x, -y, +y) of a block at image coordinate coord"""
    out = []
    for ox, oy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
        cx, cy = coord_x + ox, coord_y + oy
        out.append((np.mod(cx, n), np.mod(cy, n)) if wrap else (np.clip(cx, 0, n - 1), np.clip(cy, 0, n - 1)))
    return out


def cull_blocks(lod_bits, push, frustum, wrap, draws):
    """-> (draws after the pass, list of MAX_LOD_INDIRECT arrays (k, 8) float32: each bucket's patches in invocation order)"""
    pf = push.view(f32)
    off = push[4:6].view(np.int32)
    n = int(push[6])
    res, max_lod, edge = pf[14:16], pf[20], int(push[21])
    dist, _ = box_distances(push, frustum)
    inside = np.all(dist >= 0, axis=-1)  # the early break decides nothing: the box is kept only if every plane keeps it
    lods = half_to_float(lod_bits).reshape(n, n)
    x, y = np.meshgrid(np.arange(n), np.arange(n))
    cx, cy = x + int(off[0]), y + int(off[1])
    t = [lods[ty, tx] for tx, ty in taps(cx, cy, n, wrap)]
    centre, four = t[0], [np.maximum(v, t[0]) for v in t[1:]]
    if edge:
        for k, mask in enumerate((x == 0, x == n - 1, y == 0, y == n - 1)):
            four[k] = np.where(mask, max_lod, four[k]).astype(f32)
    least = np.minimum(centre, np.minimum(np.minimum(four[0], four[2]), np.minimum(four[1], four[3])))
    bucket = least.astype(np.int32)
    patch = np.stack([cx.astype(f32) * res[0], cy.astype(f32) * res[1], centre, np.zeros_like(centre), *four], -1).astype(f32)
    draws = np.array(draws, np.uint32).reshape(MAX_LOD_INDIRECT, 8).copy()
    out = []
    for l in range(MAX_LOD_INDIRECT):
        sel = inside & (bucket == l)
        out.append(patch[sel])  # row-major: the order of a serial run
        draws[l, 1] += np.uint32(sel.sum())
    return draws, out


def sorted_bucket(patches):
    """a bucket's patches (k, 8) as a sorted set: by offsets.y, then offsets.x (unique per block)"""
    p = np.asarray(patches, f32).reshape(-1, 8)
    return p[np.lexsort((p[:, 0], p[:, 1]))]


def buckets_of(buffer, draws, lod_stride):
    """the first instance_count entries of every bucket of an ocean-lod-data buffer, each as a sorted set"""
    flat = np.asarray(buffer).view(f32).reshape(-1, 8)
    draws = np.asarray(draws, np.uint32).reshape(MAX_LOD_INDIRECT, 8)
    return [sorted_bucket(flat[l * lod_stride:l * lod_stride + int(draws[l, 1])]) if l * lod_stride < len(flat) else np.zeros((0, 8), f32)
            for l in range(MAX_LOD_INDIRECT)]


# ---- meshes (renderer/ocean.cpp:1102-1406) -------------------------------------------------------------------------------------------
RESTART = 0xffff


def strip_indices(size, base_index=0):
    idx = []
    for s in range(size):
        base = s * (size + 1)
        for x in range(size + 1):
            idx += [base_index + base + x, base_index + base + size + 1 + x]
        idx.append(RESTART)
    return idx


def build_lod(grid_resolution, size, stride):
    """-> (vertices (size + 1)^2 x 8 uint8: pos[4], weights[4]; indices uint16)"""
    half = grid_resolution >> 1
    v = []
    for y in range(0, grid_resolution + 1, stride):
        for x in range(0, grid_resolution + 1, stride):
            w = [0, 0, 0, 0]
            if x == 0:
                w[0] = 255
            elif x == grid_resolution:
                w[1] = 255
            elif y == 0:
                w[2] = 255
            elif y == grid_resolution:
                w[3] = 255
            v.append([x & 255, y & 255, int(x < half), int(y < half)] + w)
    return np.array(v, np.uint8), np.array(strip_indices(size), np.uint16)


def lod_meshes(grid_resolution):
    out, size, stride = [], grid_resolution, 1
    while size >= 2:
        out.append(build_lod(grid_resolution, size, stride))
        size >>= 1
        stride <<= 1
    return out


def border_mesh(grid_count, grid_resolution, heightmap=True, fixed_position=False):
    """-> (positions (k, 3) float32, indices uint16): the plane grid when there is no heightmap, then, unless the position is fixed, four
    borders, four corners and four fill edges"""
    pos, idx = [], []
    if not heightmap:
        size, stride = grid_count * 2, grid_resolution >> 1
        for y in range(size + 1):
            for x in range(size + 1):
                pos.append((x * stride, y * stride, 1.0))
        idx += strip_indices(size)
    if not fixed_position:
        gc, full = grid_count, grid_count * grid_resolution
        outer, inner = full >> 3, grid_resolution >> 1
        v = lambda a, b: np.array([a, b], np.int64)

        def border(base, dx, dy):
            for i in range((gc * 2 + 1) * 2):
                p = base + (i >> 1) * dx + (i & 1) * dy
                idx.append(len(pos))
                pos.append((p[0], p[1], (i & 1) ^ 1))
            idx.append(RESTART)

        def corner(base, dx, dy):
            idx.extend(range(len(pos), len(pos) + 4))
            idx.append(RESTART)
            for p, z in ((base, 1), (base + dx, 0), (base + dy, 0), (base + dx + dy, 0)):
                pos.append((p[0], p[1], z))

        def fill_edge(base_outer, end_outer, base_inner, delta, corner_delta):
            count = gc * 2 + 3
            base_inner = base_inner.copy()
            for i in range(count):
                p = base_inner - corner_delta if i == 0 else (base_inner + corner_delta if i + 1 == count else base_inner)
                idx.append(len(pos))
                pos.append((p[0], p[1], 0.0))
                t = f32(i) / f32(count - 1)
                o = [round_half_away(f32(a) * (f32(1.0) - t) + f32(b) * t) for a, b in zip(base_outer, end_outer)]
                idx.append(len(pos))
                pos.append((o[0], o[1], 0.0))
                if i + 2 < count and i != 0:
                    base_inner = base_inner + delta

            idx.append(RESTART)

        border(v(full, 0), v(-inner, 0), v(0, -outer))
        border(v(0, 0), v(0, inner), v(-outer, 0))
        border(v(0, full), v(inner, 0), v(0, outer))
        border(v(full, full), v(0, -inner), v(outer, 0))
        corner(v(0, 0), v(0, -outer), v(-outer, 0))
        corner(v(0, full), v(-outer, 0), v(0, outer))
        corner(v(full, 0), v(outer, 0), v(0, -outer))
        corner(v(full, full), v(0, outer), v(outer, 0))
        neg, posi = float(-32 * 1024), float(f32(32 * 1024) + f32(full))
        fill_edge((posi, neg), (neg, neg), v(full, -outer), v(-inner, 0), v(-outer, 0))
        fill_edge((neg, neg), (neg, posi), v(-outer, 0), v(0, inner), v(0, outer))
        fill_edge((neg, posi), (posi, posi), v(0, outer + full), v(inner, 0), v(outer, 0))
        fill_edge((posi, posi), (posi, neg), v(outer + full, full), v(0, -inner), v(0, -outer))
    return np.array(pos, f32).reshape(-1, 3), np.array(idx, np.uint16)


def draw_data(fft_resolution, grid_count, grid_resolution, ocean_size, normal_mod, world_offset, coord_offset):
    """OceanData (renderer/ocean.cpp:826-835, 1084-1090) as 16 floats: world_offset at 0, coord_offset at 4, inv_heightmap_size at 6,
    inv_ocean_grid_size at 8, normal_uv_scale at 10, integer_to_world_mod at 12, heightmap_range at 14"""
    d = np.zeros(16, f32)
    d[0:3] = world_offset
    d[4:6] = coord_offset
    d[6:8] = f32(1.0) / f32(fft_resolution)
    d[8:10] = f32(1.0) / f32(grid_count * grid_resolution)
    d[10:12] = f32(normal_mod)
    d[12:14] = (np.array(ocean_size, f32) / f32(grid_count)) / f32(grid_resolution)
    d[14:16] = HEIGHTMAP_RANGE
    return d
